"""Reducing receives between device buffers, through the library: the message
is combined into the buffer inside the receiver's pull kernel (k_pull_reduce,
k_pull_reduce_done in src/transport/pull_kernels.h).  Every result is
compared bit for bit with torch on the CPU, which computes what
src/transport/reduce.h defines (IEEE float32 add, bf16 as the rounded float32
sum, wrapping int32), and every destination sits between sentinel elements
that must survive.

The cases run in fresh child processes (the MPIX_* switches are read once per
process), each under a time limit, chained so that nothing is started after a
child that failed or timed out:

  word / tail / event   MPIX_PULL_DONE: device loopback for f32, bf16 and i32
                        at 1 element, T + 16 B and 3T + an odd count
                        (T = 16 KiB)
  features              capture and three replays; 16 kernel-published
                        partitions of 4 KiB, two iterations; two receives
                        into one buffer; misaligned slices; a strided sender;
                        host/device mismatches
  noruns                the partitions again with MPIX_PART_RUNS=0

and examples/ring_allreduce.py's exchange between two processes on one GPU.
"""
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import run_ranks

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 180  # s; a child takes a few seconds
T = 16384
PAD = 64             # sentinel elements on both sides: a multiple of 16 B
PARTS, PART_BYTES, ITERS = 16, 4096, 2

LOOPBACK = ["loopback"]
FEATURES = ["capture", "partitions", "same_buffer", "misaligned",
            "strided_sender", "kind_mismatch"]
CHILDREN = {
    "word": ({"MPIX_PULL_DONE": "word"}, LOOPBACK),
    "tail": ({"MPIX_PULL_DONE": "tail"}, LOOPBACK),
    "event": ({"MPIX_PULL_DONE": "event"}, LOOPBACK),
    "features": ({}, FEATURES),
    "noruns": ({"MPIX_PART_RUNS": "0"}, ["partitions"]),
}
ENV_KEYS = ("MPIX_PULL_DONE", "MPIX_PART_RUNS", "MPIX_PULL_BLOCKS",
            "MPIX_DEV_PUSH_MAX", "MPIX_FAST_WAIT")


# ------------------------------------------------------------------ child

def values(torch, dtype, n, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int32:  # the whole range: sums wrap
        return torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g,
                             dtype=torch.int64).to(torch.int32)
    return (torch.randn(n, generator=g) * 3).to(dtype)


def combine(torch, a, b, op):
    if op == "sum":
        return a + b
    return torch.maximum(a, b) if op == "max" else torch.minimum(a, b)


def same_bits(torch, x, y):
    assert x.dtype == y.dtype and x.shape == y.shape
    return bool(torch.equal(x.contiguous().view(torch.uint8),
                            y.contiguous().view(torch.uint8)))


class Padded:
    """A device buffer of n elements holding `init`, `offset` elements into
    an allocation that is sentinel everywhere else."""

    def __init__(self, torch, init, offset=0):
        self.torch, self.n, self.at = torch, init.numel(), PAD + offset
        sent = torch.tensor(-77, dtype=init.dtype)
        self.whole = sent.repeat(self.n + 2 * PAD + offset).cuda()
        self.buf = self.whole[self.at:self.at + self.n]
        self.buf.copy_(init)
        self.sent = sent

    def check(self, want, what):
        got = self.whole.cpu()
        assert same_bits(self.torch, got[self.at:self.at + self.n], want), what
        assert bool((got[:self.at] == self.sent).all()), what + ": before"
        assert bool((got[self.at + self.n:] == self.sent).all()), \
            what + ": behind"


def case_loopback(mpix, torch):
    stream = torch.cuda.current_stream()
    tag = 0
    for dtype in (torch.float32, torch.bfloat16, torch.int32):
        es = torch.empty(0, dtype=dtype).element_size()
        for n in (1, (T + 16) // es, 3 * T // es + 1237):
            for op in ("sum", "max", "min"):
                tag += 1
                a = values(torch, dtype, n, 2 * tag)
                b = values(torch, dtype, n, 2 * tag + 1)
                dst = Padded(torch, a)
                msg = b.cuda()
                torch.cuda.synchronize()
                rr = mpix.irecv_reduce_enqueue(dst.buf, source=0, op=op,
                                               tag=tag, stream=stream)
                rs = mpix.isend_enqueue(msg, dest=0, tag=tag, stream=stream)
                if op == "sum":
                    mpix.waitall_enqueue([rs, rr], stream=stream)
                    torch.cuda.synchronize()
                else:  # the host wait and its status
                    st = mpix.wait(rr)
                    mpix.wait(rs)
                    assert st["error"] == 0 and st["count_bytes"] == n * es
                    torch.cuda.synchronize()
                dst.check(combine(torch, a, b, op), f"{dtype} {n} {op}")
                assert same_bits(torch, msg.cpu(), b), "the source changed"
    return {"messages": tag}


def case_capture(mpix, torch):
    """Captured once, launched three times: the buffer accumulates three
    times."""
    n = (T + 16) // 4
    a = values(torch, torch.float32, n, 1)
    b = values(torch, torch.float32, n, 2)
    dst = Padded(torch, a)
    msg = b.cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        mpix.stream_begin_capture(s.cuda_stream)
        rs = mpix.isend_enqueue(msg, dest=0, tag=3, stream=s)
        rr = mpix.irecv_reduce_enqueue(dst.buf, source=0, tag=3, stream=s)
        mpix.waitall_enqueue([rs, rr], stream=s)
        graph, gexec = mpix.stream_end_capture(s.cuda_stream)
    want = a
    for it in range(3):
        mpix.graph_launch(gexec, s.cuda_stream)
        torch.cuda.synchronize()
        want = want + b
        dst.check(want, f"replay {it}")
    mpix.graph_exec_destroy(gexec)
    mpix.graph_destroy(graph)
    return {}


def case_partitions(mpix, torch):
    """16 partitions of 4 KiB made ready by one device kernel, two
    iterations on the same requests: the second accumulates on the first."""
    per = PART_BYTES // 4
    stream = torch.cuda.current_stream()
    a = values(torch, torch.int32, PARTS * per, 5)
    dst = Padded(torch, a)
    send = torch.zeros(PARTS * per, dtype=torch.int32, device="cuda")
    pr = mpix.precv_reduce_init(dst.buf, PARTS, source=0, op="sum", tag=7)
    ps = mpix.psend_init(send, PARTS, dest=0, tag=7)
    dps = mpix.prequest_create(ps)
    dpr = mpix.prequest_create(pr)
    want = a
    for it in range(ITERS):
        b = values(torch, torch.int32, PARTS * per, 10 + it)
        send.copy_(b)
        torch.cuda.synchronize()
        mpix.start(pr)
        mpix.start(ps)
        mpix.launch_pready_all(dps, PARTS, stream.cuda_stream)
        mpix.launch_wait_arrived_all(dpr, PARTS, stream.cuda_stream)
        torch.cuda.synchronize()
        for p in range(PARTS):
            assert mpix.parrived(pr, p)
        st = mpix.wait(pr)
        mpix.wait(ps)
        assert st["error"] == 0
        want = want + b
        dst.check(want, f"iteration {it}")
    mpix.prequest_free(dps)
    mpix.prequest_free(dpr)
    mpix.request_free(ps)
    mpix.request_free(pr)
    return {}


def case_same_buffer(mpix, torch):
    """Two reducing receives from two tags into the SAME buffer, made ready
    together: the library serialises them.  Integer-valued floats: the
    result is exact whatever the order."""
    stream = torch.cuda.current_stream()
    n = 3 * T // 4 + 77
    a = torch.arange(n, dtype=torch.float32) % 1000
    b1 = torch.arange(n, dtype=torch.float32) % 77 + 1
    b2 = torch.arange(n, dtype=torch.float32) % 13 + 100
    dst = Padded(torch, a)
    m1, m2 = b1.cuda(), b2.cuda()
    torch.cuda.synchronize()
    # and a third one into an overlapping slice of it
    r1 = mpix.irecv_reduce_enqueue(dst.buf, source=0, tag=11, stream=stream)
    r2 = mpix.irecv_reduce_enqueue(dst.buf, source=0, tag=12, stream=stream)
    r3 = mpix.irecv_reduce_enqueue(dst.buf[8:4104], source=0, tag=13,
                                   stream=stream)
    s1 = mpix.isend_enqueue(m1, dest=0, tag=11, stream=stream)
    s2 = mpix.isend_enqueue(m2, dest=0, tag=12, stream=stream)
    s3 = mpix.isend_enqueue(m1[:4096], dest=0, tag=13, stream=stream)
    mpix.waitall_enqueue([r1, r2, r3, s1, s2, s3], stream=stream)
    torch.cuda.synchronize()
    want = a + b1 + b2
    want[8:4104] += b1[:4096]
    dst.check(want, "three receives into one buffer")
    return {}


def case_misaligned(mpix, torch):
    """Element-aligned, not 16-byte-aligned slices on either side: the
    element path."""
    stream = torch.cuda.current_stream()
    tag = 20
    for dtype in (torch.float32, torch.bfloat16):
        es = torch.empty(0, dtype=dtype).element_size()
        n = (T + 16) // es + 3
        for d_off, s_off in ((1, 0), (0, 1), (3, 1)):
            tag += 1
            a = values(torch, dtype, n, tag)
            b = values(torch, dtype, n, 100 + tag)
            dst = Padded(torch, a, offset=d_off)
            msg = torch.zeros(n + 8, dtype=dtype, device="cuda")
            msg[s_off:s_off + n].copy_(b)
            torch.cuda.synchronize()
            assert (dst.buf.data_ptr() % 16 != 0) == (d_off != 0)
            rr = mpix.irecv_reduce_enqueue(dst.buf, source=0, tag=tag,
                                           stream=stream)
            rs = mpix.isend_enqueue(msg[s_off:s_off + n], dest=0, tag=tag,
                                    stream=stream)
            mpix.waitall_enqueue([rs, rr], stream=stream)
            torch.cuda.synchronize()
            dst.check(a + b, f"{dtype} dst+{d_off} src+{s_off}")
    return {}


def case_strided_sender(mpix, torch):
    stream = torch.cuda.current_stream()
    a = values(torch, torch.float32, 6 * 48, 30)
    dst = Padded(torch, a)
    src = torch.ones(6, 64, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rr = mpix.irecv_reduce_enqueue(dst.buf, source=0, tag=31, stream=stream)
    rs = mpix.isend_enqueue(src[:, :48], dest=0, tag=31, stream=stream)
    st = mpix.wait(rr)
    st_s = mpix.wait(rs)  # the sender is acked and completes
    torch.cuda.synchronize()
    assert st["error"] == mpix._C.ERR_TYPE, st
    assert st_s["error"] == 0, st_s
    dst.check(a, "untouched")
    return {}


def case_kind_mismatch(mpix, torch):
    import numpy as np
    stream = torch.cuda.current_stream()
    a = values(torch, torch.float32, 1000, 40)
    # host message into a device reducing receive
    dst = Padded(torch, a)
    torch.cuda.synchronize()
    rr = mpix.irecv_reduce_enqueue(dst.buf, source=0, tag=41, stream=stream)
    rs = mpix.isend_enqueue(np.ones(1000, np.float32), dest=0, tag=41)
    st, st_s = mpix.wait(rr), mpix.wait(rs)
    torch.cuda.synchronize()
    assert st["error"] == mpix._C.ERR_TYPE and st_s["error"] == 0, (st, st_s)
    dst.check(a, "device buffer untouched")
    # device message into a host reducing receive
    host = a.numpy().copy()
    msg = torch.ones(1000, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rr = mpix.irecv_reduce_enqueue(host, source=0, tag=42)
    rs = mpix.isend_enqueue(msg, dest=0, tag=42, stream=stream)
    st, st_s = mpix.wait(rr), mpix.wait(rs)
    assert st["error"] == mpix._C.ERR_TYPE and st_s["error"] == 0, (st, st_s)
    assert host.tobytes() == a.numpy().tobytes()
    # the pair still works
    rr = mpix.irecv_reduce_enqueue(dst.buf, source=0, tag=43, stream=stream)
    rs = mpix.isend_enqueue(msg, dest=0, tag=43, stream=stream)
    mpix.waitall_enqueue([rs, rr], stream=stream)
    torch.cuda.synchronize()
    dst.check(a + 1, "after the mismatches")
    return {}


def child_main(name):
    sys.path.insert(0, REPO)
    import torch
    import mpix

    run = {"loopback": case_loopback, "capture": case_capture,
           "partitions": case_partitions, "same_buffer": case_same_buffer,
           "misaligned": case_misaligned,
           "strided_sender": case_strided_sender,
           "kind_mismatch": case_kind_mismatch}
    for case in CHILDREN[name][1]:
        # the library's counters go to stderr at finalize: mark whose
        sys.stderr.write(f"CASE-BEGIN {case}\n")
        sys.stderr.flush()
        mpix.init()
        try:
            res = run[case](mpix, torch)
        finally:
            mpix.finalize()
        print("CASE " + json.dumps({"name": case, **res}), flush=True)
    print("CHILD-DONE", flush=True)


# ----------------------------------------------------------------- parent

_results = {}  # child -> {case: {..., "stderr": its part of the stderr}}
_dead = []     # why no further process may be started


def _child(name):
    if name in _results:
        return _results[name]
    if _dead:
        pytest.fail("not started: " + _dead[0])
    env = {k: v for k, v in os.environ.items() if k not in ENV_KEYS}
    env.update(RANK="0", WORLD_SIZE="1", MPIX_STATS="1", MPIX_TRACE="1")
    env.update(CHILDREN[name][0])
    try:
        run = subprocess.run([sys.executable, os.path.abspath(__file__),
                              "--child", name], env=env, capture_output=True,
                             text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout
        done = re.findall(r'^CASE {"name": "(\w+)"', out or "", re.M)
        _dead.append(f"child {name} timed out after {CHILD_TIMEOUT} s; "
                     f"finished cases: {done}")
        pytest.fail(_dead[0])
    if run.returncode != 0 or "CHILD-DONE" not in run.stdout:
        msg = (f"child {name} failed (exit {run.returncode}):\n"
               f"{run.stdout[-2000:]}\n{run.stderr[-6000:]}")
        if run.returncode < 0:  # died on a signal: start nothing more
            _dead.append(msg)
        pytest.fail(msg)
    res = {}
    for line in run.stdout.splitlines():
        if line.startswith("CASE "):
            r = json.loads(line[5:])
            res[r["name"]] = r
    for block in run.stderr.split("CASE-BEGIN ")[1:]:
        res[block.split("\n", 1)[0].strip()]["stderr"] = block
    _results[name] = res
    return res


_STATS = re.compile(r"reducing receives: (\d+) launches for (\d+) receives "
                    r"in (\d+) entries, (\d+) runs taken as one entry")
_TRACE = re.compile(r"reduce pull batch n=(\d+) entries=(\d+) tiles=(\d+) "
                    r"total=(\d+) B")


def _counters(block):
    m = _STATS.search(block)
    assert m is not None, block[-3000:]
    return dict(zip(("launches", "receives", "entries", "runs"),
                    map(int, m.groups())))


@pytest.mark.parametrize("mode", ["word", "tail", "event"])
def test_loopback_under_each_completion_mode(mode):
    res = _child(mode)["loopback"]
    c = _counters(res["stderr"])
    # every message went through the reduce kernel, none through a copy
    assert c["receives"] == res["messages"] == 27
    assert "via memcpyAsync" not in res["stderr"]
    # the word paths say so at finalize; the event path has no words
    by_word = f"MPIX_PULL_DONE={mode}: completion word" in res["stderr"]
    assert by_word == (mode != "event"), res["stderr"][-2000:]


@pytest.mark.parametrize("case", [c for c in FEATURES if c != "partitions"])
def test_feature(case):
    res = _child("features")[case]
    if case in ("strided_sender", "kind_mismatch"):
        assert "fails with MPI_ERR_TYPE" in res["stderr"]
    if case == "same_buffer":
        # overlapping destinations never share a launch
        c = _counters(res["stderr"])
        assert c["receives"] == 3 and c["launches"] == 3
    if case == "misaligned":
        assert "via memcpyAsync" not in res["stderr"]


def test_partitions_as_runs_and_one_by_one():
    on = _child("features")["partitions"]
    off = _child("noruns")["partitions"]
    con, coff = _counters(on["stderr"]), _counters(off["stderr"])
    total = PARTS * ITERS
    assert con["receives"] == total and coff["receives"] == total
    assert coff["runs"] == 0
    # one wave stores the 16 flags with one instruction and the receives
    # were posted before: over two iterations the proxy sees adjacent flags
    # in one pass, and that run goes out as ONE reduce entry
    assert con["runs"] >= 1
    lines = [tuple(map(int, m)) for m in _TRACE.findall(on["stderr"])]
    assert sum(n for n, _, _, _ in lines) < total
    assert sum(b for _, _, _, b in lines) == total * PART_BYTES
    assert any(n == 1 and e == 1 and b > PART_BYTES for n, e, _, b in lines)
    # one by one, every partition is a receive of its own in the trace
    lines = [tuple(map(int, m)) for m in _TRACE.findall(off["stderr"])]
    assert sum(n for n, _, _, _ in lines) == total
    print(f"runs on: {con}; runs off: {coff}")


def _ring_rank(rank, size):
    sys.path.insert(0, os.path.join(REPO, "examples"))
    import torch
    import mpix
    from ring_allreduce import ring_allreduce
    mpix.init()
    try:
        stream = torch.cuda.current_stream()
        for dtype, n in ((torch.bfloat16, 2 * (T + 16)),
                         (torch.float32, 2 * 5001)):
            mine = (torch.arange(n) % 61 + 3 * rank).to(dtype)
            want = sum((torch.arange(n) % 61 + 3 * r).to(dtype)
                       for r in range(size))
            x = mine.cuda()
            ring_allreduce(x, rank, size, stream)
            torch.cuda.synchronize()
            assert same_bits(torch, x.cpu(), want), (rank, dtype)
    finally:
        mpix.finalize()


def test_ring_allreduce_two_processes_one_gpu():
    run_ranks(2, _ring_rank)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child_main(sys.argv[2])
