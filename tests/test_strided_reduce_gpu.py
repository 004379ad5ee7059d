"""Strided reducing receives between device buffers, through the library and
the Python API: irecv_reduce_strided_enqueue / precv_reduce_strided_init
combine the message into a view inside the receiver's pull kernel
(k_pull_strided_reduce, k_pull_strided_reduce_done in
src/transport/pull_kernels.h).  Every result is compared bit for bit with
torch on the CPU (IEEE float32 add, bf16 as the rounded float32 sum), and the
comparison covers the WHOLE underlying buffer, so a byte written between the
runs is seen.

The cases run in fresh child processes (the MPIX_* switches are read once per
process), each under a time limit, chained so that nothing is started after a
child that died on a signal, timed out or reported a GPU fault:

  word / tail / event   MPIX_PULL_DONE: face accumulate.  float32 grid(8, 6,
                        64): [:, 1, :] is the vector path, [:, :, 1] the
                        element path; bfloat16 m(6, 64): [:, 8:24] the vector
                        path, [:, 3:10] the element path; each from a
                        contiguous, an identically strided and a differently
                        strided sender
  div64                 the same with MPIX_STRIDED_DIV64=1
  features              capture and two replays; the graph-construction
                        call launched twice; a zero-byte message; receives
                        into overlapping views; kernel-published partitions
                        into a view that folds, one that needs the partition
                        level and a gapped contiguous one; receives started
                        after the run arrived (it expands); truncation and
                        the MPI_ERR_TYPE statuses
  noruns                the three partitioned shapes with MPIX_PART_RUNS=0
"""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 180  # s; a child takes a few seconds
PARTS, ITERS = 8, 2

FACES = ["faces"]
PART_CASES = ["parts_folded", "parts_level", "parts_gapped"]
FEATURES = (["capture", "graph", "zero_bytes", "overlap"] + PART_CASES +
            ["late_parts", "errors"])
CHILDREN = {
    "word": ({"MPIX_PULL_DONE": "word"}, FACES),
    "tail": ({"MPIX_PULL_DONE": "tail"}, FACES),
    "event": ({"MPIX_PULL_DONE": "event"}, FACES),
    "div64": ({"MPIX_STRIDED_DIV64": "1"}, FACES),
    "features": ({}, FEATURES),
    "noruns": ({"MPIX_PART_RUNS": "0"}, PART_CASES),
}
ENV_KEYS = ("MPIX_PULL_DONE", "MPIX_PART_RUNS", "MPIX_STRIDED_DIV64",
            "MPIX_PULL_BLOCKS", "MPIX_DEV_PUSH_MAX", "MPIX_FAST_WAIT")


# ------------------------------------------------------------------ child

def values(torch, dtype, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 3).to(dtype)


def combine(torch, a, b, op):
    if op == "sum":
        return a + b
    return torch.maximum(a, b) if op == "max" else torch.minimum(a, b)


def same_bits(torch, x, y):
    assert x.dtype == y.dtype and x.shape == y.shape
    return bool(torch.equal(x.contiguous().view(torch.uint8),
                            y.contiguous().view(torch.uint8)))


# (name, dtype, base shape, the view, is it the vector path?)
def face_views(torch):
    return [
        ("y-face", torch.float32, (8, 6, 64), lambda g: g[:, 1, :], True),
        ("x-face", torch.float32, (8, 6, 64), lambda g: g[:, :, 1], False),
        ("block 8:24", torch.bfloat16, (6, 64), lambda m: m[:, 8:24], True),
        ("block 3:10", torch.bfloat16, (6, 64), lambda m: m[:, 3:10], False),
    ]


def senders(torch, msg, base_shape, cut):
    """The message from a contiguous tensor, from the same view of another
    buffer, and from a view with another pitch whose rows start 8 elements
    in (16-byte aligned for both dtypes)."""
    rows = msg.shape[0]
    cols = msg.numel() // rows
    same = torch.zeros(base_shape, dtype=msg.dtype)
    cut(same).copy_(msg)
    other = torch.zeros(rows, cols + 16, dtype=msg.dtype)
    other[:, 8:8 + cols].copy_(msg.reshape(rows, cols))
    same, other = same.cuda(), other.cuda()
    return [("contiguous", msg.contiguous().cuda()),
            ("identically strided", cut(same)),
            ("differently strided", other[:, 8:8 + cols])]


def case_faces(mpix, torch):
    stream = torch.cuda.current_stream()
    tag, vec = 0, 0
    ops = ("sum", "max", "min")
    for name, dtype, shape, cut, is_vec in face_views(torch):
        base0 = values(torch, dtype, shape, 100 + tag)
        msg = values(torch, dtype, tuple(cut(base0).shape), 200 + tag)
        for kind, what in senders(torch, msg, shape, cut):
            tag += 1
            op = ops[tag % 3]
            base = base0.cuda()
            want = base0.clone()
            cut(want).copy_(combine(torch, cut(base0), msg, op))
            torch.cuda.synchronize()
            if tag % 2:  # posted first / the message arrives unexpected
                rr = mpix.irecv_reduce_strided_enqueue(
                    cut(base), source=0, op=op, tag=tag, stream=stream)
                rs = mpix.isend_enqueue(what, dest=0, tag=tag, stream=stream)
            else:
                rs = mpix.isend_enqueue(what, dest=0, tag=tag, stream=stream)
                rr = mpix.irecv_reduce_strided_enqueue(
                    cut(base), source=0, op=op, tag=tag, stream=stream)
            if tag % 3 == 0:  # the host wait and its status
                st = mpix.wait(rr)
                mpix.wait(rs)
                assert st["error"] == 0
                assert st["count_bytes"] == msg.numel() * msg.element_size()
            else:
                mpix.waitall_enqueue([rs, rr], stream=stream)
            torch.cuda.synchronize()
            assert same_bits(torch, base.cpu(), want), (name, kind, op)
            vec += is_vec
    return {"messages": tag, "vec": vec}


def case_capture(mpix, torch):
    """Captured once, launched twice: the view accumulates twice."""
    base0 = values(torch, torch.float32, (8, 6, 64), 1)
    b = values(torch, torch.float32, (8, 64), 2)
    base, msg = base0.cuda(), b.cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        mpix.stream_begin_capture(s.cuda_stream)
        rs = mpix.isend_enqueue(msg, dest=0, tag=3, stream=s)
        rr = mpix.irecv_reduce_strided_enqueue(base[:, 1, :], source=0, tag=3,
                                               stream=s)
        mpix.waitall_enqueue([rs, rr], stream=s)
        graph, gexec = mpix.stream_end_capture(s.cuda_stream)
    want = base0.clone()
    for it in range(2):
        mpix.graph_launch(gexec, s.cuda_stream)
        torch.cuda.synchronize()
        want[:, 1, :] = want[:, 1, :] + b
        assert same_bits(torch, base.cpu(), want), f"replay {it}"
    mpix.graph_exec_destroy(gexec)
    mpix.graph_destroy(graph)
    return {}


def case_graph(mpix, torch):
    """irecv_reduce_strided_graph: the library's single-node graphs chained
    recv -> send -> wait, instantiated once, launched twice: the view
    accumulates twice."""
    base0 = values(torch, torch.bfloat16, (6, 64), 3)
    b = values(torch, torch.bfloat16, (6, 16), 4)
    base, msg = base0.cuda(), b.cuda()
    torch.cuda.synchronize()
    rr, g_recv = mpix.irecv_reduce_strided_graph(base[:, 8:24], source=0,
                                                 op="sum", tag=5)
    rs, g_send = mpix.isend_graph(msg, dest=0, tag=5)
    g_wait = mpix.waitall_graph([rr, rs])
    parent, gexec = mpix.graph_chain_instantiate([g_recv, g_send, g_wait])
    s = torch.cuda.Stream()
    want = base0.clone()
    for it in range(2):
        mpix.graph_launch(gexec, s.cuda_stream)
        torch.cuda.synchronize()
        want[:, 8:24] = want[:, 8:24] + b
        assert same_bits(torch, base.cpu(), want), f"launch {it}"
    mpix.graph_exec_destroy(gexec)
    mpix.graph_destroy(parent)
    for g in (g_recv, g_send, g_wait):
        mpix.graph_destroy(g)
    return {}


def case_zero_bytes(mpix, torch):
    """A zero-byte message from a device pointer, posted and unexpected: the
    buffer stays bit-identical, the status says 0 bytes and no error."""
    stream = torch.cuda.current_stream()
    base0 = values(torch, torch.float32, (8, 6, 64), 6)
    base = base0.cuda()
    msg = torch.ones(8 * 64, device="cuda")
    torch.cuda.synchronize()
    empty = (msg.data_ptr(), 0)
    for tag, send_first in ((21, False), (22, True)):
        if send_first:
            rs = mpix.isend_enqueue(empty, dest=0, tag=tag, stream=stream)
            mpix.wait(rs)
        rr = mpix.irecv_reduce_strided_enqueue(base[:, 1, :], source=0,
                                               tag=tag, stream=stream)
        if not send_first:
            rs = mpix.isend_enqueue(empty, dest=0, tag=tag, stream=stream)
            mpix.wait(rs)
        st = mpix.wait(rr)
        torch.cuda.synchronize()
        assert st["error"] == 0 and st["count_bytes"] == 0, st
        assert same_bits(torch, base.cpu(), base0), tag
    # and the view still accumulates afterwards
    rr = mpix.irecv_reduce_strided_enqueue(base[:, 1, :], source=0, tag=24,
                                           stream=stream)
    rs = mpix.isend_enqueue(msg, dest=0, tag=24, stream=stream)
    mpix.waitall_enqueue([rs, rr], stream=stream)
    torch.cuda.synchronize()
    want = base0.clone()
    want[:, 1, :] += 1
    assert same_bits(torch, base.cpu(), want)
    return {}


def case_overlap(mpix, torch):
    """A y-face, an x-face and a contiguous slab of one grid, made ready
    together: the three share elements, the library serialises the launches.
    Integer-valued floats: the result is exact whatever the order."""
    stream = torch.cuda.current_stream()
    base0 = (torch.arange(8 * 6 * 64) % 1000).float().reshape(8, 6, 64)
    by = (torch.arange(8 * 64) % 77 + 1).float().reshape(8, 64)
    bx = (torch.arange(8 * 6) % 13 + 100).float().reshape(8, 6)
    bs = (torch.arange(6 * 64) % 5 + 7).float().reshape(6, 64)
    base = base0.cuda()
    my, mx, ms = by.cuda(), bx.cuda(), bs.cuda()
    torch.cuda.synchronize()
    r1 = mpix.irecv_reduce_strided_enqueue(base[:, 1, :], source=0, tag=11,
                                           stream=stream)
    r2 = mpix.irecv_reduce_strided_enqueue(base[:, :, 1], source=0, tag=12,
                                           stream=stream)
    r3 = mpix.irecv_reduce_enqueue(base[2], source=0, tag=13, stream=stream)
    s1 = mpix.isend_enqueue(my, dest=0, tag=11, stream=stream)
    s2 = mpix.isend_enqueue(mx, dest=0, tag=12, stream=stream)
    s3 = mpix.isend_enqueue(ms, dest=0, tag=13, stream=stream)
    mpix.waitall_enqueue([r1, r2, r3, s1, s2, s3], stream=stream)
    torch.cuda.synchronize()
    want = base0.clone()
    want[:, 1, :] += by
    want[:, :, 1] += bx
    want[2] += bs
    assert same_bits(torch, base.cpu(), want)
    return {}


def part_views(torch):
    """name -> (base shape, the view whose dimension 0 are the partitions)"""
    return {
        # 2 runs of 256 B per partition, the partitions at the pitch of the
        # runs: folds into one layout
        "parts_folded": ((2 * PARTS, 6, 64), lambda g: g[:, 1, :]),
        # the same runs, the partitions further apart: the partition level
        "parts_level": ((PARTS, 3, 6, 64), lambda g: g[:, :2, 1, :]),
        # contiguous partitions of 256 B, 320 B apart
        "parts_gapped": ((PARTS, 80), lambda m: m[:, :64]),
    }


def run_parts(mpix, torch, name, late=False):
    """PARTS partitions made ready by one device kernel into a view, ITERS
    iterations on the same requests: each accumulates on the one before.
    late: the receive is started after the run has arrived."""
    stream = torch.cuda.current_stream()
    shape, cut = part_views(torch)[name]
    base0 = values(torch, torch.float32, shape, 5)
    base = base0.cuda()
    n = cut(base0).numel()
    send = torch.zeros(n, dtype=torch.float32, device="cuda")
    word = torch.zeros(4, dtype=torch.int32, device="cuda")
    pr = mpix.precv_reduce_strided_init(cut(base), PARTS, source=0, op="sum",
                                        tag=7)
    ps = mpix.psend_init(send, PARTS, dest=0, tag=7)
    dps = mpix.prequest_create(ps)
    want = base0.clone()
    for it in range(ITERS):
        b = values(torch, torch.float32, (n,), 10 + it)
        send.copy_(b)
        torch.cuda.synchronize()
        if late:
            mpix.start(ps)
            mpix.launch_pready_all(dps, PARTS, stream.cuda_stream)
            # a message to ourselves queued behind the partitions: once it
            # has been received the run has arrived, with no receive posted
            rs = mpix.isend_enqueue(word, dest=0, tag=8, stream=stream)
            rr = mpix.irecv_enqueue(word, source=0, tag=8, stream=stream)
            mpix.waitall_enqueue([rs, rr], stream=stream)
            torch.cuda.synchronize()
            mpix.start(pr)
        else:
            mpix.start(pr)
            mpix.start(ps)
            mpix.launch_pready_all(dps, PARTS, stream.cuda_stream)
        st = mpix.wait(pr)
        mpix.wait(ps)
        torch.cuda.synchronize()
        assert st["error"] == 0, st
        cut(want).copy_(cut(want) + b.reshape(cut(want).shape))
        assert same_bits(torch, base.cpu(), want), (name, it)
    mpix.prequest_free(dps)
    mpix.request_free(ps)
    mpix.request_free(pr)
    return {}


def case_errors(mpix, torch):
    import numpy as np
    stream = torch.cuda.current_stream()
    C = mpix._C
    base0 = values(torch, torch.float32, (6, 40), 40)
    base = base0.cuda()
    view = base[:, 8:24]  # 6 runs of 64 B
    nbytes = 6 * 16 * 4
    torch.cuda.synchronize()

    def xfer(what, tag, recv=view, host_send=False):
        rr = mpix.irecv_reduce_strided_enqueue(recv, source=0, tag=tag,
                                               stream=stream)
        if host_send:
            rs = mpix.isend_enqueue(what, dest=0, tag=tag)
        else:
            rs = mpix.isend_enqueue(what, dest=0, tag=tag, stream=stream)
        st, st_s = mpix.wait(rr), mpix.wait(rs)
        torch.cuda.synchronize()
        assert st_s["error"] == 0, st_s  # the sender is acked and completes
        return st

    # a longer message: the elements that fit are combined
    longer = values(torch, torch.float32, (6 * 16 + 5,), 41)
    st = xfer(longer.cuda(), 51)
    assert st["error"] == C.ERR_TRUNCATE and st["count_bytes"] == nbytes, st
    want = base0.clone()
    want[:, 8:24] += longer[:96].reshape(6, 16)
    assert same_bits(torch, base.cpu(), want)
    # MPI_ERR_TYPE, the buffer untouched: a length that is no multiple of
    # the element; a sender whose runs are not (6-byte runs of bytes); a
    # sender whose address is not; host memory on the sending side
    raw = torch.zeros(64, 8, dtype=torch.uint8, device="cuda")
    for tag, what, host in ((52, raw.reshape(-1)[:nbytes - 2], False),
                            (53, raw[:, :6], False),
                            (54, raw.reshape(-1)[2:2 + nbytes], False),
                            (55, np.ones(96, np.float32), True)):
        st = xfer(what, tag, host_send=host)
        assert st["error"] == C.ERR_TYPE and st["count_bytes"] == 0, (tag, st)
        assert same_bits(torch, base.cpu(), want), tag
    # a device message into a host view
    host0 = base0.numpy().copy()
    host = host0.copy()
    st = xfer(torch.ones(96, device="cuda"), 56, recv=host[:, 8:24])
    assert st["error"] == C.ERR_TYPE, st
    assert host.tobytes() == host0.tobytes()
    # the pair still works
    ones = torch.ones(96, device="cuda")
    st = xfer(ones, 58)
    want[:, 8:24] += 1
    assert st["error"] == 0 and same_bits(torch, base.cpu(), want)
    return {}


def child_main(name):
    sys.path.insert(0, REPO)
    import torch
    import mpix

    run = {"faces": case_faces, "capture": case_capture,
           "graph": case_graph, "zero_bytes": case_zero_bytes,
           "overlap": case_overlap, "errors": case_errors,
           "late_parts": lambda m, t: run_parts(m, t, "parts_level", True)}
    for p in PART_CASES:
        run[p] = lambda m, t, p=p: run_parts(m, t, p)
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

GPU_FAULTS = ("illegal memory access", "Memory access fault",
              "unspecified launch failure", "HSA_STATUS_ERROR")
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
        # died on a signal, or HIP reported a fault: start nothing more
        if run.returncode < 0 or any(f in run.stderr for f in GPU_FAULTS):
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


_STATS = re.compile(r"strided reducing receives: (\d+) launches for (\d+) "
                    r"receives in (\d+) entries, (\d+) runs taken as one "
                    r"entry")
_PLAIN = re.compile(r"\] reducing receives: (\d+) launches for (\d+) "
                    r"receives")
_TRACE = re.compile(r"strided reduce pull batch n=(\d+) entries=(\d+) "
                    r"vec=(\d+) tiles=(\d+) total=(\d+) B wide=(\d)")


def _counters(block, must=True):
    m = _STATS.search(block)
    assert m is not None or not must, block[-3000:]
    return dict(zip(("launches", "receives", "entries", "runs"),
                    map(int, m.groups()) if m else (0, 0, 0, 0)))


def _plain_receives(block):
    """receives that went through the contiguous reduce kernel"""
    m = _PLAIN.search(block)
    return int(m.group(2)) if m else 0


def _trace(block):
    return [tuple(map(int, m)) for m in _TRACE.findall(block)]


@pytest.mark.parametrize("mode", ["word", "tail", "event", "div64"])
def test_faces_under_each_completion_and_division_mode(mode):
    res = _child(mode)["faces"]
    c = _counters(res["stderr"])
    # every message went through the strided reduce kernel, none through the
    # contiguous one, a plain strided pull or a copy
    assert c["receives"] == res["messages"] == 12
    assert c["entries"] == 12 and c["runs"] == 0
    assert 1 <= c["launches"] <= 12
    assert _PLAIN.search(res["stderr"]) is None
    assert "via memcpyAsync" not in res["stderr"]
    assert "] strided pull batch" not in res["stderr"]
    lines = _trace(res["stderr"])
    assert len(lines) == c["launches"]
    assert sum(n for n, *_ in lines) == 12
    # the views meant for the vector path took it
    assert sum(v for _, _, v, *_ in lines) == res["vec"] == 6
    assert all(w == (mode == "div64") for *_, w in lines)
    # the word paths say so at finalize; the event path has no words
    done = {"div64": "word"}.get(mode, mode)
    by_word = f"MPIX_PULL_DONE={done}: completion word" in res["stderr"]
    assert by_word == (done != "event"), res["stderr"][-2000:]


@pytest.mark.parametrize("case", ["capture", "graph", "zero_bytes",
                                  "overlap", "late_parts", "errors"])
def test_feature(case):
    res = _child("features")[case]
    if case in ("capture", "graph"):
        c = _counters(res["stderr"])
        assert c["receives"] == 2 and c["launches"] == 2
    if case == "zero_bytes":
        # only the last message moved data
        c = _counters(res["stderr"])
        assert c["receives"] == 1 and c["launches"] == 1
        assert "fails with MPI_ERR_TYPE" not in res["stderr"]
    if case == "overlap":
        # overlapping extents never share a launch, and the contiguous slab
        # went through the contiguous reduce kernel on the same stream
        c = _counters(res["stderr"])
        assert c["receives"] == 2 and c["launches"] == 2
        m = _PLAIN.search(res["stderr"])
        assert m is not None and m.group(2) == "1"
    if case == "late_parts":
        # the run arrived before its receives: it expands, and every
        # partition is a strided reduce entry of its own
        c = _counters(res["stderr"])
        assert c["runs"] == 0
        assert c["receives"] == c["entries"] == PARTS * ITERS
    if case == "errors":
        assert res["stderr"].count("fails with MPI_ERR_TYPE") >= 5
        assert "via memcpyAsync" not in res["stderr"]


@pytest.mark.parametrize("case", PART_CASES)
def test_partitions_as_runs_and_one_by_one(case):
    on = _child("features")[case]
    off = _child("noruns")[case]
    # a gapped contiguous partition on its own is contiguous on both sides,
    # an entry of the contiguous reduce kernel; only as a run is it strided
    gapped = case == "parts_gapped"
    con = _counters(on["stderr"])
    coff = _counters(off["stderr"], must=not gapped)
    pon, poff = _plain_receives(on["stderr"]), _plain_receives(off["stderr"])
    total = PARTS * ITERS
    assert con["receives"] + pon == total
    assert coff["receives"] + poff == total
    assert coff["runs"] == 0 and coff["entries"] == coff["receives"]
    if gapped:
        assert poff == total
    else:
        assert pon == 0 and poff == 0
    # one wave stores the 8 flags with one instruction and the receives were
    # posted before: over two iterations the proxy sees adjacent flags in one
    # pass, and that run goes out as ONE strided reduce entry
    assert con["runs"] >= 1 and con["entries"] < con["receives"]
    for block in (on["stderr"], off["stderr"]):
        assert "via memcpyAsync" not in block
        assert "] strided pull batch" not in block
    if not gapped:
        lines = _trace(on["stderr"])
        assert sum(b for *_, b, _ in lines) == total * 512
    print(f"{case}: runs on: {con} + {pon} contiguous; runs off: {coff} + "
          f"{poff} contiguous")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child_main(sys.argv[2])
