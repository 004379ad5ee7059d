"""The trigger/wait protocol of src/enqueue.cpp on the stream path, in all four
of its forms: MPIX_FAST_WAIT on or off, crossed with hipStream*Value32 memOps
or the hand-written flag kernels (MPIX_DISABLE_MEMOPS=1, which is also where
init.cpp goes on its own when its memOps probe fails).  The kernel fallback of
a classic waitall has two variants of its own: one k_wait_and_set launch per
request, or one k_waitall_and_set launch whose lanes poll all the flags
(MPIX_WAITALL_KERNEL; by default from 4 requests on).

Loopback on device buffers, in the shape of tests/test_pull_done_modes_gpu.py:
every mode is a fresh child process (this file, started with --child NAME)
with MPIX_STATS=1 and a time limit; the children are chained, so that after a
child that died on a signal or ran into its limit no further process is
started and the remaining tests fail at once.  A child that reports a wrong
result does not stop the chain.  Every case has an init/finalize of its own:
the counters printed at finalize ("triggers:" and "stream waits:") are per
case, and every test asserts on them, because they are the only proof that a
case ran the path it names and not an easier one.

A child uses ONE stream for everything and both triggers of a message are
always enqueued before any wait for it: a spin-wait kernel in front of the
trigger it needs would hang by construction.  Payloads are position-dependent
and compared with the CPU copy of what was sent; every destination sits
between sentinel elements that must survive.

Cases:
  a_roundtrips  8 B, 4100 B from a source misaligned by 4 B (the
                hipMemcpyAsync pull) and 1 MiB, each waited with wait_enqueue
                and a status, behind a gate
  b_<n>         gated waitall: torch.cuda._sleep on the stream, the triggers
                of n/2 sends and n/2 receives of 64 B, one waitall_enqueue
                over all n.  n = 2 (below the wave threshold), 4 (at it), 64
                (one full wave), 66 (two waves), 1100 (more flags than the
                1024 lanes: 76 lanes own two).  No request may be complete
                when the waitall is enqueued; the test does not trust the
                gate for that, it asserts 0 "consumed at enqueue"
  c_complete    wait_enqueue long after completion: consumed at enqueue, no
                stream work, the status is right
  d_mixed       one waitall over 16 complete and 16 gated requests
  e_consumer    20 iterations without host synchronisation: fill, enqueue,
                wait, and a kernel on the same stream copies what arrived.
                What the wait's acquire (kernel or memOp) lets through must
                be visible to the next kernel in the stream
  f_capture     the sequence of test_gpu.py::test_graph_capture_loopback:
                requests made under capture are classic in every child.  The
                fast children also pass a fast request to wait_enqueue inside
                the capture and to wait_graph: both raise and leave the
                request to a host wait
  g_partitioned the body of test_gpu.py::test_partitioned_device_kernels
  h_recycle     (a second run of each child, MPIX_NFLAGS=64) 200 rounds of 16
                pairs: 100 times as many operations as the pool has slots.
                In the classic children every slot comes back through the
                proxy's CLEANUP leg

GATE_US_PER_REQUEST and CHILD_TIMEOUT are taken from the measurements in
profiles/wait_modes.md.
"""
import json
import os
import re
import subprocess
import sys
import time
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5
PAD = 64  # sentinel bytes on either side of a destination

# The gate in front of the triggers of n requests lasts
# max(GATE_FLOOR_MS, n * GATE_US_PER_REQUEST / 1000) ms.  Measured on the
# MI355X (profiles/wait_modes.md): the slowest child spends 13.0 ms of host
# time in the enqueue loop of 1100 requests and their waitall, 11.8 us per
# request; the gate is 17 times that, 220 ms for the 1100.
GATE_US_PER_REQUEST = 200
GATE_FLOOR_MS = 20
# s; guards against a hang and is no performance figure.  The slowest child
# takes 3.8 s (profiles/wait_modes.md); this is 26 times that
CHILD_TIMEOUT = 100

BN = [2, 4, 64, 66, 1100]
WAVE_THREADS = {2: 64, 4: 64, 64: 64, 66: 128, 1100: 1024}
CASES = (["a_roundtrips"] + [f"b_{n}" for n in BN] +
         ["c_complete", "d_mixed", "e_consumer", "f_capture", "g_partitioned"])
RECYCLE_ROUNDS, RECYCLE_PAIRS = 200, 16
RECYCLE_GATED = 5  # odd: gated rounds alternate between the two wait calls
CONSUMER_ITERS = 20

# in this order: the memOps children first, the wave kernel last
CHILDREN = {
    "fast_memops": {},
    "classic_memops": {"MPIX_FAST_WAIT": "0"},
    "fast_kernels": {"MPIX_DISABLE_MEMOPS": "1"},
    "classic_kernels_each": {"MPIX_FAST_WAIT": "0", "MPIX_DISABLE_MEMOPS": "1",
                             "MPIX_WAITALL_KERNEL": "0"},
    "classic_kernels": {"MPIX_FAST_WAIT": "0", "MPIX_DISABLE_MEMOPS": "1"},
    "classic_kernels_wave": {"MPIX_FAST_WAIT": "0", "MPIX_DISABLE_MEMOPS": "1",
                             "MPIX_WAITALL_KERNEL": "1"},
}
ENV_KEYS = ("MPIX_FAST_WAIT", "MPIX_DISABLE_MEMOPS", "MPIX_WAITALL_KERNEL",
            "MPIX_DISABLE_GRAPH_MEMOPS", "MPIX_NFLAGS", "MPIX_SETTLE",
            "MPIX_TRACE", "MPIX_PULL_DONE", "MPIX_PULL_BLOCKS",
            "MPIX_PULL_NT", "MPIX_PULL_UNROLL", "MPIX_WATCHDOG",
            "MPIX_FORCE_NO_GPU", "MPIX_COPY_PRIO_STREAM")


def pattern(n, start):
    """Byte i of a message: ((start + i) * 7 + 3) % 251, computed on the CPU"""
    i = np.arange(start, start + n, dtype=np.int64)
    return ((i * 7 + 3) % 251).astype(np.uint8)


# ------------------------------------------------------------------ child

class Ctx:
    def __init__(self, name, torch, mpix, stream):
        self.name, self.torch, self.mpix, self.s = name, torch, mpix, stream
        self.cycles_per_ms = None

    def gate(self, n_requests):
        """A kernel that keeps the stream busy while the triggers and waits
        of n_requests requests are enqueued behind it.  Returns its ms."""
        ms = max(GATE_FLOOR_MS, n_requests * GATE_US_PER_REQUEST / 1000.0)
        self.torch.cuda._sleep(int(ms * self.cycles_per_ms))
        return ms

    def calibrate(self):
        """Ticks of torch.cuda._sleep per ms, from two timed sleeps"""
        torch = self.torch
        cycles, rate = 1_000_000, None
        for _ in range(2):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            torch.cuda.synchronize()
            rate = cycles / e0.elapsed_time(e1)
            cycles = int(rate * 20)
        self.cycles_per_ms = rate

    def message(self, n, start, src_off=0):
        """(source on the device, padded destination, its payload slice,
        the CPU copy of the payload)"""
        torch = self.torch
        want = pattern(n, start)
        backing = torch.zeros(n + src_off, dtype=torch.uint8, device="cuda")
        src = backing[src_off:]
        src.copy_(torch.from_numpy(want))
        full = torch.full((n + 2 * PAD,), SENT, dtype=torch.uint8,
                          device="cuda")
        return src, full, full[PAD:PAD + n], want

    @staticmethod
    def check(full, want, what):
        got = full.cpu().numpy()
        n = len(want)
        assert (got[PAD:PAD + n] == want).all(), f"payload, {what}"
        assert (got[:PAD] == SENT).all(), f"bytes before, {what}"
        assert (got[PAD + n:] == SENT).all(), f"bytes after, {what}"


def check_status(st, tag, nbytes, what):
    d = st.as_dict()
    assert (d["source"], d["tag"], d["count_bytes"], d["error"]) == \
        (0, tag, nbytes, 0), f"status of {what}: {d}"


def case_roundtrips(c):
    mpix, torch, s = c.mpix, c.torch, c.s
    for i, (n, off) in enumerate([(8, 0), (4100, 4), (1 << 20, 0)]):
        src, full, dst, want = c.message(n, 31 * i + n, src_off=off)
        if off:
            assert src.data_ptr() % 16 == off
        torch.cuda.synchronize()
        c.gate(2)
        rs = mpix.isend_enqueue(src, dest=0, tag=10 + i, stream=s)
        rr = mpix.irecv_enqueue(dst, source=0, tag=10 + i, stream=s)
        st_s, st_r = mpix.Status(), mpix.Status()
        mpix.wait_enqueue(rs, stream=s, status=st_s)
        mpix.wait_enqueue(rr, stream=s, status=st_r)
        torch.cuda.synchronize()
        c.check(full, want, f"{n} B")
        check_status(st_r, 10 + i, n, f"the receive of {n} B")
        assert st_s.as_dict()["error"] == 0
    return {}


class Pairs:
    """`pairs` loopback messages of 64 B with contents and tags of their own"""
    NB = 64

    def __init__(self, c, pairs, start, tag0):
        torch = c.torch
        self.c, self.pairs, self.tag0 = c, pairs, tag0
        self.want = pattern(pairs * self.NB, start).reshape(pairs, self.NB)
        self.src = torch.from_numpy(self.want).cuda()
        self.full = torch.full((pairs, self.NB + 2 * PAD), SENT,
                               dtype=torch.uint8, device="cuda")

    def enqueue(self):
        mpix, s = self.c.mpix, self.c.s
        reqs = []
        for k in range(self.pairs):
            reqs.append(mpix.isend_enqueue(self.src[k], dest=0,
                                           tag=self.tag0 + k, stream=s))
            reqs.append(mpix.irecv_enqueue(self.full[k, PAD:PAD + self.NB],
                                           source=0, tag=self.tag0 + k,
                                           stream=s))
        return reqs

    def check(self, what):
        got = self.full.cpu().numpy()
        assert (got[:, PAD:PAD + self.NB] == self.want).all(), \
            f"payload, {what}"
        assert (got[:, :PAD] == SENT).all(), f"bytes before, {what}"
        assert (got[:, PAD + self.NB:] == SENT).all(), f"bytes after, {what}"


def case_gated_waitall(c, n):
    mpix, torch, s = c.mpix, c.torch, c.s
    p = Pairs(c, n // 2, 1000 + n, 0)
    torch.cuda.synchronize()
    gate_ms = c.gate(n)
    t0 = time.perf_counter()
    reqs = p.enqueue()
    mpix.waitall_enqueue(reqs, stream=s)
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    p.check(f"waitall over {n}")
    return {"gate_ms": gate_ms, "enqueue_ms": round(host_ms, 3)}


def case_complete(c):
    mpix, torch, s = c.mpix, c.torch, c.s
    src, full, dst, want = c.message(4096, 77)
    rs = mpix.isend_enqueue(src, dest=0, tag=21, stream=s)
    rr = mpix.irecv_enqueue(dst, source=0, tag=21, stream=s)
    torch.cuda.synchronize()
    time.sleep(0.05)  # let the proxy complete both
    st_s, st_r = mpix.Status(), mpix.Status()
    mpix.wait_enqueue(rr, stream=s, status=st_r)
    mpix.wait_enqueue(rs, stream=s, status=st_s)
    # consumed at enqueue: the status is there without any stream work
    check_status(st_r, 21, 4096, "the late receive")
    torch.cuda.synchronize()
    c.check(full, want, "late wait")
    return {}


def case_mixed(c):
    mpix, torch, s = c.mpix, c.torch, c.s
    done = Pairs(c, 8, 5000, 100)
    live = Pairs(c, 8, 9000, 200)
    reqs = done.enqueue()
    torch.cuda.synchronize()
    time.sleep(0.05)  # let the proxy complete these 16
    c.gate(16)
    reqs += live.enqueue()
    mpix.waitall_enqueue(reqs, stream=s)
    torch.cuda.synchronize()
    done.check("the complete half")
    live.check("the gated half")
    return {}


def case_consumer(c):
    mpix, torch, s = c.mpix, c.torch, c.s
    n, pad = 1024, 16
    send = torch.zeros(n, dtype=torch.int32, device="cuda")
    full = torch.full((n + 2 * pad,), -7, dtype=torch.int32, device="cuda")
    recv = full[pad:pad + n]
    result = torch.full((CONSUMER_ITERS, n), -1, dtype=torch.int32,
                        device="cuda")
    torch.cuda.synchronize()
    for it in range(CONSUMER_ITERS):
        send.fill_(it)
        rs = mpix.isend_enqueue(send, dest=0, tag=it, stream=s)
        rr = mpix.irecv_enqueue(recv, source=0, tag=it, stream=s)
        mpix.wait_enqueue(rs, stream=s)
        mpix.wait_enqueue(rr, stream=s)
        result[it].copy_(recv)
    torch.cuda.synchronize()
    got = result.cpu().numpy()
    want = np.repeat(np.arange(CONSUMER_ITERS, dtype=np.int32)[:, None], n, 1)
    bad = [it for it in range(CONSUMER_ITERS) if (got[it] != want[it]).any()]
    assert not bad, f"iterations whose consumer saw stale data: {bad}"
    edge = full.cpu().numpy()
    assert (edge[:pad] == -7).all() and (edge[pad + n:] == -7).all()
    return {}


def case_capture(c):
    mpix, torch, s = c.mpix, c.torch, c.s
    fast = c.name.startswith("fast")
    n, pad = 512, 16
    send = torch.zeros(n, dtype=torch.int32, device="cuda")
    full = torch.full((n + 2 * pad,), -7, dtype=torch.int32, device="cuda")
    recv = full[pad:pad + n]
    if fast:  # a pair made outside any capture: fast requests
        o_src = torch.arange(16, dtype=torch.int32, device="cuda")
        o_dst = torch.zeros(16, dtype=torch.int32, device="cuda")
        o_s = mpix.isend_enqueue(o_src, dest=0, tag=30, stream=s)
        o_r = mpix.irecv_enqueue(o_dst, source=0, tag=30, stream=s)
        torch.cuda.synchronize()
        # the capture below is in global mode, in which a HIP call of the
        # proxy thread (it is still moving this pair) can invalidate it
        time.sleep(0.05)
    torch.cuda.synchronize()
    raised = []
    mpix.stream_begin_capture(s.cuda_stream)
    try:
        rs = mpix.isend_enqueue(send, dest=0, tag=3, stream=s)
        rr = mpix.irecv_enqueue(recv, source=0, tag=3, stream=s)
        if fast:
            try:
                mpix.wait_enqueue(o_s, stream=s)
            except RuntimeError:
                raised.append("capture")
        mpix.waitall_enqueue([rs, rr], stream=s)
    finally:
        graph, gexec = mpix.stream_end_capture(s.cuda_stream)
    for it in range(3):
        send.fill_(it + 10)
        torch.cuda.synchronize()
        mpix.graph_launch(gexec, s.cuda_stream)
        torch.cuda.synchronize()
        assert bool((recv == it + 10).all()), f"replay {it}"
    mpix.graph_exec_destroy(gexec)
    mpix.graph_destroy(graph)
    edge = full.cpu().numpy()
    assert (edge[:pad] == -7).all() and (edge[pad + n:] == -7).all()
    if fast:
        try:
            mpix.wait_graph(o_r)
        except RuntimeError:
            raised.append("graph")
        assert raised == ["capture", "graph"], raised
        # after each error the request is still there for a host wait
        st = mpix.wait(o_r)
        mpix.wait(o_s)
        assert (st["source"], st["tag"], st["count_bytes"]) == (0, 30, 64)
        torch.cuda.synchronize()
        assert torch.equal(o_dst, o_src)
    return {}


def case_partitioned(c):
    mpix, torch, s = c.mpix, c.torch, c.s
    parts, per = 10, 1024
    send = torch.zeros(parts * per, dtype=torch.int32, device="cuda")
    recv = torch.zeros_like(send)
    errs = torch.zeros(1, dtype=torch.int32, device="cuda")
    ps = mpix.psend_init(send, parts, dest=0, tag=6)
    pr = mpix.precv_init(recv, parts, source=0, tag=6)
    dps = mpix.prequest_create(ps)
    dpr = mpix.prequest_create(pr)
    try:
        for it in range(3):
            mpix.start(pr)
            mpix.start(ps)
            base = 1000 * (it + 1)
            mpix.launch_fill_and_pready(send.data_ptr(), per, base, dps,
                                        parts, s.cuda_stream)
            mpix.launch_wait_and_check(recv.data_ptr(), per, base, dpr,
                                       parts, errs.data_ptr(), s.cuda_stream)
            torch.cuda.synchronize()
            mpix.wait(pr)
            mpix.wait(ps)
            assert errs.item() == 0, f"iter {it}: payload errors"
    finally:
        mpix.prequest_free(dps)
        mpix.prequest_free(dpr)
        mpix.request_free(ps)
        mpix.request_free(pr)
    return {}


def case_recycle(c):
    """Even rounds: one waitall; odd rounds: a wait_enqueue per request.
    Every RECYCLE_GATED-th round is behind a gate, so that its waits find
    nothing complete and go to the stream."""
    mpix, torch, s = c.mpix, c.torch, c.s
    assert mpix.config()["nflags"] == 64
    for rnd in range(RECYCLE_ROUNDS):
        p = Pairs(c, RECYCLE_PAIRS, 64 * rnd, 0)
        if rnd % RECYCLE_GATED == 0:
            torch.cuda.synchronize()
            c.gate(2 * RECYCLE_PAIRS)
        reqs = p.enqueue()
        if rnd % 2 == 0:
            mpix.waitall_enqueue(reqs, stream=s)
        else:
            for r in reqs:
                mpix.wait_enqueue(r, stream=s)
        torch.cuda.synchronize()
        p.check(f"round {rnd}")
    return {}


def child_main(name, recycle):
    sys.path.insert(0, REPO)
    import torch
    import mpix

    run = {"a_roundtrips": case_roundtrips, "c_complete": case_complete,
           "d_mixed": case_mixed, "e_consumer": case_consumer,
           "f_capture": case_capture, "g_partitioned": case_partitioned,
           "h_recycle": case_recycle}
    for n in BN:
        run[f"b_{n}"] = lambda c, n=n: case_gated_waitall(c, n)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = Ctx(name, torch, mpix, stream)
        c.calibrate()
        for case in (["h_recycle"] if recycle else CASES):
            sys.stderr.write(f"CASE-BEGIN {case}\n")
            sys.stderr.flush()
            t0 = time.perf_counter()
            mpix.init()
            cfg = mpix.config()
            res = {"use_memops": bool(cfg["use_memops"]),
                   "use_batch_memops": bool(cfg["use_batch_memops"])}
            try:
                res.update(run[case](c))
            except Exception:
                res["error"] = traceback.format_exc()
            finally:
                torch.cuda.synchronize()
                mpix.finalize()
            res["seconds"] = round(time.perf_counter() - t0, 3)
            print("CASE " + json.dumps({"name": case, **res}), flush=True)
    print("CHILD-DONE", flush=True)


# ----------------------------------------------------------------- parent

_results = {}
_dead = []

TRIG_KEYS = ("memop_stream", "kernel_stream", "memop_capture",
             "kernel_capture")
WAIT_KEYS = ("eq", "gte", "capture_eq", "k_flag", "k_gte", "k_and_set",
             "wave_launches", "wave_flags", "wave_max_flags",
             "wave_max_threads", "consumed")
_TRIG = re.compile(r"\[mpix stats r(\d+)\] triggers: stream memOp (\d+), "
                   r"stream k_set_flag (\d+), capture memOp (\d+), capture "
                   r"k_set_flag (\d+)")
_WAIT = re.compile(r"\[mpix stats r(\d+)\] stream waits: WaitValueEq\+CLEANUP "
                   r"(\d+), WaitValueGte (\d+), capture WaitValueEq (\d+), "
                   r"k_wait_flag \(capture\) (\d+), k_wait_flag_gte (\d+), "
                   r"k_wait_and_set (\d+), k_waitall_and_set (\d+) launches "
                   r"for (\d+) flags \(largest (\d+) flags on (\d+) "
                   r"threads\), consumed at enqueue (\d+)")
_OPS = re.compile(r"\[mpix stats r(\d+)\] ops issued=(\d+) completed=(\d+)")
LEAK = "still in use at MPIX_Finalize"


def counters(text):
    """{rank: (triggers, waits, (issued, completed))} of the stats lines"""
    out = {}
    for m in _TRIG.finditer(text):
        out.setdefault(int(m.group(1)), {})["trig"] = dict(
            zip(TRIG_KEYS, map(int, m.groups()[1:])))
    for m in _WAIT.finditer(text):
        out.setdefault(int(m.group(1)), {})["wait"] = dict(
            zip(WAIT_KEYS, map(int, m.groups()[1:])))
    for m in _OPS.finditer(text):
        out.setdefault(int(m.group(1)), {})["ops"] = (int(m.group(2)),
                                                      int(m.group(3)))
    return out


def _child(name, recycle=False):
    key = (name, recycle)
    if key in _results:
        return _results[key]
    if _dead:
        pytest.fail("not started: " + _dead[0])
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", MPIX_STATS="1")
    for k in ENV_KEYS:
        env.pop(k, None)
    env.update(CHILDREN[name])
    if recycle:
        env["MPIX_NFLAGS"] = "64"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name]
    t0 = time.perf_counter()
    try:
        run = subprocess.run(cmd + (["--recycle"] if recycle else []),
                             env=env, capture_output=True, text=True,
                             timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout
        err = e.stderr.decode() if isinstance(e.stderr, bytes) else e.stderr
        done = re.findall(r'^CASE {"name": "(\w+)"', out or "", re.M)
        _dead.append(f"child {key} ran into its limit of {CHILD_TIMEOUT} s "
                     f"(a wait that never returns?); finished cases: {done}; "
                     f"its stderr ends:\n{(err or '')[-3000:]}")
        pytest.fail(_dead[0])
    wall = time.perf_counter() - t0
    if run.returncode != 0 or "CHILD-DONE" not in run.stdout:
        why = (f"child {key} failed (exit {run.returncode}):\n"
               f"{run.stdout[-2000:]}\n{run.stderr[-4000:]}")
        # it died (a signal, or an error outside the cases, where a wrong
        # result is reported and the child goes on): start nothing after it
        _dead.append(why)
        pytest.fail(why)
    res = {}
    for line in run.stdout.splitlines():
        if line.startswith("CASE "):
            r = json.loads(line[5:])
            res[r["name"]] = r
    for block in run.stderr.split("CASE-BEGIN ")[1:]:
        res[block.split("\n", 1)[0].strip()]["stderr"] = block
    print(f"child {key}: {wall:.1f} s wall")
    _results[key] = res
    return res


SINGLE = {"fast_memops": "gte", "classic_memops": "eq",
          "fast_kernels": "k_gte", "classic_kernels_each": "k_and_set",
          "classic_kernels": "k_and_set", "classic_kernels_wave": "k_and_set"}


def _wave(child, count):
    """Does a waitall over `count` requests take k_waitall_and_set?"""
    return {"classic_kernels": count >= 4,
            "classic_kernels_wave": True}.get(child, False)


def _threads(flags):
    return min(1024, max(64, (flags + 63) // 64 * 64))


def want_waits(child, singles=0, waitalls=(), consumed=0):
    """The wait counters after `singles` wait_enqueue calls that found their
    request incomplete, and waitall_enqueue calls given as (requests, of
    which incomplete)"""
    w = dict.fromkeys(WAIT_KEYS, 0)
    w["consumed"] = consumed
    w[SINGLE[child]] += singles
    for count, live in waitalls:
        if _wave(child, count) and live:
            w["wave_launches"] += 1
            w["wave_flags"] += live
            if live > w["wave_max_flags"]:
                w["wave_max_flags"] = live
                w["wave_max_threads"] = _threads(live)
        else:
            w[SINGLE[child]] += live
    return w


def want_trig(child, stream=0, capture=0):
    t = dict.fromkeys(TRIG_KEYS, 0)
    kind = "memop" if child.endswith("_memops") else "kernel"
    t[kind + "_stream"] = stream
    t[kind + "_capture"] = capture
    return t


def _case(child, case, recycle=False):
    """The case's result, after the checks every case gets"""
    if child.endswith("_memops"):
        # the default process decides whether this machine has memOps
        first = _child("fast_memops")["a_roundtrips"]
        if not first["use_memops"]:
            pytest.skip("hipStream memOps are unavailable in the default "
                        "process on this machine (the probe of init.cpp "
                        "failed): there is no memOps path to test")
    r = _child(child, recycle)[case]
    cnt = counters(r["stderr"]).get(0, {})
    print(f"{child} {case}: {r.get('seconds')} s, batched memOps "
          f"{r['use_batch_memops']}, "
          f"{ {k: v for k, v in r.items() if k.endswith('_ms')} }\n"
          f"  triggers {cnt.get('trig')}\n  waits {cnt.get('wait')}\n"
          f"  ops {cnt.get('ops')}")
    assert "error" not in r, r["error"]
    assert r["use_memops"] == child.endswith("_memops")
    assert LEAK not in r["stderr"], r["stderr"][-2000:]
    assert {"trig", "wait", "ops"} <= set(cnt), r["stderr"][-2000:]
    assert cnt["ops"][0] == cnt["ops"][1], cnt["ops"]
    return r, cnt


def _ids(recycle):
    return [(ch, "h_recycle" if recycle else ca) for ch in CHILDREN
            for ca in (["h_recycle"] if recycle else CASES)]


@pytest.mark.parametrize("child,case", _ids(False),
                         ids=[f"{a}-{b}" for a, b in _ids(False)])
def test_wait_mode(child, case):
    r, cnt = _case(child, case)
    trig, wait = cnt["trig"], cnt["wait"]
    if case == "a_roundtrips":
        assert trig == want_trig(child, stream=6)
        assert wait == want_waits(child, singles=6)
    elif case.startswith("b_"):
        n = int(case[2:])
        assert trig == want_trig(child, stream=n)
        assert wait["consumed"] == 0, \
            "a request was complete when the waitall was enqueued"
        assert wait == want_waits(child, waitalls=[(n, n)])
        if _wave(child, n):
            assert (wait["wave_launches"], wait["wave_max_flags"],
                    wait["wave_max_threads"]) == (1, n, WAVE_THREADS[n])
        else:
            assert wait[SINGLE[child]] == n
    elif case == "c_complete":
        assert trig == want_trig(child, stream=2)
        assert wait == want_waits(child, consumed=2)
    elif case == "d_mixed":
        assert trig == want_trig(child, stream=32)
        assert wait == want_waits(child, waitalls=[(32, 16)], consumed=16)
    elif case == "e_consumer":
        # no gate: a request may be complete before its wait is enqueued
        n = 2 * CONSUMER_ITERS
        assert trig == want_trig(child, stream=n)
        took = wait["consumed"]
        assert wait == want_waits(child, singles=n - took, consumed=took)
    elif case == "f_capture":
        outside = 2 if child.startswith("fast") else 0
        with_kernels = (want_trig(child, stream=outside),
                        dict(want_waits(child), k_flag=2))
        with_kernels[0]["kernel_capture"] = 2
        with_memops = (want_trig(child, stream=outside, capture=2),
                       dict(want_waits(child), capture_eq=2))
        if child.endswith("_memops"):
            # captures take memOps where they replay, kernels where not
            assert (trig, wait) in (with_kernels, with_memops)
        else:
            assert (trig, wait) == with_kernels
    elif case == "g_partitioned":
        assert trig == want_trig(child)
        assert wait == want_waits(child)
    else:
        raise AssertionError(case)


@pytest.mark.parametrize("child,case", _ids(True),
                         ids=[a for a, _ in _ids(True)])
def test_slot_recycling(child, case):
    r, cnt = _case(child, case, recycle=True)
    trig, wait = cnt["trig"], cnt["wait"]
    n = RECYCLE_ROUNDS * 2 * RECYCLE_PAIRS
    assert cnt["ops"] == (n, n)
    assert trig == want_trig(child, stream=n)
    # without a gate a request may be complete before its wait is enqueued;
    # the requests of the gated rounds are not
    live = wait[SINGLE[child]] + wait["wave_flags"]
    assert wait["consumed"] + live == n
    assert live >= RECYCLE_ROUNDS // RECYCLE_GATED * 2 * RECYCLE_PAIRS
    for k in ("eq", "gte", "capture_eq", "k_flag", "k_gte", "k_and_set"):
        assert k == SINGLE[child] or wait[k] == 0, (k, wait)
    if _wave(child, 2 * RECYCLE_PAIRS):
        gated_waitalls = RECYCLE_ROUNDS // RECYCLE_GATED // 2
        assert gated_waitalls <= wait["wave_launches"] <= RECYCLE_ROUNDS // 2
        assert (wait["wave_max_flags"], wait["wave_max_threads"]) == (32, 64)
    else:
        assert wait["wave_launches"] == 0


# ------------------------------------------------------------ two processes

def _rank_env(name):
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(CHILDREN[name])
    os.environ["MPIX_STATS"] = "1"


def _pingpong(rank, size, name):
    """The ping-pong of test_gpu.py under the switches of child `name`"""
    _rank_env(name)
    import torch
    import mpix
    mpix.init()
    try:
        assert not mpix.config()["use_memops"]
        buf = torch.zeros(1024, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream()
        for it in range(20):
            if rank == 0:
                buf.fill_(it)
                torch.cuda.synchronize()
                rs = mpix.isend_enqueue(buf, dest=1, tag=it, stream=stream)
                mpix.wait_enqueue(rs, stream=stream)
                rr = mpix.irecv_enqueue(buf, source=1, tag=it, stream=stream)
                mpix.wait_enqueue(rr, stream=stream)
                torch.cuda.synchronize()
                assert (buf == it + 1).all()
            else:
                rr = mpix.irecv_enqueue(buf, source=0, tag=it, stream=stream)
                mpix.wait_enqueue(rr, stream=stream)
                torch.cuda.synchronize()
                assert (buf == it).all()
                buf.fill_(it + 1)
                torch.cuda.synchronize()
                rs = mpix.isend_enqueue(buf, dest=0, tag=it, stream=stream)
                mpix.wait_enqueue(rs, stream=stream)
                torch.cuda.synchronize()
    finally:
        mpix.finalize()


def _two_ranks(capfd, fn, *args):
    """Run fn in two processes; the counters of both ranks"""
    from conftest import run_ranks
    if _dead:
        pytest.fail("not started: " + _dead[0])
    capfd.readouterr()
    run_ranks(2, fn, *args, timeout=CHILD_TIMEOUT)
    err = capfd.readouterr().err
    print(err[-6000:])
    assert LEAK not in err
    cnt = counters(err)
    assert set(cnt) == {0, 1}, err[-3000:]
    for rank in (0, 1):
        assert cnt[rank]["ops"][0] == cnt[rank]["ops"][1], cnt[rank]
    return cnt


@pytest.mark.parametrize("name", ["fast_kernels", "classic_kernels"])
def test_pingpong_2proc(name, capfd):
    cnt = _two_ranks(capfd, _pingpong, name)
    for rank in (0, 1):
        trig, wait = cnt[rank]["trig"], cnt[rank]["wait"]
        assert trig == want_trig(name, stream=40)
        took = wait["consumed"]
        assert wait == want_waits(name, singles=40 - took, consumed=took)
        # a receive is enqueued before the peer has sent: never all consumed
        assert wait[SINGLE[name]] > 0


def _gated_ring(rank, size):
    """Each rank: a gate, 3 sends to and 3 receives from the other rank, one
    waitall over the 6 requests."""
    _rank_env("classic_kernels")
    import torch
    import mpix
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = Ctx("classic_kernels", torch, mpix, stream)
        c.calibrate()
        mpix.init()
        try:
            assert not mpix.config()["use_memops"]
            right = (rank + 1) % size
            left = (rank - 1 + size) % size
            nb = 4096
            srcs, fulls, wants = [], [], []
            for k in range(3):
                srcs.append(torch.from_numpy(
                    pattern(nb, 1000 * rank + 100 * k)).cuda())
                wants.append(pattern(nb, 1000 * left + 100 * k))
                fulls.append(torch.full((nb + 2 * PAD,), SENT,
                                        dtype=torch.uint8, device="cuda"))
            torch.cuda.synchronize()
            c.gate(6)
            reqs = []
            for k in range(3):
                reqs.append(mpix.isend_enqueue(srcs[k], dest=right, tag=k,
                                               stream=stream))
                reqs.append(mpix.irecv_enqueue(fulls[k][PAD:PAD + nb],
                                               source=left, tag=k,
                                               stream=stream))
            mpix.waitall_enqueue(reqs, stream=stream)
            torch.cuda.synchronize()
            for k in range(3):
                c.check(fulls[k], wants[k], f"message {k}")
        finally:
            mpix.finalize()


def test_gated_ring_2proc(capfd):
    cnt = _two_ranks(capfd, _gated_ring)
    for rank in (0, 1):
        assert cnt[rank]["trig"] == want_trig("classic_kernels", stream=6)
        assert cnt[rank]["wait"] == want_waits("classic_kernels",
                                               waitalls=[(6, 6)])
        assert cnt[rank]["wait"]["wave_max_threads"] == 64


if __name__ == "__main__":
    if "--child" in sys.argv:
        child_main(sys.argv[sys.argv.index("--child") + 1],
                   "--recycle" in sys.argv)
