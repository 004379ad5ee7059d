"""Partition runs on the GPU (src/transport/part_run.h, native.cpp): a run of
partitions announced by one descriptor, taken as one copy when the receives
are posted in order and expanded otherwise, acked by ranges.

Loopback, 8 partitions.  Every case runs 3 iterations on the same requests
with a fresh position-dependent payload each time (byte i of the source is
((start + i) * 7 + 3) % 251), and the destination sits inside a larger
buffer of sentinel bytes that must survive.

MPIX_PART_RUNS is read once per process, so the cases run in two fresh child
processes, one with runs on and one with MPIX_PART_RUNS=0 (this file, started
with --child): each case must give the expected bytes in both and the same
digest and statuses in both.  A lost ack shows as a host wait that never
returns, so a child runs under a time limit and the tests fail when it
expires.  The file is chained: after a child that failed or timed out no
further process is started and the remaining tests fail at once.

The children run with MPIX_STATS=1 and a fresh init/finalize per case; the
counters printed at finalize say how many descriptors announced the 24
partitions of a case and how many partitions were received on the fast path.
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5
PAD = 64  # sentinel bytes around a destination; a multiple of 16
PARTS = 8
ITERS = 3
CHILD_TIMEOUT = 180  # s; a child takes a few seconds

# name -> keyword arguments of run_case()
CASES = {
    # one kernel flips all partitions: the full-run fast path, and 4112 B
    # partitions make the merged copy cross tile ends
    "kernel_4112": dict(per=4112, trigger="kernel"),
    # not a multiple of 16: the run is still one contiguous copy and its
    # last bytes take the tail branch
    "kernel_1000": dict(per=1000, trigger="kernel"),
    "host_ascending": dict(per=4112, order=[0, 1, 2, 3, 4, 5, 6, 7]),
    "host_descending": dict(per=4112, order=[7, 6, 5, 4, 3, 2, 1, 0]),
    "host_interleaved": dict(per=4112, order=[0, 2, 4, 6, 1, 3, 5, 7]),
    # send started and made ready first, the receive started afterwards:
    # the run arrives unexpected and expands (run_case makes sure of the
    # order with a small message sent behind the partitions)
    "late_receive": dict(per=4112, order=[0, 1, 2, 3, 4, 5, 6, 7], late=True),
    # receive partitions smaller than the send's: truncation, no fast path
    "short_receive": dict(per=4112, recv_per=4096, trigger="kernel"),
    # both fall back to hipMemcpyAsync
    "dst_plus_4": dict(per=4112, trigger="kernel", dst_off=4),
    "host_dst": dict(per=4112, trigger="kernel", host_dst=True),
}
# cases whose receives can never take a run as one copy
NEVER_FAST = ("late_receive", "short_receive", "dst_plus_4", "host_dst")


# ------------------------------------------------------------------ child

def pattern(torch, n, start, device="cuda"):
    i = torch.arange(start, start + n, dtype=torch.int64, device=device)
    return ((i * 7 + 3) % 251).to(torch.uint8)


def run_case(mpix, torch, per, trigger="host", order=None, late=False,
             recv_per=None, dst_off=0, host_dst=False, peer=0, base=0,
             peer_base=0):
    """One case on initialised mpix; returns {"digest", "status"}.  `peer`
    is both destination and source (loopback: this rank); `base` /
    `peer_base` offset the payload this rank sends / expects."""
    rper = per if recv_per is None else recv_per
    n, rn = PARTS * per, PARTS * rper
    ddev = "cpu" if host_dst else "cuda"
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = torch.full((rn + 2 * PAD + 16,), SENT, dtype=torch.uint8,
                     device=ddev)
    lo = PAD + dst_off
    stream = torch.cuda.current_stream()
    ps = mpix.psend_init((src.data_ptr(), n), PARTS, dest=peer, tag=31)
    pr = mpix.precv_init((dst.data_ptr() + lo, rn), PARTS, source=peer,
                         tag=31)
    dps = mpix.prequest_create(ps) if trigger == "kernel" else None
    digest = hashlib.sha256()
    statuses = []
    word = torch.zeros(4, dtype=torch.int32, device="cuda")

    def ready():
        if trigger == "kernel":
            mpix.launch_pready_all(dps, PARTS, stream.cuda_stream)
        else:
            for p in order:
                mpix.pready(p, ps)

    try:
        for it in range(ITERS):
            start = base + 1000 * it
            src.copy_(pattern(torch, n, start))
            dst.fill_(SENT)
            torch.cuda.synchronize()
            if late:
                mpix.start(ps)
                ready()
                # a message to ourselves queued behind the partitions: sends
                # to one rank are announced in order, so once it has been
                # received the run has arrived, with no receive posted
                rs = mpix.isend_enqueue(word, dest=peer, tag=32,
                                        stream=stream)
                rr = mpix.irecv_enqueue(word, source=peer, tag=32,
                                        stream=stream)
                mpix.waitall_enqueue([rs, rr], stream=stream)
                torch.cuda.synchronize()
                mpix.start(pr)
            else:
                mpix.start(pr)
                mpix.start(ps)
                ready()
            st_r = mpix.wait(pr)
            st_s = mpix.wait(ps)
            torch.cuda.synchronize()
            statuses.append([st_r, st_s])
            got = dst.cpu()
            # partition p of the receive holds the first rper bytes of
            # partition p of the send
            want = pattern(torch, n, peer_base + 1000 * it, device="cpu")
            want = want.view(PARTS, per)[:, :rper].reshape(-1)
            assert torch.equal(got[lo:lo + rn], want), f"payload, iter {it}"
            assert bool((got[:lo] == SENT).all()), f"bytes before, iter {it}"
            assert bool((got[lo + rn:] == SENT).all()), \
                f"bytes after, iter {it}"
            digest.update(got.numpy().tobytes())
    finally:
        if dps is not None:
            mpix.prequest_free(dps)
        mpix.request_free(ps)
        mpix.request_free(pr)
    return {"digest": digest.hexdigest(), "status": statuses}


def child_main():
    sys.path.insert(0, REPO)
    import torch
    import mpix

    for name, kw in CASES.items():
        # the library's counters go to stderr at finalize: mark whose they are
        sys.stderr.write(f"CASE-BEGIN {name}\n")
        sys.stderr.flush()
        mpix.init()
        try:
            res = run_case(mpix, torch, **kw)
        finally:
            mpix.finalize()
        print("CASE " + json.dumps({"name": name, **res}, default=str),
              flush=True)
    print("CHILD-DONE", flush=True)


# ----------------------------------------------------------------- parent

_results = {}  # mode -> {case: {"digest", "status", "descs", "msgs", "fast"}}
_dead = []     # why no further process may be started

_COUNTERS = re.compile(r"device notifies: (\d+) descriptors for (\d+) "
                       r"messages sent, (\d+) messages received")


def _child(mode):
    """Results of all cases under `mode` ("on" / "off"), from one child."""
    if mode in _results:
        return _results[mode]
    if _dead:
        pytest.fail("not started: " + _dead[0])
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", MPIX_STATS="1")
    env.pop("MPIX_PART_RUNS", None)
    if mode == "off":
        env["MPIX_PART_RUNS"] = "0"
    try:
        run = subprocess.run([sys.executable, os.path.abspath(__file__),
                              "--child"], env=env, capture_output=True,
                             text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout
        done = re.findall(r'^CASE {"name": "(\w+)"', out or "", re.M)
        _dead.append(f"child with runs {mode} timed out after "
                     f"{CHILD_TIMEOUT} s (a lost ack?); finished cases: "
                     f"{done}")
        pytest.fail(_dead[0])
    if run.returncode != 0 or "CHILD-DONE" not in run.stdout:
        _dead.append(f"child with runs {mode} failed (exit "
                     f"{run.returncode}):\n{run.stdout[-2000:]}\n"
                     f"{run.stderr[-4000:]}")
        pytest.fail(_dead[0])
    res = {}
    for line in run.stdout.splitlines():
        if line.startswith("CASE "):
            r = json.loads(line[5:])
            res[r["name"]] = r
    for block in run.stderr.split("CASE-BEGIN ")[1:]:
        name = block.split("\n", 1)[0].strip()
        m = _COUNTERS.search(block)
        assert m is not None, f"no counters for {name}:\n{block[-2000:]}"
        res[name]["descs"], res[name]["msgs"], res[name]["fast"] = \
            (int(g) for g in m.groups())
    _results[mode] = res
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    on = _child("on")[name]
    off = _child("off")[name]
    print(f"{name}: runs on {on['descs']} descriptors / {on['msgs']} "
          f"partitions, {on['fast']} on the fast path; runs off "
          f"{off['descs']} / {off['msgs']}, {off['fast']}")
    total = PARTS * ITERS
    if CASES[name].get("late"):
        total += ITERS  # the small message behind the partitions
    # the payload and sentinel checks ran in the children; here: both
    # protocols delivered the same bytes and statuses
    assert on["digest"] == off["digest"]
    assert on["status"] == off["status"]
    # every partition was announced; without runs, one descriptor each
    assert on["msgs"] == total and off["msgs"] == total
    assert off["descs"] == total and off["fast"] == 0
    assert 1 <= on["descs"] <= total
    assert on["fast"] <= total
    if name in NEVER_FAST:
        assert on["fast"] == 0
    if name == "kernel_4112":
        # one wave stores the 8 flags with one instruction, and the receives
        # were posted a kernel launch earlier: over 3 iterations the proxy
        # sees at least two adjacent flags in one pass
        assert on["fast"] > 0 and on["descs"] < total


def _ring_rank(rank, size, mode):
    if mode == "off":
        os.environ["MPIX_PART_RUNS"] = "0"
    else:
        os.environ.pop("MPIX_PART_RUNS", None)
    import torch
    import mpix
    mpix.init()
    try:
        # everyone sends to the right and receives from the left; with two
        # ranks both are the other rank
        assert size == 2
        other = 1 - rank
        run_case(mpix, torch, per=4112, trigger="kernel", peer=other,
                 base=100 * rank, peer_base=100 * other)
    finally:
        mpix.finalize()


@pytest.mark.parametrize("mode", ["on", "off"])
def test_two_rank_ring(mode):
    """The 4112 B case between two processes on one GPU: the descriptors and
    the range acks cross the shared-memory rings, the source is an IPC
    mapping."""
    from conftest import run_ranks
    if _dead:
        pytest.fail("not started: " + _dead[0])
    try:
        run_ranks(2, _ring_rank, mode, timeout=120)
    except BaseException as e:
        _dead.append(f"two-rank ring with runs {mode} failed: {e}")
        raise


if __name__ == "__main__":
    if "--child" in sys.argv:
        child_main()
