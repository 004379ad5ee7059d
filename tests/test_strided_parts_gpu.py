"""Partitioned transfers with layouts on the GPU: strided and gapped
partitions announced as runs (src/transport/part_run.h, native.cpp) and moved
by one kernel entry, folded into one layout or through the partition level of
k_pull_strided (strided_plan.h).

Loopback, 8 partitions.  A side of a case is a byte view (shape, strides in
bytes) whose dimension 0 are the partitions; psend_init / precv_init derive
the partition layout and the part stride from it.  Every case runs 3
iterations on the same requests with a fresh position-dependent payload each
time (byte i of the source BUFFER is ((start + i) * 7 + 3) % 251), and the
destination view sits inside a larger buffer of sentinel bytes that must
survive, gaps of the view included: the whole destination buffer is compared
with what numpy-style indexing on the CPU says it must be.

MPIX_PART_RUNS and MPIX_STRIDED_DIV64 are read once per process, so the cases
run in fresh child processes (this file, started with --child): all with runs
on, all with MPIX_PART_RUNS=0, and two of them with MPIX_STRIDED_DIV64=1.
Each case must give the expected bytes in every child and the same digest and
statuses in all of them.  A lost ack shows as a host wait that never returns,
so a child runs under a time limit and the tests fail when it expires.  The
file is chained: after a child that failed or timed out no further process is
started and the remaining tests fail at once.

The children run with MPIX_STATS=1 and a fresh init/finalize per case; the
counters printed at finalize say how many descriptors announced the 24
partitions of a case, how many partitions were received on the fast path and
which pull the fast runs became.

Smallest shapes that reach each path:
  rows_gap      contiguous 4112 B partitions 4352 apart: folds; the trap of
                a run whose partitions are not msg_bytes apart
  yface_fold    15 runs of 272 B, 400 apart, partitions at that pitch: folds;
                the 32640 B run crosses a 16 KiB tile and ends in a partial
  yface_nofold  the same, partitions 64 B further apart: partition level
  two_level     both sides strided differently, two levels on the send side
  gran4, gran1  the element paths
  into_strided  a plain psend into a strided receiver as one entry
  host_*        short runs, range acks in any order
  late_receive  expansion at j * part_stride
  short_receive truncation, expansion
  host_dst      device to a host view: MPI_ERR_TYPE per partition, nothing
                written, the sender still completes
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
PAD = 64  # sentinel bytes around a destination view; a multiple of 16
PARTS = 8
ITERS = 3
CHILD_TIMEOUT = 180  # s; a child takes a few seconds


def side(shape, strides):
    return dict(shape=(PARTS,) + tuple(shape), strides=tuple(strides))


def plain(per):
    return side((per,), (per, 1))


ROWS_GAP = side((4112,), (4352, 1))
YFACE_FOLD = side((15, 272), (6000, 400, 1))
YFACE_NOFOLD = side((15, 272), (6064, 400, 1))
TWO_LEVEL_S = side((2, 5, 48), (4096, 1024, 80, 1))
TWO_LEVEL_R = side((5, 96), (1024, 128, 1))

# name -> keyword arguments of run_case()
CASES = {
    "rows_gap": dict(send=ROWS_GAP, recv=plain(4112), trigger="kernel"),
    "yface_fold": dict(send=YFACE_FOLD, recv=plain(4080), trigger="kernel"),
    "yface_nofold": dict(send=YFACE_NOFOLD, recv=plain(4080),
                         trigger="kernel"),
    "two_level": dict(send=TWO_LEVEL_S, recv=TWO_LEVEL_R, trigger="kernel"),
    "gran4": dict(send=side((7, 4), (100, 12, 1)), recv=plain(28),
                  trigger="kernel"),
    "gran1": dict(send=side((5, 3), (41, 7, 1)), recv=plain(15),
                  trigger="kernel", dst_off=1),
    "into_strided": dict(send=plain(4080), recv=YFACE_NOFOLD,
                         trigger="kernel"),
    "host_descending": dict(send=YFACE_NOFOLD, recv=YFACE_NOFOLD,
                            order=[7, 6, 5, 4, 3, 2, 1, 0]),
    "host_interleaved": dict(send=YFACE_NOFOLD, recv=YFACE_NOFOLD,
                             order=[0, 2, 4, 6, 1, 3, 5, 7]),
    # send started and made ready first, the receive started afterwards: the
    # run arrives unexpected and expands (run_case makes sure of the order
    # with a small message sent behind the partitions)
    "late_receive": dict(send=YFACE_NOFOLD, recv=plain(4080),
                         order=[0, 1, 2, 3, 4, 5, 6, 7], late=True),
    "short_receive": dict(send=YFACE_NOFOLD, recv=plain(4064),
                          trigger="kernel"),
    "host_dst": dict(send=YFACE_NOFOLD, recv=YFACE_NOFOLD, trigger="kernel",
                     host_dst=True),
}
# cases whose receives can never take a run as one pull
NEVER_FAST = ("late_receive", "short_receive", "host_dst")
# cases run once more with 64-bit division forced in the kernel
DIV64_CASES = ("yface_nofold", "two_level")


# ------------------------------------------------------------------ child

def pattern(torch, n, start):
    i = torch.arange(start, start + n, dtype=torch.int64)
    return ((i * 7 + 3) % 251).to(torch.uint8)


def span(sd):
    """Bytes from the first to one past the last byte of a side's view."""
    return 1 + sum((n - 1) * s for n, s in zip(sd["shape"], sd["strides"]))


def view_of(torch, base, off, sd):
    return torch.as_strided(base, sd["shape"], sd["strides"], off)


def per_part(sd):
    n = 1
    for s in sd["shape"][1:]:
        n *= s
    return n


def run_case(mpix, torch, send, recv, trigger="host", order=None, late=False,
             dst_off=0, host_dst=False, peer=0, base=0, peer_base=0):
    """One case on initialised mpix; returns {"digest", "status"}.  `peer`
    is both destination and source (loopback: this rank); `base` /
    `peer_base` offset the payload this rank sends / expects."""
    sn = span(send) + 32
    rn = span(recv) + 2 * PAD + 16
    lo = PAD + dst_off
    src = torch.zeros(sn, dtype=torch.uint8, device="cuda")
    dst = torch.full((rn,), SENT, dtype=torch.uint8,
                     device="cpu" if host_dst else "cuda")
    stream = torch.cuda.current_stream()
    ps = mpix.psend_init(view_of(torch, src, 0, send), PARTS, dest=peer,
                         tag=41)
    pr = mpix.precv_init(view_of(torch, dst, lo, recv), PARTS, source=peer,
                         tag=41)
    dps = mpix.prequest_create(ps) if trigger == "kernel" else None
    digest = hashlib.sha256()
    statuses = []
    word = torch.zeros(4, dtype=torch.int32, device="cuda")
    # every receive partition takes the head of its send partition
    take = min(per_part(send), per_part(recv))
    assert per_part(recv) <= per_part(send)

    def ready():
        if trigger == "kernel":
            mpix.launch_pready_all(dps, PARTS, stream.cuda_stream)
        else:
            for p in order:
                mpix.pready(p, ps)

    try:
        for it in range(ITERS):
            src.copy_(pattern(torch, sn, base + 1000 * it))
            dst.fill_(SENT)
            torch.cuda.synchronize()
            if late:
                mpix.start(ps)
                ready()
                # a message to ourselves queued behind the partitions: sends
                # to one rank are announced in order, so once it has been
                # received the run has arrived, with no receive posted
                rs = mpix.isend_enqueue(word, dest=peer, tag=42,
                                        stream=stream)
                rr = mpix.irecv_enqueue(word, source=peer, tag=42,
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
            # the reference, by indexing on the CPU: what the peer's source
            # buffer held, read through the send view, written through the
            # receive view into a buffer of sentinels
            want_src = pattern(torch, sn, peer_base + 1000 * it)
            msgs = view_of(torch, want_src, 0, send).reshape(PARTS, -1)
            want = torch.full((rn,), SENT, dtype=torch.uint8)
            if not host_dst:  # host_dst: refused, nothing is written
                wv = view_of(torch, want, lo, recv)
                for p in range(PARTS):
                    wv[p].copy_(msgs[p, :take].reshape(wv[p].shape))
            bad = (got != want).nonzero().flatten()
            assert bad.numel() == 0, (
                f"iter {it}: {bad.numel()} wrong bytes, first at "
                f"{int(bad[0])} (view starts at {lo})")
            digest.update(got.numpy().tobytes())
    finally:
        if dps is not None:
            mpix.prequest_free(dps)
        mpix.request_free(ps)
        mpix.request_free(pr)
    return {"digest": digest.hexdigest(), "status": statuses}


def child_main(names):
    sys.path.insert(0, REPO)
    import torch
    import mpix

    for name in names:
        # the library's counters go to stderr at finalize: mark whose they are
        sys.stderr.write(f"CASE-BEGIN {name}\n")
        sys.stderr.flush()
        mpix.init()
        try:
            res = run_case(mpix, torch, **CASES[name])
        finally:
            mpix.finalize()
        print("CASE " + json.dumps({"name": name, **res}, default=str),
              flush=True)
    print("CHILD-DONE", flush=True)


# ----------------------------------------------------------------- parent

_results = {}  # mode -> {case: {"digest", "status", "descs", "msgs", ...}}
_dead = []     # why no further process may be started

_COUNTERS = re.compile(r"device notifies: (\d+) descriptors for (\d+) "
                       r"messages sent, (\d+) messages received")
_SHAPES = re.compile(r"fast runs: (\d+) as one contiguous copy, (\d+) folded "
                     r"into one strided entry, (\d+) as an entry with a "
                     r"partition level")


def _child(mode):
    """Results of the cases of `mode` ("on" / "off" / "div64"), from one
    child process."""
    if mode in _results:
        return _results[mode]
    if _dead:
        pytest.fail("not started: " + _dead[0])
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", MPIX_STATS="1")
    env.pop("MPIX_PART_RUNS", None)
    env.pop("MPIX_STRIDED_DIV64", None)
    names = list(CASES)
    if mode == "off":
        env["MPIX_PART_RUNS"] = "0"
    elif mode == "div64":
        env["MPIX_STRIDED_DIV64"] = "1"
        names = list(DIV64_CASES)
    try:
        run = subprocess.run([sys.executable, os.path.abspath(__file__),
                              "--child"] + names, env=env,
                             capture_output=True, text=True,
                             timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout
        done = re.findall(r'^CASE {"name": "(\w+)"', out or "", re.M)
        _dead.append(f"child '{mode}' timed out after {CHILD_TIMEOUT} s "
                     f"(a lost ack?); finished cases: {done}")
        pytest.fail(_dead[0])
    if run.returncode != 0 or "CHILD-DONE" not in run.stdout:
        _dead.append(f"child '{mode}' failed (exit {run.returncode}):\n"
                     f"{run.stdout[-2000:]}\n{run.stderr[-4000:]}")
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
        m = _SHAPES.search(block)
        res[name]["shapes"] = [int(g) for g in m.groups()] if m else [0, 0, 0]
        res[name]["err_type"] = block.count("fails with MPI_ERR_TYPE")
    _results[mode] = res
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    on = _child("on")[name]
    off = _child("off")[name]
    print(f"{name}: runs on {on['descs']} descriptors / {on['msgs']} "
          f"partitions, {on['fast']} on the fast path as (copy, folded, "
          f"partition level) = {on['shapes']}; runs off {off['descs']} / "
          f"{off['msgs']}, {off['fast']}")
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
    copy, folded, parts = on["shapes"]
    if name in NEVER_FAST:
        assert on["fast"] == 0
    # no strided or gapped run may ever be taken as one contiguous copy
    assert copy == 0
    if name in ("rows_gap", "yface_fold"):
        assert parts == 0
    else:
        assert folded == 0
    if name == "yface_fold":
        # one wave stores the 8 flags with one instruction, and the receives
        # were posted a kernel launch earlier: over 3 iterations the proxy
        # sees at least two adjacent flags in one pass
        assert on["fast"] > 0 and on["descs"] < total and folded > 0
    if name == "host_dst":
        # every partition is refused on its own, in both protocols
        assert on["err_type"] >= 1 and off["err_type"] >= 1


@pytest.mark.parametrize("name", DIV64_CASES)
def test_case_div64(name):
    """The same bytes with 64-bit division forced in the kernel."""
    on = _child("on")[name]
    wide = _child("div64")[name]
    assert wide["digest"] == on["digest"]
    assert wide["status"] == on["status"]
    assert wide["msgs"] == PARTS * ITERS
    assert 1 <= wide["descs"] <= PARTS * ITERS


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
        run_case(mpix, torch, send=YFACE_NOFOLD, recv=plain(4080),
                 trigger="kernel", peer=other, base=100 * rank,
                 peer_base=100 * other)
    finally:
        mpix.finalize()


@pytest.mark.parametrize("mode", ["on", "off"])
def test_two_rank_ring(mode):
    """yface_nofold between two processes on one GPU: the descriptor with
    its part stride and the range acks cross the shared-memory rings, the
    source is an IPC mapping."""
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
        child_main(sys.argv[sys.argv.index("--child") + 1:])
