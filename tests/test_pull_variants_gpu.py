"""The knobs that select a pull-kernel variant, through the runtime:
MPIX_PULL_UNROLL = 1 and 8 and MPIX_PULL_NT=0 under MPIX_PULL_DONE = word,
event and tail (src/transport/native.cpp, pull_kernels.h).  The rest of the
suite runs the defaults only (unroll 4, nontemporal).
tests/test_pull_kernels_gpu.py proves the kernels themselves; this file
proves that the knobs reach them and that the bytes do not depend on them.

Loopback, in the child-process scheme of tests/test_pull_done_modes_gpu.py,
whose helpers this file uses (the MPIX_* switches are read once per process):
fresh children under a time limit, chained so that nothing is started after
a child that failed or timed out.  The children run with MPIX_STATS=1 and
MPIX_TRACE=1.

Cases, each a child's own subset; the `default` child (no knob) runs all of
them and its digests are what every other child must reproduce:
  edge_u1, edge_u4, edge_u8   single messages of T - 16, T, T + 16 and T + 21
                 bytes for the tile T = 4096 U of that unroll: the last full
                 tile, the partial tile and the tail bytes.  The trace line
                 of every batch must show the tile count that only the
                 requested unroll gives: 1, 1, 2, 2
  fixed_32784    32784 B: 9, 3 and 2 tiles under unroll 1, 4 and 8.  This is
                 the assertion that the knob took effect
  kernel         8 kernel-triggered partitions of 4112 B, 5 iterations
  strided40      40 strided messages of mixed granule under ONE
                 waitall_enqueue, more than MPIX_STRIDED_BATCH = 16: a pass
                 that finds more than 16 of them matched splits its flush,
                 and under word several batches are in flight against the
                 ring of 16 completion slots.  How many messages meet in one
                 progress pass is a matter of timing (the batch sizes are
                 printed, see profiles/pull_kernels_check.md for what was
                 seen); a full table of 16 entries under every kernel is what
                 tests/test_pull_kernels_gpu.py launches.  The whole
                 destination base of every message is compared with what it
                 must hold, as in tests/test_strided_gpu.py
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_batch_handoffs_gpu as hb  # noqa: E402
import test_pull_done_modes_gpu as dm  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = hb.REPO
ITERS, PARTS = hb.ITERS, hb.PARTS
CHILD_TIMEOUT = 180  # s; a child takes a few seconds
FIXED = 32784
STRIDED_MSGS = 40
STRIDED_BATCH = 16  # MPIX_STRIDED_BATCH


def _edges(u):
    t = 4096 * u
    return [t - 16, t, t + 16, t + 21]


def _tiles(n, u):
    return -(-n // (4096 * u))


ALL_CASES = ["edge_u1", "edge_u4", "edge_u8", "fixed_32784", "kernel",
             "strided40"]
# child -> (environment, unroll in effect, completion mode, cases)
CHILDREN = {
    "default": ({}, 4, "word", ALL_CASES),
    "u1_word": ({"MPIX_PULL_UNROLL": "1", "MPIX_PULL_DONE": "word"}, 1,
                "word", ["edge_u1", "fixed_32784", "kernel", "strided40"]),
    "u8_word": ({"MPIX_PULL_UNROLL": "8", "MPIX_PULL_DONE": "word"}, 8,
                "word", ["edge_u8", "fixed_32784", "kernel"]),
    "u1_event": ({"MPIX_PULL_UNROLL": "1", "MPIX_PULL_DONE": "event"}, 1,
                 "event", ["edge_u1", "fixed_32784", "kernel", "strided40"]),
    "u8_event": ({"MPIX_PULL_UNROLL": "8", "MPIX_PULL_DONE": "event"}, 8,
                 "event", ["edge_u8", "fixed_32784", "kernel"]),
    "nt0_event": ({"MPIX_PULL_NT": "0", "MPIX_PULL_DONE": "event"}, 4,
                  "event", ["edge_u4", "fixed_32784", "kernel"]),
    "u8_nt0_tail": ({"MPIX_PULL_UNROLL": "8", "MPIX_PULL_NT": "0",
                     "MPIX_PULL_DONE": "tail"}, 8, "tail",
                    ["edge_u8", "fixed_32784", "kernel", "strided40"]),
}
VARIANTS = [c for c in CHILDREN if c != "default"]
ENV_KEYS = dm.ENV_KEYS


# ------------------------------------------------------------------ child

def case_strided40(mpix, torch):
    """The layouts of tests/test_strided_gpu.py in turn (granules 16, 8, 4,
    2 and 1, neighbours differ), 40 messages with bases of their own, posted
    before one waitall_enqueue."""
    import test_strided_gpu as sg
    names = list(sg.CASES)
    msgs = []
    for i in range(STRIDED_MSGS):
        sshape, s_of, dshape, d_of, dt = sg.CASES[names[i % len(names)]]
        dtype = dt() if dt else None
        msgs.append((s_of(sg.pattern(sshape, dtype)),
                     sg.sentinel(dshape, dtype), d_of))
    # The sends go first and wait unmatched.  The receives are enqueued
    # behind about a millisecond of other work on the stream, so that their
    # triggers fire back to back and a progress pass finds several of them
    # matched at once (posted one by one on an idle stream they arrive one
    # per pass: batches of one).  How many meet in a pass is timing; the
    # parent prints the batch sizes and asserts only what always holds.
    stream = torch.cuda.current_stream()
    busy = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reqs = []
    for tag, (s, d, d_of) in enumerate(msgs):
        reqs.append(mpix.isend_enqueue(s, dest=0, tag=300 + tag,
                                       stream=stream))
    for _ in range(8):
        busy.fill_(1)
    for tag, (s, d, d_of) in enumerate(msgs):
        reqs.append(mpix.irecv_enqueue(d_of(d), source=0, tag=300 + tag,
                                       stream=stream))
    mpix.waitall_enqueue(reqs, stream=stream)
    torch.cuda.synchronize()
    digest = hashlib.sha256()
    for i, (s, d, d_of) in enumerate(msgs):
        want = sg.expected_base(d, d_of, sg.raw(s))
        assert sg.same_bytes(d, want), f"message {i}, {names[i % len(names)]}"
        digest.update(d.reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
    return {"digest": digest.hexdigest(), "status": []}


def child_main(name):
    sys.path.insert(0, REPO)
    import torch
    import mpix

    run = {
        "fixed_32784": lambda: dm.case_single(mpix, torch, [FIXED]),
        "kernel": lambda: hb.case_transfer(mpix, torch, None),
        "strided40": lambda: case_strided40(mpix, torch),
    }
    for u in (1, 4, 8):
        run["edge_u%d" % u] = lambda u=u: dm.case_single(mpix, torch,
                                                         _edges(u))
    for case in CHILDREN[name][3]:
        sys.stderr.write(f"CASE-BEGIN {case}\n")
        sys.stderr.flush()
        mpix.init()
        try:
            res = run[case]()
        finally:
            mpix.finalize()
        print("CASE " + json.dumps({"name": case, **res}, default=str),
              flush=True)
    print("CHILD-DONE", flush=True)


# ----------------------------------------------------------------- parent

_results = {}
_dead = []

_BATCH = re.compile(r"\] pull batch n=(\d+) copies=(\d+) tiles=(\d+) "
                    r"total=(\d+) B")
_SBATCH = re.compile(r"\] strided pull batch n=(\d+) tiles=(\d+) "
                     r"total=(\d+) B wide=(\d) parts=(\d)")


def _child(name):
    if name in _results:
        return _results[name]
    if _dead:
        pytest.fail("not started: " + _dead[0])
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", MPIX_STATS="1")
    for k in ENV_KEYS:
        env.pop(k, None)
    env.update(CHILDREN[name][0], MPIX_TRACE="1")
    try:
        run = subprocess.run([sys.executable, os.path.abspath(__file__),
                              "--child", name], env=env, capture_output=True,
                             text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout
        done = re.findall(r'^CASE {"name": "(\w+)"', out or "", re.M)
        _dead.append(f"child {name} timed out after {CHILD_TIMEOUT} s (a "
                     f"lost completion word?); finished cases: {done}")
        pytest.fail(_dead[0])
    if run.returncode != 0 or "CHILD-DONE" not in run.stdout:
        _dead.append(f"child {name} failed (exit {run.returncode}):\n"
                     f"{run.stdout[-2000:]}\n{run.stderr[-4000:]}")
        pytest.fail(_dead[0])
    res = {}
    for line in run.stdout.splitlines():
        if line.startswith("CASE "):
            r = json.loads(line[5:])
            res[r["name"]] = r
    for block in run.stderr.split("CASE-BEGIN ")[1:]:
        res[block.split("\n", 1)[0].strip()]["stderr"] = block
    _results[name] = res
    return res


def _check_tiles(block, sizes, unroll):
    """every message of `sizes` was one batch of one copy, cut into the
    tiles that `unroll` gives"""
    batches = [tuple(int(g) for g in m) for m in _BATCH.findall(block)]
    print(f"unroll {unroll}: (n, copies, tiles, total) {batches}")
    assert batches == [(1, 1, _tiles(n, unroll), n) for n in sizes]


@pytest.mark.parametrize("name", list(CHILDREN))
def test_knob_selects_the_variant(name):
    """Same bytes as without the knob, and the tile counts of the requested
    unroll in the trace."""
    _, unroll, mode, cases = CHILDREN[name]
    res, ref = _child(name), _child("default")
    for case in cases:
        assert res[case]["digest"] == ref[case]["digest"], case
        assert res[case]["status"] == ref[case]["status"], case
        block = res[case]["stderr"]
        named, by_word = dm._by_word(block)
        print(f"{name}, {case}: {by_word} batches completed by word")
        if mode == "event":
            assert (named, by_word) == (None, 0), case
        else:
            assert named == mode, case
        if case.startswith("edge_u"):
            sizes = _edges(int(case[-1]))
            _check_tiles(block, sizes, unroll)
            # T + 16 is 2 tiles whatever the unroll, but only when T is the
            # tile in effect: a child runs the sizes of its own unroll
            if name != "default":
                assert int(case[-1]) == unroll
            assert mode == "event" or by_word == len(sizes), case
        elif case == "fixed_32784":
            _check_tiles(block, [FIXED], unroll)
            assert _tiles(FIXED, unroll) == {1: 9, 4: 3, 8: 2}[unroll]
            assert mode == "event" or by_word == 1, case
        elif case == "kernel":
            assert mode == "event" or \
                ITERS <= by_word <= PARTS * ITERS, case


@pytest.mark.parametrize("name", [c for c in CHILDREN
                                  if "strided40" in CHILDREN[c][3]])
def test_forty_strided_messages(name):
    """All 40 messages go through the strided kernel, in batches of at most
    16; the destination bases were compared in the child.  That a pass
    collects more than 16 and splits is not asserted: it is timing (batches
    of up to 14 were seen)."""
    mode = CHILDREN[name][2]
    block = _child(name)["strided40"]["stderr"]
    batches = [int(m[0]) for m in _SBATCH.findall(block)]
    print(f"{name}: strided batches of {batches}")
    assert sum(batches) == STRIDED_MSGS
    assert max(batches) <= STRIDED_BATCH
    assert len(batches) >= -(-STRIDED_MSGS // STRIDED_BATCH)
    assert _BATCH.search(block) is None  # nothing went the contiguous way
    named, by_word = dm._by_word(block)
    if mode == "event":
        assert (named, by_word) == (None, 0)
    else:
        # a batch that finds all 16 completion slots taken goes by event
        print(f"{name}: {by_word} of them completed by word")
        assert named == mode and 1 <= by_word <= len(batches)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child_main(sys.argv[sys.argv.index("--child") + 1])
