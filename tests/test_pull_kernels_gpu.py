"""Every pull-kernel variant of src/transport/pull_kernels.h against a
byte-exact reference: the nine contiguous kernels (unroll 1, 4, 8 x
write-through with the completion word, nontemporal, plain) and the eight
strided ones (narrow and wide division x with and without the partition level
x word and event), launched directly by tests/native/pull_kernels_check.hip
with block counts the runtime never picks, so that blocks grid-stride, step
over whole copies and enter entries of another granule in the middle.

The harness (tools/bin/pull_kernels_check GROUP) plans with the production
planners, launches with launch_pull / launch_strided / launch_tail, compares
the whole destination arena (and a guard page behind it) with
tests/native/pull_ref.h and prints one JSON line per launch.  One completion
counter and one word serve all by-word launches of a process: after each the
counter reads 0 and the word that launch's number, through grid sizes 1, 2,
3, 7, 65, 79 and 1024 in contig-u1.  tests/test_pull_ref.py shows on the CPU
that the comparison flags a subtly wrong walk.

Not covered here: that the word, once seen, implies the payload without a
synchronise (tests/test_pull_done_modes_gpu.py reads from a second stream),
and that the runtime's knobs select these kernels (same file).

Every group is a fresh child process with a time limit of its own.  The file
is chained: after a child that died on a signal or ran into its limit no
further child is started and the remaining groups fail at once with that
reason.  A child that merely reports bad bytes does not stop the chain.
"""
import json
import os
import signal
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "tools")
BINARY = os.path.join(TOOLS, "bin", "pull_kernels_check")
# s; guards against a hang, not a performance figure.  The slowest group
# took 0.39 s of wall time on an MI355X, process start and the first launch
# of each kernel included (profiles/pull_kernels_check.md): 150 times that
CHILD_TIMEOUT = 60

GROUPS = ["contig-u1", "contig-u4", "contig-u8", "strided-narrow",
          "strided-wide"]

_dead = []  # why no further process may be started


def _blocks(want, tiles):
    out = []
    for b in want:
        b = min(tiles if b == 0 else b, tiles, 1024)
        if b not in out:
            out.append(b)
    return out


def _expected(group):
    """{(variant, table, blocks): tiles} the group has to report"""
    want = {("k_pull_tail", "-", 1): 0}
    if group.startswith("contig"):
        u = int(group[-1])
        t = 4096 * u
        tables = [("edges/3", 3), ("edges/16", 16), ("edges/19", 19),
                  ("edges/T-16", t - 16), ("edges/T", t),
                  ("edges/T+16", t + 16), ("edges/T+21", t + 21),
                  ("edges/3T+21", 3 * t + 21)]
        tables = [(name, -(-n // t), [1, 2, 0]) for name, n in tables]
        # 64 copies; 8 segments of 4112 B merged + one alone
        tables.append(("full_table", 79, [1, 2, 3, 7, 65, 0]))
        tables.append(("merged_run", -(-8 * 4112 // t) + -(-4112 // t),
                       [1, 2, 0]))
        if u == 1:
            tables.append(("full_table_1024", 78 + 1024, [1024]))
        variants = [f"k_pull_multi_done<{u},WT>", f"k_pull_multi<{u},NT>",
                    f"k_pull_multi<{u},PLAIN>"]
        for name, tiles, blocks in tables:
            for v in variants:
                for b in _blocks(blocks, tiles):
                    want[(v, name, b)] = tiles
    else:
        w = 1 if group == "strided-wide" else 0
        for name, tiles, parts in (("mixed_granules", 29, (0, 1)),
                                   ("with_partitions", 22, (1,))):
            for p in parts:
                for kernel in ("k_pull_strided_done", "k_pull_strided"):
                    for b in _blocks([1, 2, 3, 0], tiles):
                        want[(f"{kernel}<wide={w},parts={p}>", name, b)] = \
                            tiles
    return want


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", TOOLS, "bin/pull_kernels_check"],
                       check=True, capture_output=True)


def _run(group):
    """One child under its own limit.  Returns the completed process, or
    fails the test (and every later one) if the child died on a signal or
    ran into the limit."""
    _ensure_built()
    if _dead:
        pytest.fail("not started: " + _dead[0])
    try:
        run = subprocess.run([BINARY, group], cwd=REPO, capture_output=True,
                             text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout
        _dead.append(f"{group} ran into its limit of {CHILD_TIMEOUT} s (a "
                     f"kernel that never ends?); last output:\n"
                     f"{(out or '')[-2000:]}")
        pytest.fail(_dead[0])
    if run.returncode < 0:
        try:
            name = signal.Signals(-run.returncode).name
        except ValueError:
            name = "signal %d" % -run.returncode
        _dead.append(f"{group} died on {name}:\n{run.stdout[-2000:]}\n"
                     f"{run.stderr[-4000:]}")
        pytest.fail(_dead[0])
    return run


@pytest.mark.parametrize("group", GROUPS)
def test_kernels_against_reference(group):
    run = _run(group)
    lines = [json.loads(l) for l in run.stdout.splitlines()
             if l.startswith("{")]
    detail = f"exit {run.returncode}\n{run.stderr[-4000:]}"
    launches = [r for r in lines if "variant" in r]
    summary = [r for r in lines if "group" in r]
    bad = [r for r in launches if r["bad"] or r["src_bad"]]
    assert not bad, f"{bad[:5]}\n{detail}"
    # every expected launch exactly once, and nothing else
    want = _expected(group)
    got = [(r["variant"], r["table"], r["blocks"]) for r in launches]
    assert sorted(got) == sorted(want), detail
    for r in launches:
        assert r["tiles"] == want[(r["variant"], r["table"], r["blocks"])], r
        assert r["first_bad"] is None, r
    # one counter and one word for the whole process
    seq, word = 0, 0
    for r in launches:
        assert r["counter"] == 0, r
        assert r["word_before"] == word, r
        if r["seq"] is not None:  # by word, or the tail kernel
            assert r["seq"] == seq + 1, r
            seq = word = r["seq"]
        assert r["word"] == word, r
    by_word = [r for r in launches if r["seq"] is not None]
    assert len(by_word) == sum("_done" in v or v == "k_pull_tail"
                               for v, _, _ in want)
    if group == "contig-u1":
        assert {1, 2, 3, 7, 65, 1024} <= {r["blocks"] for r in by_word}
    assert len(summary) == 1 and summary[0]["failed"] == 0, detail
    assert summary[0]["launches"] == len(want), detail
    print(f"{group}: {len(launches)} launches in {summary[0]['seconds']} s")
    assert run.returncode == 0, detail
