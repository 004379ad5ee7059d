"""The strided reduce kernels of src/transport/pull_kernels.h
(k_pull_strided_reduce<WIDE>, which stores nontemporal, and
k_pull_strided_reduce_done<WIDE>, which stores write-through and signals the
completion word: four kernels) against an element-by-element reference
through part_layout_offset and Red<TYPE>::combine
(tests/native/strided_reduce_ref.h), byte for byte, launched directly by
tests/native/strided_reduce_kernels_check.hip with block counts the runtime
never picks.

The harness (tools/bin/strided_reduce_kernels_check GROUP) plans with
plan_strided_reduce, launches with launch_strided_reduce, compares the whole
destination arena, the gaps between the runs and a guard page behind it
included, checks that the source is unchanged, and prints one JSON line per
launch.  One completion counter and one word serve all by-word launches of a
process: after each the counter reads 0 and the word that launch's number.
Groups (T = 16 KiB tile):

  edges   all 18 type/op pairs x entries of 1 element, 16 B, T - 16, T,
          T + 16 + 1 element, 3T + an odd number of elements, each strided on
          the destination only in runs of 1 element and of 48 B, each with 1,
          2 and `tiles` blocks;
  shapes  strided to contiguous and back, one level against two, a base
          offset by one element, runs of 3 elements, 48 B and T + 16 B, on
          the vector and the element path;
  parts   run entries of k = 4 with unrelated part strides, a folded run,
          single messages between them;
  wide    the tables of shapes and parts on the WIDE kernels;
  batch   16 mixed entries with 1, 2, 3, 7 and `tiles` blocks, 17 segments
          (two launches), overlapping and interleaved extents (two launches
          each and the sequential result).

tests/test_strided_reduce_ref.py shows on the CPU that a byte-exact
comparison with this reference flags a subtly wrong walk.

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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "tools")
BINARY = os.path.join(TOOLS, "bin", "strided_reduce_kernels_check")
CHILD_TIMEOUT = 60  # s; guards against a hang, not a performance figure

GROUPS = ["edges", "shapes", "parts", "wide", "batch"]
TYPES = {"f32": 4, "f64": 8, "bf16": 2, "f16": 2, "i32": 4, "i64": 8}
OPS = ["sum", "max", "min"]
T = 16384

_dead = []  # why no further process may be started


def _blocks(want, tiles):
    out = []
    for b in want:
        b = min(tiles if b == 0 else b, tiles, 1024)
        if b not in out:
            out.append(b)
    return out


def _expected(group):
    """{(variant, table, blocks, launch): (tiles, entries, vec)} the group
    has to report; a table is (name, [(tiles, entries, vec) per launch],
    blocks), and blocks are resolved against the first launch"""
    tables = []
    width = "wide" if group == "wide" else "narrow"
    shapes = ("shapes", [(20, 10, 5)], [1, 2, 3, 0])
    parts = ("parts", [(8, 6, 3)], [1, 2, 3, 0])
    if group == "edges":
        for t, es in TYPES.items():
            sizes = [("1el", es), ("16", 16), ("T-16", T - 16), ("T", T),
                     ("T+16+1el", T + 16 + es), ("3T+odd", 3 * T + 1237 * es)]
            for op in OPS:
                for name, n in sizes:
                    tiles = -(-n // T)
                    tables.append((f"edges/{t}/{op}/{name}/run1el",
                                   [(tiles, 1, 0)], [1, 2, 0]))
                    tables.append((f"edges/{t}/{op}/{name}/run48",
                                   [(tiles, 1, int(n % 16 == 0))], [1, 2, 0]))
    elif group == "shapes":
        tables.append(shapes)
    elif group == "parts":
        tables.append(parts)
    elif group == "wide":
        tables += [shapes, parts]
    else:
        tables.append(("batch16", [(21, 16, 8)], [1, 2, 3, 7, 0]))
        tables.append(("batch17", [(16, 16, 0), (1, 1, 0)], [1, 0]))
        tables.append(("overlap", [(1, 1, 1), (2, 2, 2)], [1, 0]))
        tables.append(("interleaved", [(1, 1, 1), (1, 1, 1)], [1, 0]))
    want = {}
    for name, launches, blocks in tables:
        for v in (f"k_pull_strided_reduce_done<{width}>",
                  f"k_pull_strided_reduce<{width}>"):
            for b in _blocks(blocks, launches[0][0]):
                for i, row in enumerate(launches):
                    want[(v, name, b, i)] = row
    return want


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", TOOLS,
                        "bin/strided_reduce_kernels_check"],
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


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_strided_reduce_kernels_against_the_reference(group):
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
    got = [(r["variant"], r["table"], r["blocks"], r["launch"])
           for r in launches]
    assert sorted(got) == sorted(want), detail
    last = {}
    for r in launches:
        key = (r["variant"], r["table"], r["blocks"])
        last[key] = max(last.get(key, 0), r["launch"])
    for r in launches:
        key = (r["variant"], r["table"], r["blocks"], r["launch"])
        assert (r["tiles"], r["entries"], r["vec"]) == want[key], r
        assert r["first_bad"] is None, r
        # the arenas are compared behind the last launch of a case
        compared = r["launch"] == last[key[:3]]
        assert (r["bad"] is not None) == compared, r
        assert (r["src_bad"] is not None) == compared, r
    # one counter and one word for the whole process
    seq, word = 0, 0
    for r in launches:
        assert r["counter"] == 0, r
        assert r["word_before"] == word, r
        if r["seq"] is not None:  # by word
            assert r["seq"] == seq + 1, r
            seq = word = r["seq"]
        assert r["word"] == word, r
    by_word = [r for r in launches if r["seq"] is not None]
    assert len(by_word) == len(launches) // 2
    assert all("_done<" in r["variant"] for r in by_word)
    assert len(summary) == 1 and summary[0]["failed"] == 0, detail
    assert summary[0]["launches"] == len(want), detail
    print(f"{group}: {len(launches)} launches in {summary[0]['seconds']} s")
    assert run.returncode == 0, detail


def test_listing_needs_no_gpu_and_matches():
    """--list prints the same launches without touching the GPU: the plan of
    every case is what this file expects."""
    _ensure_built()
    for group in GROUPS:
        run = subprocess.run([BINARY, "--list", group], cwd=REPO,
                             capture_output=True, text=True, timeout=30)
        assert run.returncode == 0, run.stderr
        rows = [json.loads(l) for l in run.stdout.splitlines()
                if l.startswith("{") and "variant" in l]
        got = {(r["variant"], r["table"], r["blocks"], r["launch"]):
               (r["tiles"], r["entries"], r["vec"]) for r in rows}
        assert len(got) == len(rows)
        assert got == _expected(group)
