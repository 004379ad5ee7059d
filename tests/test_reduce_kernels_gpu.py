"""The reduce kernels of src/transport/pull_kernels.h (k_pull_reduce, which
stores nontemporal, and k_pull_reduce_done, which stores write-through and
signals the completion word) against reduce_host of src/transport/reduce.h,
byte for byte, launched directly by tests/native/reduce_kernels_check.hip
with block counts the runtime never picks.

The harness (tools/bin/reduce_kernels_check GROUP) plans with plan_reduce,
launches with launch_reduce, compares the whole destination arena and a guard
page behind it, checks that the source is unchanged, and prints one JSON line
per launch.  One completion counter and one word serve all by-word launches
of a process: after each the counter reads 0 and the word that launch's
number.  Groups:

  edges  all 18 type/op pairs x entries of 1 element, 16 B - 1 element, 16 B,
         T - 16, T, T + 16 + 1 element, 3T + an odd number of elements
         (T = 16 KiB), each with 1, 2 and `tiles` blocks;
  paths  one table mixing all six types and three ops; one with a side of
         every entry offset by one element (the element path);
  full   64 segments, 8 of them one merged run.

tests/test_reduce_ref.py shows on the CPU that a byte-exact comparison with
this reference flags a subtly wrong combine.

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
BINARY = os.path.join(TOOLS, "bin", "reduce_kernels_check")
CHILD_TIMEOUT = 60  # s; guards against a hang, not a performance figure

GROUPS = ["edges", "paths", "full"]
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
    """{(variant, table, blocks): (tiles, entries)} the group has to report"""
    tables = []
    if group == "edges":
        for t, es in TYPES.items():
            sizes = [("1el", es), ("16-1el", 16 - es), ("16", 16),
                     ("T-16", T - 16), ("T", T), ("T+16+1el", T + 16 + es),
                     ("3T+odd", 3 * T + 1237 * es)]
            for op in OPS:
                for name, n in sizes:
                    tables.append((f"edges/{t}/{op}/{name}", -(-n // T), 1,
                                   [1, 2, 0]))
    elif group == "paths":
        tables.append(("mixed_types", 20, 18, [1, 2, 3, 0]))
        tables.append(("offset_by_one_element", 42, 24, [1, 2, 3, 0]))
    else:
        tables.append(("full_table", 66, 57, [1, 2, 3, 7, 0]))
    want = {}
    for name, tiles, entries, blocks in tables:
        for v in ("k_pull_reduce_done", "k_pull_reduce"):
            for b in _blocks(blocks, tiles):
                want[(v, name, b)] = (tiles, entries)
    return want


def _ensure_built():
    if not os.path.exists(BINARY):
        subprocess.run(["make", "-C", TOOLS, "bin/reduce_kernels_check"],
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
def test_reduce_kernels_against_reduce_host(group):
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
        assert (r["tiles"], r["entries"]) == \
            want[(r["variant"], r["table"], r["blocks"])], r
        assert r["first_bad"] is None, r
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
    assert all(r["variant"] == "k_pull_reduce_done" for r in by_word)
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
        got = {(r["variant"], r["table"], r["blocks"]):
               (r["tiles"], r["entries"]) for r in rows}
        assert got == _expected(group)
