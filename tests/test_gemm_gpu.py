"""The MFMA GEMM of bench/gemm_pready.hip, all five variants, against the
float64 reference of bench/gemm_check.h at the shapes where the kernels
branch: more than one tile row and column (the XCD remap, the grouped block
order with and without a tail group, the operand and C tile offsets), one,
two and an odd number of K-tiles, the prologue and guard branches of v5, the
minimum K of v6, and bands of one, two and four tile rows published from
inside the kernel.

Each case is `<binary> --check M N K nparts` (see run_check in the .hip
file): pass A checks all of C with publish off, pass B publishes and sends
the bands and checks C, Crecv (byte-identical to the sender's C) and the band
counters; both passes in `unit` mode (K <= 256, bit-exact) and in `uniform`
mode (|got - ref| <= 2^-8 |ref| + K 2^-23 S).  tests/test_gemm_check.py
shows on the CPU that this comparison catches a subtly wrong kernel.

Every case is a fresh child process with a time limit of its own.  The file
is chained: after a child that died on a signal or ran into its limit no
further child is started and the remaining cases fail at once with that
reason.  A child that merely reports bad elements does not stop the chain.
"""
import json
import os
import signal
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench")
MPIEXEC = "/opt/conda/bin/mpiexec"
CHILD_TIMEOUT = 60  # s; a case takes a few seconds

BINARIES = ["gemm_pready", "gemm_pready_v2", "gemm_pready_v3",
            "gemm_pready_v5", "gemm_pready_v6"]

# (binary, M, N, K, nparts, processes)
DEFAULT_CASES = [
    # v4: BM = BN = 256, BK = 64, G = 4
    ("gemm_pready", 256, 256, 64, 1, 1),    # one workgroup, one K-tile
    ("gemm_pready", 256, 256, 128, 1, 1),   # both buffers, last in buffer 1
    ("gemm_pready", 256, 256, 192, 1, 1),   # odd count, last in buffer 0
    ("gemm_pready", 256, 256, 512, 1, 1),   # the shape of a bare --check
    ("gemm_pready", 512, 768, 128, 2, 1),   # 2 x 3: tail group only, nwg 6
    ("gemm_pready", 512, 1280, 128, 2, 1),  # 2 x 5: group + tail 1, nwg 10
    ("gemm_pready", 512, 1280, 128, 1, 1),  # two tile rows in the band
    ("gemm_pready", 768, 1536, 64, 3, 1),   # 3 x 6: tail of 2, nwg 18
    ("gemm_pready", 768, 1024, 64, 3, 1),   # 3 x 4: no tail
    ("gemm_pready", 1024, 256, 64, 4, 1),   # one tile column
    ("gemm_pready", 1024, 256, 64, 2, 1),
    ("gemm_pready", 1024, 256, 64, 1, 1),
    # two processes on one GPU, the peer pulls the published bands
    ("gemm_pready", 512, 1280, 128, 2, 2),
]
ABLATION_CASES = [
    # v2: 128^2, BK = 32, B as [K][N]
    ("gemm_pready_v2", 128, 128, 32, 1, 1),
    ("gemm_pready_v2", 128, 128, 96, 1, 1),
    ("gemm_pready_v2", 256, 384, 64, 2, 1),
    # v3: 128^2, BK = 64, B as [K][N], register prefetch
    ("gemm_pready_v3", 128, 128, 64, 1, 1),
    ("gemm_pready_v3", 128, 128, 192, 1, 1),
    ("gemm_pready_v3", 256, 384, 128, 2, 1),
    # v5: 256^2, BK = 32, four buffers: 1 to 5 K-tiles take every branch of
    # the prologue (tiles > 1, tiles > 2) and of t + 2, t + 3 < tiles
    ("gemm_pready_v5", 256, 256, 32, 1, 1),
    ("gemm_pready_v5", 256, 256, 64, 1, 1),
    ("gemm_pready_v5", 256, 256, 96, 1, 1),
    ("gemm_pready_v5", 256, 256, 128, 1, 1),
    ("gemm_pready_v5", 256, 256, 160, 1, 1),
    ("gemm_pready_v5", 512, 768, 96, 2, 1),
    # v6: 256^2, BK = 64, K-tiles in pairs, at least two pairs
    ("gemm_pready_v6", 256, 256, 256, 1, 1),
    ("gemm_pready_v6", 256, 256, 384, 1, 1),
    ("gemm_pready_v6", 512, 768, 256, 2, 1),
]
CASES = DEFAULT_CASES + ABLATION_CASES
VARIANT = {"gemm_pready": 4, "gemm_pready_v2": 2, "gemm_pready_v3": 3,
           "gemm_pready_v5": 5, "gemm_pready_v6": 6}

_dead = []  # why no further process may be started


def _case_id(case):
    binary, m, n, k, nparts, procs = case
    name = "v%d-%dx%dx%d-p%d" % (VARIANT[binary], m, n, k, nparts)
    return name + ("-np%d" % procs if procs > 1 else "")


def _ensure_built():
    missing = ["bin/" + b for b in BINARIES
               if not os.path.exists(os.path.join(BENCH, "bin", b))]
    if missing:
        if not os.path.exists(os.path.join(REPO, "libmpix.so")):
            subprocess.run(["make", "-j8", "libmpix.so"], cwd=REPO,
                           check=True, capture_output=True)
        subprocess.run(["make", "-C", BENCH, "-j4"] + missing, check=True,
                       capture_output=True)


def _run(binary, args, procs=1):
    """One child under its own limit.  Returns the completed process, or
    fails the test (and every later one) if the child died on a signal or
    ran into the limit."""
    _ensure_built()
    if _dead:
        pytest.fail("not started: " + _dead[0])
    cmd = [os.path.join(BENCH, "bin", binary), "--check"] + [str(a)
                                                             for a in args]
    if procs > 1:
        assert os.path.exists(MPIEXEC), "mpiexec not found"
        cmd = [MPIEXEC, "-np", str(procs)] + cmd
    env = {**os.environ, "PATH": "/opt/conda/bin:" + os.environ["PATH"]}
    what = " ".join(cmd[-(len(args) + 2):])
    try:
        run = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                             text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout
        _dead.append(f"{what} ran into its limit of {CHILD_TIMEOUT} s (a "
                     f"band never published?); output so far:\n{out}")
        pytest.fail(_dead[0])
    # a signal: negative from a direct child; mpiexec reports 128 + signal
    rc = run.returncode
    sig = -rc if rc < 0 else rc - 128 if rc > 128 else 0
    if sig:
        try:
            name = signal.Signals(sig).name
        except ValueError:
            name = "signal %d" % sig
        _dead.append(f"{what} died on {name} (exit {rc}):\n"
                     f"{run.stdout[-2000:]}\n{run.stderr[-4000:]}")
        pytest.fail(_dead[0])
    return run


def _passes(stdout):
    out = []
    for line in stdout.splitlines():
        if line.startswith('{"check": "gemm_pready"'):
            out.append(json.loads(line))
    return out


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_gemm_against_float64(case):
    binary, m, n, k, nparts, procs = case
    run = _run(binary, [m, n, k, nparts], procs)
    passes = _passes(run.stdout)
    for p in passes:
        print(json.dumps(p))
    detail = f"exit {run.returncode}\n{run.stdout}\n{run.stderr[-4000:]}"
    # every rank reports pass A and pass B in each data mode
    modes = ["unit", "uniform"] if k <= 256 else ["uniform"]
    want = sorted((r, mode, ab) for r in range(procs) for mode in modes
                  for ab in "AB")
    assert sorted((p["rank"], p["mode"], p["pass"]) for p in passes) == want, \
        detail
    for p in passes:
        assert p["variant"] == VARIANT[binary], detail
        assert p["mnk"] == [m, n, k] and p["nparts"] == nparts, detail
        assert p["ranks"] == procs, detail
        assert not p["refused"], detail
        assert p["bad"] == 0 and p["first_bad"] is None, detail
        assert p["recv_bad"] == 0 and p["recv_identical"], detail
        assert p["bands_ok"] and p["guards_ok"], detail
        if p["mode"] == "unit":
            assert p["worst"] == 0 and p["recv_worst"] == 0, detail
        else:
            assert p["worst"] <= 1.0 and p["recv_worst"] <= 1.0, detail
        assert p["ok"], detail
    assert run.returncode == 0, detail


def test_bare_check_is_256_256_512():
    run = _run("gemm_pready", [])
    passes = _passes(run.stdout)
    detail = f"exit {run.returncode}\n{run.stdout}\n{run.stderr[-4000:]}"
    assert [(p["mode"], p["pass"]) for p in passes] == \
        [("uniform", "A"), ("uniform", "B")], detail
    for p in passes:
        assert p["mnk"] == [256, 256, 512] and p["nparts"] == 1, detail
        assert p["ok"] and p["bad"] == 0 and p["worst"] <= 1.0, detail
    assert run.returncode == 0, detail


def test_v6_refuses_a_k_below_two_pairs():
    """K = 128 is two K-tiles; v6's schedule needs two pairs.  main refuses
    it before anything is launched."""
    run = _run("gemm_pready_v6", [256, 256, 128, 1])
    assert run.returncode not in (0, None), run.stdout
    assert "FAILED: K % (2 * BK) == 0 && K >= 4 * BK" in run.stderr, \
        run.stderr[-2000:]
    assert _passes(run.stdout) == [], run.stdout
