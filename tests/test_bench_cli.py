"""bench.py command line: a plain run times only the Psend headline, --full
adds the ping-pong side measurement, --dump-outputs writes reproducible
float64 arrays.  Tiny sizes; runs on whatever device the box has (host
buffers without a GPU — same code paths)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", "--msg-mib", "1", *extra],
        capture_output=True, text=True, timeout=120,
        env={**os.environ, "RANK": "0", "WORLD_SIZE": "1"})
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout  # ONE result line
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_dump")
    plain = _bench("--dump-outputs", str(d / "a"))
    full = _bench("--full", "--pp-iters", "5", "--dump-outputs", str(d / "b"))
    return plain, full, d


def test_result_line_fields(runs):
    for res in runs[:2]:
        for k in KEYS:
            assert k in res
        assert res["steps"] == 3 and res["warmup"] == 1
        assert res["unit"] == "GB/s" and res["higher_is_better"] is True
        assert res["dtype"] == "int32"
        assert res["ms_per_step"] > 0
        # value and ms_per_step describe the same timed steps
        gbps = (1 << 20) / (res["ms_per_step"] * 1e-3) / 1e9
        assert res["value"] == pytest.approx(gbps, rel=0.02)


def test_side_measurements_only_with_full(runs):
    plain, full, _ = runs
    assert plain["full"] is False
    assert plain["config"]["pingpong_half_rtt_us"] is None
    assert full["full"] is True
    assert full["config"]["pingpong_half_rtt_us"] > 0


def test_steps_sets_the_number_of_timed_steps(monkeypatch, capsys):
    """Count the partitioned starts between the two clock reads that bracket
    the timed window: a step starts one receive and one send."""
    import types
    import time as real_time
    sys.path.insert(0, REPO)
    import bench
    import mpix
    starts, at_clock = [0], []
    real_start = mpix.start

    def counting_start(req):
        starts[0] += 1
        real_start(req)

    def clock():
        at_clock.append(starts[0])
        return real_time.perf_counter()

    monkeypatch.setattr(mpix, "start", counting_start)
    monkeypatch.setattr(bench, "time",
                        types.SimpleNamespace(perf_counter=clock))
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "4", "--warmup",
                                      "2", "--msg-mib", "1", "--no-pin"])
    bench.main()
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(at_clock) == 2  # a plain run times nothing but the steps
    assert at_clock[0] == 2 * 2  # warmup steps came before the window
    assert at_clock[1] - at_clock[0] == 2 * 4
    assert starts[0] == at_clock[1]  # and nothing ran after it
    assert res["steps"] == 4


def _fake_sysfs(root, node_of_gpu):
    """Two NUMA nodes x two L3 groups of 4 CPUs; GPU 0000:05:00.0."""
    def put(rel, text):
        f = root / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text + "\n")
    put("bus/pci/devices/0000:05:00.0/numa_node", str(node_of_gpu))
    put("devices/system/node/node0/cpulist", "0-7")
    put("devices/system/node/node1/cpulist", "8-15")
    for c in range(16):
        lo = c // 4 * 4
        put(f"devices/system/cpu/cpu{c}/cache/index3/shared_cpu_list",
            f"{lo}-{lo + 3}")
    return str(root)


def test_choose_cpus(tmp_path):
    sys.path.insert(0, REPO)
    from bench import choose_cpus
    gpu, every = "0000:05:00.0", set(range(16))
    near = _fake_sysfs(tmp_path / "near", 1)
    # one L3 group on the GPU's node; ranks take successive groups
    assert choose_cpus(gpu, 0, every, near) == {8, 9, 10, 11}
    assert choose_cpus(gpu, 1, every, near) == {12, 13, 14, 15}
    assert choose_cpus(gpu, 2, every, near) == {8, 9, 10, 11}
    # never a CPU outside the allowed set
    assert choose_cpus(gpu, 0, {9, 10, 13, 14}, near) == {9, 10}
    # node unknown (-1), GPU absent from sysfs, or no GPU: all allowed CPUs,
    # and ranks are still spread over the groups
    unknown = _fake_sysfs(tmp_path / "unknown", -1)
    for addr in (gpu, "0000:99:00.0", None):
        got = [choose_cpus(addr, r, every, unknown) for r in range(4)]
        assert got == [{0, 1, 2, 3}, {4, 5, 6, 7}, {8, 9, 10, 11},
                       {12, 13, 14, 15}]
    # a host that describes no L3: nothing to choose
    assert choose_cpus(gpu, 0, every, str(tmp_path / "empty")) is None


def test_pin_to_one_cache_reaches_later_threads_only(monkeypatch):
    """The mask must narrow for the caller and for threads started after
    (the mpix proxy), not for threads that already run."""
    import threading
    sys.path.insert(0, REPO)
    import bench
    before = os.sched_getaffinity(0)
    want = set(sorted(before)[:2]) if len(before) > 2 else set(before)
    monkeypatch.setattr(bench, "choose_cpus", lambda *a, **k: want)
    stop, masks = threading.Event(), {}
    ready = threading.Event()

    def early():
        masks["early_tid"] = threading.get_native_id()
        ready.set()
        stop.wait(30)

    t = threading.Thread(target=early)
    t.start()
    ready.wait(30)
    try:
        assert bench.pin_to_one_cache(None, 0) == want
        assert os.sched_getaffinity(0) == want
        assert os.sched_getaffinity(masks["early_tid"]) == before
        late = threading.Thread(target=lambda: masks.__setitem__(
            "late", os.sched_getaffinity(0)))
        late.start()
        late.join()
        assert masks["late"] == want
    finally:
        stop.set()
        t.join()
        os.sched_setaffinity(0, before)
    # no topology: the mask is left alone
    monkeypatch.setattr(bench, "choose_cpus", lambda *a, **k: None)
    assert bench.pin_to_one_cache(None, 0) is None
    assert os.sched_getaffinity(0) == before


def test_pinning_reported_and_optional(runs):
    """The result line says how many CPUs the host threads were confined
    to: exactly what choose_cpus gives for this host, null with --no-pin."""
    sys.path.insert(0, REPO)
    from bench import choose_cpus
    if runs[0]["config"]["trigger"].startswith("host"):  # no GPU: no address
        want = choose_cpus(None, 0, os.sched_getaffinity(0))
        assert runs[0]["config"]["host_cpus"] == (len(want) if want else None)
    else:
        assert runs[0]["config"]["host_cpus"] >= 2
    assert _bench("--no-pin")["config"]["host_cpus"] is None


def test_dump_outputs_are_the_seeded_payload(runs):
    """Loopback at one rank must deliver rank 0's send buffer: the reference
    is drawn here from the documented seed, not taken from another run."""
    import torch
    sys.path.insert(0, REPO)
    import bench
    _, _, d = runs
    n = (1 << 20) // 4
    gen = torch.Generator().manual_seed(bench.PAYLOAD_SEED)
    want = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32,
                         generator=gen).numpy().astype(np.float64)
    for sub in ("a", "b"):  # plain run and --full run
        got = np.load(d / sub / "recv.npy")
        assert got.dtype == np.float64 and got.shape == (n,)
        assert np.array_equal(got, want)
    assert np.count_nonzero(want) > n * 0.99  # a payload worth comparing


def test_dump_sampling_is_fixed_and_bounded(tmp_path):
    import torch
    sys.path.insert(0, REPO)
    import bench
    n, parts = 1 << 16, 8
    out = torch.arange(n, dtype=torch.int32)
    limit = bench.DUMP_BUDGET_BYTES // 8
    try:
        bench.DUMP_BUDGET_BYTES = 8 * 1024  # force the sampled path
        bench.dump_outputs(str(tmp_path), "x", out, parts, 1)
        bench.dump_outputs(str(tmp_path), "y", out, parts, 1)
        x, y = np.load(tmp_path / "x.npy"), np.load(tmp_path / "y.npy")
    finally:
        bench.DUMP_BUDGET_BYTES = limit * 8
    assert np.array_equal(x, y) and x.dtype == np.float64
    assert x.size <= 1024 and np.all(np.diff(x) > 0)
    per = n // parts
    edges = {p * per for p in range(parts)} | {p * per + per - 1
                                               for p in range(parts)}
    assert edges <= set(x.astype(np.int64).tolist())
