"""MPIX_FAST_WAIT=0 tier: the classic EQ protocol (COMPLETED is consumed by
the waiter, CLEANUP hands the slot back to the proxy).  Fast-wait is the
default, so the rest of the CPU suite runs the epoch protocol; this file is
the mirror of tests/test_fast_wait.py that keeps the classic state machine
covered: completion held in the slot until the wait, the proxy's
CLEANUP -> AVAILABLE leg, late orphaning, and a pool that really exhausts."""
import os

import numpy as np
import pytest

from conftest import run_ranks


def _init_classic(monkeypatch, nflags=None):
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("MPIX_FAST_WAIT", "0")
    if nflags is not None:
        monkeypatch.setenv("MPIX_NFLAGS", str(nflags))
    import mpix
    mpix.init()
    return mpix


@pytest.fixture
def mpix_classic(monkeypatch):
    mpix = _init_classic(monkeypatch)
    assert mpix.config()["nflags"] >= 64
    yield mpix
    mpix.finalize()


@pytest.fixture
def mpix_classic_256(monkeypatch):
    mpix = _init_classic(monkeypatch, 256)
    assert mpix.config()["nflags"] == 256
    yield mpix
    mpix.finalize()


@pytest.fixture
def mpix_classic_64(monkeypatch):
    """The smallest pool (64 is the enforced floor)."""
    mpix = _init_classic(monkeypatch, 64)
    assert mpix.config()["nflags"] == 64
    yield mpix
    mpix.finalize()


def test_classic_roundtrip_status(mpix_classic):
    mpix = mpix_classic
    src = np.arange(50, dtype=np.int32)
    dst = np.zeros(50, dtype=np.int32)
    rs = mpix.isend_enqueue(src, dest=0, tag=5)
    rr = mpix.irecv_enqueue(dst, source=0, tag=5)
    st = mpix.wait(rr)
    mpix.wait(rs)
    assert (dst == src).all()
    assert st["source"] == 0 and st["tag"] == 5 and st["count_bytes"] == 200


def test_classic_wait_after_completion(mpix_classic):
    """Late wait: a classic slot stays COMPLETED, with its status, until the
    wait consumes it, however much the rest of the pool churns meanwhile."""
    import time
    mpix = mpix_classic
    src = np.full(8, 9, dtype=np.int32)
    dst = np.zeros(8, dtype=np.int32)
    rs = mpix.isend_enqueue(src, dest=0, tag=6)
    rr = mpix.irecv_enqueue(dst, source=0, tag=6)
    time.sleep(0.05)  # let the proxy complete both
    for i in range(100):
        a = np.full(4, i, dtype=np.int32)
        b = np.zeros(4, dtype=np.int32)
        r1 = mpix.isend_enqueue(a, dest=0, tag=100 + i)
        r2 = mpix.irecv_enqueue(b, source=0, tag=100 + i)
        mpix.wait(r2)
        mpix.wait(r1)
        assert (b == i).all()
    st = mpix.wait(rr)
    mpix.wait(rs)
    assert (dst == 9).all()
    assert st["source"] == 0 and st["tag"] == 6 and st["count_bytes"] == 32


def test_classic_request_free_orphan(mpix_classic):
    mpix = mpix_classic
    src = np.arange(16, dtype=np.int32)
    dst = np.zeros(16, dtype=np.int32)
    rs = mpix.isend_enqueue(src, dest=0, tag=7)
    mpix.request_free(rs)  # never waited: proxy owns the cleanup
    rr = mpix.irecv_enqueue(dst, source=0, tag=7)
    mpix.wait(rr)
    assert (dst == src).all()


def test_classic_slot_recycling_many(mpix_classic_256):
    """3000 operations through 256 slots in batches of 64 pairs: every slot
    comes back more than ten times, each time through a wait."""
    mpix = mpix_classic_256
    n_ops = 3000
    batch = 64
    for b in range(0, n_ops, batch):
        reqs = []
        bufs = []
        for i in range(batch):
            tag = b + i
            a = np.full(4, tag, dtype=np.int32)
            d = np.zeros(4, dtype=np.int32)
            bufs.append((a, d, tag))
            reqs.append(mpix.isend_enqueue(a, dest=0, tag=tag))
            reqs.append(mpix.irecv_enqueue(d, source=0, tag=tag))
        for r in reqs:
            mpix.wait(r)
        for a, d, tag in bufs:
            assert (d == tag).all()


def test_classic_pool_exhaustion_and_recovery(mpix_classic_64):
    """tests/test_units.py::test_pool_exhaustion_and_recovery where the pool
    does exhaust: a classic send keeps its slot until it is waited, so the
    65th unmatched send must fail, cleanly, and the pool must be whole
    again after the drain."""
    mpix = mpix_classic_64
    n = 64
    bufs = [np.full(8, i, dtype=np.int32) for i in range(n)]
    reqs = []
    raised = False
    try:
        for i in range(n + 8):
            reqs.append(mpix.isend_enqueue(bufs[i % n], dest=0, tag=i))
    except RuntimeError:
        raised = True
    assert raised, "expected pool exhaustion error"
    assert len(reqs) == n
    # drain pair by pair (each wait frees its slot before the next alloc)
    for i, sr in enumerate(reqs):
        out = np.zeros(8, dtype=np.int32)
        mpix.wait(sr)  # buffered-send semantics: completes once staged
        rr = mpix.irecv_enqueue(out, source=0, tag=i)
        mpix.wait(rr)
        assert (out == i % n).all()
    # pool must be whole again: another full round succeeds
    reqs2 = [mpix.isend_enqueue(bufs[0], dest=0, tag=500 + i)
             for i in range(n // 2)]
    outs = [np.zeros(8, dtype=np.int32) for _ in range(n // 2)]
    rec2 = [mpix.irecv_enqueue(outs[i], source=0, tag=500 + i)
            for i in range(n // 2)]
    for r in reqs2 + rec2:
        mpix.wait(r)
    for out in outs:
        assert (out == 0).all()


def _classic_ring(rank, size):
    os.environ["MPIX_FAST_WAIT"] = "0"
    import mpix
    mpix.init()
    try:
        right = (rank + 1) % size
        left = (rank - 1 + size) % size
        for it in range(50):
            src = np.full(257, rank * 100 + it, dtype=np.int32)
            dst = np.zeros(257, dtype=np.int32)
            rs = mpix.isend_enqueue(src, dest=right, tag=it % 5)
            rr = mpix.irecv_enqueue(dst, source=left, tag=it % 5)
            st = mpix.wait(rr)
            mpix.wait(rs)
            assert (dst == left * 100 + it).all()
            assert st["source"] == left
    finally:
        mpix.finalize()


def test_classic_ring_2rank():
    run_ranks(2, _classic_ring)


def test_classic_ring_4rank():
    run_ranks(4, _classic_ring)
