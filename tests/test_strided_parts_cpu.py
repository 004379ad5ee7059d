"""Partitioned transfers with layouts between host buffers (the CPU tier):
non-contiguous numpy views as partitioned buffers, split along dimension 0.

Partition p of a view is view[p * rows:(p + 1) * rows] and its message is
that slab in C order, so the expected bytes of the whole transfer are
numpy.ascontiguousarray of the sent view.  Every case runs 2 iterations on
the same requests with a fresh payload, every destination is a view into a
sentinel-filled array whose other bytes must survive, and parrived comes to
report true for every partition.  All comparisons are exact.
"""
import time

import numpy as np
import pytest

SENT = 0xA5


def pattern(shape, dtype=np.float32, start=0):
    """Position-dependent values: element i of the base array is start + i."""
    n = int(np.prod(shape))
    return (np.arange(n, dtype=np.int64) + start).astype(dtype).reshape(shape)


def sentinel(shape, dtype=np.float32):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8).fill(SENT)
    return a


def gaps_intact(base, view):
    """Every byte of `base` outside `view` still holds the sentinel."""
    item = base.itemsize
    flat = np.zeros(base.size, dtype=bool)
    off = (view.__array_interface__["data"][0]
           - base.__array_interface__["data"][0]) // item
    marks = np.lib.stride_tricks.as_strided(
        flat[off:], shape=view.shape,
        strides=tuple(s // item for s in view.strides))
    marks[...] = True
    raw = base.reshape(-1).view(np.uint8).reshape(-1, item)
    return bool((raw[~flat] == SENT).all())


def exchange(mpix, src_base, src, dst_base, dst, parts, tag, order=None):
    """2 iterations src -> dst (loopback) on one pair of requests.  `src` and
    `dst` are views of src_base / dst_base (or those arrays themselves)."""
    ps = mpix.psend_init(src, parts, dest=0, tag=tag)
    pr = mpix.precv_init(dst, parts, source=0, tag=tag)
    try:
        for it in range(2):
            src_base[...] = pattern(src_base.shape, src_base.dtype,
                                    start=1000 * it + 1)
            dst_base.view(np.uint8).fill(SENT)
            mpix.start(pr)
            mpix.start(ps)
            for p in (order or range(parts)):
                mpix.pready(p, ps)
            # MPIX_Wait takes every partition flag back to RESERVED (the
            # flag lifecycle in src/partitioned.cpp), so parrived is asked
            # before it: every partition must come to report true
            deadline = time.monotonic() + 60
            arrived = [False] * parts
            while not all(arrived) and time.monotonic() < deadline:
                for p in range(parts):
                    arrived[p] = arrived[p] or mpix.parrived(pr, p)
            assert all(arrived), f"parrived {arrived}, iter {it}"
            st = mpix.wait(pr)
            mpix.wait(ps)
            assert st["error"] == 0
            assert st["count_bytes"] == src.nbytes
            want = np.ascontiguousarray(src).reshape(-1)
            got = np.ascontiguousarray(dst).reshape(-1)
            assert want.tobytes() == got.tobytes(), f"payload, iter {it}"
            if dst is not dst_base:
                assert gaps_intact(dst_base, dst), f"gaps, iter {it}"
    finally:
        mpix.request_free(ps)
        mpix.request_free(pr)


def test_yface_to_contiguous(mpix_env):
    grid = np.zeros((8, 5, 6), dtype=np.float32)
    face = grid[:, 0, :]
    assert not face.flags["C_CONTIGUOUS"]
    recv = sentinel((8, 6))
    exchange(mpix_env, grid, face, recv, recv, 4, tag=1)
    # the other faces of the same grid, other partition counts and orders
    recv2 = sentinel((8, 6))
    exchange(mpix_env, grid, grid[:, 3, :], recv2, recv2, 8, tag=2,
             order=[7, 0, 3, 4, 1, 6, 2, 5])
    recv3 = sentinel((8, 5))
    exchange(mpix_env, grid, grid[:, :, 2], recv3, recv3, 2, tag=3)
    recv4 = sentinel((8, 3, 2))
    exchange(mpix_env, grid, grid[:, 1:4, 2:4], recv4, recv4, 1, tag=4)


def test_contiguous_into_strided_view(mpix_env):
    send = np.zeros((8, 6), dtype=np.float32)
    base = sentinel((8, 5, 6))
    view = base[:, 2, :]
    exchange(mpix_env, send, send, base, view, 4, tag=5)
    # two strided levels inside one partition
    send2 = np.zeros((4, 3, 2), dtype=np.int16)
    base2 = sentinel((4, 5, 7), np.int16)
    exchange(mpix_env, send2, send2, base2, base2[:, 1:4, 3:5], 4, tag=6,
             order=[3, 2, 1, 0])


def test_rows_of_a_padded_array(mpix_env):
    """Contiguous rows with a gap between them: the partition layout comes
    out contiguous, the part stride is the pitch."""
    src_base = np.zeros((8, 70), dtype=np.float32)
    rows = src_base[:, :64]
    dst_base = sentinel((8, 96))
    exchange(mpix_env, src_base, rows, dst_base, dst_base[:, 16:80], 8, tag=7)
    # two rows per partition on one side, four on the other
    recv = sentinel((8, 64))
    exchange(mpix_env, src_base, rows, recv, recv, 4, tag=8)
    exchange(mpix_env, src_base, rows, dst_base, dst_base[:, 16:80], 2, tag=9)


def test_strided_to_differently_strided(mpix_env):
    """Only the byte sequence of a partition has to agree."""
    src_base = np.zeros((4, 9), dtype=np.int16)
    src = src_base[:, 2:8]            # 4 partitions of 12 B in one run
    dst_base = sentinel((4, 3, 10), np.int16)
    dst = dst_base[:, :, 4:6]         # 4 partitions of 3 runs of 4 B
    exchange(mpix_env, src_base, src, dst_base, dst, 4, tag=10)


def test_errors(mpix_env):
    mpix = mpix_env
    grid = pattern((8, 5, 6))
    face = grid[:, 0, :]
    with pytest.raises(ValueError, match="dimension 0"):
        mpix.psend_init(face, 3, dest=0, tag=20)
    with pytest.raises(ValueError, match="dimension 0"):
        mpix.precv_init(face, 16, source=0, tag=20)
    # flipped: along the partition dimension and inside a partition
    with pytest.raises(ValueError, match="negative strides"):
        mpix.psend_init(grid[::-1, 0, :], 4, dest=0, tag=20)
    with pytest.raises(ValueError, match="negative strides"):
        mpix.psend_init(grid[::-1, 0, :], 8, dest=0, tag=20)
    with pytest.raises(ValueError, match="negative strides"):
        mpix.precv_init(grid[:, 0, ::-1], 4, source=0, tag=20)
    with pytest.raises(ValueError, match="nbytes"):
        mpix.psend_init(face, 4, dest=0, tag=20, nbytes=face.nbytes)
    # more than a run plus two levels inside one partition
    cube = pattern((4, 4, 4, 8))
    with pytest.raises(ValueError, match=r"\(2, 2, 2, 2\)"):
        mpix.psend_init(cube[:, :2, :2, :2], 2, dest=0, tag=20)
    # the same view fits when every slab is one partition
    r = mpix.psend_init(cube[:, :2, :2, :2], 4, dest=0, tag=20)
    mpix.request_free(r)


def test_overlapping_partitions_rejected(mpix_env):
    """MPI_ERR_ARG (12) from the C call: a part stride below the layout's
    extent."""
    from mpix import _C
    buf = np.zeros(4096, dtype=np.uint8)
    addr = buf.ctypes.data
    # 4 runs of 16 B, 32 apart: extent 112
    for is_send in (True, False):
        with pytest.raises(RuntimeError, match="rc=12"):
            _C.psend_precv_init_strided(is_send, addr, 4, 16, 4, 1, 32, 128,
                                        111, 0, 21)
        with pytest.raises(RuntimeError, match="rc=12"):
            _C.psend_precv_init_strided(is_send, addr, 4, 16, 4, 1, 32, 128,
                                        0, 0, 21)
        with pytest.raises(RuntimeError, match="rc=12"):
            _C.psend_precv_init_strided(is_send, addr, 4, 16, 4, 1, 32, 128,
                                        -128, 0, 21)
        # an illegal layout (stride below the run) and an overflowing whole
        with pytest.raises(RuntimeError, match="rc=12"):
            _C.psend_precv_init_strided(is_send, addr, 4, 16, 4, 1, 8, 128,
                                        128, 0, 21)
        with pytest.raises(RuntimeError, match="rc=12"):
            _C.psend_precv_init_strided(is_send, addr, 4, 16, 4, 1, 32, 128,
                                        1 << 62, 0, 21)
    # exactly the extent is legal, and one partition needs no stride at all
    r = _C.psend_precv_init_strided(True, addr, 4, 16, 4, 1, 32, 128, 112, 0,
                                    21)
    mpix_env.request_free(r)
    r = _C.psend_precv_init_strided(False, addr, 1, 16, 4, 1, 32, 128, 0, 0,
                                    21)
    mpix_env.request_free(r)
