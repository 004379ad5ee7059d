"""Strided transfers between host buffers (the CPU tier): non-contiguous numpy
views go out and come in without packing by the caller.

The expected bytes are numpy.ascontiguousarray of the sent view.  Every
destination is a view into a sentinel-filled array whose other bytes must
survive.  All comparisons are exact.
"""
import numpy as np
import pytest

from conftest import run_ranks

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
    # the view's elements, marked through an identically-strided bool view
    marks = np.lib.stride_tricks.as_strided(
        flat[off:], shape=view.shape,
        strides=tuple(s // item for s in view.strides))
    marks[...] = True
    raw = base.reshape(-1).view(np.uint8).reshape(-1, item)
    return bool((raw[~flat] == SENT).all())


def xfer(mpix, src, dst, tag, send_first=False):
    """One loopback message src -> dst; returns the receive status."""
    if send_first:
        rs = mpix.isend_enqueue(src, dest=0, tag=tag)
        mpix.wait(rs)  # buffered: completes with no receive posted
        rr = mpix.irecv_enqueue(dst, source=0, tag=tag)
        return mpix.wait(rr)
    rr = mpix.irecv_enqueue(dst, source=0, tag=tag)
    rs = mpix.isend_enqueue(src, dest=0, tag=tag)
    st = mpix.wait(rr)
    mpix.wait(rs)
    return st


def test_strided_to_contiguous(mpix_env):
    grid = pattern((6, 5, 8))
    for tag, view in enumerate([grid[:, :, 3], grid[:, 2, :], grid[1:5, 1:4, 2:6],
                                grid[:, :, 1:3]]):
        assert not view.flags["C_CONTIGUOUS"]
        want = np.ascontiguousarray(view)
        recv = np.zeros(view.shape, dtype=grid.dtype)
        st = xfer(mpix_env, view, recv, tag)
        assert st["error"] == 0 and st["count_bytes"] == want.nbytes
        assert np.array_equal(recv, want)


def test_contiguous_to_strided(mpix_env):
    send = pattern((6, 5))
    base = sentinel((6, 5, 8))
    view = base[:, :, 7]  # z-face: 4-byte runs
    st = xfer(mpix_env, send, view, 1)
    assert st["error"] == 0 and st["count_bytes"] == send.nbytes
    assert np.array_equal(view, send)
    assert gaps_intact(base, view)


def test_strided_to_strided_different_shapes(mpix_env):
    """(4, 6) elements out of a (4, 9) array into a (3, 8) block of a
    (5, 3, 10) array: only the byte sequence agrees."""
    src = pattern((4, 9), np.int16)[:, 2:8]
    base = sentinel((5, 3, 10), np.int16)
    view = base[1, :, 1:9]
    assert src.size == view.size
    st = xfer(mpix_env, src, view, 2)
    assert st["error"] == 0 and st["count_bytes"] == src.nbytes
    assert np.array_equal(view.reshape(-1), np.ascontiguousarray(src).reshape(-1))
    assert gaps_intact(base, view)
    # two strided levels on both sides
    src3 = pattern((4, 8, 96), np.uint8)[:3, :5, :64]
    base3 = sentinel((6, 6, 80), np.uint8)
    view3 = base3[1:4, 1:6, 8:72]
    xfer(mpix_env, src3, view3, 3)
    assert np.array_equal(view3, src3)
    assert gaps_intact(base3, view3)


@pytest.mark.parametrize("send_first", [False, True],
                         ids=["posted", "unexpected"])
def test_runs_straddle_chunks(mpix_env, send_first):
    """120000 B in 400-byte runs: the 64 KiB stage chunks start and end in
    the middle of runs on both sides."""
    src = pattern((300, 128))[:, :100]
    base = sentinel((300, 112))
    view = base[:, 6:106]
    st = xfer(mpix_env, src, view, 4, send_first=send_first)
    assert st["error"] == 0 and st["count_bytes"] == 120000
    assert np.array_equal(view, src)
    assert gaps_intact(base, view)


def test_unexpected_small(mpix_env):
    src = pattern((6, 5, 8))[:, 1, :]
    base = sentinel((6, 3, 8))
    view = base[:, 2, :]
    xfer(mpix_env, src, view, 5, send_first=True)
    assert np.array_equal(view, src)
    assert gaps_intact(base, view)


def test_truncation(mpix_env):
    """The first recv_total message bytes are delivered, status says
    truncated."""
    src = pattern((10, 8))[:, :4]          # 160 B in 16-byte runs
    base = sentinel((3, 16))
    view = base[:, 4:12]                   # room for 96 B in 32-byte runs
    st = xfer(mpix_env, src, view, 6)
    assert st["error"] != 0
    assert st["count_bytes"] == 96
    want = np.ascontiguousarray(src).reshape(-1)[:24]
    assert np.array_equal(view.reshape(-1), want)
    assert gaps_intact(base, view)
    # and a short message into a larger strided receive
    base2 = sentinel((10, 8))
    view2 = base2[:, :4]
    short = pattern((6,), start=500)
    st = xfer(mpix_env, short, view2, 7)
    assert st["error"] == 0 and st["count_bytes"] == 24
    got = base2.copy()
    assert np.array_equal(got[0, :4], short[:4])
    assert np.array_equal(got[1, :2], short[4:])
    marked = sentinel((10, 8))
    marked[0, :4] = short[:4]
    marked[1, :2] = short[4:]
    assert np.array_equal(base2.view(np.uint8), marked.view(np.uint8))


def test_rejected_views(mpix_env):
    mpix = mpix_env
    torch = pytest.importorskip("torch")
    row = torch.arange(8, dtype=torch.float32)
    for bad in (row.expand(4, 8),                       # zero stride
                np.arange(12, dtype=np.int32)[::-1],    # flipped
                np.flip(pattern((4, 6)), axis=1),
                pattern((4, 6)).T,                      # steps backwards
                pattern((4, 4, 4, 4))[:, :2, :2, :2]):  # three strided levels
        with pytest.raises(ValueError, match="shape"):
            mpix.isend_enqueue(bad, dest=0, tag=8)
        with pytest.raises(ValueError, match="shape"):
            mpix.irecv_enqueue(bad, source=0, tag=8)
    with pytest.raises(ValueError, match="nbytes"):
        mpix.isend_enqueue(pattern((4, 6))[:, :3], dest=0, tag=8, nbytes=16)


def test_c_layout_validation(mpix_env):
    """The C entry points validate on their own (MPI_ERR_ARG): overlap, zero
    and negative strides, overflowing sizes.  Nothing is enqueued."""
    mpix = mpix_env
    buf = np.zeros(64, dtype=np.uint8)
    addr = buf.ctypes.data
    bad = [(4, 3, 1, 2, 0),            # runs overlap
           (4, 3, 1, 0, 0),            # zero stride
           (4, 3, 1, -8, 0),           # negative stride
           (4, 3, 2, 8, 16),           # planes overlap (need >= 20)
           (1 << 32, 1 << 32, 1, 1 << 32, 0)]  # size overflows
    for run, c0, c1, s0, s1 in bad:
        for is_send in (True, False):
            with pytest.raises(RuntimeError, match="strided_enqueue failed"):
                mpix._C.sendrecv_strided(is_send, addr, run, c0, c1, s0, s1,
                                         0, 13, mpix.QUEUE_STREAM, 0)
    # a legal one right after: the pool is untouched
    recv = np.zeros(12, dtype=np.uint8)
    buf[:] = np.arange(64, dtype=np.uint8)
    rr = mpix.irecv_enqueue(recv, source=0, tag=13)
    rs = mpix._C.sendrecv_strided(True, addr, 4, 3, 1, 8, 0, 0, 13,
                                  mpix.QUEUE_STREAM, 0)
    mpix.wait(rr)
    mpix.wait(rs)
    assert recv.tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19]


def test_torch_cpu_view(mpix_env):
    torch = pytest.importorskip("torch")
    grid = torch.arange(6 * 5 * 8, dtype=torch.float32).reshape(6, 5, 8)
    view = grid[:, :, 0]
    recv = torch.zeros(6, 5)
    st = xfer(mpix_env, view, recv, 9)
    assert st["count_bytes"] == 120
    assert torch.equal(recv, view)


def test_contiguous_in_disguise(mpix_env):
    """A view with a size-1 dimension of odd stride is contiguous memory: it
    takes the plain path (either way the bytes must be right)."""
    base = pattern((4, 6))
    view = base[1:2, :]
    recv = np.zeros((1, 6), dtype=base.dtype)
    xfer(mpix_env, view, recv, 10)
    assert np.array_equal(recv, view)
    col = np.lib.stride_tricks.as_strided(base, shape=(1, 6), strides=(4, 4))
    xfer(mpix_env, col, recv, 11)
    assert np.array_equal(recv, base[:1, :])


def test_graph_construction_variant(mpix_env):
    """isend_graph / irecv_graph take views too.  Graph queues need a GPU:
    without one the strided entry point must refuse like the plain one."""
    mpix = mpix_env
    src = pattern((6, 8))[:, 2:5]
    base = sentinel((6, 8))
    view = base[:, 1:4]
    if not mpix.config()["have_gpu"]:
        with pytest.raises(RuntimeError, match="strided_enqueue"):
            mpix.isend_graph(src, dest=0, tag=12)
        with pytest.raises(RuntimeError, match="strided_enqueue"):
            mpix.irecv_graph(view, source=0, tag=12)
        return
    import torch
    rr, g_recv = mpix.irecv_graph(view, source=0, tag=12)
    rs, g_send = mpix.isend_graph(src, dest=0, tag=12)
    g_wait = mpix.waitall_graph([rr, rs])
    parent, exe = mpix.graph_chain_instantiate([g_recv, g_send, g_wait])
    stream = torch.cuda.current_stream()
    mpix.graph_launch(exe, stream.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(view, src)
    assert gaps_intact(base, view)
    mpix.graph_exec_destroy(exe)
    mpix.graph_destroy(parent)


def _two_rank_exchange(rank, world):
    import numpy as np
    import mpix
    mpix.init()
    try:
        peer = 1 - rank
        grid = (np.arange(6 * 5 * 8, dtype=np.float32) + 1000 * rank
                ).reshape(6, 5, 8)
        halo = np.empty((6, 5, 8), dtype=np.float32)
        halo.view(np.uint8).fill(0xA5)
        # y-face out, y-face in; and a large one that spans stage chunks
        big = (np.arange(300 * 128, dtype=np.float32) + 7 * rank
               ).reshape(300, 128)
        big_in = np.zeros((300, 100), dtype=np.float32)
        reqs = [mpix.irecv_enqueue(halo[:, 4, :], source=peer, tag=1),
                mpix.irecv_enqueue(big_in, source=peer, tag=2),
                mpix.isend_enqueue(grid[:, 0, :], dest=peer, tag=1),
                mpix.isend_enqueue(big[:, :100], dest=peer, tag=2)]
        sts = [mpix.wait(r) for r in reqs]
        assert all(s["error"] == 0 for s in sts), sts
        want = (np.arange(6 * 5 * 8, dtype=np.float32) + 1000 * peer
                ).reshape(6, 5, 8)[:, 0, :]
        assert np.array_equal(halo[:, 4, :], want)
        rest = np.delete(halo, 4, axis=1).view(np.uint8)
        assert (rest == 0xA5).all()
        want_big = (np.arange(300 * 128, dtype=np.float32) + 7 * peer
                    ).reshape(300, 128)[:, :100]
        assert np.array_equal(big_in, want_big)
    finally:
        mpix.finalize()


def test_two_ranks():
    run_ranks(2, _two_rank_exchange)
