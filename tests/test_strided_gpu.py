"""Strided device transfers (k_pull_strided + strided_plan.h) on the GPU.

A non-contiguous tensor view is sent from and received into device memory
with no pack or unpack by the caller.  Payloads are position-dependent (byte
i of a source base tensor is (i * 7 + 3) % 251), every destination is a view
into a sentinel-filled base tensor, and the WHOLE destination base is compared
with what it must hold: the message bytes in the view, the sentinel
everywhere else.  All comparisons are exact.

Shapes are the smallest that reach each branch: granule 16 (vector path) and
8 / 4 / 2 / 1 (element path), one and two strided levels, a message that
spans tiles (16 KiB) with runs straddling their ends, a batch that mixes
strided and contiguous pulls, capture and replay, two processes over the IPC
mapping, and the error status for mixed memory kinds.
"""
import numpy as np
import pytest

from conftest import run_ranks

pytestmark = pytest.mark.gpu

SENT = 0xA5


def _torch():
    import torch
    return torch


def pattern(shape, dtype=None):
    """Base tensor whose BYTES follow the pattern, whatever the dtype."""
    torch = _torch()
    dtype = dtype or torch.uint8
    item = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape)) * item
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    return ((i * 7 + 3) % 251).to(torch.uint8).view(dtype).reshape(shape)


def sentinel(shape, dtype=None):
    torch = _torch()
    dtype = dtype or torch.uint8
    item = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape)) * item
    return torch.full((n,), SENT, dtype=torch.uint8,
                      device="cuda").view(dtype).reshape(shape)


def raw(t):
    """Message bytes of a view, in C order."""
    torch = _torch()
    return t.contiguous().reshape(-1).view(torch.uint8)


def expected_base(dst_base, dst_of, msg):
    """dst_base's required content: sentinel, with the first len(msg) message
    bytes of the view dst_of(base) replaced by msg."""
    torch = _torch()
    want = sentinel(tuple(dst_base.shape), dst_base.dtype)
    view = dst_of(want)
    cur = raw(view).clone()
    cur[:msg.numel()] = msg
    view.copy_(cur.view(want.dtype).reshape(view.shape))
    return want.reshape(-1).view(torch.uint8)


def same_bytes(a, b):
    torch = _torch()
    return torch.equal(a.reshape(-1).view(torch.uint8),
                       b.reshape(-1).view(torch.uint8))


def exchange(mpix, pairs):
    """pairs = [(src_view, dst_view)]; posts every pair, then ONE
    waitall_enqueue, so that they can share a progress pass."""
    torch = _torch()
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    reqs = []
    for tag, (s, d) in enumerate(pairs):
        reqs.append(mpix.irecv_enqueue(d, source=0, tag=300 + tag,
                                       stream=stream))
        reqs.append(mpix.isend_enqueue(s, dest=0, tag=300 + tag,
                                       stream=stream))
    mpix.waitall_enqueue(reqs, stream=stream)
    torch.cuda.synchronize()


def roundtrip(mpix, src_view, dst_base, dst_of):
    exchange(mpix, [(src_view, dst_of(dst_base))])
    want = expected_base(dst_base, dst_of, raw(src_view))
    assert same_bytes(dst_base, want)


def _i64():
    return _torch().int64


def _f32():
    return _torch().float32


# name -> (src base shape, src view, dst base shape, dst view, dtype)
# dtype None = uint8, so shapes are in bytes
CASES = {
    # vector path (granule 16)
    "run16_to_contig": ((5, 32), lambda b: b[:, :16],
                        (5 * 16 + 32,), lambda b: b[16:16 + 80], None),
    "contig_to_run48": ((4 * 48,), lambda b: b,
                        (4, 64), lambda b: b[:, 16:], None),
    "run4112_tiles": ((8, 4128), lambda b: b[:, :4112],
                      (8, 4144), lambda b: b[:, 16:4128], None),
    "two_levels": ((4, 8, 96), lambda b: b[:3, :5, :64],
                   (5, 7, 80), lambda b: b[1:4, 2:7, 16:], None),
    "two_levels_to_one": ((4, 8, 96), lambda b: b[:3, :5, :64],
                          (20, 64), lambda b: b[:, :48], None),
    # element path
    "u8_run7_g1": ((6, 9), lambda b: b[:, 1:8],
                   (6, 16), lambda b: b[:, 3:10], None),
    "u8_run6_g2": ((5, 8), lambda b: b[:, 2:8],
                   (5, 10), lambda b: b[:, :6], None),
    "f32_zface_g4": ((6, 5, 8), lambda b: b[:, :, 3],
                     (6, 5, 8), lambda b: b[:, :, 7], _f32),
    "i64_col_g8": ((7, 3), lambda b: b[:, 1],
                   (7, 5), lambda b: b[:, 2], _i64),
    "run8_g8": ((9, 24), lambda b: b[:, 8:16],
                (80,), lambda b: b[8:], None),
    "vector_shape_base_plus4": ((4, 64), lambda b: b[:, :48],
                                (4 + 192 + 12,), lambda b: b[4:196], None),
    "src_base_plus1": ((4 * 64 + 16,), lambda b: b[1:257].reshape(4, 64)[:, :32],
                       (144,), lambda b: b[16:], None),
    # element path over more than one tile (20000 B of 4-byte runs)
    "f32_zface_tiles": ((50, 100, 4), lambda b: b[:, :, 1],
                        (5000, 2), lambda b: b[:, 1], _f32),
}


@pytest.mark.parametrize("name", list(CASES))
def test_layouts(mpix_env, name):
    sshape, s_of, dshape, d_of, dt = CASES[name]
    dtype = dt() if dt else None
    src = pattern(sshape, dtype)
    dst = sentinel(dshape, dtype)
    view = s_of(src)
    assert not (view.is_contiguous() and d_of(dst).is_contiguous())
    roundtrip(mpix_env, view, dst, d_of)


@pytest.fixture
def mpix_div64(monkeypatch):
    """mpix with the 64-bit-division kernel forced (the path a message of
    2^31 units takes)."""
    monkeypatch.setenv("MPIX_STRIDED_DIV64", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    import mpix
    mpix.init()
    yield mpix
    mpix.finalize()


@pytest.mark.parametrize("name", ["run4112_tiles", "two_levels",
                                  "f32_zface_tiles", "u8_run7_g1"])
def test_layouts_wide_division(mpix_div64, name):
    sshape, s_of, dshape, d_of, dt = CASES[name]
    dtype = dt() if dt else None
    roundtrip(mpix_div64, s_of(pattern(sshape, dtype)),
              sentinel(dshape, dtype), d_of)


def test_truncation(mpix_env):
    """160 B in 16-byte runs into room for 96 B in 32-byte runs: the first
    96 message bytes arrive, the status says truncated; then a short
    message into a larger strided receive."""
    torch = _torch()
    mpix = mpix_env
    stream = torch.cuda.current_stream()
    src = pattern((10, 32))[:, :16]
    dst = sentinel((3, 64))
    d_of = lambda b: b[:, 16:48]  # noqa: E731
    torch.cuda.synchronize()
    rr = mpix.irecv_enqueue(d_of(dst), source=0, tag=1, stream=stream)
    rs = mpix.isend_enqueue(src, dest=0, tag=1, stream=stream)
    st = mpix.wait(rr)
    mpix.wait(rs)
    torch.cuda.synchronize()
    assert st["error"] != 0 and st["count_bytes"] == 96
    assert same_bytes(dst, expected_base(dst, d_of, raw(src)[:96]))

    short = pattern((48,))
    dst2 = sentinel((10, 32))
    d2_of = lambda b: b[:, :16]  # noqa: E731
    rr = mpix.irecv_enqueue(d2_of(dst2), source=0, tag=2, stream=stream)
    rs = mpix.isend_enqueue(short, dest=0, tag=2, stream=stream)
    st = mpix.wait(rr)
    mpix.wait(rs)
    torch.cuda.synchronize()
    assert st["error"] == 0 and st["count_bytes"] == 48
    assert same_bytes(dst2, expected_base(dst2, d2_of, raw(short)))


def test_six_face_batch(mpix_env):
    """Two faces of each orientation of a (8, 8, 16) float grid under one
    waitall: the x-faces are contiguous, so contiguous and strided pulls
    meet in one pass."""
    f32 = _f32()
    grid = pattern((8, 8, 16), f32)
    halo = sentinel((8, 8, 16), f32)
    faces = [lambda b: b[0], lambda b: b[7],
             lambda b: b[:, 0, :], lambda b: b[:, 7, :],
             lambda b: b[:, :, 0], lambda b: b[:, :, 15]]
    assert faces[0](grid).is_contiguous()
    exchange(mpix_env, [(f(grid), f(halo)) for f in faces])
    # faces share edges; every edge holds the same grid values either way
    want = sentinel((8, 8, 16), f32)
    for f in faces:
        f(want).copy_(f(grid))
    assert same_bytes(halo, want)


def test_capture_and_replay(mpix_env):
    torch = _torch()
    mpix = mpix_env
    src = torch.zeros((6, 64), dtype=torch.uint8, device="cuda")
    dst = sentinel((6, 80))
    d_of = lambda b: b[:, 16:64]  # noqa: E731
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        mpix.stream_begin_capture(s.cuda_stream)
        rs = mpix.isend_enqueue(src[:, :48], dest=0, tag=3, stream=s)
        rr = mpix.irecv_enqueue(d_of(dst), source=0, tag=3, stream=s)
        mpix.waitall_enqueue([rs, rr], stream=s)
        graph, gexec = mpix.stream_end_capture(s.cuda_stream)
    for it in range(2):
        src.copy_(pattern((6 * 64 + it,))[it:].reshape(6, 64))
        dst.fill_(SENT)
        torch.cuda.synchronize()
        mpix.graph_launch(gexec, s.cuda_stream)
        torch.cuda.synchronize()
        assert same_bytes(dst, expected_base(dst, d_of, raw(src[:, :48]))), it
    mpix.graph_exec_destroy(gexec)
    mpix.graph_destroy(graph)


def test_mixed_memory_kinds(mpix_env):
    """Device strided send into a host view, and host strided send into a
    device buffer: the receive completes with an error status, the send
    completes too, nothing hangs, and plain traffic still works after."""
    torch = _torch()
    mpix = mpix_env
    stream = torch.cuda.current_stream()
    dev = pattern((6, 32))
    host = np.full((6, 32), SENT, dtype=np.uint8)
    torch.cuda.synchronize()
    rr = mpix.irecv_enqueue(host[:, :16], source=0, tag=4)
    rs = mpix.isend_enqueue(dev[:, :16], dest=0, tag=4, stream=stream)
    st = mpix.wait(rr)
    mpix.wait(rs)
    assert st["error"] != 0 and st["count_bytes"] == 0
    assert (host == SENT).all()

    hsrc = np.arange(6 * 32, dtype=np.uint8).reshape(6, 32)
    ddst = sentinel((6 * 16,))
    rs = mpix.isend_enqueue(hsrc[:, :16], dest=0, tag=5)
    rr = mpix.irecv_enqueue(ddst, source=0, tag=5, stream=stream)
    st = mpix.wait(rr)
    mpix.wait(rs)
    torch.cuda.synchronize()
    assert st["error"] != 0 and st["count_bytes"] == 0
    assert bool((ddst == SENT).all())

    roundtrip(mpix, dev[:, :16], sentinel((6, 48)), lambda b: b[:, 16:32])


def _two_proc_yface(rank, size):
    import numpy as np  # noqa: F401
    import torch
    import mpix
    mpix.init()
    try:
        peer = 1 - rank
        shape = (8, 8, 16)
        n = 8 * 8 * 16

        def grid_of(r):
            return (torch.arange(n, dtype=torch.float32, device="cuda")
                    + 10000 * r).reshape(shape)

        grid = grid_of(rank)
        halo = torch.full(shape, -1.0, dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream()
        torch.cuda.synchronize()
        rr = mpix.irecv_enqueue(halo[:, 7, :], source=peer, tag=1,
                                stream=stream)
        rs = mpix.isend_enqueue(grid[:, 0, :], dest=peer, tag=1,
                                stream=stream)
        mpix.waitall_enqueue([rr, rs], stream=stream)
        torch.cuda.synchronize()
        want = torch.full(shape, -1.0, dtype=torch.float32, device="cuda")
        want[:, 7, :] = grid_of(peer)[:, 0, :]
        assert torch.equal(halo, want)
    finally:
        mpix.finalize()


def test_two_processes_yface():
    run_ranks(2, _two_proc_yface, timeout=240)
