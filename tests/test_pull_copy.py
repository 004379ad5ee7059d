"""The batched pull copy (k_pull_multi + pull_plan.h) on the GPU, single
process over loopback.

Payloads are position-dependent (byte i of the whole source tensor is
(i * 7 + 3) % 251), so a vector that lands in the wrong place shows.  Every
destination sits inside a larger tensor filled with a sentinel, and the
sentinel bytes before, between and after the destinations must survive.

This file runs the default kernel only: unroll 4 (tiles of 16384 B),
write-through with the completion word.  The lengths below are one vector,
one tile -/+ 16 B and tails (n % 16 != 0); they bracket 32768 B as well, the
tile of unroll 8, but here that is just two tiles of unroll 4.  Unroll 1 and
8 and the nontemporal and plain kernels run in
tests/test_pull_kernels_gpu.py (every variant, launched directly, against a
byte-exact reference) and tests/test_pull_variants_gpu.py (selected by
MPIX_PULL_UNROLL / MPIX_PULL_NT through the runtime).
"""
import pytest

pytestmark = pytest.mark.gpu

SENT = 0xA5
PAD = 64  # sentinel bytes around a destination; a multiple of 16
SIZES = [16, 48, 4080, 16368, 16384, 16400, 32752, 32768, 32784, 32807,
         1048597]

_pattern_cache = {}


def _torch():
    import torch
    return torch


def pattern(n, start=0):
    """Bytes start..start+n of the fixed pattern, on the GPU (computed once
    for the largest request so far and sliced; never modified)."""
    torch = _torch()
    need = start + n
    have = _pattern_cache.get("t")
    if have is None or have.numel() < need:
        i = torch.arange(max(need, (1 << 20) + 4096), dtype=torch.int64)
        have = ((i * 7 + 3) % 251).to(torch.uint8).cuda()
        _pattern_cache["t"] = have
    return have[start:start + n]


def sentinel(n):
    torch = _torch()
    return torch.full((n,), SENT, dtype=torch.uint8, device="cuda")


def up16(n):
    return (n + 15) // 16 * 16


def check_sentinels(dst, used):
    """`used` = list of (offset, length) inside dst; all other bytes must
    still be the sentinel."""
    torch = _torch()
    keep = torch.ones(dst.numel(), dtype=torch.bool, device=dst.device)
    for off, n in used:
        keep[off:off + n] = False
    assert bool((dst[keep] == SENT).all()), "sentinel bytes overwritten"


def exchange(mpix, pairs):
    """pairs = [((src_tensor, offset), (dst_tensor, offset), nbytes)]; posts
    every pair, then ONE waitall_enqueue, so that they can share a batch."""
    torch = _torch()
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    reqs = []
    for tag, ((s, so), (d, do), n) in enumerate(pairs):
        reqs.append(mpix.isend_enqueue((s.data_ptr() + so, n), dest=0,
                                       tag=100 + tag, stream=stream))
        reqs.append(mpix.irecv_enqueue((d.data_ptr() + do, n), source=0,
                                       tag=100 + tag, stream=stream))
    mpix.waitall_enqueue(reqs, stream=stream)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", SIZES)
def test_single_message(mpix_env, n):
    torch = _torch()
    src = pattern(n + 16).clone()  # payload starts at offset 16
    dst = sentinel(n + 2 * PAD)
    exchange(mpix_env, [((src, 16), (dst, PAD), n)])
    assert torch.equal(dst[PAD:PAD + n], pattern(n, 16))
    check_sentinels(dst, [(PAD, n)])


def test_mixed_batch(mpix_env):
    torch = _torch()
    sizes = [16, 32807, 4080, 16400, 48, 32768, 16368, 1048597]
    total = sum(up16(n) for n in sizes)
    src = pattern(total).clone()
    dst = sentinel(total + PAD * (len(sizes) + 1))
    pairs, used, want = [], [], []
    so, do = 0, PAD
    for n in sizes:
        pairs.append(((src, so), (dst, do), n))
        used.append((do, n))
        want.append((do, so, n))
        so += up16(n)
        do += up16(n) + PAD
    exchange(mpix_env, pairs)
    for do, so, n in want:
        assert torch.equal(dst[do:do + n], pattern(n, so)), (do, so, n)
    check_sentinels(dst, used)


@pytest.mark.parametrize("order", [
    [0, 1, 2, 3, 4, 5, 6, 7],
    [7, 6, 5, 4, 3, 2, 1, 0],
    [0, 2, 4, 6, 1, 3, 5, 7],
], ids=["ascending", "descending", "interleaved"])
def test_partitioned_tile_straddling(mpix_env, order):
    """8 partitions of 4112 B: a multiple of 16 but not of a tile, so a
    merged run straddles tile ends.  Three iterations reuse the requests."""
    torch = _torch()
    mpix = mpix_env
    parts, per = 8, 4112
    n = parts * per
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = sentinel(n + 2 * PAD)
    ps = mpix.psend_init((src.data_ptr(), n), parts, dest=0, tag=21)
    pr = mpix.precv_init((dst.data_ptr() + PAD, n), parts, source=0, tag=21)
    try:
        for it in range(3):
            src.copy_(pattern(n, 1000 * it))
            dst.fill_(SENT)
            torch.cuda.synchronize()
            mpix.start(pr)
            mpix.start(ps)
            for p in order:
                mpix.pready(p, ps)
            mpix.wait(pr)
            mpix.wait(ps)
            assert torch.equal(dst[PAD:PAD + n], pattern(n, 1000 * it)), it
            check_sentinels(dst, [(PAD, n)])
    finally:
        mpix.request_free(ps)
        mpix.request_free(pr)


@pytest.mark.parametrize("gapped", ["dst", "src"])
def test_gapped_slices(mpix_env, gapped):
    """Four messages whose slices are consecutive on one side and separated
    by 16-byte gaps on the other: must not be merged across the gaps."""
    torch = _torch()
    k, per, gap = 4, 4112, 16
    dense_off = [i * per for i in range(k)]
    gap_off = [PAD + i * (per + gap) for i in range(k)]
    if gapped == "dst":
        src = pattern(k * per).clone()
        dst = sentinel(2 * PAD + k * (per + gap))
        s_off, d_off = dense_off, gap_off
    else:
        src = pattern(2 * PAD + k * (per + gap)).clone()
        dst = sentinel(k * per + 2 * PAD)
        s_off, d_off = gap_off, [PAD + o for o in dense_off]
    pairs = [((src, s), (dst, d), per) for s, d in zip(s_off, d_off)]
    exchange(mpix_env, pairs)
    for s, d in zip(s_off, d_off):
        assert torch.equal(dst[d:d + per], pattern(per, s)), (s, d)
    check_sentinels(dst, [(d, per) for d in d_off])


def test_misaligned_buffers(mpix_env):
    """address + 4 on both sides: not 16-byte aligned, so the message rides
    hipMemcpyAsync and not the pull kernel; the bytes must match all the
    same."""
    torch = _torch()
    n = 16400
    src = pattern(n + 4).clone()
    dst = sentinel(n + 2 * PAD)
    assert (src.data_ptr() + 4) % 16 == 4 and (dst.data_ptr() + PAD + 4) % 16 == 4
    exchange(mpix_env, [((src, 4), (dst, PAD + 4), n)])
    assert torch.equal(dst[PAD + 4:PAD + 4 + n], pattern(n, 4))
    check_sentinels(dst, [(PAD + 4, n)])


def test_empty_message(mpix_env):
    src = pattern(64).clone()
    dst = sentinel(2 * PAD)
    exchange(mpix_env, [((src, 16), (dst, PAD), 0)])
    check_sentinels(dst, [])


def test_device_host_plain(mpix_env):
    """4100 B (a 4-byte tail behind the last vector) between device and host
    memory, host waits.  Device -> host: a pull whose destination no kernel
    may touch, so it rides hipMemcpyAsync.  Host -> device: chunks staged
    through shared memory and copied in on the copy stream."""
    import numpy as np
    torch = _torch()
    mpix = mpix_env
    stream = torch.cuda.current_stream()
    n = 4100
    want = pattern(n, 16).cpu().numpy()

    src = pattern(n + 16).clone()
    host = np.full(n + 2 * PAD, SENT, dtype=np.uint8)
    torch.cuda.synchronize()
    rr = mpix.irecv_enqueue((host.ctypes.data + PAD, n), source=0, tag=31)
    rs = mpix.isend_enqueue((src.data_ptr() + 16, n), dest=0, tag=31,
                            stream=stream)
    st = mpix.wait(rr)
    mpix.wait(rs)
    assert st["error"] == 0 and st["count_bytes"] == n
    assert (host[PAD:PAD + n] == want).all()
    assert (host[:PAD] == SENT).all() and (host[PAD + n:] == SENT).all()

    hsrc = np.concatenate([np.zeros(16, dtype=np.uint8), want])
    dst = sentinel(n + 2 * PAD)
    torch.cuda.synchronize()
    rs = mpix.isend_enqueue((hsrc.ctypes.data + 16, n), dest=0, tag=32)
    rr = mpix.irecv_enqueue((dst.data_ptr() + PAD, n), source=0, tag=32,
                            stream=stream)
    st = mpix.wait(rr)
    mpix.wait(rs)
    torch.cuda.synchronize()
    assert st["error"] == 0 and st["count_bytes"] == n
    assert torch.equal(dst[PAD:PAD + n], pattern(n, 16))
    check_sentinels(dst, [(PAD, n)])


def _misaligned_pair(rank, size):
    import torch
    import mpix
    mpix.init()
    try:
        peer = 1 - rank
        n = 16400
        src = pattern(n + 4, 100 * rank).clone()
        dst = sentinel(n + 2 * PAD)
        assert (src.data_ptr() + 4) % 16 == 4
        assert (dst.data_ptr() + PAD + 4) % 16 == 4
        stream = torch.cuda.current_stream()
        torch.cuda.synchronize()
        rr = mpix.irecv_enqueue((dst.data_ptr() + PAD + 4, n), source=peer,
                                tag=7, stream=stream)
        rs = mpix.isend_enqueue((src.data_ptr() + 4, n), dest=peer, tag=7,
                                stream=stream)
        mpix.waitall_enqueue([rr, rs], stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(dst[PAD + 4:PAD + 4 + n],
                           pattern(n, 100 * peer + 4))
        check_sentinels(dst, [(PAD + 4, n)])
    finally:
        mpix.finalize()


def test_misaligned_two_ranks():
    """test_misaligned_buffers between two processes: the hipMemcpyAsync
    pull reads the peer's memory, and its ack goes back through the peer's
    descriptor ring and not through the loopback shortcut."""
    from conftest import run_ranks
    run_ranks(2, _misaligned_pair, timeout=120)
