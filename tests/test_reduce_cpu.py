"""Reducing receives between host buffers (the CPU tier), through the
library: irecv_reduce_enqueue / precv_reduce_init combine the message into the
buffer with reduce_host (src/transport/reduce.h) as the 64 KiB stage chunks
arrive, or from the heap copy of an unexpected message.

Expected values come from numpy on the same inputs (IEEE add for float32 and
float64, float16 sums rounded once, wrapping integers, np.maximum/minimum) and
every comparison is bit-exact.  Message sizes sit on the chunk boundary:
1 element, 65536 B -/+ one element, 3 chunks + 1 element.
"""
import numpy as np
import pytest

from conftest import run_ranks

CHUNK = 65536
DTYPES = ["float32", "float64", "float16", "int32", "int64"]
OPS = ["sum", "max", "min"]


def sizes(dtype):
    """Element counts around the 64 KiB staging chunk."""
    per = CHUNK // np.dtype(dtype).itemsize
    return [1, per - 1, per, per + 1, 3 * per + 1]


_inputs = {}


def inputs(dtype, n):
    """(buffer, message): the same arrays for every test that asks; never
    modified (tests work on copies)."""
    key = (dtype, n)
    if key not in _inputs:
        rng = np.random.default_rng(1234 + n)
        if dtype.startswith("int"):
            info = np.iinfo(dtype)
            a = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
            b = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
        else:
            a = rng.standard_normal(n).astype(dtype)
            b = (rng.standard_normal(n) * 3).astype(dtype)
        a.setflags(write=False)
        b.setflags(write=False)
        _inputs[key] = (a, b)
    return _inputs[key]


def expected(a, b, op):
    with np.errstate(over="ignore"):
        if op == "sum":
            return a + b
        return np.maximum(a, b) if op == "max" else np.minimum(a, b)


def same_bits(x, y):
    return x.dtype == y.dtype and x.tobytes() == y.tobytes()


def reduce_xfer(mpix, buf, msg, op, tag, send_first=False, peer=0):
    """One loopback message combined into buf; returns the receive status."""
    if send_first:
        rs = mpix.isend_enqueue(msg, dest=peer, tag=tag)
        mpix.wait(rs)  # buffered: completes with no receive posted
        rr = mpix.irecv_reduce_enqueue(buf, source=peer, op=op, tag=tag)
        return mpix.wait(rr)
    rr = mpix.irecv_reduce_enqueue(buf, source=peer, op=op, tag=tag)
    rs = mpix.isend_enqueue(msg, dest=peer, tag=tag)
    st = mpix.wait(rr)
    mpix.wait(rs)
    return st


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_loopback_every_type_and_op(mpix_env, dtype, op):
    for tag, n in enumerate(sizes(dtype)):
        for send_first in (False, True):  # posted, unexpected
            a, b = inputs(dtype, n)
            buf = a.copy()
            st = reduce_xfer(mpix_env, buf, b, op, tag, send_first)
            assert st["error"] == 0 and st["count_bytes"] == b.nbytes
            assert same_bits(buf, expected(a, b, op)), (dtype, op, n)


def _two_rank_body(rank, world):
    import mpix
    mpix.init()
    try:
        tag = 0
        for dtype in DTYPES:
            for op in OPS:
                for n in (sizes(dtype)[1], sizes(dtype)[4]):
                    a, b = inputs(dtype, n)
                    tag += 1
                    if rank == 1:
                        mpix.wait(mpix.isend_enqueue(b, dest=0, tag=tag))
                        continue
                    buf = a.copy()
                    st = mpix.wait(mpix.irecv_reduce_enqueue(
                        buf, source=1, op=op, tag=tag))
                    assert st["error"] == 0 and st["source"] == 1
                    assert st["count_bytes"] == b.nbytes
                    assert same_bits(buf, expected(a, b, op)), (dtype, op, n)
        # both directions at once, unexpected on one side: rank 1 also
        # reduces what rank 0 sends
        a, b = inputs("float32", 3 * CHUNK // 4 + 1)
        buf = a.copy()
        rs = mpix.isend_enqueue(b, dest=1 - rank, tag=900)
        mpix.wait(rs)
        st = mpix.wait(mpix.irecv_reduce_enqueue(buf, source=1 - rank,
                                                 op="sum", tag=900))
        assert st["error"] == 0
        assert same_bits(buf, a + b)
    finally:
        mpix.finalize()


def test_two_ranks():
    run_ranks(2, _two_rank_body)


def test_truncation_combines_what_fits(mpix_env):
    a, b = inputs("float32", CHUNK // 4 + 1)
    buf = a[:1000].copy()
    guard = np.concatenate([buf, np.full(8, 7.0, np.float32)])
    st = reduce_xfer(mpix_env, guard[:1000], b, "sum", 1)
    assert st["error"] == mpix_env._C.ERR_TRUNCATE
    assert st["count_bytes"] == 4000
    assert same_bits(guard[:1000], a[:1000] + b[:1000])
    assert (guard[1000:] == 7.0).all()
    # unexpected, and longer than one chunk on the wire
    guard = np.concatenate([buf, np.full(8, 7.0, np.float32)])
    st = reduce_xfer(mpix_env, guard[:1000], b, "sum", 2, send_first=True)
    assert st["error"] == mpix_env._C.ERR_TRUNCATE
    assert same_bits(guard[:1000], a[:1000] + b[:1000])
    assert (guard[1000:] == 7.0).all()


@pytest.mark.parametrize("send_first", [False, True],
                         ids=["posted", "unexpected"])
def test_length_not_a_multiple_of_the_element(mpix_env, send_first):
    a, _ = inputs("float32", 1000)
    buf = a.copy()
    for tag, nbytes in enumerate((7, CHUNK + 2)):
        msg = np.arange(nbytes, dtype=np.uint8)
        st = reduce_xfer(mpix_env, buf, msg, "sum", 10 + tag, send_first)
        assert st["error"] == mpix_env._C.ERR_TYPE, nbytes
        assert same_bits(buf, a)  # untouched
    # the pair still works afterwards
    a, b = inputs("float32", 1000)
    st = reduce_xfer(mpix_env, buf, b, "sum", 20)
    assert st["error"] == 0 and same_bits(buf, a + b)


def test_zero_byte_message(mpix_env):
    a, _ = inputs("float64", 16)
    buf = a.copy()
    for send_first in (False, True):
        st = reduce_xfer(mpix_env, buf, np.zeros(0, np.float64), "sum", 30,
                         send_first)
        assert st["error"] == 0 and st["count_bytes"] == 0
        assert same_bits(buf, a)
    # an empty receive takes an empty message too
    st = reduce_xfer(mpix_env, np.zeros(0, np.float64),
                     np.zeros(0, np.float64), "max", 31)
    assert st["error"] == 0 and st["count_bytes"] == 0


def test_partitioned_accumulates_on_reuse(mpix_env):
    mpix = mpix_env
    parts, per = 4, 5000  # 20000 B per partition: chunks end inside none
    a, b = inputs("float32", parts * per)
    buf = a.copy()
    msg = b.copy()
    pr = mpix.precv_reduce_init(buf, parts, source=0, op="sum", tag=40)
    ps = mpix.psend_init(msg, parts, dest=0, tag=40)
    want = a.copy()
    for it in range(2):
        msg[:] = b * (it + 1)
        want = want + msg
        mpix.start(pr)
        mpix.start(ps)
        for p in (2, 0, 3, 1):
            mpix.pready(p, ps)
        mpix.wait(pr)
        mpix.wait(ps)
        for p in range(parts):
            assert not mpix.parrived(pr, p)  # reset by the wait
        # the second iteration accumulated on top of the first
        assert same_bits(buf, want), it
    mpix.request_free(ps)
    mpix.request_free(pr)


def test_plain_receives_beside_reducing_ones_overwrite(mpix_env):
    mpix = mpix_env
    a, b = inputs("int32", 3000)
    red, plain = a.copy(), a.copy()
    r1 = mpix.irecv_reduce_enqueue(red, source=0, op="sum", tag=50)
    r2 = mpix.irecv_enqueue(plain, source=0, tag=51)
    s2 = mpix.isend_enqueue(b, dest=0, tag=51)
    s1 = mpix.isend_enqueue(b, dest=0, tag=50)
    for r in (r1, r2, s1, s2):
        assert mpix.wait(r)["error"] == 0
    assert same_bits(red, a + b)
    assert same_bits(plain, b)
    # same tag: matched in post order, reducing first
    red, plain = a.copy(), a.copy()
    r1 = mpix.irecv_reduce_enqueue(red, source=0, op="max", tag=52)
    r2 = mpix.irecv_enqueue(plain, source=0, tag=52)
    s1 = mpix.isend_enqueue(b, dest=0, tag=52)
    s2 = mpix.isend_enqueue(b, dest=0, tag=52)
    for r in (r1, r2, s1, s2):
        assert mpix.wait(r)["error"] == 0
    assert same_bits(red, np.maximum(a, b))
    assert same_bits(plain, b)


def test_value_errors(mpix_env):
    mpix = mpix_env
    ok = np.zeros(8, np.float32)
    for bad in (np.zeros(8, np.uint8), np.zeros(8, np.int16),
                np.zeros(8, np.complex64), np.zeros(8, bool)):
        with pytest.raises(ValueError, match="dtype"):
            mpix.irecv_reduce_enqueue(bad, source=0)
        with pytest.raises(ValueError, match="dtype"):
            mpix.precv_reduce_init(bad, 2, source=0)
    view = np.zeros((8, 8), np.float32)[:, 2]
    for call in (lambda: mpix.irecv_reduce_enqueue(view, source=0),
                 lambda: mpix.irecv_reduce_graph(view, source=0),
                 lambda: mpix.precv_reduce_init(view, 2, source=0)):
        with pytest.raises(ValueError, match="contiguous"):
            call()
    for call in (lambda: mpix.irecv_reduce_enqueue(ok, source=0, op="prod"),
                 lambda: mpix.irecv_reduce_graph(ok, source=0, op="avg"),
                 lambda: mpix.precv_reduce_init(ok, 2, source=0, op=0)):
        with pytest.raises(ValueError, match="op"):
            call()
    with pytest.raises(ValueError, match="partitions"):
        mpix.precv_reduce_init(ok, 3, source=0)
    with pytest.raises(TypeError):
        mpix.irecv_reduce_enqueue((ok.ctypes.data, 32), source=0)


def test_err_arg_at_the_call(mpix_env):
    C = mpix_env._C
    buf = np.zeros(64, np.float64)
    addr = buf.ctypes.data
    arg = f"rc={C.ERR_ARG}$"

    def enq(addr, count, typ, op):
        return C.irecv_reduce(addr, count, typ, op, 0, 60, C.QUEUE_STREAM, 0)

    def pinit(addr, count, typ, op):
        return C.precv_init_reduce(addr, 2, count, typ, op, 0, 61)

    for call in (enq, pinit):
        for typ, op in ((6, C.SUM), (-1, C.SUM), (C.F32, 3), (C.F32, -1)):
            with pytest.raises(RuntimeError, match=arg):
                call(addr, 4, typ, op)
        with pytest.raises(RuntimeError, match=arg):
            call(addr, -1, C.F32, C.SUM)
        # aligned for the 16-bit types, not for the wider ones
        for typ in (C.F32, C.F64, C.I32, C.I64):
            with pytest.raises(RuntimeError, match=arg):
                call(addr + 2, 4, typ, C.SUM)
        for typ in (C.F16, C.BF16):
            with pytest.raises(RuntimeError, match=arg):
                call(addr + 1, 4, typ, C.SUM)
    # the same slots still serve a good call: nothing leaked a request
    r = enq(addr + 2, 4, C.F16, C.SUM)
    msg = np.ones(4, np.float16)
    mpix_env.wait(mpix_env.isend_enqueue(msg, dest=0, tag=60))
    assert mpix_env.wait(r)["error"] == 0
    assert (buf.view(np.float16)[1:5] == 1).all()
