"""Strided reducing receives between host buffers (the CPU tier), through the
library: irecv_reduce_strided_enqueue / precv_reduce_strided_init combine the
message into a view, run by run (layout_reduce_in of src/transport/layout.h)
as the 64 KiB stage chunks arrive, or from the heap copy of an unexpected
message.

Expected values come from numpy on the same inputs: the message's elements,
in C order, combined into the view's elements in C order (IEEE add for
float32 and float64, wrapping int32, np.maximum / np.minimum).  Every
comparison is bit-exact and covers the WHOLE underlying buffer, so a byte
written between the runs is seen.  Inputs are finite, no sum overflows, and
no MAX/MIN pair is +0 / -0 (the definition leaves those open).
"""
import numpy as np
import pytest

CHUNK = 65536
DTYPES = ["float32", "float64", "int32"]
OPS = ["sum", "max", "min"]


def values(dtype, n, seed):
    rng = np.random.default_rng(seed)
    if dtype.startswith("int"):
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    v = rng.standard_normal(n).astype(dtype)
    v[v == 0] = 1  # no +0 / -0 pairs under max / min
    return v


def combine(a, b, op):
    if op == "sum":
        return a + b
    return np.maximum(a, b) if op == "max" else np.minimum(a, b)


def same_bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and \
        x.tobytes() == y.tobytes()


# (name, base shape, the view of the base)
SHAPES = [
    ("y-face g[:, 1, :]", (5, 4, 6), lambda g: g[:, 1, :]),
    ("x-face g[:, :, 1]", (5, 4, 6), lambda g: g[:, :, 1]),
    ("column block m[:, 8:24]", (7, 40), lambda m: m[:, 8:24]),
]


def senders(view_shape, dtype, seed):
    """(name, what to send) x 3: the same elements from a contiguous array,
    from a view strided like nothing in particular, and from one with
    another pitch; all hold `msg` in C order."""
    n = int(np.prod(view_shape))
    msg = values(dtype, n, seed).reshape(view_shape)
    rows, cols = view_shape[0], n // view_shape[0]
    wide = np.zeros((rows, cols + 3), dtype)
    wide[:, 1:cols + 1] = msg.reshape(rows, cols)
    cube = np.zeros((n, 2), dtype)
    cube[:, 1] = msg.reshape(-1)
    return msg, [("contiguous", np.ascontiguousarray(msg)),
                 ("row pitch", wide[:, 1:cols + 1]),
                 ("every other element", cube[:, 1])]


def xfer(mpix, view, what, op, tag, send_first=False):
    """One loopback message combined into `view`; the receive's status."""
    if send_first:
        mpix.wait(mpix.isend_enqueue(what, dest=0, tag=tag))
        return mpix.wait(mpix.irecv_reduce_strided_enqueue(
            view, source=0, op=op, tag=tag))
    rr = mpix.irecv_reduce_strided_enqueue(view, source=0, op=op, tag=tag)
    rs = mpix.isend_enqueue(what, dest=0, tag=tag)
    st = mpix.wait(rr)
    mpix.wait(rs)
    return st


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_views_from_every_kind_of_sender(mpix_env, shape, dtype):
    _, base_shape, cut = shape
    tag = 0
    for op in OPS:
        base0 = values(dtype, int(np.prod(base_shape)), 7).reshape(base_shape)
        msg, kinds = senders(cut(base0).shape, dtype, 11 + tag)
        for kind, what in kinds:
            for send_first in (False, True):  # posted, unexpected
                base = base0.copy()
                want = base0.copy()
                cut(want)[...] = combine(cut(base0), msg, op)
                tag += 1
                st = xfer(mpix_env, cut(base), what, op, tag, send_first)
                assert st["error"] == 0, (kind, op)
                assert st["count_bytes"] == msg.nbytes
                assert same_bits(base, want), (kind, op, send_first)


def test_identically_strided_sender_and_contiguous_receiver(mpix_env):
    g = values("float32", 5 * 4 * 6, 1).reshape(5, 4, 6)
    src = values("float32", 5 * 4 * 6, 2).reshape(5, 4, 6)
    base = g.copy()
    st = xfer(mpix_env, base[:, 1, :], src[:, 1, :], "sum", 1)
    want = g.copy()
    want[:, 1, :] += src[:, 1, :]
    assert st["error"] == 0 and same_bits(base, want)
    # any sender matches whatever the receive's own layout: a contiguous
    # buffer given to the strided call takes a strided message
    flat = g[:, 1, :].copy()
    st = xfer(mpix_env, flat, src[:, 1:3, ::2], "max", 2)
    assert st["error"] == 0 and st["count_bytes"] == flat.nbytes
    assert same_bits(flat.reshape(-1),
                     np.maximum(g[:, 1, :].reshape(-1),
                                src[:, 1:3, ::2].reshape(-1)))


def test_runs_straddle_the_chunk_boundary(mpix_env):
    rows = 3000  # 72000 B in 24-byte runs: 65536 is no multiple of 24
    m0 = values("float64", rows * 5, 3).reshape(rows, 5)
    msg = values("float64", rows * 3, 4).reshape(rows, 3)
    assert msg.nbytes > CHUNK and CHUNK % 24 != 0
    for send_first in (False, True):
        m = m0.copy()
        st = xfer(mpix_env, m[:, 1:4], msg, "sum", 5, send_first)
        want = m0.copy()
        want[:, 1:4] += msg
        assert st["error"] == 0 and st["count_bytes"] == msg.nbytes
        assert same_bits(m, want), send_first


def test_partitioned_view_accumulates_on_restart(mpix_env):
    mpix = mpix_env
    parts = 4
    g0 = values("float32", 8 * 6 * 16, 5).reshape(8, 6, 16)
    b = values("float32", 8 * 16, 6)
    g = g0.copy()
    msg = b.copy()
    pr = mpix.precv_reduce_strided_init(g[:, 1, :], parts, source=0,
                                        op="sum", tag=40)
    ps = mpix.psend_init(msg, parts, dest=0, tag=40)
    want = g0.copy()
    for it in range(2):
        msg[:] = b * (it + 1)
        want[:, 1, :] = want[:, 1, :] + msg.reshape(8, 16)
        mpix.start(pr)
        mpix.start(ps)
        for p in (2, 0, 3, 1):
            mpix.pready(p, ps)
        assert mpix.wait(pr)["error"] == 0
        mpix.wait(ps)
        assert same_bits(g, want), it  # the second round on top of the first
    mpix.request_free(ps)
    mpix.request_free(pr)
    # a contiguous buffer through the same call, from a strided sender
    flat0 = values("int32", 4 * 10, 7)
    flat = flat0.copy()
    src = values("int32", 4 * 10 * 2, 8).reshape(4, 10, 2)
    pr = mpix.precv_reduce_strided_init(flat, parts, source=0, op="min",
                                        tag=41)
    ps = mpix.psend_init(src[:, :, 1], parts, dest=0, tag=41)
    mpix.start(pr)
    mpix.start(ps)
    for p in range(parts):
        mpix.pready(p, ps)
    assert mpix.wait(pr)["error"] == 0
    mpix.wait(ps)
    assert same_bits(flat, np.minimum(flat0, src[:, :, 1].reshape(-1)))
    mpix.request_free(ps)
    mpix.request_free(pr)


def test_truncation_combines_the_elements_that_fit(mpix_env):
    m0 = values("float32", 7 * 40, 9).reshape(7, 40)
    msg = values("float32", 7 * 16 + 5, 10)
    for send_first in (False, True):
        m = m0.copy()
        st = xfer(mpix_env, m[:, 8:24], msg, "sum", 50, send_first)
        assert st["error"] == mpix_env._C.ERR_TRUNCATE
        assert st["count_bytes"] == 7 * 16 * 4
        want = m0.copy()
        want[:, 8:24] += msg[:7 * 16].reshape(7, 16)
        assert same_bits(m, want)


@pytest.mark.parametrize("send_first", [False, True],
                         ids=["posted", "unexpected"])
def test_length_not_a_multiple_of_the_element(mpix_env, send_first):
    m0 = values("float32", 7 * 40, 12).reshape(7, 40)
    m = m0.copy()
    for tag, nbytes in enumerate((7, 7 * 16 * 4 - 2)):
        st = xfer(mpix_env, m[:, 8:24], np.arange(nbytes, dtype=np.uint8),
                  "sum", 60 + tag, send_first)
        assert st["error"] == mpix_env._C.ERR_TYPE, nbytes
        assert same_bits(m, m0)  # untouched
    # the pair still works afterwards
    msg = values("float32", 7 * 16, 13).reshape(7, 16)
    st = xfer(mpix_env, m[:, 8:24], msg, "sum", 70)
    want = m0.copy()
    want[:, 8:24] += msg
    assert st["error"] == 0 and same_bits(m, want)


def test_zero_byte_message(mpix_env):
    m0 = values("float64", 6 * 8, 14).reshape(6, 8)
    m = m0.copy()
    for send_first in (False, True):
        st = xfer(mpix_env, m[:, 2:5], np.zeros(0, np.float64), "sum", 80,
                  send_first)
        assert st["error"] == 0 and st["count_bytes"] == 0
        assert same_bits(m, m0)
    st = xfer(mpix_env, m[:0, 2:5], np.zeros(0, np.float64), "max", 81)
    assert st["error"] == 0 and st["count_bytes"] == 0


def test_value_errors(mpix_env):
    mpix = mpix_env
    ok = np.zeros((8, 8), np.float32)[:, 2:6]
    calls = (lambda b, **k: mpix.irecv_reduce_strided_enqueue(b, source=0, **k),
             lambda b, **k: mpix.irecv_reduce_strided_graph(b, source=0, **k),
             lambda b, **k: mpix.precv_reduce_strided_init(b, 2, source=0, **k))
    for call in calls:
        for bad in (np.zeros((8, 8), np.uint8)[:, 2:6],
                    np.zeros((8, 8), np.int16)[:, 2:6],
                    np.zeros(8, np.complex64)):
            with pytest.raises(ValueError, match="dtype"):
                call(bad)
        with pytest.raises(ValueError, match="op"):
            call(ok, op="prod")
        # views that do not fit a layout: three strided levels, a transpose
        with pytest.raises(ValueError, match="strided levels"):
            call(np.zeros((4, 4, 4, 4), np.float32)[:, :2, :2, :2])
        with pytest.raises(ValueError, match="transposed"):
            call(np.zeros((4, 6), np.float32).T)
    with pytest.raises(ValueError, match="partitions"):
        mpix.precv_reduce_strided_init(ok, 3, source=0)
    with pytest.raises(ValueError, match="partitions"):
        mpix.precv_reduce_strided_init(np.zeros(8, np.float32), 3, source=0)
    with pytest.raises(TypeError):
        mpix.irecv_reduce_strided_enqueue((ok.ctypes.data, 32), source=0)


def test_err_arg_at_the_call(mpix_env):
    C = mpix_env._C
    buf = np.zeros(256, np.float64)
    addr = buf.ctypes.data
    arg = f"rc={C.ERR_ARG}$"

    def enq(addr, run, c0, c1, s0, s1, typ, op=C.SUM):
        return C.irecv_reduce_strided(addr, run, c0, c1, s0, s1, typ, op, 0,
                                      90, C.QUEUE_STREAM, 0)

    def pinit(addr, run, c0, c1, s0, s1, typ, op=C.SUM, part_stride=512):
        return C.precv_init_reduce_strided(addr, 2, run, c0, c1, s0, s1,
                                           part_stride, typ, op, 0, 91)

    for call in (enq, pinit):
        # unknown type or op
        for typ, op in ((6, C.SUM), (-1, C.SUM), (C.F32, 3), (C.F32, -1)):
            with pytest.raises(RuntimeError, match=arg):
                call(addr, 16, 4, 1, 32, 128, typ, op)
        # an illegal layout: the stride steps into the run
        with pytest.raises(RuntimeError, match=arg):
            call(addr, 16, 4, 1, 8, 128, C.F32)
        # buffer not aligned to the element
        with pytest.raises(RuntimeError, match=arg):
            call(addr + 2, 16, 4, 1, 32, 128, C.F32)
        # run, stride[0], stride[1] not multiples of the element
        with pytest.raises(RuntimeError, match=arg):
            call(addr, 6, 4, 1, 32, 128, C.F32)
        with pytest.raises(RuntimeError, match=arg):
            call(addr, 8, 4, 1, 36, 144, C.F64)
        with pytest.raises(RuntimeError, match=arg):
            call(addr, 8, 2, 2, 16, 100, C.F64)
    # part_stride: a multiple of the element, and the rules of precv_init
    with pytest.raises(RuntimeError, match=arg):
        pinit(addr, 16, 4, 1, 32, 128, C.F64, part_stride=516)
    with pytest.raises(RuntimeError, match=arg):
        pinit(addr, 16, 4, 1, 32, 128, C.F64, part_stride=64)
    # the same shape is fine for a smaller element
    mpix_env.request_free(pinit(addr, 6, 4, 1, 32, 128, C.F16))
    # a stride of an unused level may be anything
    r = enq(addr, 16, 1, 1, 3, 5, C.F64)
    mpix_env.wait(mpix_env.isend_enqueue(np.ones(2), dest=0, tag=90))
    assert mpix_env.wait(r)["error"] == 0
    assert (buf[:2] == 1).all() and (buf[2:] == 0).all()
