"""mpix — MI355X-native accelerator-triggered MPI extensions.

Python surface over the MPIX_* C API (see include/mpix/mpix.h).  Buffers may
be torch tensors (CPU or HIP), numpy arrays, or raw (address, nbytes) pairs;
streams are torch.cuda.Stream objects or raw hipStream_t addresses.

The native extension (mpix/_C.so) is REQUIRED — there is no Python/eager
fallback.  Build with `make python` (hipcc, gfx950).
"""
from __future__ import annotations

import os

# Load torch's bundled HIP runtime FIRST if torch is present: torch ships its
# own libamdhip64 (same SONAME libamdhip64.so.7 as /opt/rocm's). If _C.so
# loads the /opt/rocm runtime first, torch later loads a SECOND copy (its
# DT_NEEDED is the unversioned "libamdhip64.so", which never matches an
# already-loaded soname) and two HSA runtimes in one process leave
# torch.cuda.is_available() == False on a live GPU. Importing torch first
# means _C.so's libamdhip64.so.7 dependency resolves to torch's
# already-loaded copy and both stacks share one runtime.
try:  # pragma: no cover - torch is optional for pure C-API consumers
    import torch as _torch  # noqa: F401
except ImportError:
    pass

try:
    from . import _C  # type: ignore[attr-defined]
except ImportError as e:  # pragma: no cover
    raise ImportError(
        "mpix native extension not built. Run `make python` at the repo root "
        f"(hipcc --offload-arch=gfx950). Original error: {e}"
    ) from e

QUEUE_STREAM = _C.QUEUE_STREAM
QUEUE_GRAPH = _C.QUEUE_GRAPH
ANY_SOURCE = _C.ANY_SOURCE
ANY_TAG = _C.ANY_TAG

Request = _C.Request
Status = _C.Status
Prequest = _C.Prequest


def _addr_len(buf, nbytes=None):
    """Resolve (address, nbytes) from a tensor / ndarray / (addr, len)."""
    if hasattr(buf, "data_ptr"):  # torch tensor
        addr = buf.data_ptr()
        n = buf.numel() * buf.element_size()
    elif hasattr(buf, "ctypes"):  # numpy array
        addr = buf.ctypes.data
        n = buf.nbytes
    elif isinstance(buf, tuple):
        addr, n = buf
    else:
        raise TypeError(f"unsupported buffer type {type(buf)}")
    if nbytes is not None:
        n = nbytes
    return int(addr), int(n)


def _layout_of(buf):
    """Layout of a non-contiguous tensor / ndarray view, or None when `buf`
    is contiguous (C order), a tuple, or empty.

    Returns (address, (run_bytes, count0, count1, stride0, stride1)): the
    view's elements in C order are runs of run_bytes bytes, count0 of them
    stride0 bytes apart per plane, count1 planes stride1 bytes apart
    (MPIX_Layout).  Dimensions are collapsed from the innermost outwards;
    a view that needs more than a run plus two strided levels, or that has
    zero or negative strides (expand, flip) or steps backwards over itself
    (a transpose), raises ValueError."""
    if hasattr(buf, "data_ptr"):  # torch tensor
        if buf.is_contiguous() or buf.numel() == 0:
            return None
        item = buf.element_size()
        shape = tuple(buf.shape)
        strides = tuple(s * item for s in buf.stride())
        addr = buf.data_ptr()
    elif hasattr(buf, "ctypes"):  # numpy array
        if buf.flags["C_CONTIGUOUS"] or buf.size == 0:
            return None
        item = buf.itemsize
        shape = tuple(buf.shape)
        strides = tuple(buf.strides)
        addr = buf.ctypes.data
    else:
        return None

    def bad(why):
        return ValueError(
            f"cannot send/receive a view of shape {shape} with byte strides "
            f"{strides}: {why}")

    run = item
    levels = []  # [count, stride], innermost first
    for size, stride in zip(reversed(shape), reversed(strides)):
        if size == 1:
            continue
        if stride <= 0:
            raise bad("zero or negative strides (expand, flip) are not "
                      "supported")
        if not levels and stride == run:
            run *= size
        elif levels and stride == levels[-1][0] * levels[-1][1]:
            levels[-1][0] *= size
        else:
            levels.append([size, stride])
    if len(levels) > 2:
        raise bad("it does not collapse into a contiguous run plus two "
                  "strided levels")
    extent = run
    for count, stride in levels:
        if stride < extent:
            raise bad("an outer dimension steps over less than the inner "
                      "ones span (transposed or overlapping view)")
        extent = stride * (count - 1) + extent
    while len(levels) < 2:
        levels.append([1, extent])
    return int(addr), (int(run), int(levels[0][0]), int(levels[1][0]),
                       int(levels[0][1]), int(levels[1][1]))


def _sendrecv(is_send, buf, peer, tag, qtype, stream, nbytes):
    """Contiguous buffers and (addr, nbytes) tuples take the plain bindings;
    non-contiguous views go out as a layout."""
    lay = _layout_of(buf)
    if lay is None:
        addr, n = _addr_len(buf, nbytes)
        if qtype == QUEUE_GRAPH:
            f = _C.isend_graph if is_send else _C.irecv_graph
            return f(addr, n, peer, tag)
        f = _C.isend_enqueue if is_send else _C.irecv_enqueue
        return f(addr, n, peer, tag, QUEUE_STREAM, _stream_addr(stream))
    if nbytes is not None:
        raise ValueError("nbytes= cannot be combined with a non-contiguous "
                         "buffer: the view defines the message")
    addr, (run, c0, c1, s0, s1) = lay
    return _C.sendrecv_strided(is_send, addr, run, c0, c1, s0, s1, peer, tag,
                               qtype, _stream_addr(stream))


def _stream_addr(stream):
    if stream is None:
        return 0
    if hasattr(stream, "cuda_stream"):  # torch.cuda.Stream
        return int(stream.cuda_stream)
    return int(stream)


def init():
    """Initialize mpix.  Call after MPI_Init (MPI mode) or with
    RANK/WORLD_SIZE/MASTER_ADDR in the environment (torchrun mode)."""
    _C.init()


def finalize():
    _C.finalize()


def world():
    """(rank, world_size)."""
    return _C.world()


def have_gpu():
    return _C.have_gpu()


def config():
    """Resolved runtime config (after init): gpu, memOps probe, mode."""
    return _C.config()


def isend_enqueue(buf, dest, tag=0, stream=None, nbytes=None):
    """Send `buf`: a tensor / ndarray (contiguous or a strided view whose
    elements go out in C order, see _layout_of) or an (address, nbytes)
    pair."""
    return _sendrecv(True, buf, dest, tag, QUEUE_STREAM, stream, nbytes)


def irecv_enqueue(buf, source, tag=0, stream=None, nbytes=None):
    return _sendrecv(False, buf, source, tag, QUEUE_STREAM, stream, nbytes)


def isend_graph(buf, dest, tag=0, nbytes=None):
    """Graph-construction enqueue: returns (request, graph_handle)."""
    return _sendrecv(True, buf, dest, tag, QUEUE_GRAPH, None, nbytes)


def irecv_graph(buf, source, tag=0, nbytes=None):
    return _sendrecv(False, buf, source, tag, QUEUE_GRAPH, None, nbytes)


# ------------------------- reducing receives ------------------------------

_REDUCE_OPS = {"sum": _C.SUM, "max": _C.MAX, "min": _C.MIN}
_REDUCE_TYPES = {"float32": _C.F32, "float64": _C.F64, "bfloat16": _C.BF16,
                 "float16": _C.F16, "int32": _C.I32, "int64": _C.I64}


def _reduce_args(buf, op, views=False):
    """(address, elements, type, op) of a reducing receive into `buf`: a
    contiguous torch tensor (float32, float64, bfloat16, float16, int32,
    int64) or numpy array (the same without bfloat16).  ValueError for any
    other dtype, a non-contiguous view (unless `views`: the strided reducing
    receives, which take the address and the layout from the view) or an
    unknown op."""
    if op not in _REDUCE_OPS:
        raise ValueError(f"unknown reduce op {op!r}: one of "
                         f"{sorted(_REDUCE_OPS)}")
    if hasattr(buf, "data_ptr"):  # torch tensor
        name = str(buf.dtype).replace("torch.", "")
        contiguous = buf.is_contiguous()
        addr, count = buf.data_ptr(), buf.numel()
    elif hasattr(buf, "ctypes"):  # numpy array
        name = buf.dtype.name
        contiguous = bool(buf.flags["C_CONTIGUOUS"])
        addr, count = buf.ctypes.data, buf.size
    else:
        raise TypeError(f"unsupported buffer type {type(buf)}: a reducing "
                        f"receive takes its element type from the dtype")
    if name not in _REDUCE_TYPES:
        raise ValueError(f"cannot reduce into dtype {name}: one of "
                         f"{sorted(_REDUCE_TYPES)}")
    if not contiguous and not views:
        raise ValueError("a reducing receive needs a contiguous buffer (for "
                         "a view: irecv_reduce_strided_enqueue, "
                         "irecv_reduce_strided_graph, "
                         "precv_reduce_strided_init)")
    return int(addr), int(count), _REDUCE_TYPES[name], _REDUCE_OPS[op]


def irecv_reduce_enqueue(buf, source, op="sum", tag=0, stream=None):
    """Receive a message and COMBINE it into `buf`: on completion
    buf[i] = buf[i] op msg[i] (op: "sum", "max", "min").  The element type
    is the dtype of `buf`; the sender uses the plain calls.  The request
    behaves like irecv_enqueue's."""
    addr, count, typ, rop = _reduce_args(buf, op)
    return _C.irecv_reduce(addr, count, typ, rop, source, tag, QUEUE_STREAM,
                           _stream_addr(stream))


def irecv_reduce_graph(buf, source, op="sum", tag=0):
    """Graph-construction variant: returns (request, graph_handle).  Every
    launch of the graph combines again."""
    addr, count, typ, rop = _reduce_args(buf, op)
    return _C.irecv_reduce(addr, count, typ, rop, source, tag, QUEUE_GRAPH, 0)


def precv_reduce_init(buf, partitions, source, op="sum", tag=0):
    """Partitioned reducing receive: `buf` is cut into `partitions` equal
    slices and each arriving partition is combined into its slice.  Every
    iteration (start) accumulates again; reset `buf` in between."""
    addr, count, typ, rop = _reduce_args(buf, op)
    if partitions <= 0 or count % partitions != 0:
        raise ValueError(f"{count} elements do not divide evenly into "
                         f"{partitions} partitions")
    return _C.precv_init_reduce(addr, partitions, count // partitions, typ,
                                rop, source, tag)


def _irecv_reduce_strided(buf, source, op, tag, qtype, stream):
    _, count, typ, rop = _reduce_args(buf, op, views=True)
    lay = _layout_of(buf)  # ValueError for what does not fit a layout
    if lay is None:
        addr, n = _addr_len(buf)
        layout = (n, 1, 1, n, n)
    else:
        addr, layout = lay
    return _C.irecv_reduce_strided(addr, *layout, typ, rop, source, tag,
                                   qtype, _stream_addr(stream))


def irecv_reduce_strided_enqueue(buf, source, op="sum", tag=0, stream=None):
    """irecv_reduce_enqueue into `buf`, a contiguous tensor / ndarray or any
    view irecv_enqueue accepts (see _layout_of): the message's elements are
    combined into the view's elements in C order, and what lies between them
    is neither read nor written.  The sender may send a contiguous buffer or
    any view with the same number of bytes."""
    return _irecv_reduce_strided(buf, source, op, tag, QUEUE_STREAM, stream)


def irecv_reduce_strided_graph(buf, source, op="sum", tag=0):
    """Graph-construction variant: returns (request, graph_handle).  Every
    launch of the graph combines again."""
    return _irecv_reduce_strided(buf, source, op, tag, QUEUE_GRAPH, None)


def precv_reduce_strided_init(buf, partitions, source, op="sum", tag=0):
    """Partitioned reducing receive into `buf`, a contiguous tensor / ndarray
    cut into `partitions` equal slices or a view whose dimension 0 is split
    into `partitions` equal slabs (as precv_init): each arriving partition
    is combined into its slab.  Every iteration (start) accumulates
    again."""
    _, count, typ, rop = _reduce_args(buf, op, views=True)
    if not _is_view(buf):
        if partitions <= 0 or count % partitions != 0:
            raise ValueError(f"{count} elements do not divide evenly into "
                             f"{partitions} partitions")
        addr, n = _addr_len(buf)
        per = n // partitions
        layout, part_stride = (per, 1, 1, per, per), per
    else:
        addr, layout, part_stride = _view_partitions(buf, partitions)
    return _C.precv_init_reduce_strided(addr, partitions, *layout,
                                        part_stride, typ, rop, source, tag)


def waitall_graph(reqs):
    return _C.waitall_graph(list(reqs))


def wait_graph(req):
    """Per-request wait graph (explicit-construction composition)."""
    return _C.wait_graph(req)


def wait_enqueue(req, stream=None, status=None):
    _C.wait_enqueue(req, status, _stream_addr(stream))


def waitall_enqueue(reqs, stream=None):
    _C.waitall_enqueue(list(reqs), _stream_addr(stream))


def wait(req):
    """Host-side wait; returns a status dict."""
    return _C.wait(req)


def waitall(reqs):
    return [wait(r) for r in reqs]


def request_free(req):
    _C.request_free(req)


# ----------------------------- partitioned --------------------------------

def _is_view(buf):
    """A non-empty tensor / ndarray that is not C-contiguous."""
    if hasattr(buf, "data_ptr"):
        return buf.numel() > 0 and not buf.is_contiguous()
    if hasattr(buf, "ctypes"):
        return buf.size > 0 and not buf.flags["C_CONTIGUOUS"]
    return False


def _pinit(is_send, buf, partitions, peer, tag, nbytes):
    """Contiguous buffers and (addr, nbytes) tuples take the plain bindings;
    a non-contiguous view is split along dimension 0 into partitions that
    are laid out alike."""
    if not _is_view(buf):
        addr, n = _addr_len(buf, nbytes)
        assert n % partitions == 0, "buffer must divide evenly into partitions"
        f = _C.psend_init if is_send else _C.precv_init
        return f(addr, partitions, n // partitions, peer, tag)
    if nbytes is not None:
        raise ValueError("nbytes= cannot be combined with a non-contiguous "
                         "buffer: the view defines the partitions")
    addr, layout, part_stride = _view_partitions(buf, partitions)
    return _C.psend_precv_init_strided(is_send, addr, partitions, *layout,
                                       part_stride, peer, tag)


def _view_partitions(buf, partitions):
    """(address, layout, part_stride) of the `partitions` equal slabs that
    dimension 0 of the non-contiguous view `buf` splits into."""
    shape = tuple(buf.shape)
    if hasattr(buf, "data_ptr"):
        item = buf.element_size()
        strides = tuple(s * item for s in buf.stride())
        addr = buf.data_ptr()
    else:
        item = buf.itemsize
        strides = tuple(buf.strides)
        addr = buf.ctypes.data
    if partitions <= 0 or shape[0] % partitions != 0:
        raise ValueError(
            f"cannot split a view of shape {shape} into {partitions} "
            f"partitions: they split dimension 0, which must divide evenly")
    rows = shape[0] // partitions
    part_stride = rows * strides[0]
    if partitions > 1 and part_stride <= 0:
        raise ValueError(
            f"cannot send/receive a view of shape {shape} with byte strides "
            f"{strides} as partitions: zero or negative strides (expand, "
            f"flip) are not supported")
    part = buf[:rows]
    lay = _layout_of(part)  # ValueError for what does not fit a layout
    if lay is None:  # one partition of the view is contiguous
        n = rows * item
        for size in shape[1:]:
            n *= size
        layout = (n, 1, 1, n, n)
    else:
        layout = lay[1]
    return int(addr), layout, int(part_stride)


def psend_init(buf, partitions, dest, tag=0, nbytes=None):
    """Partitioned send of `buf`: a contiguous tensor / ndarray or an
    (address, nbytes) pair cut into `partitions` equal slices, or a
    non-contiguous view whose dimension 0 is split into `partitions` equal
    slabs (each one partition, sent in C order without packing)."""
    return _pinit(True, buf, partitions, dest, tag, nbytes)


def precv_init(buf, partitions, source, tag=0, nbytes=None):
    return _pinit(False, buf, partitions, source, tag, nbytes)


def start(req):
    _C.start(req)


def startall(reqs):
    for r in reqs:
        _C.start(r)


def pready(partition, req):
    _C.pready(partition, req)


def parrived(req, partition):
    return _C.parrived(req, partition)


def prequest_create(req):
    return _C.prequest_create(req)


def prequest_free(preq):
    _C.prequest_free(preq)


# ----------------------------- graph helpers ------------------------------

graph_chain_instantiate = _C.graph_chain_instantiate
graph_instantiate = _C.graph_instantiate
graph_launch = _C.graph_launch
graph_exec_destroy = _C.graph_exec_destroy
graph_destroy = _C.graph_destroy
stream_begin_capture = _C.stream_begin_capture
stream_end_capture = _C.stream_end_capture

# ----------------------------- test kernels -------------------------------

launch_pready_all = _C.launch_pready_all
launch_wait_arrived_all = _C.launch_wait_arrived_all
launch_fill_and_pready = _C.launch_fill_and_pready
launch_wait_and_check = _C.launch_wait_and_check
