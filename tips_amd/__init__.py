"""tips_amd — MI355X-native gradient-bucket reduction behind TiPS's allreduce API.

Drop-in surface of `tips.tensorflow` for the collective-allreduce path
(reference tips/tensorflow/__init__.py:20-103,189-227, ops.py, basics.py,
compression.py), over numpy arrays and torch tensors instead of TF tensors
(TensorFlow is not in this image). Everything below reaches the GPU through
libtips_hip.so (include/tips_hip.h); there is no CPU fallback.
"""
import os as _os

from .basics import TipsBasics, init, is_initialized, rank, shutdown, size
from .compression import Compression, Compressor, FP16Compressor, MXFP8Compressor, MXFP8ErrorFeedback, NoneCompressor
from .ops import (Handle, allgather_async, allgather_op, allreduce_async, broadcast_async, allreduce_async_many, synchronize_many, allreduce_op, broadcast_op, poll, synchronize, broadcast_variables, bucket_sum, fused_allreduce,
                  fused_allreduce_, rank_op, registered_host_buffer, set_algorithm, set_consistency_check, size_op)
from .ops import fused_allreduce_cast, fused_allreduce_flat, fused_allreduce_host, fused_allreduce_host_flat, fusion_stats
from .ops import set_op_scaling, allreduce_reduce_op
from .ops import adasum_op, fused_adasum_flat
from .ops import (allreduce_mxfp8, fused_allreduce_mxfp8, mxfp8_dequantize, mxfp8_fold, mxfp8_quantize,
                  mxfp8_wire_bytes)
from .ops import allreduce_mxfp8_ef, fused_allreduce_mxfp8_ef, mxfp8_ef_bytes, mxfp8_fold_ef, mxfp8_quantize_ef
from .ops import mxfp8_fold_segs, reducescatter_mxfp8_layout
from ._lib import TipsError, TipsLibraryError
from . import ops as _ops
from . import tensors as _tensors

Average = 'Average'
Sum = 'Sum'
Min = 'Min'
Max = 'Max'
Adasum = 'Adasum'


class IndexedSlices(object):
    """A sparse gradient: rows `values` of a dense tensor of `dense_shape`, at row `indices`
    (what tf.IndexedSlices carries, e.g. an embedding gradient). The represented tensor is the
    sum over repeated indices."""

    def __init__(self, values, indices, dense_shape=None):
        self.values = values
        self.indices = indices
        self.dense_shape = dense_shape

__all__ = [
    "allreduce", "IndexedSlices", "allreduce_async", "broadcast_async", "allgather_async", "allreduce_async_many", "synchronize_many", "poll", "synchronize", "Handle", "allreduce_grads", "allreduce_op", "allgather_op", "broadcast_op", "broadcast_variables",
    "set_consistency_check", "registered_host_buffer", "bucket_sum", "fused_allreduce", "fused_allreduce_", "init",
    "shutdown",
    "is_initialized", "size", "rank", "size_op", "rank_op", "set_algorithm", "Compression", "Compressor",
    "NoneCompressor", "FP16Compressor", "Average", "Sum", "TipsBasics", "TipsError", "TipsLibraryError",
    "DistributedOptimizer", "DistributedGradientTape", "fused_allreduce_cast", "fused_allreduce_flat", "fused_allreduce_host", "fused_allreduce_host_flat", "fusion_stats",
    "allreduce_scaled", "set_op_scaling", "Min", "Max", "allreduce_reduce_op",
    "sparse_allreduce", "set_sparse_reduce", "sparse_stats",
    "Adasum", "adasum_op", "fused_adasum_flat",
    "MXFP8Compressor", "allreduce_mxfp8", "fused_allreduce_mxfp8", "mxfp8_quantize", "mxfp8_fold", "mxfp8_dequantize",
    "mxfp8_wire_bytes",
    "MXFP8ErrorFeedback", "allreduce_mxfp8_ef", "fused_allreduce_mxfp8_ef", "mxfp8_ef_bytes", "mxfp8_fold_ef",
    "mxfp8_quantize_ef",
    "reducescatter", "grouped_reducescatter",
    "reducescatter_mxfp8_layout", "mxfp8_fold_segs",
]


def reducescatter(tensor, op=Average, prescale_factor=1.0, postscale_factor=1.0, name=None, compression=Compression.none):
    """This rank's rows of the reduction of `tensor` over all ranks (Horovod's reducescatter;
    tips_reducescatter; DESIGN.md, Reduce-scatter).

    `tensor` [rows, ...] is split along dimension 0: with base = rows // size() and rem = rows % size(),
    rank q owns base + (q < rem) rows from row q * base + min(q, rem), possibly none. Returns a new
    tensor [own rows, ...] of the same dtype holding postscale_factor * SUM over ranks of
    (prescale_factor * x), ranks in ascending order, in fp32 (f64 for float64, the integer type for
    integers), every multiply and add a separate operation and one rounding at the store: the same
    bits on every run, and bit for bit that slice of the direct allreduce, so
    allgather_op(reducescatter(x, op=Sum)) is allreduce's result under TIPS_ALGO=direct. op=Average
    divides by size() through the postscale factor, whatever set_op_scaling says; op=Max / Min are the
    exact compares of allreduce_reduce_op. A dense device torch tensor (made contiguous if it is not)
    of float32, float64, float16, bfloat16, int32 or int64; the same op, factors and shape on every
    rank. ValueError, before anything is initialised, for a 0-dim, host or sparse tensor, an integer
    dtype with op=Average or a factor, op=Max / Min with a factor, op=Adasum, and a `name` (named
    requests carry SUM allreduce only).

    compression=Compression.fp8 sends a float32 tensor through the MXFP8 reduce-scatter
    (tips_reducescatter_mxfp8): every peer's slice travels as e4m3fn bytes with one
    power-of-two scale per 32 elements, quantised once; this rank's own slice is not quantised; the
    fold is in f32 in rank order, times the one factor prescale_factor * postscale_factor (divided by
    size() for Average) - a quarter of the plain reduce-scatter's bytes on the links. Tensors of every
    other dtype travel uncompressed. ValueError for op=Max / Min with it, and for an MXFP8ErrorFeedback
    object: error feedback for the reduce-scatter is not implemented. Any other compressor
    (Compression.fp16) composes as for allreduce: compress, reduce-scatter in the compressed dtype,
    decompress."""
    return _reducescatter_compressed([tensor], op, prescale_factor, postscale_factor, name, compression)[0]


def grouped_reducescatter(tensors, op=Average, prescale_factor=1.0, postscale_factor=1.0, name=None,
                          compression=Compression.none):
    """reducescatter of every tensor of a list, one exchange and one fold launch per (dtype, device)
    group (tips_grouped_reducescatter): rank q receives every tensor's slice q in one RCCL group and
    the fold writes the outputs straight from the staged bytes. Returns the list of this rank's
    shards; None entries pass through. Arguments and refusals as reducescatter; under
    compression=Compression.fp8 every (float32, device) group is one tips_grouped_reducescatter_mxfp8."""
    return _reducescatter_compressed(tensors, op, prescale_factor, postscale_factor, name, compression)


def _reducescatter_compressed(tensors, op, prescale_factor, postscale_factor, name, compression):
    if _is_ef(compression):
        raise ValueError("reducescatter takes no MXFP8ErrorFeedback: error feedback for the reduce-scatter's wire is not "
                         "implemented (use Compression.fp8)")
    if compression is MXFP8Compressor:
        if op in (Max, Min):
            raise ValueError("op=%s does not combine with Compression.fp8: the MXFP8 wire carries SUM (and Average) only" % op)
        return _ops.grouped_reducescatter_op(tensors, op, prescale_factor, postscale_factor, name, mxfp8=True)
    if compression is NoneCompressor:
        return _ops.grouped_reducescatter_op(tensors, op, prescale_factor, postscale_factor, name)
    tensors = list(tensors)
    _ops._check_reducescatter(tensors, op, float(prescale_factor), float(postscale_factor), name)
    packed = [(None, None) if t is None else compression.compress(t) for t in tensors]
    outs = _ops.grouped_reducescatter_op([c for c, _ in packed], op, prescale_factor, postscale_factor, name)
    return [None if o is None else compression.decompress(o, ctx) for o, (_, ctx) in zip(outs, packed)]


def allreduce_scaled(tensor, prescale_factor=1.0, postscale_factor=1.0, name=None):
    """postscale_factor * SUM over ranks of (prescale_factor * tensor): the scaled allreduce, whatever
    set_op_scaling says (ops.allreduce_scaled_op: the factors sit inside the library's sum kernels;
    with a `name` they are applied unfused around the named SUM). Float dtypes; the same factors on
    every rank."""
    return _ops.allreduce_scaled_op(tensor, prescale_factor, postscale_factor, name=name)


def _op_scale(op, prescale_factor=1.0, postscale_factor=1.0):
    """(prescale, postscale) a reduction runs with under set_op_scaling(True), or None for the plain
    SUM (the switch is off, or nothing to scale): op=Average divides postscale by size(); op=Sum and
    None sum, as the sparse branch treats them."""
    if not _ops.op_scaling():
        return None
    pre, post = float(prescale_factor), float(postscale_factor)
    if op == Average:
        post = post / size()
    return None if (pre == 1.0 and post == 1.0) else (pre, post)


def _no_mxfp8_op(compression, op):
    """Compression.fp8 rides the sum only: Max, Min and Adasum with it raise before any collective."""
    if (compression is MXFP8Compressor or _is_ef(compression)) and op in (Max, Min, Adasum):
        raise ValueError("op=%s does not combine with Compression.fp8: the MXFP8 wire carries SUM (and Average) only"
                         % op)


def _is_ef(compression):
    return isinstance(compression, MXFP8ErrorFeedback)


def _no_integer_average(tensor, op):
    if op == Average and _ops.op_scaling() and _ops._is_integer(tensor):
        raise ValueError("op=Average is not defined for integer tensors (dtype %s): reduce with op=Sum" % tensor.dtype)


def allreduce(tensor,
              average=None,
              device_dense='',
              device_sparse='',
              compression=Compression.none,
              op=None,
              prescale_factor=1.0,
              postscale_factor=1.0,
              name=None):
    """Sum `tensor` over all ranks — mirrors tips.tensorflow.allreduce (__init__.py:20-91).

    Same arguments as the reference. By default, as in the reference, `op`,
    `prescale_factor` and `postscale_factor` do not reach the reduction (they
    are commented out at the C++ boundary, __init__.py:82-87), so the result
    is the plain SUM for op=Average too — parity with the
    reference, not a recommendation. After set_op_scaling(True) (or with
    TIPS_OP_SCALING=1) they do: the result is postscale_factor * SUM over
    ranks of (prescale_factor * tensor), op=Average dividing postscale_factor
    by size() (op=Sum and None sum), computed by allreduce_scaled with the
    factors inside the sum kernels; an integer tensor with op=Average raises
    ValueError. `average`, `device_dense` and `device_sparse` are accepted for
    signature compatibility.

    Sparse gradients take the reference's allgather branch (__init__.py:59-74).
    An `IndexedSlices` gets its values and indices allgathered, and they are
    divided by size() for op=Average, as the reference does there. A torch
    sparse COO tensor gets the same treatment on its nonzeros. The result
    represents the summed tensor.

    op=Max / op=Min return the elementwise maximum / minimum over the ranks
    (ops.allreduce_reduce_op -> tips_allreduce_op), whatever set_op_scaling
    says: exact in the tensor's dtype, integers compared signed, floats by
    IEEE 754-2019 maximum / minimum (a NaN on any rank gives a NaN, -0 < +0).
    `compression` composes as for the sum. They raise ValueError with a scale
    factor other than 1, a sparse input or a `name` (named requests carry SUM
    only).

    op=Adasum returns the Adasum of the ranks' tensors (ops.adasum_op ->
    tips_allreduce_adasum), whatever set_op_scaling says: the
    binary tree over a power-of-two number of ranks of ca a + cb b with
    ca = 1 - a.b / (2 a.a), cb = 1 - a.b / (2 b.b), the dot products over the
    whole tensor in f64. Dense device float tensors; `compression` composes as
    for the sum (the tree then runs in the compressed dtype). It raises
    ValueError with a scale factor other than 1, a `name`, a sparse input, an
    integer dtype or a host tensor.

    compression=Compression.fp8 sends a dense float32 device tensor through the
    MXFP8 collective (ops.allreduce_mxfp8): e4m3fn bytes with one
    power-of-two scale per 32 elements on the wire, the ranks' blocks folded in
    rank order in f32 and requantised once. Under set_op_scaling(True) the
    factors travel as one float32 factor prescale * postscale applied at the
    dequantise. Every other tensor - host, another dtype, sparse, or a call with
    a `name` - travels uncompressed, exactly as under Compression.none. op=Max,
    Min or Adasum with it raises ValueError before any collective.

    compression=Compression.fp8.error_feedback() (an MXFP8ErrorFeedback object,
    DESIGN.md §17) does the same with the quantisers' residuals carried from call
    to call (ops.allreduce_mxfp8_ef). The state of a tensor is keyed by
    (name, numel, device), so `name` is required - without one the call raises
    ValueError - and it names the state only: the tensor does not become a named
    request. Tensors that are not dense float32 device tensors travel
    uncompressed under that name.
    """
    _no_mxfp8_op(compression, op)
    if _is_ef(compression) and name is None:
        raise ValueError("allreduce(compression=<MXFP8ErrorFeedback>) needs a name: the tensor's residual state is keyed by "
                         "(name, numel, device)")
    if op in (Max, Min):
        return _allreduce_minmax(tensor, compression, op, prescale_factor, postscale_factor, name)
    if op == Adasum:
        return _allreduce_adasum(tensor, compression, prescale_factor, postscale_factor, name)
    if isinstance(tensor, IndexedSlices):
        values = allgather_op(tensor.values)
        indices = allgather_op(tensor.indices)
        new_values = (values / size()) if op == Average else values
        return IndexedSlices(new_values, indices, dense_shape=tensor.dense_shape)
    if _tensors.is_torch(tensor) and tensor.is_sparse:
        torch = _ops._torch()
        idx = tensor._indices().t().contiguous()  # (nnz, ndim): rows concatenate along dim 0
        vals = tensor._values().contiguous()
        g_idx = allgather_op(idx).t()
        g_vals = allgather_op(vals)
        if op == Average:
            g_vals = g_vals / size()
        return torch.sparse_coo_tensor(g_idx, g_vals, tensor.shape)
    _no_integer_average(tensor, op)
    scale = _op_scale(op, prescale_factor, postscale_factor)
    if compression is MXFP8Compressor and name is None and _ops.is_mxfp8_tensor(tensor):
        return allreduce_mxfp8(tensor, 1.0 if scale is None else scale[0] * scale[1])
    if _is_ef(compression) and _ops.is_mxfp8_tensor(tensor):
        init()
        state = compression.tensor_state(name, tensor.numel(), tensor.device, size())
        return allreduce_mxfp8_ef(tensor, state, 1.0 if scale is None else scale[0] * scale[1])
    tensor_compressed, ctx = compression.compress(tensor)
    if scale is not None:
        summed_tensor_compressed = allreduce_scaled(tensor_compressed, scale[0], scale[1], name=name)
    else:
        summed_tensor_compressed = allreduce_op(tensor_compressed, name=name)
    return compression.decompress(summed_tensor_compressed, ctx)


def _no_factors(op, prescale_factor, postscale_factor, why):
    if float(prescale_factor) != 1.0 or float(postscale_factor) != 1.0:
        raise ValueError("op=%s takes no prescale_factor / postscale_factor: %s" % (op, why))


def _no_name(op, name):
    if name is not None:
        raise ValueError("op=%s takes no name: named requests go through the negotiation, which carries SUM only" % op)


def _allreduce_minmax(tensor, compression, op, prescale_factor, postscale_factor, name):
    """allreduce(op=Max | Min): the argument checks (before anything is initialised), then compress,
    reduce, decompress."""
    _no_factors(op, prescale_factor, postscale_factor, "scaling does not combine with a maximum or minimum")
    if isinstance(tensor, IndexedSlices) or (_tensors.is_torch(tensor) and tensor.is_sparse):
        raise ValueError("op=%s is not defined for sparse inputs (their allgather branch sums repeated indices): "
                         "densify first" % op)
    _no_name(op, name)
    tensor_compressed, ctx = compression.compress(tensor)
    return compression.decompress(allreduce_reduce_op(tensor_compressed, op), ctx)


def _allreduce_adasum(tensor, compression, prescale_factor, postscale_factor, name):
    """allreduce(op=Adasum): the argument checks (before anything is initialised), then compress,
    reduce, decompress."""
    _no_factors(Adasum, prescale_factor, postscale_factor, "there is no scaled Adasum")
    _no_name(Adasum, name)
    if isinstance(tensor, IndexedSlices):
        raise ValueError("op=Adasum is not defined for sparse inputs: densify first")
    _ops.check_adasum_tensor(tensor)
    tensor_compressed, ctx = compression.compress(tensor)
    return compression.decompress(adasum_op(tensor_compressed), ctx)


def _adasum_grads(grads, compression, fused):
    """allreduce_grads(op=Adasum) at N > 1: the argument checks for the whole list first, then the
    dense device float gradients per (dtype, device) through fused_adasum_flat, each gradient a segment
    of its own (fused=False: one adasum_op each). With a compression every gradient is compressed on
    its own, the compressed list is reduced, and every result decompressed (unfused casts)."""
    for g in grads:
        if g is None:
            continue
        if isinstance(g, IndexedSlices):
            raise ValueError("op=Adasum is not defined for sparse gradients: densify first")
        _ops.check_adasum_tensor(g, "allreduce_grads(op=Adasum)")
    out = list(grads)
    groups = {}
    for i, g in enumerate(grads):
        if g is None:
            continue
        c, ctx = compression.compress(g)
        c = c if c.is_contiguous() else c.contiguous()
        if not fused:
            out[i] = compression.decompress(adasum_op(c), ctx)
            continue
        groups.setdefault((c.dtype, c.device), []).append((i, c, ctx))
    for members in groups.values():
        for (i, _, ctx), s in zip(members, fused_adasum_flat([c for _, c, _ in members])):
            out[i] = compression.decompress(s, ctx)
    return out


_sparse_reduce = _os.environ.get("TIPS_SPARSE_REDUCE", "0") == "1"


def set_sparse_reduce(enabled):
    """Whether allreduce_grads(..., sparse_as_dense=True), DistributedOptimizer and
    DistributedGradientTape send device sparse gradients through sparse_allreduce (TIPS_SPARSE_REDUCE=1
    sets the initial value). Off, the default, is today's route: torch.index_add_ builds the dense
    table on every rank and the whole table is allreduced. On, only the entries cross the links and
    the ordered row-sum kernels build the table - the same on every rank and from run to run. Host
    sparse gradients, and any list reduced with a compression, keep today's route. The setting must be
    the same on every rank."""
    global _sparse_reduce
    _sparse_reduce = bool(enabled)


def _sparse_parts(slices, scaled):
    """(values [n, ...] contiguous, indices [n] int64, dense_shape) of an IndexedSlices or a torch
    sparse COO tensor, on one device; ValueError for what sparse_allreduce does not take (`scaled`:
    the call carries a factor or op=Average, which integer values refuse)."""
    if isinstance(slices, IndexedSlices):
        if slices.dense_shape is None:
            raise ValueError("sparse_allreduce needs the IndexedSlices' dense_shape")
        values, indices = slices.values, slices.indices
        shape = tuple(int(d) for d in slices.dense_shape)
    elif _tensors.is_torch(slices) and slices.is_sparse:
        if slices.sparse_dim() != 1:
            raise ValueError("sparse_allreduce takes a COO tensor with one sparse dimension (the row index) and dense "
                             "trailing dimensions; this one has %d sparse dimensions" % slices.sparse_dim())
        values, indices = slices._values(), slices._indices()[0]
        shape = tuple(int(d) for d in slices.shape)
    else:
        raise ValueError("sparse_allreduce takes an IndexedSlices or a torch sparse COO tensor (got %s)" % type(slices).__name__)
    if scaled and _ops._is_integer(values):
        raise ValueError("integer values (dtype %s) take no scale factor and no op=Average: reduce with op=Sum"
                         % values.dtype)
    if not (_tensors.is_device(values) and _tensors.is_device(indices)):
        raise ValueError("sparse_allreduce takes device tensors only (host pointers are not staged): host sparse "
                         "gradients go through the allgather branch, allreduce(IndexedSlices)")
    if values.device != indices.device:
        raise ValueError("values and indices must be on one device")
    torch = _ops._torch()
    if indices.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        raise ValueError("indices must be integers (got %s)" % indices.dtype)
    if len(shape) < 1 or indices.dim() != 1 or values.dim() < 1 or values.shape[0] != indices.shape[0] or \
            tuple(int(d) for d in values.shape[1:]) != shape[1:]:
        raise ValueError("values %s / indices %s do not fit dense_shape %s" %
                         (tuple(values.shape), tuple(indices.shape), shape))
    return values.contiguous(), indices.to(torch.int64).contiguous(), shape


def sparse_allreduce(slices, op=None, prescale_factor=1.0, postscale_factor=1.0, coalesced=False):
    """The dense sum of a sparse gradient over all ranks, by the ordered row-sum kernels
    (tips_sparse_allreduce; DESIGN.md, Sparse allreduce).

    `slices`: an IndexedSlices with dense_shape, or a torch sparse COO tensor whose first dimension
    is the only sparse one. Device tensors of float32, float64, float16, bfloat16, int32 or int64.
    Returns dense[j] = postscale_factor * (sum over the entries with index j of prescale_factor *
    values[i]), the entries taken in ascending (rank, position) order and folded left to right in
    fp32 (f64 for float64, the integer type for integers), rounded once: the same bits on every rank
    and on every run; rows nothing names are +0. Entries whose index is outside [0, rows) are skipped
    and counted (sparse_stats); under set_consistency_check(True) they raise ValueError after the
    reduction (one synchronisation). With coalesced=True: an IndexedSlices of the ascending unique
    indices (torch.unique of the gathered indices) and their summed rows, taken from the dense
    result. op=Average divides by size() through the postscale factor, whatever set_op_scaling says;
    op=Max / Min, an integer dtype with a factor (or op=Average), and host tensors raise ValueError
    before anything is initialised."""
    if op in (Max, Min):
        raise ValueError("op=%s is not defined for sparse inputs: the row sum adds repeated indices" % op)
    pre, post = float(prescale_factor), float(postscale_factor)
    values, indices, shape = _sparse_parts(slices, op == Average or pre != 1.0 or post != 1.0)
    code = _tensors.dtype_code(values)
    torch = _ops._torch()
    init()
    if op == Average:
        post = post / size()
    rows = shape[0]
    row_elems = 1
    for d in shape[1:]:
        row_elems *= d
    n = int(indices.shape[0])
    with torch.cuda.device(values.device):
        dense = torch.empty(shape, dtype=values.dtype, device=values.device)
        _ops._lib.call("tips_sparse_allreduce", values.data_ptr() if n else None, indices.data_ptr() if n else None, n,
                       rows, row_elems, code, pre, post, dense.data_ptr() if dense.numel() else None,
                       _tensors.stream_of(values))
        gathered = None
        if _ops._check or coalesced:
            gathered = allgather_op(indices) if size() > 1 else indices
        if _ops._check and gathered.numel():
            lo, hi = int(gathered.min()), int(gathered.max())
            if lo < 0 or hi >= rows:
                raise ValueError("sparse_allreduce: indices outside [0, %d) (min %d, max %d) were skipped" % (rows, lo, hi))
        if not coalesced:
            return dense
        uniq = torch.unique(gathered)
        uniq = uniq[(uniq >= 0) & (uniq < rows)]
        return IndexedSlices(dense.index_select(0, uniq), uniq, dense_shape=shape)


def sparse_stats():
    """(calls, entries, bad_indices) of this process's row sums: launches, the entries they covered,
    and the entries skipped for an index outside [0, rows). Synchronises the device."""
    import ctypes
    v = [ctypes.c_int64() for _ in range(3)]
    _ops._lib.call("tips_sparse_stats", *[ctypes.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def _device_sparse(g):
    """A sparse gradient sparse_allreduce takes: device values and indices, a dense shape, one sparse dimension."""
    if isinstance(g, IndexedSlices):
        return g.dense_shape is not None and _tensors.is_device(g.values) and _tensors.is_device(g.indices)
    return _tensors.is_torch(g) and g.is_sparse and g.is_cuda and g.sparse_dim() == 1


def _no_minmax_grads(op):
    if op in (Max, Min):
        raise ValueError("op=%s is not supported for gradient lists: the fused reductions carry SUM only "
                         "(reduce single tensors with allreduce(tensor, op=%s))" % (op, op))


def _allreduce_cond(tensor, *args, **kwargs):
    """size() > 1 ? allreduce(tensor) : tensor  (__init__.py:94-103)."""
    if size() > 1:
        return allreduce(tensor, *args, **kwargs)
    return tensor


def _to_dense(g):
    """tf.convert_to_tensor of an IndexedSlices (rows summed over repeated indices), or a torch
    sparse tensor's dense form; anything else unchanged."""
    if isinstance(g, IndexedSlices):
        if g.dense_shape is None:
            raise ValueError("sparse_as_dense needs the IndexedSlices' dense_shape")
        if _tensors.is_torch(g.values):
            torch = _ops._torch()
            dense = torch.zeros(tuple(int(d) for d in g.dense_shape), dtype=g.values.dtype, device=g.values.device)
            idx = g.indices if _tensors.is_torch(g.indices) else torch.as_tensor(g.indices)
            return dense.index_add_(0, idx.to(dense.device, torch.int64), g.values)
        import numpy as np
        dense = np.zeros(tuple(int(d) for d in g.dense_shape), dtype=np.asarray(g.values).dtype)
        np.add.at(dense, np.asarray(g.indices), np.asarray(g.values))
        return dense
    if _tensors.is_torch(g) and g.is_sparse:
        return g.to_dense()
    return g


def allreduce_grads(grads, compression=Compression.none, op=None, fused=True, sparse_as_dense=False,
                    gradient_predivide_factor=1.0):
    """Allreduce a list of gradients (None entries pass through).

    Mirrors the per-gradient loop of _make_cached_allreduce_grads_fn
    (__init__.py:203-222), including the size()==1 identity of
    _allreduce_cond and `sparse_as_dense` (__init__.py:205-210: sparse
    gradients are densified first and then take the dense path). With
    fused=True, device tensors are summed through the fusion buckets (one
    allreduce per <=64 MiB bucket instead of one per gradient); outputs are
    new tensors, inputs are left unchanged. Under set_op_scaling(True),
    op=Average returns the average: the device lists through
    tips_fused_allreduce_flat_scaled (postscale 1/size() inside each bucket's
    sums); Compression.fp16 lists through the cast path followed by one
    tips_scale per output buffer (unfused); host tensors one scaled allreduce
    each. gradient_predivide_factor f (op=Average only) splits the division:
    prescale 1/f before the sums, postscale f/size() after them.

    op=Adasum takes effect whatever set_op_scaling says: dense device float
    gradients go per (dtype, device) through fused_adasum_flat, each gradient
    a segment with its own coefficients (fused=False: one adasum_op each);
    None entries and size() == 1 pass through as for the sum. Under
    Compression.fp16 each gradient is compressed, the list is reduced in
    float16 and each result decompressed - unfused casts, one launch per
    gradient each way. Host or sparse gradients raise ValueError.

    Compression.fp8: the dense float32 device gradients go through the MXFP8
    collective - per device one fused_allreduce_mxfp8 call with fused=True, one
    allreduce_mxfp8 per gradient otherwise - with the factor prescale * postscale
    under set_op_scaling(True); every other gradient (host, another dtype,
    sparse) is reduced uncompressed, exactly as under Compression.none.
    op=Max, Min or Adasum with it raises ValueError.

    Compression.fp8.error_feedback() (an MXFP8ErrorFeedback object, DESIGN.md
    §17): as Compression.fp8, with the dense float32 device gradients of each
    device through fused_allreduce_mxfp8_ef over the object's state of
    (device, counts, size()) - zeros at a signature's first step, carried from
    step to step after it. fused=False raises ValueError (a state belongs to a
    list).
    """
    _no_mxfp8_op(compression, op)
    if _is_ef(compression) and not fused:
        raise ValueError("allreduce_grads(fused=False) does not combine with MXFP8 error feedback: the residual state "
                         "belongs to the fused list")
    _no_minmax_grads(op)
    if op == Adasum:
        if gradient_predivide_factor != 1.0:
            raise ValueError("gradient_predivide_factor not supported with op != Average")
        if sparse_as_dense:
            grads = [_to_dense(g) if g is not None else g for g in grads]
        if size() <= 1:
            return list(grads)
        return _adasum_grads(grads, compression, fused)
    if sparse_as_dense and _sparse_reduce and compression is Compression.none and any(_device_sparse(g) for g in grads):
        return _reduce_grads_sparse(grads, compression, op, fused, gradient_predivide_factor)
    if sparse_as_dense:
        grads = [_to_dense(g) if g is not None else g for g in grads]
    if size() <= 1:
        return list(grads)
    return _reduce_checked(grads, compression, op, fused, gradient_predivide_factor)


def _reduce_grads_sparse(grads, compression, op, fused, gradient_predivide_factor):
    """allreduce_grads(sparse_as_dense=True) under set_sparse_reduce(True): the device sparse
    gradients go through sparse_allreduce, one call each - with the factors the dense route would
    apply (_average_scale: op=Average divides only under set_op_scaling, as for the dense gradients
    of the same list) - and come back dense and reduced; the rest of the list takes today's route."""
    scale = _average_scale(op, gradient_predivide_factor) if size() > 1 else None
    pre, post = scale if scale is not None else (1.0, 1.0)
    out, rest = list(grads), []
    for i, g in enumerate(grads):
        if g is not None and _device_sparse(g):
            out[i] = sparse_allreduce(g, prescale_factor=pre, postscale_factor=post)
            rest.append(None)
        else:
            rest.append(_to_dense(g) if g is not None else g)
    if size() > 1 and any(g is not None for g in rest):
        rest = _reduce_checked(rest, compression, op, fused, gradient_predivide_factor)
    return _merged(out, rest)


def _merged(out, rest):
    """`out` with every entry of `rest` that is not None in its place: a list reduced in two parts."""
    for i, g in enumerate(rest):
        if g is not None:
            out[i] = g
    return out


def _average_scale(op, gradient_predivide_factor=1.0):
    """_op_scale of a gradient reduction: op=Average with gradient_predivide_factor f is
    prescale 1/f, postscale f/size()."""
    f = float(gradient_predivide_factor)
    return _op_scale(op, 1.0 / f, f) if op == Average else _op_scale(op)


def _route(g, compression, scale, fused):
    """The way one gradient of a list takes through _reduce_grads - the route table. `scale` is
    (prescale, postscale), or None for the plain sum (set_op_scaling off, or nothing to scale).

      gradient                                      scale is None       under a scale
      sparse (IndexedSlices, torch sparse)          "own"               "own"
      dense, fused=False                            "own"               "scaled"
      device float32 under Compression.fp16         "cast"              "cast"
      device, Compression.none                      "dev"               "dev"
      device, another compressor or dtype           "dev"               "scaled"
      host (numpy, CPU torch)                       "host"              "scaled"

    "own": allreduce(g, compression=compression, op=op), inside the loop - a sparse gradient's
    allgather branch, which divides for op=Average whatever the switch says. "dev": compressed, then
    with its (dtype, device) group through tips_fused_allreduce_flat, under a scale
    tips_fused_allreduce_flat_scaled with the factors inside each bucket's sums. "cast": with its
    device's group through the fused cast path, fp16 on the wire; under a scale followed by one
    tips_scale per flat output buffer (unfused). "host": compressed, then with its dtype group through
    fused_allreduce_host_flat. "scaled": compressed, one allreduce_scaled, inside the loop - the host
    path and the compressed device groups have no scaled entry. Under a scale an integer gradient that
    is not sparse raises ValueError, and no plan is looked up or remembered."""
    if scale is None and not fused:
        return "own"
    kind = _kind(g)
    if kind is None:
        return "own"
    if scale is not None and _ops._is_integer(g):
        raise ValueError("op=Average is not defined for integer gradients (dtype %s)" % g.dtype)
    if fused and kind == "dev":
        if compression is FP16Compressor and g.dtype == _ops._torch().float32:
            return "cast"
        if scale is None or compression is Compression.none:
            return "dev"
    return "host" if scale is None else "scaled"


def _reduce_grads(grads, compression=Compression.none, op=None, fused=True, gradient_predivide_factor=1.0):
    """What allreduce_grads runs at N > 1 (bench.py times it on one rank, where allreduce_grads
    itself is the identity). With fused=True:
      - dense device gradients, per dtype: fused_allreduce_flat - the outputs are views of one flat
        buffer laid out as the fusion buckets, each bucket packed into it and allreduced in place
        (a layout depends on the counts only, so fresh gradient tensors every step hit the caches);
      - dense host gradients (numpy / CPU torch: the reference's op is a CPU op, ops.cc:118), per
        dtype: fused_allreduce_host_flat - packed into page-locked pieces by host threads,
        pipelined H2D -> allreduce -> D2H straight into one page-locked flat host buffer, the
        outputs views of it (reused as the device flat outputs are);
      - the rest (sparse) one by one, through the reference's allgather branch.
    Under set_op_scaling(True) with something to scale (op=Average at N > 1) every gradient is
    postscale * SUM(prescale * g); _route says which entry carries the factors."""
    if op in (Max, Min):
        _no_minmax_grads(op)
    if not fused and _is_ef(compression):
        raise ValueError("fused=False does not combine with MXFP8 error feedback")
    return _reduce_checked(grads, compression, op, fused, gradient_predivide_factor)


def _reduce_checked(grads, compression, op, fused, gradient_predivide_factor):
    """_reduce_grads behind its argument checks (allreduce_grads has made them already)."""
    if compression is MXFP8Compressor or _is_ef(compression):
        return _reduce_grads_mxfp8(grads, op, fused, gradient_predivide_factor, compression if _is_ef(compression) else None)
    none = compression is Compression.none
    scale = _average_scale(op, gradient_predivide_factor)
    if fused and grads and scale is None and compression is FP16Compressor:  # (one list of dense f32 device tensors)
        res = _ops._dev_list_cast(grads)
        if res is not None:
            return res
    if fused and none and grads:
        res = _ops._dev_list_flat(grads, scale)  # (one dtype of dense device tensors: the common case)
        if res is not None:
            return res
        plan = _find_plan(grads) if scale is None else None
        if plan is not None:  # the same tensor objects as a recent call: no per-tensor inspection
            res = plan.run(grads)
            if res is not None:
                return res
            _PLANS.remove(plan)
    out = list(grads)
    dev, host, cast = {}, {}, {}
    simple = fused and none and scale is None  # only dense, contiguous device tensors: the split can be remembered
    for i, g in enumerate(grads):
        if g is None:
            continue
        route = _route(g, compression, scale, fused)
        if route == "own":
            out[i] = allreduce(g, compression=compression, op=op)
            simple = False
        elif route == "cast":
            # Compression.fp16 fused into the buckets: cast while packed, fp16 on the wire, cast back
            # while unpacked (tips_fused_allreduce_cast) - no per-tensor cast launches
            cast.setdefault(g.device, []).append((i, g if g.is_contiguous() else g.contiguous()))
        else:
            c, ctx = (g, None) if none else compression.compress(g)
            if route == "scaled":
                s = allreduce_scaled(c, scale[0], scale[1])
                out[i] = s if none else compression.decompress(s, ctx)
            elif route == "dev":
                if not c.is_contiguous():
                    c = c.contiguous()
                    simple = False
                dev.setdefault((c.dtype, c.device), []).append((i, c, ctx))
            else:
                c = _tensors.contiguous(c)
                host.setdefault(str(c.dtype), []).append((i, c, ctx))
    plan_groups = []
    for members in dev.values():
        ts = [c for _, c, _ in members]
        sums = _ops._flat_call(ts, _tensors.dtype_code(ts[0]), list(map(_ops._torch().Tensor.data_ptr, ts)), scale)
        for (i, _, ctx), s in zip(members, sums):
            out[i] = s if none else compression.decompress(s, ctx)
        plan_groups.append(([i for i, _, _ in members], None, None))
    for members in cast.values():
        for (i, _), s in zip(members, _ops.fused_allreduce_cast([c for _, c in members], "float16", scale)):
            out[i] = s
    for members in host.values():
        ts = [c for _, c, _ in members]
        sums = _ops.fused_allreduce_host_flat(ts)
        if simple:
            # a plan re-reads the pointers with the fast reader and re-checks shapes and dtypes:
            # only for lists of the inputs themselves (contiguous, not copies) that it reads right
            ok = all(c is grads[i] for i, c, _ in members) and \
                _tensors.host_data_ptrs(ts) == [_tensors.data_ptr(t) for t in ts]
            if ok:
                plan_groups.append(([i for i, _, _ in members], _ops._host_flat_outputs(ts),
                                    [(t.shape, t.dtype) for t in ts]))
            else:
                simple = False
        for (i, _, ctx), s in zip(members, sums):
            out[i] = s if none else compression.decompress(s, ctx)
    if simple:
        _remember_plan(grads, plan_groups)
    return out


def _reduce_grads_mxfp8(grads, op, fused, gradient_predivide_factor, ef=None):
    """_reduce_grads under Compression.fp8: the dense float32 device gradients through the MXFP8
    collective (per device one fused_allreduce_mxfp8, or one allreduce_mxfp8 each with fused=False),
    the factor prescale * postscale of set_op_scaling multiplied in double; the rest of the list as
    under Compression.none. `ef`: an MXFP8ErrorFeedback - per device one fused_allreduce_mxfp8_ef over
    its state of (device, counts, size())."""
    scale = _average_scale(op, gradient_predivide_factor)
    factor = 1.0 if scale is None else scale[0] * scale[1]
    out, rest, groups = list(grads), [], {}
    for i, g in enumerate(grads):
        if g is not None and _ops.is_mxfp8_tensor(g):
            g = g if g.is_contiguous() else g.contiguous()
            if fused:
                groups.setdefault(g.device, []).append((i, g))
            else:
                out[i] = allreduce_mxfp8(g, factor)
            rest.append(None)
        else:
            rest.append(g)
    for device, members in groups.items():
        ts = [g for _, g in members]
        if ef is None:
            sums = fused_allreduce_mxfp8(ts, factor)
        else:
            sums = fused_allreduce_mxfp8_ef(ts, ef.list_state(device, [g.numel() for g in ts], size()), factor)
        for (i, _), s in zip(members, sums):
            out[i] = s
    if any(g is not None for g in rest):
        rest = _reduce_checked(rest, Compression.none, op, fused, gradient_predivide_factor)
    return _merged(out, rest)


_PLANS = []       # recent _GradPlans, most recent first


class _GradPlan(object):
    """How _reduce_grads split one list of dense gradients, kept for a later call with the SAME
    tensor objects (a training loop whose .grad tensors persist, or a set of gradient buffers used
    in turn): such a call is recognised through weak references and skips the per-tensor Python
    inspection (kind, dtype, contiguity, shape), which costs more host time for 1000 gradients than
    the fused allreduce's device work. A plan whose tensors one has died never matches again (a
    weak-reference callback marks it), and a position that was None must be None again: a dead
    gradient cannot pass for a None one. Tensors can still change in place (.data =, set_, resize_,
    a numpy array's shape), so every call re-reads each group through the checking readers: device
    groups through _ops._dev_list_flat (pointers, counts, dtype, contiguity in C++), host groups
    through their recorded shapes and dtypes; any difference plans again."""

    def __init__(self, grads, groups):
        import weakref
        self.dead = False

        def died(_ref, plan=weakref.ref(self)):
            p = plan()
            if p is not None:
                p.dead = True
        self.refs = [weakref.ref(g, died) if g is not None else _NONE_REF for g in grads]
        self.n = len(grads)
        # [(positions, None, None)] for device groups, [(positions, _HostFlatOutputs,
        # [(shape, dtype)])] for host groups
        self.groups = groups
        self.whole = len(groups) == 1 and groups[0][0] == list(range(self.n))

    def matches(self, grads):
        import operator
        import weakref
        if self.dead or len(grads) != self.n:
            return False
        # a live tensor's reference returns it; a None position's returns None (_NONE_REF)
        return all(map(operator.is_, map(weakref.ref.__call__, self.refs), grads))

    def run(self, grads):
        """The outputs, or None when a tensor changed in place (the caller plans again)."""
        out = list(grads)
        for pos, fo, meta in self.groups:
            ts = grads if self.whole else [grads[i] for i in pos]
            if meta is None:
                sums = _ops._dev_list_flat(ts)  # (None: not one dtype of dense contiguous device tensors now)
                if sums is None:
                    return None
            else:
                if any(t.shape != shp or t.dtype is not dt for t, (shp, dt) in zip(ts, meta)):
                    return None
                sums = _ops._host_flat_run(fo, _tensors.host_data_ptrs(ts))
            if self.whole:
                return sums
            for i, s in zip(pos, sums):
                out[i] = s
        return out


class _Gone(object):
    pass


def _dead():
    import weakref
    return weakref.ref(_Gone())  # (the object is gone at once: the reference reads None, as a None gradient)


_NONE_REF = _dead()  # the reference of a position that held None (only a plan's None positions use it)


def _find_plan(grads):
    for k, p in enumerate(_PLANS):
        if p.matches(grads):
            if k:
                _PLANS.insert(0, _PLANS.pop(k))
            return p
    return None


def _remember_plan(grads, groups):
    if not groups:
        return
    _PLANS.insert(0, _GradPlan(grads, groups))
    del _PLANS[8:]


def _kind(g):
    """'dev' for a dense device tensor, 'host' for a dense host tensor (numpy, CPU torch), None for
    anything reduced on its own (sparse)."""
    if _tensors.is_torch(g):
        if g.is_sparse:
            return None
        return "dev" if g.is_cuda else "host"
    if isinstance(g, IndexedSlices):
        return None
    return "host"


def _fusable(g):
    """Dense device tensors go through the fusion buckets; sparse and host ones are reduced one by one."""
    return g is not None and _tensors.is_device(g) and not g.is_sparse


from .optim import DistributedGradientTape, DistributedOptimizer  # noqa: E402  (uses allreduce_grads above)
