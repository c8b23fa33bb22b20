"""Op bindings — mirrors tips/tensorflow/ops.py:24-95 over the C-ABI.

`allreduce_op` is the MPIAllreduce op (ops.cc:79-136): an out-of-place SUM of
one tensor over all ranks, output of the input's shape and dtype. Device
(torch CUDA/HIP) tensors stay in HBM and are ordered on the caller's current
stream; host tensors (numpy / CPU torch) are staged through HBM and the call
returns when the result is in host memory, like the reference's CPU op.
"""
import os
import re
import threading

from . import _fast  # (built in-tree by `make`: tips_amd/_fast*.so; no Python fallback)
from . import _lib
from . import basics
from . import tensors
from .tensors import _torch  # torch, imported on first use (tips_amd/__init__.py uses this accessor too)


def _normalize_name(name):
    """Normalizes operation name to TensorFlow rules (ops.py:33-35)."""
    return re.sub('[^a-zA-Z0-9_]', '_', name)


def size_op(name=None):
    """Number of ranks (ops.py:45-47; MPISize, ops.cc:21-48)."""
    return basics.size()


def rank_op(name=None):
    """This process's rank (ops.py:53-55; MPIRank, ops.cc:50-77)."""
    return basics.rank()


_check = os.environ.get("TIPS_CHECK_CONSISTENCY", "0") == "1"


def set_consistency_check(enabled):
    """Validate dtype/shape across ranks before every allreduce (the reference's rank-0
    negotiation, coordinator.cc:90-186): one small exchange per call. Off by default."""
    global _check
    _check = bool(enabled)


_op_scaling = os.environ.get("TIPS_OP_SCALING", "0") == "1"


def set_op_scaling(enabled):
    """Whether `op`, `prescale_factor`, `postscale_factor` and `gradient_predivide_factor` reach the
    reduction (TIPS_OP_SCALING=1 sets the initial value). Off, the default, is the reference's
    behaviour: they are accepted and the result is the plain SUM. On, allreduce / allreduce_grads /
    DistributedGradientTape / DistributedOptimizer compute postscale * SUM(prescale * x), op=Average
    dividing postscale by size(), through the scaled entry points of the library (the factors sit
    inside its sum kernels). The setting, like the factors, must be the same on every rank."""
    global _op_scaling
    _op_scaling = bool(enabled)


def op_scaling():
    return _op_scaling


def _shape(t):
    return tuple(int(d) for d in t.shape)


def _is_integer(t):
    return tensors.dtype_code(t) in (_lib.INT32, _lib.INT64)


def scale_(tensor, factor):
    """tensor *= factor in place on the device (tips_scale: one multiply per element in fp32, or
    f64 for float64, rounded once); a contiguous device tensor of a float dtype."""
    n = tensors.numel(tensor)
    if n:
        _lib.call("tips_scale", tensors.data_ptr(tensor), tensors.data_ptr(tensor), n, tensors.dtype_code(tensor),
                  float(factor), tensors.stream_of(tensor))
    return tensor


def allreduce_scaled_op(tensor, prescale_factor=1.0, postscale_factor=1.0, name=None):
    """postscale_factor * SUM over ranks of (prescale_factor * tensor), out of place
    (tips_allreduce_scaled): every element is multiplied by prescale_factor where a sum kernel first
    reads it and every finished sum by postscale_factor where it is written, each multiply and add a
    separate IEEE operation in fp32 (f64 for float64), rounded once per kernel - the bytes moved are
    those of the plain allreduce. Float dtypes; always scales, whatever set_op_scaling says; the
    factors must be the same on every rank. Device or host tensors, as allreduce_op.

    With a `name` the request goes through the negotiation as the named SUM does today, and the
    factors are applied UNFUSED around it: a scaled copy (tips_scale), the named SUM, tips_scale of
    the result - two more passes over the tensor. Device tensors only on that path."""
    basics.init()
    code = tensors.dtype_code(tensor)
    src = tensors.contiguous(tensor)
    pre, post = float(prescale_factor), float(postscale_factor)
    n = tensors.numel(src)
    if name is not None:
        if not tensors.is_device(src):
            raise TypeError("allreduce_scaled with a name takes a device tensor (tips_scale runs on the device)")
        tmp = tensors.empty_like(src)
        if n:
            _lib.call("tips_scale", tensors.data_ptr(tmp), tensors.data_ptr(src), n, code, pre, tensors.stream_of(src))
        return scale_(synchronize(allreduce_async(tmp, _normalize_name(name))), post)
    out = _HOST_OUT.take(src) if not tensors.is_device(src) else tensors.empty_like(src)
    if n:
        _lib.call("tips_allreduce_scaled", tensors.data_ptr(src), tensors.data_ptr(out), n, code, pre, post,
                  tensors.stream_of(src))
    return out


_REDUCE_OPS = {"Sum": _lib.OP_SUM, "Max": _lib.OP_MAX, "Min": _lib.OP_MIN}


def allreduce_reduce_op(tensor, op, name=None):
    """`op` ('Sum', 'Max' or 'Min') of `tensor` over all ranks, out of place (tips_allreduce_op):
    Max / Min are exact in the tensor's dtype - integers compared signed, floats by IEEE 754-2019
    maximum / minimum (a NaN on any rank gives a NaN, -0 < +0, subnormals kept) - and independent of
    the schedule; 'Sum' is allreduce_op's sum. Device or host tensors, as allreduce_op; `op` must be
    the same on every rank. A `name` is refused for Max / Min: named requests carry SUM only."""
    if op not in _REDUCE_OPS:
        raise ValueError("allreduce_reduce_op: op must be one of %s (got %r)" % (sorted(_REDUCE_OPS), op))
    if name is not None:
        if op != "Sum":
            raise ValueError("op=%s takes no name: named requests go through the negotiation, which carries SUM only" % op)
        return allreduce_op(tensor, name=name)
    basics.init()
    code = tensors.dtype_code(tensor)
    src = tensors.contiguous(tensor)
    out = _HOST_OUT.take(src) if not tensors.is_device(src) else tensors.empty_like(src)
    n = tensors.numel(src)
    if n:
        _lib.call("tips_allreduce_op", tensors.data_ptr(src), tensors.data_ptr(out), n, code, _REDUCE_OPS[op],
                  tensors.stream_of(src))
    return out


def allreduce_op(tensor, name=None):
    """Sum `tensor` over all ranks (ops.py:61-65 -> MPIAllreduce, ops.cc:86-115). With a `name`,
    through the negotiation like the reference's op (rank 0 validates and orders it; the name
    normalised as ops.py:33-35 does), and returns when it has run; without one, stream-ordered."""
    if name is not None:
        return synchronize(allreduce_async(tensor, _normalize_name(name)))
    basics.init()
    code = tensors.dtype_code(tensor)
    src = tensors.contiguous(tensor)
    out = _HOST_OUT.take(src) if not tensors.is_device(src) else tensors.empty_like(src)
    n = tensors.numel(src)
    if _check:
        shape = _shape(src) or (1,)  # scalars travel as shape [1] (CreateNoEmptyTfShape, coordinator.cc:212-221)
        sp, _keep = _lib.i64_array(shape)
        _lib.call("tips_allreduce_checked", tensors.data_ptr(src), tensors.data_ptr(out), sp, len(shape), code,
                  _lib.OP_SUM, tensors.stream_of(src))
    elif n:
        _lib.call("tips_allreduce", tensors.data_ptr(src), tensors.data_ptr(out), n, code, _lib.OP_SUM,
                  tensors.stream_of(src))
    return out


class _HostOutPool(object):
    """Outputs of host allreduces of at least 1 MiB (the reference's op works on CPU tensors,
    ops.cc:118): kept page-locked (tips_host_register) and handed out again once the caller has
    released them - no Python reference left and, for torch, no other tensor on the storage (numpy
    views hold a reference to their base). A fresh numpy / torch array of that size is new pages every
    call, and the D2H into it pays their first-touch faults: one 97.6 MiB numpy buffer took 16.7 ms
    per allreduce that way (profiles/r03/p_numa_probe.jsonl). Up to PER_KEY outputs per (kind, dtype,
    shape), TIPS_HOST_OUT_POOL_MIB (4096) page-locked in all; past that, fresh outputs as before."""

    MIN_BYTES = 1 << 20
    PER_KEY = 2

    def __init__(self):
        self.sets = {}
        self.bytes = 0
        self.lock = threading.Lock()

    @staticmethod
    def _free(e):
        import sys
        a = e[0]
        if sys.getrefcount(a) > 3:  # (the entry, the local a, getrefcount's argument)
            return False
        if e[1] is not None:  # torch: no other tensor on the storage
            torch = _torch()
            return torch._C._storage_Use_Count(a.untyped_storage()._cdata) == e[1]
        return True

    def take(self, src):
        is_t = tensors.is_torch(src)
        nbytes = src.numel() * src.element_size() if is_t else src.nbytes
        if nbytes < self.MIN_BYTES:
            return tensors.empty_like(src)
        key = (is_t, str(src.dtype), tuple(src.shape))
        with self.lock:  # (the check and the hand-out together: another thread cannot get it too)
            lst = self.sets.setdefault(key, [])
            for e in lst:
                if self._free(e):
                    return e[0]
            out = tensors.empty_like(src)
            cap = int(os.environ.get("TIPS_HOST_OUT_POOL_MIB", "4096")) << 20
            if len(lst) < self.PER_KEY and self.bytes + nbytes <= cap:
                if _lib.lib().tips_host_register(tensors.data_ptr(out), nbytes) == 0:
                    use0 = None
                    if is_t:
                        torch = _torch()
                        use0 = torch._C._storage_Use_Count(out.untyped_storage()._cdata)
                    lst.append((out, use0))
                    self.bytes += nbytes
            return out


_HOST_OUT = _HostOutPool()


def allgather_op(tensor, name=None):
    """Concatenate `tensor` from all ranks along dimension 0 (ops.py:72-76 -> MPIAllgather,
    ops.cc:156-212; sizes exchanged as GatherFirstRankSizes does, coordinator.cc:40-88). With a
    `name`, through the negotiation (allgather_async), as allreduce_op."""
    if name is not None:
        return synchronize(allgather_async(tensor, _normalize_name(name)))
    basics.init()
    code = tensors.dtype_code(tensor)
    src = tensors.contiguous(tensor)
    shape = _shape(src)
    if not shape:
        raise ValueError("An empty tensor found")
    if _check:
        rec = [_lib.REQ_ALLGATHER, code, len(shape)] + list(shape) + [0] * (_lib.MAX_DIMS - len(shape))
        table = _gather_records(rec)
        _lib.call("tips_check_requests", _lib.i64_array(table)[0], len(table) // _lib.REQUEST_WORDS)
    firsts = _allgather_i64([shape[0]])
    row = 1
    for d in shape[1:]:
        row *= d
    counts = [int(f) * row for f in firsts]
    out_shape = (sum(int(f) for f in firsts),) + shape[1:]
    if tensors.is_torch(src):
        torch = _torch()
        out = torch.empty(out_shape, dtype=src.dtype, device=src.device)
    else:
        import numpy as np
        out = np.empty(out_shape, dtype=src.dtype)
    cp, _keep = _lib.i64_array(counts)
    _lib.call("tips_allgatherv", tensors.data_ptr(src), tensors.numel(src), tensors.data_ptr(out), cp, code,
              tensors.stream_of(src))
    return out


def _allgather_i64(values):
    """Every rank's int64 words, rank-major (tips_allgather_i64)."""
    import ctypes
    p = basics.size()
    vp, _keep = _lib.i64_array(values)
    out = (ctypes.c_int64 * (p * len(values)))()
    _lib.call("tips_allgather_i64", vp, len(values), out)
    return [int(v) for v in out]


def _gather_records(rec):
    """Every rank's request record (rank-major table for tips_check_requests)."""
    return _allgather_i64(rec)


def broadcast_op(tensor, root_rank=0, name=None):
    """`tensor` of rank `root_rank`, on every rank (ops.py:83-87 -> MPIBroadcast, ops.cc:214-286).
    With a `name`, through the negotiation (broadcast_async), as allreduce_op."""
    if name is not None:
        return synchronize(broadcast_async(tensor, root_rank, _normalize_name(name)))
    basics.init()
    code = tensors.dtype_code(tensor)
    src = tensors.contiguous(tensor)
    out = _HOST_OUT.take(src) if not tensors.is_device(src) else tensors.empty_like(src)
    n = tensors.numel(src)
    if n:
        _lib.call("tips_broadcast", tensors.data_ptr(src), tensors.data_ptr(out), n, code, int(root_rank),
                  tensors.stream_of(src))
    return out


def broadcast_variables(variables, root_rank=0):
    """Overwrite each tensor in place with root_rank's value (functions.py:36-46)."""
    for v in variables:
        b = broadcast_op(v, root_rank)
        if tensors.is_torch(v):
            v.copy_(b)
        else:
            v[...] = b
    return variables


def fused_allreduce_(tensor_list):
    """In-place SUM of a list of same-dtype device tensors through fusion buckets.

    No reference counterpart (the reference issues one op per gradient,
    tips/tensorflow/__init__.py:212-222): the tensors are packed into buckets
    of at most TIPS_FUSION_THRESHOLD bytes (default 64 MiB), each bucket is
    allreduced once, and the sums are unpacked in place.
    """
    basics.init()
    if not tensor_list:
        return tensor_list
    code = _check_fusable(tensor_list, "fused_allreduce_")
    pp, _keep1 = _lib.ptr_array([t.data_ptr() for t in tensor_list])
    cp, _keep2 = _lib.i64_array([t.numel() for t in tensor_list])
    _lib.call("tips_fused_allreduce", pp, cp, len(tensor_list), code, tensors.stream_of(tensor_list[0]))
    return tensor_list


def fused_allreduce(tensor_list, out_list=None):
    """Out-of-place SUM of a list of same-dtype device tensors through the fusion buckets
    (tips_fused_allreduce_oop): returns new tensors (or fills `out_list`), inputs unchanged.
    Pack reads each input once and unpack writes each output once: 4 x the bytes in HBM
    traffic, no extra copy."""
    basics.init()
    if not tensor_list:
        return []
    code = _check_fusable(tensor_list, "fused_allreduce")
    outs = [tensors.empty_like(t) for t in tensor_list] if out_list is None else list(out_list)
    if len(outs) != len(tensor_list) or any(o.shape != t.shape or o.dtype != t.dtype or not o.is_contiguous()
                                            for o, t in zip(outs, tensor_list)):
        raise ValueError("out_list must hold one contiguous tensor of each input's shape and dtype")
    pi, _keep1 = _lib.ptr_array([t.data_ptr() for t in tensor_list])
    po, _keep2 = _lib.ptr_array([o.data_ptr() for o in outs])
    cp, _keep3 = _lib.i64_array([t.numel() for t in tensor_list])
    _lib.call("tips_fused_allreduce_oop", pi, po, cp, len(tensor_list), code, tensors.stream_of(tensor_list[0]))
    return outs


_WIRE_CODES = {"float16": _lib.FLOAT16, "bfloat16": _lib.BFLOAT16}


def fused_allreduce_cast(tensor_list, wire="float16", scale=None):
    """SUM of a list of float32 device tensors reduced in a 16-bit wire type
    (tips_fused_allreduce_cast): each tensor is cast to `wire` (round to nearest even) as it is
    packed into a fusion bucket, every bucket is allreduced in the wire type, and the sums are cast
    back to float32 as they are unpacked - Compression.fp16's compress -> allreduce -> decompress
    (tips/tensorflow/compression.py:49-66) with one pack and one unpack launch per bucket instead of
    two casts per tensor. Returns float32 views of one flat buffer (reused, as fused_allreduce_flat's,
    once every view is released); inputs unchanged.

    scale = (prescale, postscale): the cast path as above, then ONE tips_scale of the float32 flat
    output buffer by prescale * postscale - unfused (one more pass over the outputs), and the 16-bit
    sums on the wire are not predivided."""
    basics.init()
    if not tensor_list:
        return []
    code = _check_fusable(tensor_list, "fused_allreduce_cast")
    if code != _lib.FLOAT32:
        raise TypeError("fused_allreduce_cast: float32 tensors only (got dtype code %d)" % code)
    if wire not in _WIRE_CODES:
        raise ValueError("fused_allreduce_cast: wire must be one of %s" % sorted(_WIRE_CODES))
    res = _dev_list_cast(tensor_list, _WIRE_CODES[wire], scale)  # (dense, contiguous, one device: C++ reads the list)
    if res is not None:
        return res
    fo, pi, flat, views = _take_outputs(tensor_list, code)
    _lib.call("tips_fused_allreduce_cast", pi[0], _out_ptrs(fo, flat), fo.cp[0], len(tensor_list), code,
              _WIRE_CODES[wire], tensors.stream_of(tensor_list[0]))
    if scale is not None:
        scale_(flat, float(scale[0]) * float(scale[1]))
    return views


def _cache_put(cache, key, value, limit=16):
    """cache[key] = value in a small dict kept in insertion order: at `limit` entries the oldest goes
    first. Returns value."""
    if len(cache) >= limit:
        cache.pop(next(iter(cache)))
    cache[key] = value
    return value


class _OutputSets(object):
    """What the output sets of one list signature share, device (_FlatOutputs) or host
    (_HostFlatOutputs): the layout's byte offsets (tips_fused_layout: a function of the counts
    alone), the count array and dtype code of the library call, the pointer array of the previous
    call, and up to MAX_SETS sets of {one flat buffer, one view of it per tensor}, sets[i][0] the
    flat buffer. A subclass says how a set is allocated (_new_set) and how its release by the caller
    is measured (_released)."""

    MAX_SETS = 4

    def __init__(self, numels, code):
        import ctypes
        self.numels, self.code = numels, code
        self.cp = _lib.i64_array(numels)
        offs = (ctypes.c_int64 * len(numels))()
        self.total = _lib.check("tips_fused_layout", _lib.lib().tips_fused_layout(self.cp[0], len(numels), code, offs))
        self.offs = [int(o) for o in offs]
        self.sets = []
        self.last = (None, None)  # (pointer list, its ptr_array) of the previous call
        self.lock = threading.Lock()  # (the free check and the hand-out together, as _HostOutPool)

    def take(self):
        """(flat buffer, a new list of its views) for this call: a released set, or a new one (kept
        while there are fewer than MAX_SETS). The list is made here, before the library call releases
        the GIL, so another thread's take() already sees the set's views referenced and does not hand
        it out twice."""
        with self.lock:  # another thread's take() cannot see a set free between the check and the copy
            for s in self.sets:
                if self._released(s):
                    return s[0], list(s[1])
            return self._new_set(len(self.sets) < self.MAX_SETS)


class _FlatOutputs(_OutputSets):
    """Output sets of fused_allreduce_flat for one list signature (dtype, device, shapes). A set is
    handed out again once every tensor of it has been released by the caller: no Python reference
    to any of its views, and no other tensor sharing its storage (derived views included).
    Allocating the buffer and 1000 views per call costs milliseconds of host time - more than the
    device work of the whole allreduce."""

    def __init__(self, shapes, numels, code, dtype, device):
        _OutputSets.__init__(self, numels, code)
        self.es = _itemsize(dtype, True)
        self.shapes, self.dtype, self.device = shapes, dtype, device
        # bound here, once per signature: the release check and the stream lookup run on every call
        self.use_count = _torch()._C._storage_Use_Count
        self.cur_stream = _torch().cuda.current_stream

    def _released(self, s):
        flat, views, use0, rc0 = s
        if self.use_count(flat.untyped_storage()._cdata) != use0:
            return False
        return _fast.max_refcount(views) <= rc0

    def _new_set(self, keep):
        es = self.es
        flat = _torch().empty(max(1, self.total // es), dtype=self.dtype, device=self.device)
        views = [flat[o // es:o // es + n].view(shp) for o, n, shp in zip(self.offs, self.numels, self.shapes)]
        if keep:
            use0 = self.use_count(flat.untyped_storage()._cdata)
            rc0 = _fast.max_refcount(views)
            self.sets.append((flat, views, use0, rc0))
        return flat, list(views)


_FLAT_OUTPUTS = {}  # (dtype, device, shapes, layout settings) -> _FlatOutputs (small LRU)


def _layout_settings():
    """The settings a fusion layout depends on besides the counts (fusion.cc reads them per call):
    part of every flat-output cache key, so a changed setting never reuses offsets of another layout."""
    env = os.environ
    return (env.get("TIPS_FUSION_THRESHOLD"), env.get("TIPS_COPY_TILE_BYTES"), env.get("TIPS_FUSION_BALANCE"))


def fused_allreduce_flat(tensor_list, scale=None):
    """Out-of-place SUM of a list of same-dtype device tensors (tips_fused_allreduce_flat): the
    outputs are views of ONE flat buffer laid out as the fusion buckets - each bucket packed straight
    into it and allreduced there in place, no slot and no unpack (2 x the bytes of HBM traffic). The
    flat buffer and views are reused for a later call of the same list signature once the caller has
    released every output (_FlatOutputs). Inputs unchanged. scale = (prescale, postscale): each
    bucket's allreduce carries the factors inside its sums (tips_fused_allreduce_flat_scaled)."""
    basics.init()
    if not tensor_list:
        return []
    code = _check_fusable(tensor_list, "fused_allreduce_flat")
    return _flat_call(tensor_list, code, [t.data_ptr() for t in tensor_list], scale)


def _flat_outputs(tensor_list, code):
    """The _FlatOutputs of this list's signature (dtype, device, shapes)."""
    t0 = tensor_list[0]
    shapes = tuple(t.shape for t in tensor_list)
    key = (t0.dtype, t0.device, shapes, _layout_settings())
    fo = _FLAT_OUTPUTS.get(key)
    if fo is None:
        fo = _cache_put(_FLAT_OUTPUTS, key,
                        _FlatOutputs(shapes, [t.numel() for t in tensor_list], code, t0.dtype, t0.device))
    return fo


def _take_outputs(tensor_list, code):
    """(output set object of this list, (void** of its data pointers, keep-alive), flat buffer, views):
    what every flat entry that reads the list through Python starts from."""
    fo = _flat_outputs(tensor_list, code)
    pp = _lib.ptr_array([t.data_ptr() for t in tensor_list])
    return (fo, pp) + fo.take()


def _flat_issue(fo, pp, n, flat, device, scale):
    """The flat call itself: tips_fused_allreduce_flat of the n tensors at void** pp into `flat`, a
    buffer of output set `fo`, on `device`'s current stream; with scale = (prescale, postscale)
    tips_fused_allreduce_flat_scaled, the factors inside each bucket's sums."""
    if scale is not None:
        _lib.call("tips_fused_allreduce_flat_scaled", pp, fo.cp[0], n, fo.code, flat.data_ptr(), float(scale[0]),
                  float(scale[1]), fo.cur_stream(device).cuda_stream)
    else:
        _lib.call("tips_fused_allreduce_flat", pp, fo.cp[0], n, fo.code, flat.data_ptr(),
                  fo.cur_stream(device).cuda_stream)


def _flat_run(fo, tensor_list, ptrs, scale=None):
    """The flat call (_flat_issue: plain, or scaled by scale = (prescale, postscale)) of `tensor_list`,
    whose data pointers are `ptrs`, into an output set of `fo`; returns the outputs."""
    last = fo.last  # (one read: another thread may replace it)
    if ptrs == last[0]:
        pp = last[1]
    else:
        pp = _lib.ptr_array(ptrs)
        fo.last = (ptrs, pp)
    flat, views = fo.take()
    _flat_issue(fo, pp[0], len(ptrs), flat, tensor_list[0].device, scale)
    return views


# c10::ScalarType -> tips dtype code (Float, Double, Int, Long, Half, BFloat16)
_ST_CODES = {6: _lib.FLOAT32, 7: _lib.FLOAT64, 3: _lib.INT32, 4: _lib.INT64, 5: _lib.FLOAT16, 15: _lib.BFLOAT16}
_LIST_BUFS = threading.local()  # .d: n -> (pointer array, count array, their addresses), per thread:
                                # the library call releases the GIL while it reads them
_FAST_FLAT = {}   # (scalar type, device, n, shape hash, layout settings) -> (_FlatOutputs, count bytes)


def _list_scratch(n):
    """This thread's (pointer array, count array, their addresses) for _fast.dev_list of n tensors."""
    mine = getattr(_LIST_BUFS, "d", None)
    if mine is None:
        mine = _LIST_BUFS.d = {}
    bufs = mine.get(n)
    if bufs is None:
        import ctypes
        pa, na = (ctypes.c_void_p * n)(), (ctypes.c_int64 * n)()
        bufs = _cache_put(mine, n, (pa, na, ctypes.addressof(pa), ctypes.addressof(na)))
    return bufs


def _fast_list(tensor_list, want=None):
    """(the _FlatOutputs of the list, the scratch holding its data pointers and counts) of a list of
    dense, contiguous device tensors of one dtype (of dtype code `want`, when given) on one device,
    with the per-tensor host work in C++ (_fast.dev_list: data pointers, counts, a hash of the
    shapes); None when the list is not such a list. A training loop hands over fresh gradient tensors
    every step; this costs tens of nanoseconds per tensor where reading them through Python cost
    ~0.2 us."""
    n = len(tensor_list)
    try:
        bufs = _LIST_BUFS.d[n]  # (_list_scratch's entry, read without the call on the per-step path)
    except (AttributeError, KeyError):
        bufs = _list_scratch(n)
    r = _fast.dev_list(tensor_list, bufs[2], bufs[3], 1, n)
    if r is None:
        return None
    code = _ST_CODES.get(r[0])
    if code is None or (want is not None and code != want):
        return None
    import ctypes
    key = (r[0], r[1], n, r[2], _layout_settings())
    hit = _FAST_FLAT.get(key)
    counts = ctypes.string_at(bufs[3], 8 * n)
    if hit is None or hit[1] != counts:
        hit = _cache_put(_FAST_FLAT, key, (_flat_outputs(tensor_list, code), counts))
    return hit[0], bufs


def _dev_list_flat(tensor_list, scale=None):
    """fused_allreduce_flat of a list _fast_list takes: the outputs, or None when the list is not
    such a list (the caller's general path then inspects it tensor by tensor)."""
    hit = _fast_list(tensor_list)
    if hit is None:
        return None
    fo, bufs = hit
    flat, views = fo.take()
    _flat_issue(fo, bufs[0], len(tensor_list), flat, tensor_list[0].device, scale)
    return views


def _dev_list_cast(tensor_list, wire=_lib.FLOAT16, scale=None):
    """fused_allreduce_cast of a float32 list _fast_list takes (Compression.fp16's fast path in
    allreduce_grads); the float32 outputs, or None when the list is not such a list."""
    hit = _fast_list(tensor_list, _lib.FLOAT32)
    if hit is None:
        return None
    fo, bufs = hit
    flat, views = fo.take()
    _lib.call("tips_fused_allreduce_cast", bufs[0], _out_ptrs(fo, flat), fo.cp[0], len(tensor_list), _lib.FLOAT32, wire,
              fo.cur_stream(tensor_list[0].device).cuda_stream)
    if scale is not None:  # unfused: one tips_scale of the float32 output buffer
        scale_(flat, float(scale[0]) * float(scale[1]))
    return views


def _out_ptrs(fo, flat):
    """The data pointers of an output set's views (flat buffer + each view's offset), as a void**,
    cached per flat buffer."""
    cache = fo.__dict__.setdefault("out_ptrs", {})
    base = flat.data_ptr()
    hit = cache.get(base)
    if hit is None:
        import ctypes
        import numpy as np
        arr = np.asarray(fo.offs, dtype=np.uint64) + np.uint64(base)
        hit = _cache_put(cache, base, (arr, ctypes.cast(arr.ctypes.data, ctypes.POINTER(ctypes.c_void_p))),
                         2 * fo.MAX_SETS)
    return hit[1]


_ADASUM_FLOATS = (_lib.FLOAT32, _lib.FLOAT64, _lib.FLOAT16, _lib.BFLOAT16)


def check_adasum_tensor(t, what="op=Adasum"):
    """The dtype code of a tensor Adasum takes - a dense device float tensor - or ValueError; touches
    no library state."""
    if tensors.is_torch(t) and t.is_sparse:
        raise ValueError("%s is not defined for sparse inputs: densify first" % what)
    code = tensors.dtype_code(t)
    if code not in _ADASUM_FLOATS:
        raise ValueError("%s is defined for float dtypes only (got %s)" % (what, t.dtype))
    if not tensors.is_device(t):
        raise ValueError("%s takes device tensors only (host tensors are not staged)" % what)
    return code


def adasum_op(tensor):
    """Adasum of `tensor` over all ranks, out of place (tips_allreduce_adasum): the
    binary tree by recursive doubling of out = ca a + cb b, ca = 1 - d / (2 na), cb = 1 - d / (2 nb)
    with the dot products d, na, nb accumulated in f64 over the whole tensor. A power-of-two number
    of ranks; one rank returns a copy. A dense device float tensor; stream-ordered."""
    code = check_adasum_tensor(tensor, "adasum_op")
    basics.init()
    src = tensors.contiguous(tensor)
    out = tensors.empty_like(src)
    n = tensors.numel(src)
    if n:
        _lib.call("tips_allreduce_adasum", tensors.data_ptr(src), tensors.data_ptr(out), n, code, tensors.stream_of(src))
    return out


def fused_adasum_flat(tensor_list):
    """Adasum of a list of same-dtype device float tensors, each tensor a segment of its own - its own
    dot products and coefficients (tips_fused_allreduce_adasum_flat): the list is packed into one flat
    buffer laid out as fused_allreduce_flat's and reduced there, log2(size()) exchanges of the whole
    buffer. The outputs are views of that buffer, reused like fused_allreduce_flat's. Inputs unchanged."""
    if not tensor_list:
        return []
    for t in tensor_list:
        check_adasum_tensor(t, "fused_adasum_flat")
    basics.init()
    code = _check_fusable(tensor_list, "fused_adasum_flat")
    fo, pp, flat, views = _take_outputs(tensor_list, code)
    _lib.call("tips_fused_allreduce_adasum_flat", pp[0], fo.cp[0], len(tensor_list), code, flat.data_ptr(),
              fo.cur_stream(tensor_list[0].device).cuda_stream)
    return views


def is_mxfp8_tensor(t):
    """A tensor the MXFP8 collectives take: a dense float32 device tensor."""
    return tensors.is_torch(t) and t.is_cuda and not t.is_sparse and t.dtype == _torch().float32


def _check_mxfp8_list(tensor_list, what):
    for t in tensor_list:
        if not is_mxfp8_tensor(t):
            raise ValueError("%s takes dense float32 device tensors only" % what)
        if not t.is_contiguous():
            raise ValueError("%s needs contiguous tensors" % what)


def mxfp8_wire_bytes(flat_elems):
    """(bytes of the MXFP8 wire buffer of `flat_elems` flat elements, offset of its scale bytes):
    round_up(E, 256) + round_up(E / 32, 256) and round_up(E, 256) (tips_mxfp8_wire_bytes; pure host)."""
    import ctypes
    so = ctypes.c_int64()
    return int(_lib.call("tips_mxfp8_wire_bytes", int(flat_elems), ctypes.byref(so))), int(so.value)


def mxfp8_flat_elems(counts):
    """Flat elements of the list's layout (tips_fused_layout bytes / 4) and the tensors' element offsets."""
    import ctypes
    cp, _keep = _lib.i64_array(counts)
    offs = (ctypes.c_int64 * max(1, len(counts)))()
    total = _lib.check("tips_fused_layout", _lib.lib().tips_fused_layout(cp, len(counts), _lib.FLOAT32, offs))
    return total // 4, [int(o) // 4 for o in offs[:len(counts)]]


def mxfp8_quantize(tensor_list, wire=None):
    """The MXFP8 wire buffer (a uint8 device tensor) of a list of float32 device tensors
    (tips_mxfp8_quantize): one e4m3fn byte per flat element, one power-of-two scale byte per block of
    32; every byte of the buffer is written. `wire`: a 16-B aligned uint8 tensor to fill."""
    torch = _torch()
    _check_mxfp8_list(tensor_list, "mxfp8_quantize")
    counts = [t.numel() for t in tensor_list]
    elems, _ = mxfp8_flat_elems(counts)
    nbytes, _ = mxfp8_wire_bytes(elems)
    if wire is None:
        wire = torch.empty(nbytes, dtype=torch.uint8, device=tensor_list[0].device if tensor_list else "cuda")
    if tensor_list:
        pp, _k1 = _lib.ptr_array([t.data_ptr() for t in tensor_list])
        cp, _k2 = _lib.i64_array(counts)
        _lib.call("tips_mxfp8_quantize", pp, cp, len(counts), wire.data_ptr(), tensors.stream_of(tensor_list[0]))
    return wire


def mxfp8_fold(dst_wire, src_wires, flat_elems, block_begin, block_count):
    """Blocks [block_begin, block_begin + block_count) of dst_wire = quantise(((y0 + y1) + y2) + ...)
    of the sources' dequantised blocks, in source order (tips_mxfp8_fold); dst_wire may be a source."""
    pp, _k1 = _lib.ptr_array([w.data_ptr() for w in src_wires])
    _lib.call("tips_mxfp8_fold", dst_wire.data_ptr(), pp, len(src_wires), int(flat_elems), int(block_begin),
              int(block_count), tensors.stream_of(dst_wire))
    return dst_wire


def mxfp8_dequantize(wire, out_list, factor=1.0):
    """Fill the float32 device tensors of `out_list` from their list's wire buffer
    (tips_mxfp8_dequantize): decode * 2^(scale - 127), then * float32(factor) when factor != 1."""
    _check_mxfp8_list(out_list, "mxfp8_dequantize")
    if out_list:
        pp, _k1 = _lib.ptr_array([t.data_ptr() for t in out_list])
        cp, _k2 = _lib.i64_array([t.numel() for t in out_list])
        _lib.call("tips_mxfp8_dequantize", pp, cp, len(out_list), wire.data_ptr(), float(factor), tensors.stream_of(wire))
    return out_list


def allreduce_mxfp8(tensor, factor=1.0):
    """factor * SUM of `tensor` over all ranks with an MXFP8 wire, out of place (tips_allreduce_mxfp8;
    DESIGN.md §16): every rank's tensor is quantised once to e4m3fn bytes with one power-of-two scale
    per 32 elements, rank q folds chunk q of all ranks in rank order in f32 and requantises it once,
    the reduced chunks are gathered and dequantised - a quarter of the float32 bytes on the links,
    the same bits on every rank and every run; one rank returns the round trip. A dense float32
    device tensor; the same factor on every rank; stream-ordered."""
    if not is_mxfp8_tensor(tensor):
        raise ValueError("allreduce_mxfp8 takes a dense float32 device tensor")
    basics.init()
    src = tensors.contiguous(tensor)
    out = tensors.empty_like(src)
    n = tensors.numel(src)
    if n:
        _lib.call("tips_allreduce_mxfp8", tensors.data_ptr(src), tensors.data_ptr(out), n, float(factor),
                  tensors.stream_of(src))
    return out


def fused_allreduce_mxfp8(tensor_list, factor=1.0):
    """allreduce_mxfp8 of a list of float32 device tensors in one call
    (tips_fused_allreduce_mxfp8_flat): the outputs are views of one flat float32 buffer laid out and
    reused as fused_allreduce_flat's. Inputs unchanged."""
    if not tensor_list:
        return []
    _check_mxfp8_list(tensor_list, "fused_allreduce_mxfp8")
    basics.init()
    fo, pp, flat, views = _take_outputs(tensor_list, _lib.FLOAT32)
    _lib.call("tips_fused_allreduce_mxfp8_flat", pp[0], fo.cp[0], len(tensor_list), flat.data_ptr(), float(factor),
              fo.cur_stream(tensor_list[0].device).cuda_stream)
    return views


def mxfp8_ef_bytes(flat_elems, nranks):
    """Bytes of the error-feedback state of a list of `flat_elems` flat elements on `nranks` ranks
    (tips_mxfp8_ef_bytes; pure host): 4 * (round_up(E, 256) + 32 * per), the sender
    residual and the owner residual of the largest chunk (per = 0 on one rank)."""
    return int(_lib.call("tips_mxfp8_ef_bytes", int(flat_elems), int(nranks)))


def _check_mxfp8_state(t, what):
    if not (is_mxfp8_tensor(t) and t.is_contiguous()):
        raise ValueError("%s must be a contiguous float32 device tensor" % what)


def mxfp8_quantize_ef(tensor_list, residual, wire=None):
    """mxfp8_quantize with error feedback (tips_mxfp8_quantize_ef): c = x + residual is quantised and
    residual = c - dequantise(c) is left for the next step, +0 over a poisoned block. `residual`: a
    float32 device tensor of round_up(E, 256) elements at the flat layout's positions, 16-B aligned,
    zeros before the first step; updated in place."""
    torch = _torch()
    _check_mxfp8_list(tensor_list, "mxfp8_quantize_ef")
    _check_mxfp8_state(residual, "residual")
    counts = [t.numel() for t in tensor_list]
    elems, _ = mxfp8_flat_elems(counts)
    nbytes, so = mxfp8_wire_bytes(elems)
    if residual.numel() < so:
        raise ValueError("residual holds %d elements, the list's flat layout needs %d" % (residual.numel(), so))
    if wire is None:
        wire = torch.empty(nbytes, dtype=torch.uint8, device=tensor_list[0].device if tensor_list else "cuda")
    if tensor_list:
        pp, _k1 = _lib.ptr_array([t.data_ptr() for t in tensor_list])
        cp, _k2 = _lib.i64_array(counts)
        _lib.call("tips_mxfp8_quantize_ef", pp, cp, len(counts), wire.data_ptr(), residual.data_ptr(),
                  tensors.stream_of(tensor_list[0]))
    return wire


def mxfp8_fold_ef(dst_wire, src_wires, flat_elems, block_begin, block_count, residual):
    """mxfp8_fold with error feedback (tips_mxfp8_fold_ef): c = acc + residual is quantised and
    residual = c - dequantise(c) kept. `residual`: 32 * block_count float32 device elements, element 0
    belonging to block `block_begin`; updated in place."""
    _check_mxfp8_state(residual, "residual")
    if residual.numel() < 32 * int(block_count):
        raise ValueError("residual holds %d elements, %d blocks need %d" % (residual.numel(), block_count, 32 * block_count))
    pp, _k1 = _lib.ptr_array([w.data_ptr() for w in src_wires])
    _lib.call("tips_mxfp8_fold_ef", dst_wire.data_ptr(), pp, len(src_wires), int(flat_elems), int(block_begin),
              int(block_count), residual.data_ptr(), tensors.stream_of(dst_wire))
    return dst_wire


def allreduce_mxfp8_ef(tensor, state, factor=1.0):
    """allreduce_mxfp8 with error feedback (tips_allreduce_mxfp8_ef): `state` is the
    caller's float32 device tensor of mxfp8_ef_bytes(E, size()) bytes, zeros before the first step,
    updated in place - the sender residual and this rank's owner residual."""
    if not is_mxfp8_tensor(tensor):
        raise ValueError("allreduce_mxfp8_ef takes a dense float32 device tensor")
    _check_mxfp8_state(state, "state")
    basics.init()
    src = tensors.contiguous(tensor)
    out = tensors.empty_like(src)
    n = tensors.numel(src)
    if n:
        _lib.call("tips_allreduce_mxfp8_ef", tensors.data_ptr(src), tensors.data_ptr(out), n, float(factor),
                  state.data_ptr(), state.numel() * 4, tensors.stream_of(src))
    return out


def fused_allreduce_mxfp8_ef(tensor_list, state, factor=1.0):
    """fused_allreduce_mxfp8 with error feedback (tips_fused_allreduce_mxfp8_ef_flat): one state
    tensor for the list, as allreduce_mxfp8_ef's."""
    if not tensor_list:
        return []
    _check_mxfp8_list(tensor_list, "fused_allreduce_mxfp8_ef")
    _check_mxfp8_state(state, "state")
    basics.init()
    fo, pp, flat, views = _take_outputs(tensor_list, _lib.FLOAT32)
    _lib.call("tips_fused_allreduce_mxfp8_ef_flat", pp[0], fo.cp[0], len(tensor_list), flat.data_ptr(), float(factor),
              state.data_ptr(), state.numel() * 4, fo.cur_stream(tensor_list[0].device).cuda_stream)
    return views


def _flat_call(tensor_list, code, ptrs, scale=None):
    return _flat_run(_flat_outputs(tensor_list, code), tensor_list, ptrs, scale)


def fused_allreduce_host(tensor_list, out_list=None):
    """Out-of-place SUM of a list of same-dtype HOST tensors (numpy / CPU torch) through
    tips_fused_allreduce_host: packed by the library's host threads into page-locked pieces,
    each piece H2D -> allreduce -> D2H pipelined, unpacked into the outputs. Returns when done."""
    basics.init()
    if not tensor_list:
        return []
    code = tensors.dtype_code(tensor_list[0])
    srcs = []
    for t in tensor_list:
        if tensors.is_device(t):
            raise ValueError("fused_allreduce_host needs host tensors")
        if tensors.dtype_code(t) != code:
            raise TypeError("fused_allreduce_host needs one dtype per call")
        srcs.append(tensors.contiguous(t))
    outs = [tensors.empty_like(s) for s in srcs] if out_list is None else list(out_list)
    pi, _k1 = _lib.ptr_array([tensors.data_ptr(s) for s in srcs])
    po, _k2 = _lib.ptr_array([tensors.data_ptr(o) for o in outs])
    cp, _k3 = _lib.i64_array([tensors.numel(s) for s in srcs])
    _lib.call("tips_fused_allreduce_host", pi, po, cp, len(srcs), code)
    return outs


class _HostFlatOutputs(_OutputSets):
    """Output sets of fused_allreduce_host_flat for one host list signature (numpy, or CPU torch):
    one flat host buffer laid out as tips_fused_layout, page-locked once (tips_host_register) so
    the device writes the sums straight into it, and one view of it per tensor. A set is handed out
    again once every output of it has been released (as _FlatOutputs: no reference to a view, no
    other array or tensor on its memory)."""

    def __init__(self, shapes, numels, code, dtype, is_torch):
        _OutputSets.__init__(self, numels, code)
        self.total = max(256, self.total)
        self.shapes, self.dtype, self.is_torch = shapes, dtype, is_torch
        self.es = _itemsize(dtype, is_torch)

    def _released(self, s):
        return self._refs(s) == s[2]

    def _refs(self, s):
        """(references to the flat buffer, most references to one view) of set s. Measured the same
        way when a set is made (its baseline) and when it is looked at again, so a set is free
        exactly when nothing beyond the set itself refers to it: a view held, or an array / tensor
        made from one (numpy collapses every view's .base to the owner; torch counts storage users)."""
        import sys
        if self.is_torch:
            n = _torch()._C._storage_Use_Count(s[0].untyped_storage()._cdata)
        else:
            n = sys.getrefcount(s[0])
        return n, max(map(sys.getrefcount, s[1]), default=0)

    def _new_set(self, keep):
        import numpy as np
        mem = np.empty(self.total, dtype=np.uint8)
        if self.is_torch:
            flat = _torch().from_numpy(mem)  # (the storage keeps `mem` alive: see _register_until_freed)
            views = [flat[o:o + n * self.es].view(self.dtype).view(shp)
                     for o, n, shp in zip(self.offs, self.numels, self.shapes)]
        else:
            flat = mem
            views = [flat[o:o + n * self.es].view(self.dtype).reshape(shp)
                     for o, n, shp in zip(self.offs, self.numels, self.shapes)]
        if not keep:
            return flat, views
        # a kept set is page-locked while its memory lives (the device's D2H lands in it
        # directly); one past MAX_SETS is not (it is freed with its last output)
        _register_until_freed(mem, self.total)
        del mem
        st = [flat, views, None]
        del flat, views  # (the baseline counts the set's own references only)
        st[2] = self._refs(st)
        self.sets.append(st)
        return st[0], list(st[1])


def _register_until_freed(mem, nbytes):
    """Page-lock a numpy host buffer (tips_host_register) and unregister it just before its memory
    is freed: numpy views hold their base, and a torch tensor made by torch.from_numpy holds the
    array from its storage, so the array dies with the last output that uses its memory. A set
    evicted from _HOST_FLAT is therefore unregistered once its last output is released - never while
    a call writes into it (the call holds the buffer) - and no later allocation at the same address
    finds a stale registration."""
    import weakref
    ptr = mem.ctypes.data
    _lib.call("tips_host_register", ptr, nbytes)
    weakref.finalize(mem, _unregister, ptr).atexit = False  # (at exit the process's pages go anyway)


def _unregister(ptr):
    try:
        _lib.lib().tips_host_unregister(ptr)
    except Exception:  # noqa: BLE001 - at interpreter exit the library may be gone
        pass


def _itemsize(dtype, is_torch):
    if is_torch:
        return _torch().empty((), dtype=dtype).element_size()
    import numpy as np
    return np.dtype(dtype).itemsize


_HOST_FLAT = {}  # (dtype, torch?, shapes, layout settings) -> _HostFlatOutputs


def fused_allreduce_host_flat(tensor_list):
    """Out-of-place SUM of a list of same-dtype HOST tensors (numpy / CPU torch), the outputs views
    of one page-locked flat host buffer (tips_fused_allreduce_host_flat): host threads pack the
    inputs into page-locked pieces, each piece H2D -> allreduce -> D2H straight into the output
    buffer - no unpack. The buffer and its views are reused by a later call of the same list
    signature once the caller has released every output. Returns when the outputs are written."""
    basics.init()
    if not tensor_list:
        return []
    code = tensors.dtype_code(tensor_list[0])
    srcs = []
    for t in tensor_list:
        if tensors.is_device(t):
            raise ValueError("fused_allreduce_host_flat needs host tensors")
        if tensors.dtype_code(t) != code:
            raise TypeError("fused_allreduce_host_flat needs one dtype per call")
        srcs.append(tensors.contiguous(t))
    return _host_flat_run(_host_flat_outputs(srcs), [tensors.data_ptr(s) for s in srcs])


def _host_flat_outputs(srcs):
    """The _HostFlatOutputs of this host list's signature (dtype, numpy or torch, shapes); srcs are
    contiguous host tensors of one dtype."""
    is_torch = tensors.is_torch(srcs[0])
    shapes = tuple(tuple(s.shape) for s in srcs)
    key = (str(srcs[0].dtype), is_torch, shapes, _layout_settings())
    fo = _HOST_FLAT.get(key)
    if fo is None:
        fo = _cache_put(_HOST_FLAT, key, _HostFlatOutputs(shapes, [tensors.numel(s) for s in srcs],
                                                     tensors.dtype_code(srcs[0]), srcs[0].dtype, is_torch))
    return fo


def _host_flat_run(fo, ptrs):
    """tips_fused_allreduce_host_flat of the host tensors at `ptrs` into an output set of `fo`;
    returns the outputs (views of the set's flat buffer)."""
    last = fo.last  # (one read: another thread may replace it)
    if ptrs == last[0]:
        pp = last[1]
    else:
        pp = _lib.ptr_array(ptrs)
        fo.last = (ptrs, pp)
    flat, views = fo.take()
    _lib.call("tips_fused_allreduce_host_flat", pp[0], fo.cp[0], len(ptrs), fo.code, tensors.data_ptr(flat))
    return views


def fusion_stats():
    """{layouts_built, layout_hits, tables_built, table_hits} of this process's fusion caches
    (tips_fusion_stats): layouts depend on the counts only, tables on the pointers."""
    import ctypes
    v = [ctypes.c_int64() for _ in range(4)]
    _lib.call("tips_fusion_stats", *[ctypes.byref(x) for x in v])
    return dict(zip(("layouts_built", "layout_hits", "tables_built", "table_hits"), [x.value for x in v]))


class FusedList(object):
    """A list of device tensors reduced in place together, step after step (a model's gradients).

    fused_allreduce_ validates every tensor and rebuilds the pointer arrays on each call; for a
    list that keeps the same tensors (or a new tensor at the same address) that host work is
    repeated for nothing, and for 1000 gradients it costs more than the pack + unpack kernels
    themselves. This keeps the validated arrays and, per call, only re-reads the data pointers:
    when they are unchanged the cached arrays go straight to tips_fused_allreduce.

    `counts` fixes the element count of each position (a parameter's gradient always has the
    parameter's shape, which torch enforces on assignment); a list whose counts differ is refused."""

    def __init__(self, counts):
        self._counts = [int(c) for c in counts]
        self._ptrs = None
        self._arrays = None
        self._cp = _lib.i64_array(self._counts)
        self._count_bytes = self._cp[1].tobytes()  # (little-endian int64, as _fast.dev_list writes them)

    def allreduce_(self, tensor_list):
        if not tensor_list:
            return tensor_list
        import ctypes
        n = len(tensor_list)
        sc = _list_scratch(n)  # (this thread's: another thread's call can run before the compare below)
        # pointers, counts and dtype read in C++ (_fast.dev_list); the Python checks below only when
        # the list is not one dtype of dense contiguous device tensors, or its pointers changed
        r = _fast.dev_list(tensor_list, sc[2], sc[3], 1, n)
        cur = ctypes.string_at(sc[2], 8 * n) if r is not None else None
        if r is None or cur != self._ptrs:
            code = _check_fusable(tensor_list, "fused_allreduce_")
            basics.init()
            if len(tensor_list) != len(self._counts) or (r is not None and ctypes.string_at(sc[3], 8 * n) != self._count_bytes) \
                    or (r is None and [t.numel() for t in tensor_list] != self._counts):
                raise ValueError("FusedList: the tensors' element counts changed")
            ptrs = [t.data_ptr() for t in tensor_list]
            self._ptrs, self._arrays = cur, (code,) + _lib.ptr_array(ptrs)
        code, pp = self._arrays[0], self._arrays[1]
        _lib.call("tips_fused_allreduce", pp, self._cp[0], n, code, tensors.stream_of(tensor_list[0]))
        return tensor_list


def _check_fusable(tensor_list, what):
    code = tensors.dtype_code(tensor_list[0])
    for t in tensor_list:
        if not tensors.is_device(t):
            raise ValueError("%s needs device tensors" % what)
        if tensors.dtype_code(t) != code:
            raise TypeError("%s needs one dtype per call" % what)
        if not t.is_contiguous():
            raise ValueError("%s needs contiguous tensors" % what)
    return code


def bucket_sum(a, b, out=None):
    """out = a + b on the device: the per-chunk reduction kernel on its own (tips_bucket_sum)."""
    if not (tensors.is_device(a) and tensors.is_device(b)):
        raise ValueError("bucket_sum needs device tensors")
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("bucket_sum needs equal shapes and dtypes")
    a, b = a.contiguous(), b.contiguous()
    if out is None:
        out = tensors.empty_like(a)
    _lib.call("tips_bucket_sum", out.data_ptr(), a.data_ptr(), b.data_ptr(), a.numel(), tensors.dtype_code(a),
              tensors.stream_of(a))
    return out


_INFLIGHT = {}  # handle -> Handle: the buffers of every named request stay alive until it has run


class Handle(object):
    """An in-flight named request (tips_enqueue_allreduce / _broadcast / _allgather); see
    allreduce_async, broadcast_async, allgather_async. Until the request has run (synchronize /
    poll reports it, or it failed) the module holds it, with its input and output: the library
    reads and writes them when rank 0's order reaches the name, possibly after the caller dropped
    its own references (a freed host buffer would be written into; a freed device block could
    already belong to another tensor)."""

    def __init__(self, handle, output, name):
        self.handle = handle
        self.output = output
        self.name = name
        self.done = False
        self._finish = None  # allgather: builds the output once the request has run

    def _track(self):
        _INFLIGHT[self.handle] = self
        return self

    def _release(self):
        _INFLIGHT.pop(self.handle, None)

    def _complete(self):
        self._release()
        self.done = True
        if self._finish is not None:
            self.output = self._finish()
            self._finish = None


def allreduce_async(tensor, name):
    """Start a negotiated SUM of a device tensor under `name` and return a Handle.

    The reference's op path (MPIAllreduce -> EnqueueTensorCollective -> rank-0
    negotiation, ops.cc:86-115, coordinator.cc:223-513): ranks may call this in
    any order; each named tensor is reduced once every rank has enqueued it, in
    rank 0's order, with the reference's dtype/shape validation. `name` must be
    the same on every rank (the reference uses the TF node name). Device tensors are reduced
    stream-ordered; host tensors (numpy / CPU torch: the reference's op is a CPU op) on the
    negotiation thread, done when synchronize() returns."""
    basics.init()
    code = tensors.dtype_code(tensor)
    src = tensors.contiguous(tensor)
    out = tensors.empty_like(src)
    shape = _shape(src)  # validated across ranks with ConstructResponseMessage's rule (coordinator.cc:129-146)
    sp, _keep = _lib.i64_array(shape or [1])
    h = _lib.lib().tips_enqueue_allreduce_shaped(name.encode(), tensors.data_ptr(src), tensors.data_ptr(out), sp,
                                                 len(shape), code, tensors.stream_of(src))
    if h < 0:
        raise _lib.TipsError("tips_enqueue_allreduce", int(h), _lib.last_error())
    hd = Handle(int(h), out, name)
    hd._keep = src  # the input must stay alive until the reduction has run
    return hd._track()


def broadcast_async(tensor, root_rank, name):
    """Start a negotiated broadcast of a device tensor under `name` (MPIBroadcast, ops.cc:214-286 ->
    EnqueueTensorCollective(RequestType_BROADCAST)); the Handle's output is root_rank's tensor.
    Ranks may call it in any order; rank 0 checks dtype, shape and root on every rank. Device or
    host tensors, as allreduce_async."""
    basics.init()
    code = tensors.dtype_code(tensor)
    src = tensors.contiguous(tensor)
    out = tensors.empty_like(src)
    shape = _shape(src)
    sp, _keep = _lib.i64_array(shape or [1])
    h = _lib.lib().tips_enqueue_broadcast(name.encode(), tensors.data_ptr(src), tensors.data_ptr(out), sp, len(shape),
                                          code, int(root_rank), tensors.stream_of(src))
    if h < 0:
        raise _lib.TipsError("tips_enqueue_broadcast", int(h), _lib.last_error())
    hd = Handle(int(h), out, name)
    hd._keep = src
    return hd._track()


def allgather_async(tensor, name):
    """Start a negotiated allgather of a device tensor under `name` (MPIAllgather, ops.cc:156-212
    -> RequestType_ALLGATHER): every rank's tensor concatenated along dimension 0 in rank order.
    Rank 0 checks all but the first dimension (GatherFirstRankSizes, coordinator.cc:40-88) and
    sends every rank the first dimensions; the output is allocated then, on the negotiation
    thread, through a callback (as the reference's allocate_output in PerformCollectiveOp). Device
    or host tensors, as allreduce_async (a host tensor gets a host output)."""
    import ctypes
    import numpy as np
    basics.init()
    code = tensors.dtype_code(tensor)
    src = tensors.contiguous(tensor)
    shape = _shape(src)
    if not shape:
        raise ValueError("An empty tensor found")
    sp, _keep = _lib.i64_array(shape)
    rows = ctypes.c_int64(-1)
    hd = Handle(0, None, name)
    box = {}

    torch_src = tensors.is_torch(src)
    req_stream = None
    if torch_src and src.is_cuda:
        torch = _torch()
        req_stream = torch.cuda.current_stream(src.device)  # the stream the request runs on

    def alloc(_ctx, nbytes):
        if torch_src:
            import contextlib
            torch = _torch()
            # allocated on the negotiation thread, but the transfer writes it on the request's
            # stream: allocate under that stream, so the caching allocator ties the block to it
            with torch.cuda.stream(req_stream) if req_stream is not None else contextlib.nullcontext():
                buf = torch.empty(int(nbytes), dtype=torch.uint8, device=src.device)
        else:
            buf = np.empty(int(nbytes), dtype=np.uint8)
        box["buf"] = buf
        return tensors.data_ptr(buf)

    cb = _lib.ALLOC_FN(alloc)

    def finish():
        out_shape = (int(rows.value),) + tuple(shape[1:])
        if "buf" in box:
            return box.pop("buf").view(src.dtype).reshape(out_shape)
        if torch_src:
            torch = _torch()
            return torch.empty(out_shape, dtype=src.dtype, device=src.device)
        return np.empty(out_shape, dtype=src.dtype)

    h = _lib.lib().tips_enqueue_allgather(name.encode(), tensors.data_ptr(src), sp, len(shape), code,
                                          tensors.stream_of(src), ctypes.cast(cb, ctypes.c_void_p), None,
                                          ctypes.byref(rows))
    if h < 0:
        raise _lib.TipsError("tips_enqueue_allgather", int(h), _lib.last_error())
    hd.handle = int(h)
    hd._keep = (src, sp, rows, cb)  # alive until the request has run (the callback, the out-param)
    hd._finish = finish
    return hd._track()


def allreduce_async_many(tensor_list, names):
    """allreduce_async over a list in one library call (tips_enqueue_allreduce_n): what a
    gradient hook hands over at once. Same negotiation per name; returns one Handle each."""
    import ctypes
    basics.init()
    if len(tensor_list) != len(names):
        raise ValueError("one name per tensor")
    if not tensor_list:
        return []
    code = tensors.dtype_code(tensor_list[0])
    srcs, outs = [], []
    for t in tensor_list:
        if not tensors.is_device(t):
            raise ValueError("allreduce_async_many needs device tensors")
        if tensors.dtype_code(t) != code:
            raise ValueError("allreduce_async_many needs one dtype (call it once per dtype)")
        srcs.append(t.contiguous())
        outs.append(tensors.empty_like(srcs[-1]))
    n = len(srcs)
    nm = (ctypes.c_char_p * n)(*[x.encode() for x in names])
    pi, _k1 = _lib.ptr_array([x.data_ptr() for x in srcs])
    po, _k2 = _lib.ptr_array([x.data_ptr() for x in outs])
    shapes = [_shape(x) for x in srcs]
    nd = (ctypes.c_int * n)(*[len(s) for s in shapes])
    pd, _k3 = _lib.i64_array([d for s in shapes for d in s] or [0])
    hs = (ctypes.c_int64 * n)()
    _lib.call("tips_enqueue_allreduce_shaped_n", nm, pi, po, nd, pd, n, code, tensors.stream_of(srcs[0]), hs)
    out = []
    for h, o, x, name in zip(hs, outs, srcs, names):
        hd = Handle(int(h), o, name)
        hd._keep = x
        out.append(hd._track())
    return out


def synchronize_many(handles):
    """synchronize() over a list in one library call (tips_wait_n); returns the outputs."""
    import ctypes
    pend = [h for h in handles if not h.done]
    if pend:
        arr = (ctypes.c_int64 * len(pend))(*[h.handle for h in pend])
        try:
            _lib.call("tips_wait_n", arr, len(pend))
        except _lib.TipsError:
            for h in pend:  # every handle has been waited on (tips_wait_n waits for all of them)
                h._release()
            raise
        for h in pend:
            h._complete()
    return [h.output for h in handles]


def poll(handle):
    """True once the named allreduce has completed on the device."""
    if handle.done:
        return True
    try:
        rc = _lib.call("tips_poll", handle.handle)
    except _lib.TipsError:
        handle._release()
        raise
    if rc == 1:
        handle._complete()
    return handle.done


def synchronize(handle):
    """Wait for a Handle and return its output tensor (raises TipsError on a negotiation error)."""
    if not handle.done:
        try:
            _lib.call("tips_wait", handle.handle)
        except _lib.TipsError:
            handle._release()
            raise
        handle._complete()
    return handle.output


class registered_host_buffer(object):
    """Context manager: page-lock a long-lived host (numpy / CPU torch) buffer for the
    duration, so host-memory allreduces on it use asynchronous DMA (tips_host_register)."""

    def __init__(self, array):
        self.array = array

    def __enter__(self):
        basics.init()
        _lib.call("tips_host_register", tensors.data_ptr(self.array),
                  tensors.numel(self.array) * self.array.dtype.itemsize if not tensors.is_torch(self.array)
                  else self.array.numel() * self.array.element_size())
        return self.array

    def __exit__(self, *exc):
        _lib.call("tips_host_unregister", tensors.data_ptr(self.array))
        return False


def set_algorithm(algo):
    """Select 'auto', 'ring', 'direct', 'oneshot', 'peer' or 'rccl'; returns the previous selection's name."""
    names = {"auto": _lib.ALGO_AUTO, "ring": _lib.ALGO_RING, "direct": _lib.ALGO_DIRECT, "rccl": _lib.ALGO_RCCL,
             "oneshot": _lib.ALGO_ONESHOT, "peer": _lib.ALGO_PEER}
    inv = {v: k for k, v in names.items()}
    prev = _lib.lib().tips_get_algorithm()
    _lib.call("tips_set_algorithm", names[algo])
    return inv.get(prev, str(prev))


def reducescatter_rows(rows, nranks, rank):
    """(first row, rows) rank `rank` of `nranks` owns of a [rows, ...] tensor (tips_reducescatter_rows)."""
    import ctypes
    begin = ctypes.c_int64()
    own = _lib.call("tips_reducescatter_rows", int(rows), int(nranks), int(rank), ctypes.byref(begin))
    return int(begin.value), int(own)


def _check_reducescatter(tensor_list, op, pre, post, name):
    """The argument checks of reducescatter / grouped_reducescatter, before anything is initialised."""
    if name is not None:
        raise ValueError("reducescatter takes no name: named requests go through the negotiation, which carries SUM "
                         "allreduce only")
    if op == "Adasum":
        raise ValueError("op=Adasum is not defined for reducescatter")
    if op not in ("Average", "Sum", "Max", "Min"):
        raise ValueError("reducescatter: op must be Average, Sum, Max or Min (got %r)" % (op,))
    scaled = pre != 1.0 or post != 1.0
    if op in ("Max", "Min") and scaled:
        raise ValueError("op=%s takes no prescale_factor / postscale_factor: there is no scaled Max / Min" % op)
    for t in tensor_list:
        if t is None:
            continue
        if not tensors.is_torch(t):
            raise ValueError("reducescatter takes device torch tensors (got %s): host tensors are not staged" % type(t).__name__)
        if t.is_sparse:
            raise ValueError("reducescatter is not defined for sparse tensors: densify first")
        if t.dim() == 0:
            raise ValueError("reducescatter splits dimension 0: a 0-dim tensor has none")
        try:
            tensors.dtype_code(t)
        except TypeError as e:
            raise ValueError(str(e))
        if _is_integer(t) and (op == "Average" or scaled):
            raise ValueError("integer tensors (dtype %s) take no scale factor and no op=Average: reduce with op=Sum" % t.dtype)
        if not t.is_cuda:
            raise ValueError("reducescatter takes device tensors only (host pointers are not staged)")


def grouped_reducescatter_op(tensor_list, op="Average", prescale_factor=1.0, postscale_factor=1.0, name=None, mxfp8=False):
    """This rank's rows of the reduction of every tensor of the list over all ranks
    (tips_grouped_reducescatter; DESIGN.md, Reduce-scatter): one call of the library per (dtype, device)
    group, None entries passed through. See tips_amd.grouped_reducescatter. `mxfp8`: every float32 group
    goes through the MXFP8 reduce-scatter (tips_grouped_reducescatter_mxfp8) with the
    one factor prescale * postscale; op is Average or Sum."""
    tensor_list = list(tensor_list)
    pre, post = float(prescale_factor), float(postscale_factor)
    _check_reducescatter(tensor_list, op, pre, post, name)
    if mxfp8 and op not in ("Average", "Sum"):
        raise ValueError("op=%s does not combine with the MXFP8 wire: it carries SUM (and Average) only" % op)
    basics.init()
    torch = _torch()
    p, r = basics.size(), basics.rank()
    if op == "Average":
        post = post / p
    code_op = _REDUCE_OPS["Sum" if op == "Average" else op]
    outs = [None] * len(tensor_list)
    groups = {}
    for i, t in enumerate(tensor_list):
        if t is not None:
            groups.setdefault((t.dtype, t.device), []).append(i)
    for (dtype, device), members in groups.items():
        srcs = [tensor_list[i].contiguous() for i in members]
        rows = [int(s.shape[0]) for s in srcs]
        row_elems = [s.numel() // s.shape[0] if s.shape[0] else _prod(s.shape[1:]) for s in srcs]
        with torch.cuda.device(device):
            for i, s in zip(members, srcs):
                outs[i] = torch.empty((reducescatter_rows(s.shape[0], p, r)[1],) + tuple(s.shape[1:]), dtype=dtype,
                                      device=device)
            stream = tensors.stream_of(srcs[0])
            code = tensors.dtype_code(srcs[0])
            if mxfp8 and dtype == torch.float32:
                if len(members) == 1:
                    _lib.call("tips_reducescatter_mxfp8", srcs[0].data_ptr(), outs[members[0]].data_ptr(), rows[0], row_elems[0],
                              pre * post, stream)
                else:
                    pi, _k1 = _lib.ptr_array([s.data_ptr() for s in srcs])
                    po, _k2 = _lib.ptr_array([outs[i].data_ptr() for i in members])
                    pr, _k3 = _lib.i64_array(rows)
                    pe, _k4 = _lib.i64_array(row_elems)
                    _lib.call("tips_grouped_reducescatter_mxfp8", pi, po, pr, pe, len(members), pre * post, stream)
            elif len(members) == 1:
                _lib.call("tips_reducescatter", srcs[0].data_ptr(), outs[members[0]].data_ptr(), rows[0], row_elems[0],
                          code, code_op, pre, post, stream)
            else:
                pi, _k1 = _lib.ptr_array([s.data_ptr() for s in srcs])
                po, _k2 = _lib.ptr_array([outs[i].data_ptr() for i in members])
                pr, _k3 = _lib.i64_array(rows)
                pe, _k4 = _lib.i64_array(row_elems)
                _lib.call("tips_grouped_reducescatter", pi, po, pr, pe, len(members), code, code_op, pre, post, stream)
    return outs


def reducescatter_mxfp8_layout(rows, row_elems, nranks, rank):
    """(E, offsets) of region `rank` of the MXFP8 reduce-scatter (tips_reducescatter_mxfp8_layout; pure
    host): the flat elements of the list of every tensor's slice `rank` under
    tips_fused_layout, and each slice's flat element offset (0 for an empty slice)."""
    import ctypes
    pr, _k1 = _lib.i64_array([int(r) for r in rows])
    pe, _k2 = _lib.i64_array([int(e) for e in row_elems])
    offs = (ctypes.c_int64 * max(1, len(rows)))()
    elems = _lib.call("tips_reducescatter_mxfp8_layout", pr, pe, len(rows), int(nranks), int(rank), offs)
    return int(elems), [int(o) for o in offs[:len(rows)]]


def mxfp8_fold_segs(outs, own, wires, own_pos, factor=1.0):
    """The MXFP8 reduce-scatter's fold alone (tips_reducescatter_mxfp8_fold): outs[i] =
    factor * (((y_0 + y_1) + ...) + y_{nsrc-1}) with y_own_pos = own[i], not quantised, and y_j the
    dequantised elements of tensor i in the wire buffer wires[j] of the list's layout (mxfp8_quantize
    of a list with own's element counts); wires[own_pos] is ignored and may be None. float32 device
    tensors; returns outs."""
    _check_mxfp8_list(list(outs) + list(own), "mxfp8_fold_segs")
    if len(outs) != len(own) or any(o.numel() != w.numel() for o, w in zip(outs, own)):
        raise ValueError("mxfp8_fold_segs: outs and own are lists of tensors of the same sizes")
    if own:
        po, _k1 = _lib.ptr_array([t.data_ptr() for t in outs])
        pw, _k2 = _lib.ptr_array([t.data_ptr() for t in own])
        pc, _k3 = _lib.i64_array([t.numel() for t in own])
        ps, _k4 = _lib.ptr_array([0 if (j == own_pos or w is None) else w.data_ptr() for j, w in enumerate(wires)])
        _lib.call("tips_reducescatter_mxfp8_fold", po, pw, pc, len(own), ps, len(wires), int(own_pos), float(factor),
                  tensors.stream_of(own[0]))
    return outs


def _prod(dims):
    v = 1
    for d in dims:
        v *= int(d)
    return v
