"""A directed tensor list for the fusion pack / unpack / cast kernels, the census of the tile
classes it reaches, its placements in one allocation, and the runs the GPU tests make over it.

A helper module (numpy at import; torch and the library only inside the functions that run on a
device) for test_fusion_table.py (CPU: the census holds, and the interpreter reads every table
kind) and test_gpu_fusion_variants.py (GPU: every shipped instantiation of copy_segs_kernel,
copy_segs_groups_kernel and cast_segs_kernel moves the list bit for bit).

The list (`directed`, ~159 tensors, under 1 MB, with TIPS_FUSION_THRESHOLD = THRESHOLD) is built so
that, at each tile size T of 4096 / 8192 / 16384 bytes and each element size of 2 / 4 / 8 bytes, a
tile of copy_seg_tile takes each of its routes at least once:
  - T / 256 one-element tensors in one tile (the LDS segment list at its largest: a binary search
    5 to 7 steps deep), three segments in a tile, other multi-segment tiles;
  - two segments (the two-record select);
  - one segment that does not cover the tile;
  - one segment covering the tile, both sides 16-B aligned (the buffer-descriptor fast path), and
    covering with a misaligned side (tensor "B", placed one element past a 16-B boundary);
and the buckets' tile counts are not whole rounds of 8 workgroups. `census` counts these classes from
the layout alone - the records tips_fusion_mode_table returns, which hold the layout's offsets and
buckets - never from anything a kernel wrote; `assert_census` is the condition the CPU test and,
before every launch, the GPU tests assert.
"""
import ctypes

import numpy as np

THRESHOLD = 192 << 10
TILES = (4096, 8192, 16384)
SLOT, COPY, FLAT, SLOT_CAST = 0, 1, 2, 3  # fusion.cc's table kinds (tips_fusion_mode_table's mode)
F32, F64, I32, I64, F16, BF16 = 0, 1, 2, 3, 4, 5
CODE_OF_ES = {2: F16, 4: F32, 8: I64}
UINT_OF = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
CLASSES = ("full_list", "three", "multi_other", "two", "one_partial", "cover_aligned", "cover_misaligned")
CLASS_TEXT = {"full_list": "T/256 segments (LDS list at its largest)", "three": "3 segments (LDS list)",
              "multi_other": "more than 3 segments (LDS list)", "two": "2 segments (two-record select)",
              "one_partial": "one segment, not covering the tile", "cover_aligned": "one segment covering, 16-B aligned (fast path)",
              "cover_misaligned": "one segment covering, a side misaligned"}


def directed(es):
    """([count], {label: index}) for element size `es`; see the module docstring."""
    items = [(1, None)] * 130                       # one element each: a tile of T/256 segments at every T
    items += [((3 * 16384 + 256) // es + 1, "A")]   # covers whole tiles, ragged end
    items += [(300 // es + 1, None), (3, None), ((2 * 16384) // es + 3, "ragged")]  # boundaries inside tiles
    items += [((5 * 16384) // es + 1, "B")]         # placed one element past a 16-B boundary
    items += [(0, "empty"), (700 // es + 1, None), (900 // es, None), (1, None)]   # three segments in one tile
    items += [((2 * 16384) // es, "exact")]         # an exact multiple of every tile size
    items += [(7, None), ((4096 - 256) // es + 1, None), (5, None)]
    items += [((200 << 10) // es, "direct")]        # at least the threshold: reduced where it lies
    items += [((40 << 10) // es + 1, None)] * 5
    items += [(2, None)] * 9 + [((9 * 16384) // es + 2, "last")]
    return [c for c, _ in items], {name: i for i, (_, name) in enumerate(items) if name}


# ---------------------------------------------------------------------------
# the layout and its records (host only: the development library, nothing uploaded)

class Tables(object):
    """tips_fusion_mode_table's answer: `tables` (1 or 2) lists of (src, dst, begin, end) records,
    each [2 per tile | 1 per segment]; the tile size; the buckets (offset, bytes, first tile, tiles)."""

    def __init__(self, tables, ntiles, tile, buckets):
        self.tables, self.ntiles, self.tile, self.buckets = tables, ntiles, tile, buckets

    def segments(self, table=0):
        return self.tables[table][2 * self.ntiles:]


def mode_tables(counts, code, mode, ins, outs, base=0):
    """The records fusion.cc builds for `mode` under the current environment (threshold, tile, order)."""
    from tips_amd import _lib
    L = _lib.dev()
    n = len(counts)
    c, pi, po = (ctypes.c_int64 * n)(*counts), (ctypes.c_int64 * n)(*ins), (ctypes.c_int64 * n)(*outs)
    nt, tb, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    nrec = L.tips_fusion_mode_table(c, n, code, mode, pi, po, base, None, 0, ctypes.byref(nt), ctypes.byref(tb), None, 0,
                                    ctypes.byref(nb))
    assert nrec >= 0, L.tips_last_error()
    rec = (ctypes.c_int64 * (4 * nrec))()
    bk = (ctypes.c_int64 * (4 * max(1, nb.value)))()
    assert L.tips_fusion_mode_table(c, n, code, mode, pi, po, base, rec, nrec, ctypes.byref(nt), ctypes.byref(tb), bk,
                                    nb.value, ctypes.byref(nb)) == nrec, L.tips_last_error()
    flat = np.frombuffer(rec, dtype=np.int64).reshape(-1, 4).tolist()
    r = [tuple(x) for x in flat]
    ntab = 2 if mode in (SLOT, SLOT_CAST) else 1
    per = nrec // ntab
    assert per * ntab == nrec
    buckets = [tuple(bk[4 * b:4 * b + 4]) for b in range(nb.value)]
    return Tables([r[t * per:(t + 1) * per] for t in range(ntab)], nt.value, tb.value, buckets)


def segment_tensors(counts, es, threshold):
    """Tensor index of segment k (fusion.cc: the bucketed tensors in list order, then the ones of at
    least the threshold, which are reduced where they lie; empty tensors have no segment)."""
    return ([i for i, c in enumerate(counts) if 0 < c * es < threshold] +
            [i for i, c in enumerate(counts) if c * es >= threshold])


class Census(object):
    """Per tile of every bucket: the segments it meets and its class. Computed from the segment
    records' [begin, end) ranges, their addresses' alignment and the buckets alone."""

    def __init__(self, tabs, counts, es, threshold):
        T = self.tile = tabs.tile
        segs = tabs.segments(0)
        self.seg_tensor = segment_tensors(counts, es, threshold)
        assert len(segs) == len(self.seg_tensor)
        self.begin = {i: s[2] for i, s in zip(self.seg_tensor, segs)}  # tensor -> its offset in the flat space
        self.cls = {}        # tile -> class
        self.nsegs = {}      # tile -> segments met
        self.per_bucket = [b[3] for b in tabs.buckets]
        self.count = dict.fromkeys(CLASSES, 0)
        k = 0
        for off, nbytes, tile0, ntiles in tabs.buckets:
            assert off == tile0 * T
            for j in range(tile0, tile0 + ntiles):
                start, stop = j * T, (j + 1) * T
                while k < len(segs) and segs[k][3] <= start:
                    k += 1
                e = k
                while e < len(segs) and segs[e][2] < stop:
                    e += 1
                n = e - k
                assert n >= 1, "tile %d meets no segment" % j
                if n == 1:
                    src, dst, b, en = segs[k]
                    c = ("one_partial" if not (b <= start and en >= stop) else
                         "cover_aligned" if ((src | dst) & 15) == 0 else "cover_misaligned")
                else:
                    c = "two" if n == 2 else "three" if n == 3 else "full_list" if n >= T // 256 else "multi_other"
                self.cls[j], self.nsegs[j] = c, n
                self.count[c] += 1
        self.max_segments = max(self.nsegs.values()) if self.nsegs else 0

    def where(self, tensor, byte):
        """The tile and tile class of byte `byte` (in the layout's element type) of tensor `tensor`."""
        if tensor not in self.begin:
            return "an empty tensor"
        j = (self.begin[tensor] + byte) // self.tile
        if j not in self.cls:
            return "tile %d, outside the buckets (a tensor of at least the threshold, reduced where it lies)" % j
        return "tile %d of %d bytes: %s" % (j, self.tile, CLASS_TEXT[self.cls[j]])


def census(counts, code, mode, ins, outs, threshold=THRESHOLD):
    es = 2 if code in (F16, BF16) else 8 if code in (F64, I64) else 4
    return Census(mode_tables(counts, code, mode, ins, outs), counts, es, threshold)


def assert_census(c, aligned=True):
    """Every tile class occurs, and the segment list reaches exactly T / 256 entries. (A placement
    that aligns nothing - `aligned` False - need not reach the aligned fast path.)"""
    for name in CLASSES:
        if name == "cover_aligned" and not aligned:
            continue
        assert c.count[name] >= 1, "no tile of class %r at tile %d: %r" % (name, c.tile, c.count)
    assert c.max_segments == c.tile // 256, (c.max_segments, c.tile)
    assert len(c.per_bucket) >= 3, c.per_bucket                # pack(b + 2) reuses a slot; merged launches have groups
    assert any(n % 8 for n in c.per_bucket), c.per_bucket      # workgroups past a bucket's last tile


# ---------------------------------------------------------------------------
# placements: the list's tensors as views of one base allocation

class Placement(object):
    """Element offsets of each view in a base of `total` elements of `itemsize` bytes.
    "aligned": every view starts on 16 B, except B one element past; "offset": views packed from
    element 1 with a one-element gap, so nearly every side is only element-aligned. In both, each
    view is followed by a gap of at least one element."""

    def __init__(self, counts, itemsize, kind, b_index):
        assert kind in ("aligned", "offset")
        per16 = 16 // itemsize
        self.kind, self.counts, self.itemsize = kind, counts, itemsize
        self.starts = []
        off = 0 if kind == "aligned" else 1
        for i, c in enumerate(counts):
            if kind == "aligned":
                off = -(-off // per16) * per16 + (1 if i == b_index else 0)
            self.starts.append(off)
            off += c + 1
        self.total = off + per16
        self.view = np.zeros(self.total, dtype=bool)  # True inside a view, False in the gaps
        self.owner = np.full(self.total, -1, dtype=np.int64)
        for i, (s, c) in enumerate(zip(self.starts, counts)):
            assert not self.view[s:s + c].any() and (c == 0 or not self.view[s + c])
            self.view[s:s + c] = True
            self.owner[s:s + c] = i

    def device_views(self, base):
        return [base[s:s + c] for s, c in zip(self.starts, self.counts)]


def random_bytes(rng, nelem, itemsize):
    """Every bit pattern (NaN payloads, infinities, subnormals among them), as unsigned integers."""
    return rng.integers(0, 256, size=nelem * itemsize, dtype=np.uint8).view(UINT_OF[itemsize])


def to_device(host, torch_dtype):
    import torch
    signed = {2: np.int16, 4: np.int32, 8: np.int64}[host.itemsize]
    return torch.from_numpy(host.view(signed).copy()).cuda().view(torch_dtype)


def from_device(t):
    import torch
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()]
    return t.contiguous().view(it).cpu().numpy().view(UINT_OF[t.element_size()])


def explain(what, got, want, pl, cen, wire_bytes_per_elem=None):
    """'' when the two images of a base are equal, else what differs first: the tensor (or the gap
    behind one), the byte offset within it and the tile class of that offset."""
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return ""
    k = int(bad[0])
    i = int(pl.owner[k])
    if i < 0:
        prev = int(np.searchsorted(np.asarray(pl.starts), k, side="right")) - 1
        return "%s: %d elements differ, first in the gap behind tensor %d (element %d of the base): got %#x, expected %#x" % (
            what, bad.size, prev, k, int(got[k]), int(want[k]))
    e = k - pl.starts[i]
    per = wire_bytes_per_elem or pl.itemsize
    return "%s: %d elements differ, first in tensor %d (%d elements, %s placement) at byte +%d (element %d): got %#x, expected %#x; %s" % (
        what, bad.size, i, pl.counts[i], pl.kind, e * pl.itemsize, e, int(got[k]), int(want[k]), cen.where(i, e * per))


# ---------------------------------------------------------------------------
# the GPU runs (one rank). `setenv(name, value)` changes this process's environment: the fusion
# knobs used here are read at every call.

_KEEP = []  # every input base stays allocated, so no later case meets an earlier one's pointers


def _pointers(views):
    return [v.data_ptr() for v in views]


def _built(tips, s0, what):
    """A new pointer table was built (and so filled under the current order): a cached one would be
    keyed on the pointers and the mode only."""
    s1 = tips.fusion_stats()
    assert s1["tables_built"] > s0["tables_built"], "%s found a cached table: the order under test was not applied" % what
    return s1


def run_copy_routes(tips, setenv, es, kind, seed, routes=("inplace", "oop", "copy", "flat0", "flat1")):
    """The directed list of element size `es` in placement `kind` through the copy routes, bit for
    bit against the input bytes; gaps and inputs unchanged. The caller has set the threshold, the
    tile, the store policy and the order. Returns the census."""
    import torch
    from tips_amd import _lib
    tdt = {2: torch.float16, 4: torch.float32, 8: torch.int64}[es]
    code = CODE_OF_ES[es]
    counts, names = directed(es)
    pl = Placement(counts, es, kind, names["B"])
    rng = np.random.default_rng([seed, es, kind == "offset"])
    host = random_bytes(rng, pl.total, es)
    base = to_device(host, tdt)
    _KEEP.append(base)
    views = pl.device_views(base)
    ptrs = _pointers(views)
    setenv("TIPS_FUSION_MEASURE_PACK", "1")
    setenv("TIPS_PACK_MERGE", "0")
    cen = census(counts, code, SLOT, ptrs, ptrs)
    assert_census(cen, aligned=kind == "aligned")
    assert base.data_ptr() % 256 == 0 and (kind == "offset" or views[names["B"]].data_ptr() % 16 == pl.itemsize)
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def fresh_out():
        out_host = random_bytes(rng, pl.total, es)
        out = to_device(out_host, tdt)
        want = np.where(pl.view, host, out_host)
        return out, want

    if "inplace" in routes:  # kSlot pack and unpack tables, per-bucket launches
        s0 = tips.fusion_stats()
        tips.fused_allreduce_(views)
        torch.cuda.synchronize()
        _built(tips, s0, "in place")
        msg = explain("in place (slot tables)", from_device(base), host, pl, cen)
        assert not msg, msg
    for route, measure in (("oop", "1"), ("copy", "0")):  # kSlot with other outputs; the one-launch kCopy copy
        if route not in routes:
            continue
        setenv("TIPS_FUSION_MEASURE_PACK", measure)
        out, want = fresh_out()
        s0 = tips.fusion_stats()
        tips.fused_allreduce(views, out_list=pl.device_views(out))
        torch.cuda.synchronize()
        _built(tips, s0, route)
        what = "out of place, measure-pack %s" % measure
        msg = explain(what + ": outputs", from_device(out), want, pl, cen)
        assert not msg, msg
        msg = explain(what + ": inputs", from_device(base), host, pl, cen)
        assert not msg, msg
        del out
    setenv("TIPS_FUSION_MEASURE_PACK", "1")
    flat_routes = [r for r in ("flat0", "flat1") if r in routes]
    held = []
    if flat_routes:
        cp, _k1 = _lib.i64_array(counts)
        offs = (ctypes.c_int64 * len(counts))()
        total = _lib.check("tips_fused_layout", _lib.lib().tips_fused_layout(cp, len(counts), code, offs))
        assert total % es == 0 and all(o % es == 0 for o in offs)
        pp, _k2 = _lib.ptr_array(ptrs)
    for route in flat_routes:  # kFlat: per-bucket launches, or copy_segs_groups_kernel (merged, no signals at one rank)
        setenv("TIPS_PACK_MERGE", route[-1])
        # through the C-ABI into a flat buffer of this test's, so the padding between tensors is seen
        flat_host = random_bytes(rng, total // es + 16 // es, es)
        want = flat_host.copy()
        for i, c in enumerate(counts):
            want[offs[i] // es:offs[i] // es + c] = host[pl.starts[i]:pl.starts[i] + c]
        flat = to_device(flat_host, tdt)
        s0 = tips.fusion_stats()
        _lib.call("tips_fused_allreduce_flat", pp, cp, len(counts), code, flat.data_ptr(), stream())
        torch.cuda.synchronize()
        _built(tips, s0, route)
        got = from_device(flat)
        held.append(flat)  # (the merged run's flat buffer must not be this one again: it would find this table)
        bad = np.nonzero(got != want)[0]
        if bad.size:
            k = int(bad[0]) * es
            inside = [i for i, c in enumerate(counts) if offs[i] <= k < offs[i] + c * es]
            where = ("tensor %d at byte +%d; %s" % (inside[0], k - offs[inside[0]], cen.where(inside[0], k - offs[inside[0]]))
                     if inside else "padding")
            raise AssertionError("flat, merge %s: %d elements differ, first at flat byte %d (%s): got %#x, expected %#x" % (
                route[-1], bad.size, k, where, int(got[bad[0]]), int(want[bad[0]])))
        # and through the Python surface (the outputs are views of a pooled flat buffer)
        outs = tips.fused_allreduce_flat(views)
        torch.cuda.synchronize()
        for i, (o, c) in enumerate(zip(outs, counts)):
            assert np.array_equal(from_device(o), host[pl.starts[i]:pl.starts[i] + c]), "flat, merge %s: output %d" % (route[-1], i)
        del outs
        msg = explain("flat, merge %s: inputs" % route[-1], from_device(base), host, pl, cen)
        assert not msg, msg
    setenv("TIPS_PACK_MERGE", "0")
    return cen


def cast_values(wire_code, pl, counts, names, seed):
    """float32 values for the cast runs, from edge_values' cast set (ties, wire subnormals, overflow
    to inf, NaNs, +-0): drawn at random everywhere (gaps too), then the structured part of the set
    laid, in order, over the one-element tensors, the last n % 4 elements of every ragged tensor and
    the whole of B (which moves element by element)."""
    import edge_values as ev
    pool = ev.cast_set(wire_code)
    edge = pool[:pool.size - 4096]  # (the set ends with 4096 random patterns)
    rng = np.random.default_rng([seed, wire_code, pl.kind == "offset"])
    x = pool[rng.integers(0, pool.size, size=pl.total)].copy()
    at = 0

    def lay(start, n):
        nonlocal at
        idx = (at + np.arange(n)) % edge.size
        x[start:start + n] = edge[idx]
        at += n

    for i, c in enumerate(counts):
        if c == 1:
            lay(pl.starts[i], 1)
        elif c % 4:
            lay(pl.starts[i] + c - c % 4, c % 4)
    lay(pl.starts[names["B"]], counts[names["B"]])
    assert at >= edge.size  # the whole structured part is somewhere in the list
    return x


def run_cast_routes(tips, setenv, wire, kind, seed):
    """The directed list (laid out in the 16-bit wire type, the tensors float32) through
    tips_fused_allreduce_cast: out of place through the Python surface and through the C-ABI into
    views of a second base, then in place (in == out); bit for bit against the oracle's casts.
    The caller has set the threshold and TIPS_CAST_TILE_BYTES."""
    import torch
    import oracle_bind
    from tips_amd import _lib
    wcode = F16 if wire == "float16" else BF16
    ocode = oracle_bind.F16 if wire == "float16" else oracle_bind.BF16
    counts, names = directed(2)
    pl = Placement(counts, 4, kind, names["B"])
    x = cast_values(wcode, pl, counts, names, seed)
    host = x.view(np.uint32)
    cast_all = oracle_bind.cast_from16(oracle_bind.cast_to16(x, ocode), ocode).view(np.uint32)
    base = to_device(host, torch.float32)
    _KEEP.append(base)
    views = pl.device_views(base)
    ptrs = _pointers(views)
    cen = census(counts, wcode, SLOT_CAST, ptrs, ptrs)
    assert_census(cen, aligned=kind == "aligned")
    assert base.data_ptr() % 256 == 0 and (kind == "offset" or views[names["B"]].data_ptr() % 16 == pl.itemsize)
    stream = torch.cuda.current_stream().cuda_stream
    # out of place, Python surface
    s0 = tips.fusion_stats()
    outs = tips.fused_allreduce_cast(views, wire)
    torch.cuda.synchronize()
    _built(tips, s0, "cast, out of place")
    for i, (o, c) in enumerate(zip(outs, counts)):
        got, want = from_device(o), cast_all[pl.starts[i]:pl.starts[i] + c]
        if not np.array_equal(got, want):
            e = int(np.nonzero(got != want)[0][0])
            raise AssertionError("cast %s out of place: tensor %d (%d elements, %s placement) at element %d (f32 byte +%d): input %#x, "
                                 "got %#x, expected %#x; %s" % (wire, i, c, kind, e, 4 * e, int(host[pl.starts[i] + e]), int(got[e]),
                                                               int(want[e]), cen.where(i, 2 * e)))
    del outs
    msg = explain("cast %s out of place: inputs" % wire, from_device(base), host, pl, cen, 2)
    assert not msg, msg
    # out of place through the C-ABI into views of a second base (output sides placed as the inputs)
    out_host = random_bytes(np.random.default_rng([seed, 5]), pl.total, 4)
    out = to_device(out_host, torch.float32)
    pi, _k1 = _lib.ptr_array(ptrs)
    po, _k2 = _lib.ptr_array(_pointers(pl.device_views(out)))
    cp, _k3 = _lib.i64_array(counts)
    s0 = tips.fusion_stats()
    _lib.call("tips_fused_allreduce_cast", pi, po, cp, len(counts), _lib.FLOAT32, wcode, stream)
    torch.cuda.synchronize()
    _built(tips, s0, "cast, out of place (C-ABI)")
    msg = explain("cast %s out of place into views: outputs" % wire, from_device(out), np.where(pl.view, cast_all, out_host), pl, cen, 2)
    assert not msg, msg
    msg = explain("cast %s out of place into views: inputs" % wire, from_device(base), host, pl, cen, 2)
    assert not msg, msg
    del out
    # in place through the C-ABI
    s0 = tips.fusion_stats()
    _lib.call("tips_fused_allreduce_cast", pi, pi, cp, len(counts), _lib.FLOAT32, wcode, stream)
    torch.cuda.synchronize()
    _built(tips, s0, "cast, in place")
    msg = explain("cast %s in place" % wire, from_device(base), np.where(pl.view, cast_all, host), pl, cen, 2)
    assert not msg, msg
    return cen
