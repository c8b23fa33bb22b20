"""CPU: the fusion pack / unpack tables against copy_segs_kernel's rules, without a GPU.

tips_fusion_tile_table returns the records fusion.cc builds for one pointer set (the same code
that fills the device table). `run_table` below applies copy_segs_kernel's per-workgroup and
per-lane rules (tips_amd/csrc/kernels.hip) to them - the tile's byte offset from its second record,
the one-tensor fast path, the two-record select, the LDS segment list with its binary search, and
the per-vector length at a tensor's ragged end - and collects the byte ranges each launch copies.
For random lists (ragged sizes, empty tensors, tensors past the threshold, 4-B aligned tensors,
several buckets) every input byte must land at its output address exactly once and nothing else
may be written, for each tile size and for both launch orders (TIPS_COPY_ORDER: tile order, and a
group's boundary tiles first).

tips_fusion_mode_table returns the records of the other table kinds too, which the same rules (and,
for the fused cast, `run_cast_table`: a restatement of cast_segs_kernel's) are applied to below:
the bucket slots' pack and unpack tables, the flat output's pack, and the cast's pack and unpack
tables with the float32 side at base + 2 v. They run over fusion_cases' directed list (whose census
of tile classes is asserted here) and over the random lists; `test_perturbed_*` show that one wrong
record field makes these checks fail."""
import ctypes
import os
import random

import pytest

import fusion_cases as fc

VEC = 16
LANES = 256


def table(counts, ins, outs, dtype):
    from tips_amd import _lib
    L = _lib.dev()
    n = len(counts)
    c = (ctypes.c_int64 * n)(*counts)
    pi = (ctypes.c_int64 * n)(*ins)
    po = (ctypes.c_int64 * n)(*outs)
    nt, tb = ctypes.c_int64(), ctypes.c_int64()
    nrec = L.tips_fusion_tile_table(c, n, dtype, pi, po, None, 0, ctypes.byref(nt), ctypes.byref(tb))
    assert nrec >= 0, _lib.last_error()
    rec = (ctypes.c_int64 * (4 * nrec))()
    assert L.tips_fusion_tile_table(c, n, dtype, pi, po, rec, nrec, ctypes.byref(nt), ctypes.byref(tb)) == nrec
    r = [tuple(rec[4 * k:4 * k + 4]) for k in range(nrec)]
    return r, nt.value, tb.value


def run_table(rec, ntiles, T, slots=None):
    """[(dst, src, length)] copied by one launch over all tiles (or over the record slots `slots`:
    one bucket's launch), per copy_segs_kernel."""
    U = T // (LANES * VEC)
    max_seg = T // 256 + 1
    out = []
    for q in (range(ntiles) if slots is None else slots):
        a, b = rec[2 * q], rec[2 * q + 1]
        multi, two = a[3] < 0, b[3] > 0
        tb = (b[2] & ~(T - 1)) if two else b[2]
        if not multi and not two and a[2] <= tb and a[3] >= tb + T and ((a[0] | a[1]) & 15) == 0:
            out.append((a[1] + tb, a[0] + tb, T))
            continue
        segs = None
        if multi:
            cnt = min(a[1], max_seg)
            if cnt <= 0:
                continue
            segs = rec[2 * ntiles + a[0]:2 * ntiles + a[0] + cnt]
        for u in range(U):
            for tid in range(LANES):
                v = tb + u * LANES * VEC + tid * VEC
                if multi:
                    lo, hi = 0, len(segs) - 1
                    while lo < hi:
                        mid = (lo + hi + 1) >> 1
                        if segs[mid][2] <= v:
                            lo = mid
                        else:
                            hi = mid - 1
                    g = segs[lo]
                else:
                    g = b if (two and v >= b[2]) else a
                left = g[3] - v
                ln = min(left, VEC) if (v >= g[2] and left > 0) else 0
                if ln:
                    out.append((g[1] + v, g[0] + v, ln))
    return out


def check(counts, ins, outs, es, copies):
    """every byte of tensor i copied from ins[i] + k to outs[i] + k exactly once; nothing else"""
    want = sorted((o, i, c * es) for i, (o, c) in enumerate(zip(outs, counts)) if c > 0)
    got = sorted(copies)
    # merge the copied ranges per tensor, in destination order
    k = 0
    for dst0, i, nbytes in want:
        pos = dst0
        while pos < dst0 + nbytes:
            assert k < len(got), "tensor %d: bytes from %d not copied" % (i, pos - dst0)
            d, s, ln = got[k]
            assert d == pos, "tensor %d: expected a copy to +%d, next copy is to %d" % (i, pos - dst0, d - dst0)
            assert s - d == ins[i] - outs[i], "tensor %d: wrong source at +%d" % (i, pos - dst0)
            pos += ln
            k += 1
        assert pos == dst0 + nbytes, "tensor %d: copied past its end" % i
    assert k == len(got), "%d copies outside every tensor" % (len(got) - k)


def random_list(rng, n, es, threshold):
    counts = []
    for _ in range(n):
        r = rng.random()
        if r < 0.08:
            counts.append(0)
        elif r < 0.12:
            counts.append((threshold + rng.randrange(1, 4096)) // es)  # reduced where it lies
        elif r < 0.5:
            counts.append(rng.randrange(1, 300))
        else:
            counts.append(rng.randrange(1, 12000))
    # distinct, non-overlapping addresses: mostly 256-B aligned, some only 4-B aligned
    ins, outs = [], []
    nxt = 1 << 32
    for c in counts:
        for lst in (ins, outs):
            al = 4 if rng.random() < 0.15 else 256
            nxt = (nxt + 4095) // 4096 * 4096 + rng.randrange(0, 4096 // al) * al
            lst.append(nxt)
            nxt += c * es + 8192
    return counts, ins, outs


@pytest.mark.parametrize("tile", [4096, 8192, 16384])
@pytest.mark.parametrize("order", ["0", "1"])
def test_tables_copy_every_byte_once(monkeypatch, tile, order):
    from tips_amd import _lib
    threshold = 96 << 10  # several buckets from a short list
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(threshold))
    monkeypatch.setenv("TIPS_COPY_TILE_BYTES", str(tile))
    monkeypatch.setenv("TIPS_COPY_ORDER", order)
    rng = random.Random(tile * 7 + int(order))
    for dtype, es in ((_lib.FLOAT32, 4), (_lib.FLOAT16, 2), (_lib.FLOAT64, 8)):
        counts, ins, outs = random_list(rng, 40, es, threshold)
        rec, ntiles, T = table(counts, ins, outs, dtype)
        assert T == tile
        check(counts, ins, outs, es, run_table(rec, ntiles, T))


def test_boundary_tiles_come_first_in_each_group(monkeypatch):
    """TIPS_COPY_ORDER=1 (the default): within each bucket the tiles that meet a tensor boundary
    occupy the first record slots, the tiles inside one tensor the rest; the set of tiles per
    bucket is unchanged (the tile offsets in the records are a permutation of the bucket's)."""
    from tips_amd import _lib
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(96 << 10))
    monkeypatch.delenv("TIPS_COPY_ORDER", raising=False)
    rng = random.Random(5)
    counts, ins, outs = random_list(rng, 60, 4, 96 << 10)
    ins = [x // 256 * 256 for x in ins]
    outs = [x // 256 * 256 for x in outs]
    rec, ntiles, T = table(counts, ins, outs, _lib.FLOAT32)
    offs = []
    slow = []
    for q in range(ntiles):
        a, b = rec[2 * q], rec[2 * q + 1]
        two = b[3] > 0
        tb = (b[2] & ~(T - 1)) if two else b[2]
        offs.append(tb)
        slow.append(a[3] < 0 or two or not (a[2] <= tb and a[3] >= tb + T))
    assert sorted(offs) == [q * T for q in range(ntiles)]
    monkeypatch.setenv("TIPS_COPY_ORDER", "0")
    rec0, _, _ = table(counts, ins, outs, _lib.FLOAT32)
    base = [(rec0[2 * q + 1][2] & ~(T - 1)) if rec0[2 * q + 1][3] > 0 else rec0[2 * q + 1][2] for q in range(ntiles)]
    assert base == [q * T for q in range(ntiles)]
    # boundary-first within each run of slots holding one bucket's tiles: once a fast tile is seen,
    # no slow tile of the same bucket follows (buckets are the contiguous tile ranges of tips_fused_layout)
    assert any(slow) and not all(slow)
    assert slow[0]


def _striped_tables_child():
    """(run in a child process: TIPS_PACK_STRIPE_KIB is read once per process)"""
    from tips_amd import _lib
    threshold = 1 << 20
    os.environ["TIPS_FUSION_THRESHOLD"] = str(threshold)
    rng = random.Random(11)
    for dtype, es in ((_lib.FLOAT32, 4), (_lib.FLOAT16, 2)):
        counts, ins, outs = random_list(rng, 160, es, threshold)
        rec, ntiles, T = table(counts, ins, outs, dtype)
        check(counts, ins, outs, es, run_table(rec, ntiles, T))
    # the slot and flat tables of the directed list under the same stripes, at every tile size
    os.environ["TIPS_FUSION_THRESHOLD"] = str(fc.THRESHOLD)
    for tile in fc.TILES:
        os.environ["TIPS_COPY_TILE_BYTES"] = str(tile)
        for name, counts, ins, outs in lists_for(4, 4, tile)[:2]:
            offs, total = layout_offsets(counts, _lib.FLOAT32)
            check_slot_tables(fc.mode_tables(counts, _lib.FLOAT32, fc.SLOT, ins, outs, BASE), counts, ins, outs, 4, offs,
                              fc.THRESHOLD, "striped slot tables: " + name)
            check_flat_table(fc.mode_tables(counts, _lib.FLOAT32, fc.FLAT, ins, outs, BASE), counts, ins, 4, offs, total,
                             "striped flat table: " + name)
    print("striped tables ok")


@pytest.mark.parametrize("stripe_kib", ["16", "64"])
def test_striped_pack_tables_copy_every_byte_once(stripe_kib):
    """TIPS_PACK_STRIPE_KIB (opt-in): the pack launch deals stripes of slots round-robin over the
    XCDs and fusion.cc's tile_order places each XCD's boundary tiles by that map. The records stay
    a permutation of the layout's tiles: every byte copied exactly once (stripes small enough that
    1 MiB buckets hold several rounds of 8)."""
    import subprocess
    import sys
    env = dict(os.environ, TIPS_PACK_STRIPE_KIB=stripe_kib)
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_fusion_table as t; t._striped_tables_child()" % (
        os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "striped tables ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------
# the directed list's census, and the table kinds tips_fusion_tile_table does not return

BASE = 7 << 36  # the slot base / the flat output, clear of every tensor


@pytest.mark.parametrize("es", [2, 4, 8])
@pytest.mark.parametrize("tile", fc.TILES)
def test_directed_list_reaches_every_tile_class(monkeypatch, tile, es):
    """fusion_cases.directed: at every tile and element size each of copy_seg_tile's routes is taken by
    some tile and the LDS segment list reaches exactly T / 256 entries (fusion_cases.assert_census, the
    condition the GPU tests assert before they launch) - for the copy tables and, with float32
    tensors laid out in a 16-bit wire type, for the cast's."""
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(fc.THRESHOLD))
    monkeypatch.setenv("TIPS_COPY_TILE_BYTES", str(tile))
    monkeypatch.setenv("TIPS_CAST_TILE_BYTES", str(tile))
    counts, names = fc.directed(es)
    assert len(counts) < 170 and sum(counts) * es < (1 << 20)
    modes = [(fc.SLOT, fc.CODE_OF_ES[es], es), (fc.COPY, fc.CODE_OF_ES[es], es), (fc.FLAT, fc.CODE_OF_ES[es], es)]
    if es == 2:
        modes += [(fc.SLOT_CAST, fc.F16, 4), (fc.SLOT_CAST, fc.BF16, 4)]
    seen = []
    for mode, code, item in modes:
        for kind in ("aligned", "offset"):
            pl = fc.Placement(counts, item, kind, names["B"])
            ptrs = [(1 << 32) + s * item for s in pl.starts]
            assert all(p % 16 == 0 for i, p in enumerate(ptrs) if i != names["B"]) or kind == "offset"
            assert ptrs[names["B"]] % 16 == item or kind == "offset"
            c = fc.census(counts, code, mode, ptrs, ptrs)
            assert c.tile == tile
            fc.assert_census(c, aligned=kind == "aligned")
            seen.append((c.per_bucket, [c.count[k] for k in fc.CLASSES[:5]]))
    assert all(s == seen[0] for s in seen)  # the layout is the counts' alone: every mode and placement meets the same tiles
    # 16 KiB stripes deal C = 16384 / tile tiles at a time: some bucket holds more than 8 stripes' worth
    assert max(seen[0][0]) > 8 * (16384 // tile)


def addresses(rng, counts, itemsize):
    """random_list's addresses for elements of `itemsize` bytes."""
    ins, outs = [], []
    nxt = 1 << 32
    for c in counts:
        for lst in (ins, outs):
            al = 4 if rng.random() < 0.15 else 256
            nxt = (nxt + 4095) // 4096 * 4096 + rng.randrange(0, 4096 // al) * al
            lst.append(nxt)
            nxt += c * itemsize + 8192
    return ins, outs


def lists_for(es, item, seed):
    """[(name, counts, ins, outs)]: the directed list in both placements and a random list, the
    tensors' elements `item` bytes wide (4 with es = 2 for the cast: float32 tensors, 16-bit layout)."""
    out = []
    counts, names = fc.directed(es)
    for kind in ("aligned", "offset"):
        pl = fc.Placement(counts, item, kind, names["B"])
        out.append(("directed, " + kind, counts, [(1 << 32) + s * item for s in pl.starts],
                    [(1 << 33) + 4096 + s * item for s in pl.starts]))
    rng = random.Random(seed)
    counts, ins, outs = random_list(rng, 60, es, fc.THRESHOLD)
    if item != es:
        ins, outs = addresses(rng, counts, item)
    out.append(("random", counts, ins, outs))
    return out


def layout_offsets(counts, dtype):
    from tips_amd import _lib
    L = _lib.dev()
    n = len(counts)
    c, offs = (ctypes.c_int64 * n)(*counts), (ctypes.c_int64 * n)()
    total = L.tips_fused_layout(c, n, dtype, offs)
    assert total >= 0, L.tips_last_error()
    return list(offs), total


def check_moves(want, moves, ds=1, ss=1, what=""):
    """want: [(dst, src, n)] per tensor; moves: [(dst, src, n)] made: every element of every tensor
    moved exactly once from src + k * ss to dst + k * ds, and nothing else moved."""
    want = sorted(w for w in want if w[2] > 0)
    got = sorted(moves)
    k = 0
    for dst0, src0, n in want:
        pos = 0
        while pos < n:
            assert k < len(got), "%s: tensor at %#x: elements from %d not moved" % (what, dst0, pos)
            d, s, ln = got[k]
            assert d == dst0 + pos * ds, "%s: tensor at %#x: expected a move to element %d, next is to %#x" % (what, dst0, pos, d)
            assert s == src0 + pos * ss, "%s: tensor at %#x: wrong source %#x at element %d" % (what, dst0, s, pos)
            pos += ln
            k += 1
        assert pos == n, "%s: tensor at %#x: moved past its end" % (what, dst0)
    assert k == len(got), "%s: %d moves outside every tensor" % (what, len(got) - k)


def slot_of(tabs, off, threshold, base):
    """(bucket, address in its slot) of flat offset `off`: bucket b lives in slot b % 2."""
    for b, (o, nbytes, _t0, _nt) in enumerate(tabs.buckets):
        if o <= off < o + nbytes:
            return b, base + (b % 2) * threshold + (off - o)
    raise AssertionError("offset %d lies in no bucket" % off)


def bucket_members(tabs, counts, offs, es, threshold):
    """per bucket: [(tensor, address in the slot)], from tips_fused_layout's offsets"""
    members = [[] for _ in tabs.buckets]
    for i, c in enumerate(counts):
        if 0 < c * es < threshold:
            b, addr = slot_of(tabs, offs[i], threshold, BASE)
            members[b].append((i, addr))
    assert all(members)
    return members


def check_slot_tables(tabs, counts, ins, outs, es, offs, threshold, what):
    """kSlot: per bucket launch, the pack moves every input byte once to base + (bk % 2) * threshold +
    (offset - bucket offset), inside the two slots; the unpack reads exactly those addresses and
    writes every output byte once."""
    T = tabs.tile
    for b, mem in enumerate(bucket_members(tabs, counts, offs, es, threshold)):
        _off, _nbytes, t0, nt = tabs.buckets[b]
        pack = run_table(tabs.tables[0], tabs.ntiles, T, range(t0, t0 + nt))
        assert all(BASE <= d and d + ln <= BASE + 2 * threshold for d, _s, ln in pack), "%s: a pack outside the slots" % what
        check_moves([(addr, ins[i], counts[i] * es) for i, addr in mem], pack, what="%s, pack of bucket %d" % (what, b))
        unpack = run_table(tabs.tables[1], tabs.ntiles, T, range(t0, t0 + nt))
        check_moves([(outs[i], addr, counts[i] * es) for i, addr in mem], unpack, what="%s, unpack of bucket %d" % (what, b))


def check_flat_table(tabs, counts, ins, es, offs, total, what):
    """kFlat: one launch over the whole space lands every tensor at its tips_fused_layout offset."""
    moves = run_table(tabs.tables[0], tabs.ntiles, tabs.tile)
    assert all(BASE <= d and d + ln <= BASE + total for d, _s, ln in moves), "%s: a copy outside the flat output" % what
    check_moves([(BASE + offs[i], ins[i], c * es) for i, c in enumerate(counts)], moves, what=what)


@pytest.mark.parametrize("order", ["0", "1", "2"])
@pytest.mark.parametrize("tile", fc.TILES)
def test_slot_and_flat_tables_move_every_byte_once(monkeypatch, tile, order):
    """The slot tables (pack and unpack, one launch per bucket) and the flat table of the directed list
    in both placements and of a random list, for every element size, tile and launch order."""
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(fc.THRESHOLD))
    monkeypatch.setenv("TIPS_COPY_TILE_BYTES", str(tile))
    monkeypatch.setenv("TIPS_COPY_ORDER", order)
    for es in (2, 4, 8):
        dtype = fc.CODE_OF_ES[es]
        for name, counts, ins, outs in lists_for(es, es, tile + int(order) + es):
            offs, total = layout_offsets(counts, dtype)
            what = "%s, %d-byte elements" % (name, es)
            tabs = fc.mode_tables(counts, dtype, fc.SLOT, ins, outs, BASE)
            assert tabs.tile == tile and len(tabs.tables) == 2
            check_slot_tables(tabs, counts, ins, outs, es, offs, fc.THRESHOLD, "slot tables: " + what)
            tabs = fc.mode_tables(counts, dtype, fc.FLAT, ins, outs, BASE)
            assert len(tabs.tables) == 1
            check_flat_table(tabs, counts, ins, es, offs, total, "flat table: " + what)


def run_cast_table(rec, ntiles, T, direction, slots, staged=True):
    """[(dst, src, elements)] moved by one cast_segs_kernel launch over record slots `slots`
    (direction 0: float32 source -> wire destination, 1: back), per the kernel's rules: a tile inside
    one segment with both record bases 16-B aligned is staged whole (unless `staged` is off: the
    TIPS_CAST_VARIANT kernels); else lane `tid` takes the quads at wire byte
    v = tile byte + u * 256 * 8 + tid * 8, u < 2 U, each `len` = min(8, segment end - v) wire bytes
    when v lies in its segment; the float32 side is at base + 2 v; a quad is moved whole when len = 8,
    the float32 side is 16-B and the wire side 8-B aligned, else element by element."""
    Q = 2 * (T // (LANES * VEC))
    max_seg = T // 256 + 1
    out = []
    for q in slots:
        a, b = rec[2 * q], rec[2 * q + 1]
        multi, two = a[3] < 0, b[3] > 0
        tb = (b[2] & ~(T - 1)) if two else b[2]
        if staged and not multi and not two and a[2] <= tb and a[3] >= tb + T and ((a[0] | a[1]) & 15) == 0:
            if direction == 0:
                out.append((a[1] + tb, a[0] + 2 * tb, T // 2))
            else:
                out.append((a[1] + 2 * tb, a[0] + tb, T // 2))
            continue
        segs = None
        if multi:
            cnt = min(a[1], max_seg)
            if cnt <= 0:
                continue
            segs = rec[2 * ntiles + a[0]:2 * ntiles + a[0] + cnt]
        for u in range(Q):
            for tid in range(LANES):
                v = tb + u * LANES * 8 + tid * 8
                if multi:
                    lo, hi = 0, len(segs) - 1
                    while lo < hi:
                        mid = (lo + hi + 1) >> 1
                        if segs[mid][2] <= v:
                            lo = mid
                        else:
                            hi = mid - 1
                    g = segs[lo]
                else:
                    g = b if (two and v >= b[2]) else a
                left = g[3] - v
                ln = min(left, 8) if (v >= g[2] and left > 0) else 0
                sp = g[0] + (2 * v if direction == 0 else v)
                dp = g[1] + (v if direction == 0 else 2 * v)
                f32_side, wire_side = (sp, dp) if direction == 0 else (dp, sp)
                if ln == 8 and f32_side % 16 == 0 and wire_side % 8 == 0:
                    out.append((dp, sp, 4))
                else:
                    e = 0
                    while 2 * e < ln:
                        out.append((dp + (2 if direction == 0 else 4) * e, sp + (4 if direction == 0 else 2) * e, 1))
                        e += 1
    return out


def check_cast_tables(tabs, counts, ins, outs, offs, threshold, what, staged=True):
    """kSlotCast: per bucket launch, the pack reads every float32 element once and writes every wire
    element once, at base + (bk % 2) * threshold + (offset - bucket offset) + 2 k inside the slots;
    the unpack the converse into the outputs; nothing else is touched."""
    T = tabs.tile
    for b, mem in enumerate(bucket_members(tabs, counts, offs, 2, threshold)):
        _off, _nbytes, t0, nt = tabs.buckets[b]
        pack = run_cast_table(tabs.tables[0], tabs.ntiles, T, 0, range(t0, t0 + nt), staged)
        assert all(BASE <= d and d + 2 * n <= BASE + 2 * threshold for d, _s, n in pack), "%s: a pack outside the slots" % what
        check_moves([(addr, ins[i], counts[i]) for i, addr in mem], pack, 2, 4, "%s, pack of bucket %d" % (what, b))
        unpack = run_cast_table(tabs.tables[1], tabs.ntiles, T, 1, range(t0, t0 + nt), staged)
        check_moves([(outs[i], addr, counts[i]) for i, addr in mem], unpack, 4, 2, "%s, unpack of bucket %d" % (what, b))


def cast_case(monkeypatch, tile):
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(fc.THRESHOLD))
    monkeypatch.setenv("TIPS_CAST_TILE_BYTES", str(tile))
    monkeypatch.setenv("TIPS_COPY_TILE_BYTES", str(tile))  # (tips_fused_layout, the expected offsets' source, walks the copy's tile)


@pytest.mark.parametrize("tile", fc.TILES)
def test_cast_tables_move_every_element_once(monkeypatch, tile):
    """The fused cast's pack and unpack tables under run_cast_table, for both wire types; at 8 KiB
    tiles with an f16 wire also as the TIPS_CAST_VARIANT 0-5 kernels walk them (no staged tiles)."""
    cast_case(monkeypatch, tile)
    for wire in (fc.F16, fc.BF16):
        for name, counts, ins, outs in lists_for(2, 4, tile + wire):
            offs, _total = layout_offsets(counts, wire)
            tabs = fc.mode_tables(counts, wire, fc.SLOT_CAST, ins, outs, BASE)
            assert tabs.tile == tile and len(tabs.tables) == 2
            check_cast_tables(tabs, counts, ins, outs, offs, fc.THRESHOLD, "cast tables: " + name)
            if tile == 8192 and wire == fc.F16:  # TIPS_CAST_VARIANT 0-5: no staged tiles
                check_cast_tables(tabs, counts, ins, outs, offs, fc.THRESHOLD, "cast tables, quads only: " + name, staged=False)


def perturbed(tabs, table, index, field, delta):
    """tabs with `delta` added to one field of one record of one table (a copy)."""
    t = [list(x) for x in tabs.tables]
    r = list(t[table][index])
    r[field] += delta
    t[table][index] = tuple(r)
    return fc.Tables(t, tabs.ntiles, tabs.tile, tabs.buckets)


def first_slot(tabs, table, pred):
    for _off, _nbytes, t0, nt in tabs.buckets:
        for q in range(t0, t0 + nt):
            if pred(tabs.tables[table][2 * q], tabs.tables[table][2 * q + 1]):
                return q
    raise LookupError("no such tile")  # (never an AssertionError: the callers expect those of the checks)


SRC, DST, BEGIN, END = 0, 1, 2, 3


@pytest.mark.parametrize("which", ["slot offset of a tile record", "slot offset of a listed segment", "unpack source",
                                   "second record of a two-segment tile", "segment end", "tile byte"])
def test_perturbed_slot_records_fail_the_checks(monkeypatch, which):
    """One field of one record off (a slot offset by 256, a source by 16, an end by one element, a
    tile's byte offset by one tile): the checks of the slot tables fail. Unperturbed, they pass."""
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(fc.THRESHOLD))
    monkeypatch.setenv("TIPS_COPY_TILE_BYTES", "8192")
    name, counts, ins, outs = lists_for(4, 4, 1)[0]
    offs, _total = layout_offsets(counts, fc.F32)
    tabs = fc.mode_tables(counts, fc.F32, fc.SLOT, ins, outs, BASE)
    check_slot_tables(tabs, counts, ins, outs, 4, offs, fc.THRESHOLD, name)
    nt = tabs.ntiles
    if which == "slot offset of a tile record":
        bad = perturbed(tabs, 0, 2 * first_slot(tabs, 0, lambda a, b: a[3] > 0 and b[3] == 0), DST, 256)
    elif which == "slot offset of a listed segment":
        q = first_slot(tabs, 0, lambda a, b: a[3] < 0)
        bad = perturbed(tabs, 0, 2 * nt + tabs.tables[0][2 * q][0] + 1, DST, 256)
    elif which == "unpack source":
        bad = perturbed(tabs, 1, 2 * first_slot(tabs, 1, lambda a, b: a[3] > 0 and b[3] == 0), SRC, 16)
    elif which == "second record of a two-segment tile":
        bad = perturbed(tabs, 0, 2 * first_slot(tabs, 0, lambda a, b: b[3] > 0) + 1, DST, 256)
    elif which == "segment end":
        bad = perturbed(tabs, 0, 2 * first_slot(tabs, 0, lambda a, b: 0 < a[3] < b[2] + tabs.tile and b[3] == 0), END, -4)
    else:
        bad = perturbed(tabs, 0, 2 * first_slot(tabs, 0, lambda a, b: a[3] > 0 and b[3] == 0) + 1, BEGIN, tabs.tile)
    with pytest.raises(AssertionError):
        check_slot_tables(bad, counts, ins, outs, 4, offs, fc.THRESHOLD, name)


@pytest.mark.parametrize("which", ["f32 base with v for 2 v", "f32 base of a listed segment", "unpack f32 base", "slot offset"])
def test_perturbed_cast_records_fail_the_checks(monkeypatch, which):
    """The cast's records with the float32 base computed as in - b instead of in - 2 b (so the
    float32 side would be read at base + v + b, not base + 2 v), or a slot offset off by 256: the
    checks of the cast tables fail."""
    cast_case(monkeypatch, 8192)
    name, counts, ins, outs = lists_for(2, 4, 2)[0]
    offs, _total = layout_offsets(counts, fc.F16)
    tabs = fc.mode_tables(counts, fc.F16, fc.SLOT_CAST, ins, outs, BASE)
    check_cast_tables(tabs, counts, ins, outs, offs, fc.THRESHOLD, name)
    nt = tabs.ntiles
    if which == "f32 base with v for 2 v":
        q = first_slot(tabs, 0, lambda a, b: a[3] > 0 and a[2] > 0 and b[3] == 0)
        bad = perturbed(tabs, 0, 2 * q, SRC, tabs.tables[0][2 * q][2])
    elif which == "f32 base of a listed segment":
        q = first_slot(tabs, 0, lambda a, b: a[3] < 0 and a[0] > 0)
        k = 2 * nt + tabs.tables[0][2 * q][0] + 1
        bad = perturbed(tabs, 0, k, SRC, tabs.tables[0][k][2])
    elif which == "unpack f32 base":
        q = first_slot(tabs, 1, lambda a, b: a[3] > 0 and a[2] > 0 and b[3] == 0)
        bad = perturbed(tabs, 1, 2 * q, DST, tabs.tables[1][2 * q][2])
    else:
        bad = perturbed(tabs, 0, 2 * first_slot(tabs, 0, lambda a, b: a[3] > 0 and b[3] == 0), DST, 256)
    with pytest.raises(AssertionError):
        check_cast_tables(bad, counts, ins, outs, offs, fc.THRESHOLD, name)
