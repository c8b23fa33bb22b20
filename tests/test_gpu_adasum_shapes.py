"""-m gpu: the Adasum pair (tips_adasum_pair) at the launch shapes, list layouts and
edge values test_gpu_adasum.py does not reach, against the numpy restatement (tests/adasum_util.py),
bit for bit - the output and, read back from the workspace, every chunk's partial sums (d, na, nb) and
every segment's f64 coefficients (ca, cb): the values that carry the summation order, which the fp32
rounding of the coefficients hides from the output bits.

Shapes: single segments of 128, 129, 256 and 257 chunks (the last grid on contiguous eighths, the
first striped one with its idle workgroups, the last one-row coefficient pass, its second row),
again one element past a 16-B boundary and in place. Lists: every start 16-B aligned (the vector
path under a device table, with empty segments at every place and more than 128 chunks), one odd
count that misaligns and a later one that re-aligns, 301 segments, the operands aligned differently
from each other and from dst. Every call's workspace is exactly tips_adasum_workspace bytes between
two guards, and dst has spare elements on both sides; all of them must come back untouched. Edge
values run as the middle segment of a list, aligned and one element off. Then the layout cache past
its 32 entries.

test_adasum_cpu.py vouches for the restatement at these sizes and shows that the operands used at 257
chunks tell the kernels' order from other ones."""
import numpy as np
import pytest

from adasum_util import (ES, bf16_round_bits, chunk_elems, long_pair, pair_intermediates, pair_ref, seeded_pair, shape_counts,
                         to_work, workspace_bytes)
from gpu_util import BF16, F16, F32, F64, NPDT, bits, same_bits, stream

pytestmark = pytest.mark.gpu

FLOATS = [F32, F64, F16, BF16]
GUARD = 4096  # bytes on each side of the workspace
FILL = 0xA5  # every byte a kernel must not write
SIGN = {F32: 1 << 31, F64: 1 << 63, F16: 1 << 15, BF16: 1 << 15}
_REF = {}  # (dtype, counts, salt) -> (a, b, output, partials, coefficients): computed once, never written
_CLEAN = {}  # (dtype, salt) -> the device's run of the edge list with a seeded middle segment


def KE(dtype):
    return chunk_elems(dtype), 16 // ES[dtype]


def restate(a, b, counts, dtype):
    parts, coef = pair_intermediates(a, b, counts, dtype)
    return pair_ref(a, b, counts, dtype), parts, coef


def case(dtype, counts, salt=0):
    """Seeded independent operands; salt "long": the single-segment shape cases' (b near 2 a, so
    that the coefficients' bits carry the dots' last ones: adasum_util.LONG_SALT)."""
    key = (dtype, tuple(counts), salt)
    if key not in _REF:
        a, b = long_pair(dtype, counts[0]) if salt == "long" else seeded_pair(dtype, counts, salt)
        _REF[key] = (a, b) + restate(a, b, counts, dtype)
        for x in _REF[key]:
            x.setflags(write=False)
    return _REF[key]


def _buffer(x, off, dtype):
    """A device byte buffer with x from element E + off on (E elements = 16 B) and FILL around it:
    at least one spare element before x and 16 B after it. Returns (buffer, x's first byte)."""
    import torch
    lead = (16 // ES[dtype] + off) * ES[dtype]
    buf = torch.full((lead + x.nbytes + 16,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[lead:lead + x.nbytes] = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()
    return buf, lead


def _read(buf, lead, nbytes, dtype):
    """The nbytes from `lead` on, after asserting that every byte around them still holds FILL."""
    h = buf.cpu().numpy()
    assert (h[:lead] == FILL).all(), "written before the first element"
    assert (h[lead + nbytes:] == FILL).all(), "written after the last element"
    return h[lead:lead + nbytes].copy().view(NPDT[dtype])


def pair_ws(a, b, counts, dtype, oa=0, ob=0, od=0, into=None):
    """tips_adasum_pair with a, b and dst each `o` elements past a 16-B boundary of a buffer of its own
    (into = "a" / "b": in place into that operand), FILL on both sides of each, and a workspace of
    exactly tips_adasum_workspace bytes between two guards of GUARD bytes. Asserts that nothing was
    written outside dst's elements and the workspace's partials and coefficients, and that an operand
    which is not dst kept its bytes. Returns (output, partials (nchunks, 3), coefficients (nseg, 2))."""
    import torch
    from tips_amd import _lib
    n, nseg = sum(counts), len(counts)
    assert len(a) == len(b) == n
    need = _lib.lib().tips_adasum_workspace(n, nseg)
    assert need == workspace_bytes(n, nseg) and need % 8 == 0
    nchunks = sum(-(-c // chunk_elems(dtype)) for c in counts)
    used = 8 * (3 * nchunks + 2 * nseg)
    assert used <= need
    ba, la = _buffer(a, oa, dtype)
    bb, lb = _buffer(b, ob, dtype)
    if into is None:
        ld = (16 // ES[dtype] + od) * ES[dtype]
        bd = torch.full((ld + a.nbytes + 16,), FILL, dtype=torch.uint8, device="cuda")
        assert bd.data_ptr() % 16 == 0
    else:
        bd, ld = {"a": (ba, la), "b": (bb, lb)}[into]
    ws = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert (ws.data_ptr() + GUARD) % 8 == 0
    cp, _keep = _lib.i64_array(list(counts))
    _lib.call("tips_adasum_pair", bd.data_ptr() + ld, ba.data_ptr() + la, bb.data_ptr() + lb, cp, nseg, dtype,
              ws.data_ptr() + GUARD, need, stream())
    torch.cuda.synchronize()
    out = _read(bd, ld, a.nbytes, dtype)
    if into != "a":
        assert np.array_equal(bits(_read(ba, la, a.nbytes, dtype)), bits(a)), "a was written"
    if into != "b":
        assert np.array_equal(bits(_read(bb, lb, b.nbytes, dtype)), bits(b)), "b was written"
    w = _read(ws, GUARD, used, F64)  # (the guards, and what the formula leaves spare after the coefficients)
    return out, w[:3 * nchunks].reshape(nchunks, 3), w[3 * nchunks:].reshape(nseg, 2)


def check(got, exp, dtype, what=""):
    """Output, partials and coefficients, all bit for bit (any NaN matches any NaN)."""
    out, parts, coef = got
    eo, ep, ec = exp
    assert parts.shape == ep.shape and coef.shape == ec.shape, what
    bad = [i for i in range(len(ep)) if not same_bits(parts[i], ep[i], F64)]
    assert not bad, "%s: %d of %d chunks' partials differ, first %s" % (what, len(bad), len(ep), bad[:8])
    bad = [i for i in range(len(ec)) if not same_bits(coef[i], ec[i], F64)]
    assert not bad, "%s: %d of %d segments' coefficients differ, first %s" % (what, len(bad), len(ec), bad[:8])
    assert same_bits(out, eo, dtype), what


def aligned_list(dtype):
    """Every segment starts on a 16-B boundary (every count a multiple of E, those that do not depend
    on the dtype of 8): a count below a wave, exactly K, 2 K, K + E (one vector in its last chunk,
    next to the next segment's first), 3 K + 8, empty segments first, twice in the middle and last,
    and a long one that takes the call past 128 chunks - 130, a striped grid of 256."""
    K, E = KE(dtype)
    return [0, 40, K, 2 * K, 0, 0, K + E, 120 * K, 3 * K + 8, 0]


def realign_list(dtype):
    """K + 1 misaligns what follows it, the K + E - 1 after it restores 16 B: segments 0, 1, 4 and 5 take
    vectors, 2 and 3 elements, in one call."""
    K, E = KE(dtype)
    return [2 * K, 48, K + 1, K + E - 1, 2 * K + 8, 40]


# ---------------------------------------------------------------------------
# launch shapes: one segment


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("which", range(4), ids=["128", "129", "256", "257"])
def test_single_segments_at_the_grid_and_coefficient_boundaries(gpu, dtype, which):
    n = shape_counts(dtype)[which]
    a, b, *exp = case(dtype, [n], "long")
    assert len(exp[1]) == (128, 129, 256, 257)[which]
    check(pair_ws(a, b, [n], dtype), exp, dtype)


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("which", [1, 3], ids=["129", "257"])
def test_striped_map_on_the_element_path_and_in_place(gpu, dtype, which):
    """One element past a 16-B boundary every access is an element access, under the striped map; in
    place into a every lane stores where it has loaded. The same partials and outputs as aligned."""
    n = shape_counts(dtype)[which]
    a, b, *exp = case(dtype, [n], "long")
    check(pair_ws(a, b, [n], dtype, oa=1, ob=1, od=1), exp, dtype, "one element off")
    check(pair_ws(a, b, [n], dtype, into="a"), exp, dtype, "in place into a")


# ---------------------------------------------------------------------------
# lists: the vector path under a device table


@pytest.mark.parametrize("dtype", FLOATS)
def test_aligned_list(gpu, dtype):
    counts = aligned_list(dtype)
    K, E = KE(dtype)
    assert all(o * ES[dtype] % 16 == 0 for o in np.cumsum([0] + counts)) and sum(-(-c // K) for c in counts) > 128
    a, b, *exp = case(dtype, counts)
    got = pair_ws(a, b, counts, dtype)
    check(got, exp, dtype)
    for s, c in enumerate(counts):
        if c == 0:
            assert tuple(got[2][s]) == (1.0, 1.0), s


@pytest.mark.parametrize("dtype", FLOATS)
def test_one_odd_count_misaligns_and_a_later_one_realigns(gpu, dtype):
    counts = realign_list(dtype)
    starts = [o * ES[dtype] % 16 == 0 for o in np.cumsum([0] + counts)[:-1]]
    assert starts == [True, True, True, False, True, True]
    a, b, *exp = case(dtype, counts)
    check(pair_ws(a, b, counts, dtype), exp, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_many_segments_equal_their_segments_one_by_one(gpu, dtype):
    """301 segments (the binary search nine levels deep, a coefficient grid of 301), empty ones and
    two-chunk ones among them."""
    K, E = KE(dtype)
    counts = ([3, 0, K + 5, 64, 1, 0, 17] * 43)[:301]
    a, b, *exp = case(dtype, counts)
    whole = pair_ws(a, b, counts, dtype)
    check(whole, exp, dtype)
    o = c0 = 0
    for s, c in enumerate(counts):
        if c:
            out, parts, coef = pair_ws(a[o:o + c], b[o:o + c], [c], dtype)
            m = len(parts)
            assert np.array_equal(bits(out), bits(whole[0][o:o + c])), s
            assert np.array_equal(bits(parts), bits(whole[1][c0:c0 + m])) and np.array_equal(bits(coef[0]), bits(whole[2][s])), s
            c0 += m
        o += c


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("shape", ["segment", "list"])
def test_operands_and_dst_aligned_differently(gpu, dtype, shape):
    """The dots pass chooses vectors or elements from a and b, the combine from a, b and dst: with
    dst alone misaligned the two passes decide differently, with b alone or a alone misaligned both
    take elements. The aligned call's bits every time."""
    K, E = KE(dtype)
    counts = [3 * K + E + 1] if shape == "segment" else aligned_list(dtype)
    a, b, *exp = case(dtype, counts)
    base = pair_ws(a, b, counts, dtype)
    check(base, exp, dtype, "aligned")
    for what, kw in [("dst off", dict(od=1)), ("b off", dict(ob=1)), ("a off, into b", dict(oa=1, into="b"))]:
        got = pair_ws(a, b, counts, dtype, **kw)
        for g, e in zip(got, base):
            assert np.array_equal(bits(g), bits(e)), what


def test_workspace_at_the_tight_cut(gpu):
    """f64, 64 segments of 4097 elements: two chunks each, and the workspace formula leaves not one
    spare byte - the last coefficient ends where the guard begins."""
    counts = [4097] * 64
    assert workspace_bytes(sum(counts), 64) == 8 * (3 * 128 + 2 * 64)
    a, b, *exp = case(F64, counts)
    check(pair_ws(a, b, counts, F64), exp, F64)
    check(pair_ws(a, b, counts, F64, oa=1, ob=1, od=1), exp, F64, "one element off")


# ---------------------------------------------------------------------------
# edge values: the middle segment of a list, aligned and one element off


def stored(x, dtype):
    """Values -> the storage type, rounded to nearest."""
    return bf16_round_bits(np.asarray(x, np.float32)) if dtype == BF16 else np.asarray(x).astype(NPDT[dtype])


def negated(x, dtype):
    return x ^ np.uint16(0x8000) if dtype == BF16 else -x


def nan_at(x, dtype):
    return np.isnan(to_work(x, dtype))


def edge_len(dtype):
    return chunk_elems(dtype) + 40  # a whole chunk and a partial one of whole vectors


def edge_run(dtype, ea, eb, salt):
    """The list [72, len(ea), 4104] with (ea, eb) between seeded neighbours, run aligned and with
    every pointer one element off; both are held to the restatement. Returns the aligned run's
    (output, partials, coefficients), the restatement's, and the middle segment's bounds."""
    counts = [72, len(ea), 4104]
    a, b = seeded_pair(dtype, counts, salt)
    lo, hi = 72, 72 + len(ea)
    a[lo:hi], b[lo:hi] = ea, eb
    exp = restate(a, b, counts, dtype)
    got = pair_ws(a, b, counts, dtype)
    check(got, exp, dtype, "aligned")
    check(pair_ws(a, b, counts, dtype, oa=1, ob=1, od=1), exp, dtype, "one element off")
    key = (dtype, salt)
    if key not in _CLEAN:  # the same neighbours around a seeded middle segment, on the device
        ca, cb, *cexp = case(dtype, counts, salt)
        _CLEAN[key] = pair_ws(ca, cb, counts, dtype)
        check(_CLEAN[key], cexp, dtype, "clean")
    clean = _CLEAN[key][0]  # the neighbours see nothing of the middle segment
    assert np.array_equal(bits(got[0][:lo]), bits(clean[:lo])) and np.array_equal(bits(got[0][hi:]), bits(clean[hi:]))
    return got, exp, lo, hi


@pytest.mark.parametrize("dtype", FLOATS)
def test_antiparallel_operands_give_plus_zero(gpu, dtype):
    """b = -a: d = -na = -nb bit for bit, ca = cb = 1.5, and fl(1.5 a) - fl(1.5 a) = +0."""
    ea = seeded_pair(dtype, [edge_len(dtype)], 1)[0]
    ea[[3, 70]] = 0  # (1.5 (+0) + 1.5 (-0) = +0 too)
    got, exp, lo, hi = edge_run(dtype, ea, negated(ea, dtype), 1)
    assert tuple(got[2][1]) == (1.5, 1.5)
    assert not bits(got[0][lo:hi]).any()


@pytest.mark.parametrize("dtype", FLOATS)
def test_minus_zero_is_kept_under_positive_coefficients(gpu, dtype):
    n = edge_len(dtype)
    ea = np.abs(seeded_pair(F64, [n], 2)[0]) + 0.5
    eb = ea.copy()
    eb[::3] = np.abs(seeded_pair(F64, [n], 2)[1][::3]) + 0.5
    at = [0, 5, 63, 64, chunk_elems(dtype) - 1, chunk_elems(dtype), n - 1]
    ea[at] = eb[at] = -0.0
    got, exp, lo, hi = edge_run(dtype, stored(ea, dtype), stored(eb, dtype), 2)
    assert (exp[2][1] > 0).all()  # (the restatement's: all operands positive, ca and cb near 1 / 2)
    assert (bits(got[0][lo:hi])[at] == SIGN[dtype]).all()


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_subnormal_only_segments_are_not_flushed(gpu, dtype):
    """Segments of subnormals alone (fp32 subnormals too, in bf16): their norms are far inside f64's
    range, so the coefficients are those of the directions; and with a == b, ca = cb = 0.5 exactly
    and 0.5 a + 0.5 a = a - halving is exact in fp32 - so every subnormal comes back as it went in."""
    n = edge_len(dtype)
    rng = np.random.default_rng([20261020, dtype, 3])
    mant = {F16: 10, BF16: 7}[dtype]
    ua = (rng.integers(1, 1 << mant, n) | (rng.integers(0, 2, n) << 15)).astype(np.uint16)
    ub = ua.copy()
    ub[::3] = rng.integers(1, 1 << mant, len(ub[::3])).astype(np.uint16)
    ea, eb = (ua, ub) if dtype == BF16 else (ua.view(np.float16), ub.view(np.float16))
    got, exp, lo, hi = edge_run(dtype, ea, eb, 3)
    assert not np.array_equal(exp[2][1], [1.0, 1.0])
    assert np.count_nonzero(bits(exp[0][lo:hi]) & 0x7fff) > n // 2  # (so a flushed output cannot match)
    got, exp, lo, hi = edge_run(dtype, ea, ea.copy(), 3)
    assert tuple(got[2][1]) == (0.5, 0.5)
    assert np.array_equal(bits(got[0][lo:hi]), ua)


def test_f16_store_overflows_where_the_restatement_does(gpu):
    """Finite f16 inputs whose result is not: two elements of 60000 in both operands, two more with
    opposite signs so that d stays small and ca, cb near 1 - 120000 at the store is inf, the rest finite."""
    n = edge_len(F16)
    ea, eb = seeded_pair(F16, [n], 4)
    up, down = [100, chunk_elems(F16) + 17], [200, chunk_elems(F16) + 30]
    ea[up] = eb[up] = ea[down] = 60000
    eb[down] = -60000
    got, exp, lo, hi = edge_run(F16, ea, eb, 4)
    want = np.zeros(n, bool)
    want[up] = True
    assert np.array_equal(np.isinf(exp[0][lo:hi]), want) and np.isfinite(exp[0][lo:hi][~want]).all()
    assert np.array_equal(np.isinf(got[0][lo:hi]), want) and (got[0][lo:hi][up] > 0).all()


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_coefficient_beyond_the_working_type(gpu, dtype):
    """a tiny, b large and of a's signs: ca = 1 - d / 2 na is finite in f64 and, for f32 and bf16
    (a near 2^-100, b near 2^100), far beyond fp32 - it rounds to -inf, so every element is an
    infinity of the sign opposite to a_i's, and NaN (inf 0) where a_i = 0.
    f16 cannot get there: |d / na| <= |b| / |a| <= sqrt(n) 65504 / 2^-24, inside fp32 for any n that
    fits a buffer. Its case keeps the construction (a subnormal, b near 2^14) and checks what does
    hold: ca, beyond 2^30, is still finite in fp32, and the device has the restatement's bits."""
    n = edge_len(dtype)
    x, y = seeded_pair(F64, [n], 5)
    x[x == 0] = 1.0
    zero = [0, 9, 64, chunk_elems(dtype) + 3]
    x[zero] = 0.0
    small, large = (2.0 ** -100, 2.0 ** 100) if dtype != F16 else (2.0 ** -23, 2.0 ** 12)
    ea = stored(x * small, dtype)
    eb = stored(np.where(x < 0, -1.0, 1.0) * (np.abs(y) + 0.5) * large, dtype)
    got, exp, lo, hi = edge_run(dtype, ea, eb, 5)
    ca = exp[2][1][0]
    out = to_work(got[0][lo:hi], dtype)
    a_w = to_work(ea, dtype)
    is_zero = a_w == 0
    assert np.isfinite(ca) and ca < 0
    assert np.isfinite(to_work(eb, dtype)).all() and is_zero[zero].all()
    if dtype == F16:
        assert 2.0 ** 30 < abs(ca) < np.finfo(np.float32).max
        assert not np.isnan(out).any()
    else:
        assert abs(ca) > np.finfo(np.float32).max and is_zero.sum() == len(zero)
        assert np.array_equal(np.isnan(out), is_zero)
        assert np.array_equal(out[~is_zero], np.where(a_w[~is_zero] > 0, -np.inf, np.inf).astype(np.float32))


def test_f64_norms_that_overflow_make_the_segment_nan(gpu):
    ea, eb = seeded_pair(F64, [edge_len(F64)], 6)
    got, exp, lo, hi = edge_run(F64, ea * 1e200, eb * 1e200, 6)
    assert np.isnan(got[0][lo:hi]).all()


def test_f64_norms_that_underflow_to_zero_give_the_bucket_sum(gpu):
    """Values near 1e-200: every product underflows to exact zero, na = nb = 0 is not > 0, both
    coefficients are 1 and the result is a + b - tips_bucket_sum's bits."""
    import torch
    from tips_amd import _lib
    ea, eb = seeded_pair(F64, [edge_len(F64)], 7)
    ea, eb = ea * 1e-200, eb * 1e-200
    assert np.count_nonzero(ea) > len(ea) // 2 and not (ea * ea).any() and not (eb * eb).any() and not (ea * eb).any()
    got, exp, lo, hi = edge_run(F64, ea, eb, 7)
    assert not got[1][1:3].any() and tuple(got[2][1]) == (1.0, 1.0)  # (the middle segment's two chunks)
    da, db = torch.from_numpy(ea).cuda(), torch.from_numpy(eb).cuda()
    dc = torch.empty_like(da)
    _lib.call("tips_bucket_sum", dc.data_ptr(), da.data_ptr(), db.data_ptr(), len(ea), F64, stream())
    torch.cuda.synchronize()
    assert np.array_equal(bits(got[0][lo:hi]), bits(dc.cpu().numpy()))


@pytest.mark.parametrize("dtype", FLOATS)
def test_infinity_in_b_stays_in_its_segment(gpu, dtype):
    """+inf in b alone: nb = inf, d = +-inf, cb = 1 - NaN / 2 - the segment is NaN throughout; its
    neighbours are the clean run's (edge_run asserts it)."""
    ea, eb = seeded_pair(dtype, [edge_len(dtype)], 8)
    eb[chunk_elems(dtype) + 11] = 0x7f80 if dtype == BF16 else np.inf
    got, exp, lo, hi = edge_run(dtype, ea, eb, 8)
    assert nan_at(got[0][lo:hi], dtype).all()
    assert not nan_at(got[0][:lo], dtype).any() and not nan_at(got[0][hi:], dtype).any()


# ---------------------------------------------------------------------------
# the segment-layout cache


def test_layout_cache_evicts_and_uploads_again(gpu):
    """40 layouts through a cache of 32: the first ones are evicted (and freed) and uploaded again;
    the same counts under f32 and f64 are two layouts (another chunk size, other first chunks);
    shutdown releases them all. Every call exact."""
    import torch

    def run(counts, dtype):
        a, b, *exp = case(dtype, counts, 9)
        check(pair_ws(a, b, counts, dtype), exp, dtype, str(counts))

    lists = [[3 + i, 2, 40 - i] for i in range(40)]
    for counts in lists + [lists[0], lists[39], lists[1]]:
        run(counts, F32)
    same = [5000, 9000, 3]  # 1 + 2 + 1 chunks in f32, 2 + 3 + 1 in f64
    for dtype in (F32, F64, F32, F16, BF16):
        run(same, dtype)
    torch.cuda.synchronize()
    gpu.shutdown()
    gpu.init()
    run(same, F64)
    run(lists[0], F32)
