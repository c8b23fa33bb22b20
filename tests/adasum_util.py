"""Adasum in numpy: the restatement of the definition the GPU tests compare with bit
for bit - the kernels' summation order, the coefficient formula, the combine and the rank tree - and a
second, order-free reference (exact products, math.fsum, the combine in f64) with the bound the
definition allows against it.

Storage arrays are numpy arrays of gpu_util.NPDT[dtype] (bf16 as uint16 bit patterns)."""
import math

import numpy as np

from gpu_util import BF16, F16, F32, F64, NPDT, rand

CHUNK_BYTES = 32768  # of each operand per chunk: 256 lanes x 8 vectors of 16 B
LANES, VECS = 256, 8
ES = {F32: 4, F64: 8, F16: 2, BF16: 2}
U_W = {F32: 2.0 ** -24, F64: 2.0 ** -53, F16: 2.0 ** -24, BF16: 2.0 ** -24}
U_S = {F32: 0.0, F64: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}


def chunk_elems(dtype):
    return CHUNK_BYTES // ES[dtype]


def workspace_bytes(count, nseg):
    return (8 * (3 * (count // 4096 + nseg) + 2 * nseg) + 255) // 256 * 256


def to_work(x, dtype):
    """Storage -> the working type W (fp32, or f64 for F64); exact."""
    if dtype == BF16:
        return (x.astype(np.uint32) << 16).view(np.float32)
    return x.astype(np.float64 if dtype == F64 else np.float32)


def to_f64(x, dtype):
    return to_work(x, dtype).astype(np.float64)


def bf16_round_bits(w):
    """fp32 -> bf16 bits, round to nearest even, NaN kept quiet (kernels_device.h bf16_round_bits)."""
    x = np.ascontiguousarray(w, np.float32).view(np.uint32).astype(np.uint64)
    nan = (x & 0x7fffffff) > 0x7f800000
    r = (x + 0x7fff + ((x >> 16) & 1)) >> 16
    return np.where(nan, (x >> 16) | 0x40, r).astype(np.uint16)


def round_store(w, dtype):
    """W -> storage: the one rounding at the store."""
    with np.errstate(over="ignore"):
        if dtype == BF16:
            return bf16_round_bits(w)
        return w.astype(NPDT[dtype])


def _tree256(v):
    """256 values (last axis) to one: in each wave of 64 x[l] += x[l + 32], x[l] += x[l + 16], ...
    x[l] += x[l + 1]; then ((w0 + w1) + w2) + w3."""
    v = v.reshape(v.shape[:-1] + (4, 64))
    for d in (32, 16, 8, 4, 2, 1):
        v = v[..., :d] + v[..., d:2 * d]
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def chunk_partials(a, b, dtype, tree=_tree256):
    """The (m, 3) chunk sums (d, na, nb) of one segment of m chunks in the kernels' order - what the
    dots pass leaves in the workspace. Element i belongs to chunk i // K and to lane
    (i % K // E) % 256 of it; a lane adds its products in ascending i from +0; a chunk's 256 lane
    sums go through `tree`. (Zero padding is bit-neutral: an accumulator that started at +0 is never
    -0, and x + 0 = x.)"""
    E, K = 16 // ES[dtype], chunk_elems(dtype)
    n = len(a)
    m = -(-n // K)
    if m == 0:
        return np.zeros((0, 3), np.float64)
    x = np.zeros(m * K, np.float64)
    y = np.zeros(m * K, np.float64)
    x[:n], y[:n] = to_f64(a, dtype), to_f64(b, dtype)
    x, y = x.reshape(m, VECS, LANES, E), y.reshape(m, VECS, LANES, E)
    acc = np.zeros((3, m, LANES), np.float64)
    with np.errstate(all="ignore"):
        for u in range(VECS):
            for j in range(E):
                xs, ys = x[:, u, :, j], y[:, u, :, j]
                # f32 / f16 / bf16: the products are exact in f64 (the kernel's fma rounds once, as
                # this add does); F64: a rounded multiply, then the add - what the kernel does
                acc[0] = acc[0] + xs * ys
                acc[1] = acc[1] + xs * xs
                acc[2] = acc[2] + ys * ys
        return np.ascontiguousarray(tree(acc).T)


def fold_chunks(c, tree=_tree256):
    """(d, na, nb) from a segment's (m, 3) chunk sums, the coefficient pass's order: lane t adds chunk
    sums t, t + 256, ... from +0 and the 256 lane sums go through `tree`."""
    m = len(c)
    if m == 0:
        return 0.0, 0.0, 0.0
    rows = -(-m // LANES)
    cp = np.zeros((3, rows * LANES), np.float64)
    cp[:, :m] = c.T
    cp = cp.reshape(3, rows, LANES)
    lane = np.zeros((3, LANES), np.float64)
    with np.errstate(all="ignore"):
        for r in range(rows):
            lane = lane + cp[:, r, :]
        t = tree(lane)
    return float(t[0]), float(t[1]), float(t[2])


def segment_dots(a, b, dtype):
    """(d, na, nb) of one segment in the kernels' order: chunk_partials, then fold_chunks."""
    return fold_chunks(chunk_partials(a, b, dtype))


def coefficients(d, na, nb):
    """ca, cb in f64, every operation separate; the threshold is exact zero (a NaN norm is not > 0)."""
    d, na, nb = np.float64(d), np.float64(na), np.float64(nb)
    with np.errstate(all="ignore"):
        ca = np.float64(1.0) - np.float64(0.5) * (d / na) if na > 0 else np.float64(1.0)
        cb = np.float64(1.0) - np.float64(0.5) * (d / nb) if nb > 0 else np.float64(1.0)
    return ca, cb


def combine(a, b, ca, cb, dtype):
    W = np.float64 if dtype == F64 else np.float32
    with np.errstate(all="ignore"):
        caw, cbw = W(ca), W(cb)  # the one rounding f64 -> W
        x = to_work(a, dtype) * caw
        y = to_work(b, dtype) * cbw
        return round_store(x + y, dtype)


def segments(seg_counts):
    o = 0
    for c in seg_counts:
        yield o, o + c
        o += c


def pair_ref(a, b, seg_counts, dtype, dots=segment_dots):
    """The restatement: out = ca a + cb b per segment, storage bits."""
    assert len(a) == len(b) == sum(seg_counts)
    out = np.empty_like(a)
    for lo, hi in segments(seg_counts):
        ca, cb = coefficients(*dots(a[lo:hi], b[lo:hi], dtype))
        out[lo:hi] = combine(a[lo:hi], b[lo:hi], ca, cb, dtype)
    return out


def pair_intermediates(a, b, seg_counts, dtype):
    """What a pair call leaves in its workspace: the call's chunk sums, (nchunks, 3) f64 in global
    chunk order (an empty segment has none), and the per-segment (ca, cb), (nseg, 2) f64."""
    assert len(a) == len(b) == sum(seg_counts)
    parts, coef = [np.zeros((0, 3), np.float64)], np.empty((len(seg_counts), 2), np.float64)
    for s, (lo, hi) in enumerate(segments(seg_counts)):
        c = chunk_partials(a[lo:hi], b[lo:hi], dtype)
        parts.append(c)
        coef[s] = coefficients(*fold_chunks(c))
    return np.concatenate(parts), coef


def shape_counts(dtype):
    """The single-segment sizes at which the launch shape changes: 128 chunks (the last grid on
    contiguous eighths), 129 (the first striped grid, a one-element last chunk), 256 (the last
    one-row coefficient pass) and 257 (its second row; one whole vector and one element in the last chunk)."""
    K, E = chunk_elems(dtype), 16 // ES[dtype]
    return [128 * K, 128 * K + 1, 256 * K, 256 * K + E + 1]


def long_count(dtype):
    return shape_counts(dtype)[-1]


def seeded_pair(dtype, counts, salt=0, along=0.0):
    """The seeded normal operands (a, b) of a test case: the GPU tests and the CPU tests that vouch for
    them draw the same ones. along != 0: b = along a + a quarter of the independent draw."""
    rng = np.random.default_rng([20261020, dtype, salt, len(counts), sum(counts)])
    n = sum(counts)
    a, b = rand(dtype, n, rng), rand(dtype, n, rng)
    if along:
        W = to_work(a, dtype).dtype.type
        b = round_store(W(along) * to_work(a, dtype) + W(0.25) * to_work(b, dtype), dtype)
    return a, b


# Independent operands hide the dots' last bits from the coefficients: d / na is near 0 and
# 1 - 0.5 (d / na) rounds them away. With b near 2 a, d / na is near 2 and ca = 1 - 0.5 (d / na) is an
# exact difference that keeps every bit of the quotient, so a dot product off by an ulp shows in
# ca's f64 bits. The salts are those at which both wrong orders of test_adasum_cpu.py do show.
LONG_SALT = {F32: 4, F64: 0, F16: 1, BF16: 0}


def long_pair(dtype, count):
    """The operands of the single-segment launch-shape cases (shape_counts)."""
    return seeded_pair(dtype, [count], LONG_SALT[dtype], along=2.0)


def tree_ref(values, seg_counts, dtype, pair=pair_ref):
    """Every rank's result of the recursive-doubling tree over p = len(values) ranks (a power of
    two): at level k rank r pairs with r ^ 2^k, a = the value of the partner whose bit k is clear."""
    p = len(values)
    assert p >= 1 and p & (p - 1) == 0
    cur = [v.copy() for v in values]
    bit = 1
    while bit < p:
        cur = [pair(cur[r & ~bit], cur[r | bit], seg_counts, dtype) for r in range(p)]
        bit <<= 1
    return cur


# ---------------------------------------------------------------------------
# the order-free reference


def _two_prod(x, y):
    """p + e = x y exactly (Dekker / Veltkamp), barring overflow and underflow."""
    p = x * y
    cx, cy = 134217729.0 * x, 134217729.0 * y
    xh, yh = cx - (cx - x), cy - (cy - y)
    xl, yl = x - xh, y - yh
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return p, e


def exact_dot(x, y, dtype):
    """SUM x_i y_i, correctly rounded: f32 / f16 / bf16 products are exact in f64; F64 products are
    split into a rounded product and its exact error."""
    if dtype == F64:
        p, e = _two_prod(x, y)
        return math.fsum(np.concatenate([p, e]).tolist())
    return math.fsum((x * y).tolist())


def free_ref(a, b, seg_counts, dtype):
    """(ref, bound): ca a + cb b in f64 with math.fsum dots - no summation order - and the bound
    4 u_W (|ca a_i| + |cb b_i|) + u_S |ref_i| the definition allows around it (one coefficient
    rounding, two multiplies, one add, the store)."""
    ref = np.empty(len(a), np.float64)
    bound = np.empty(len(a), np.float64)
    for lo, hi in segments(seg_counts):
        x, y = to_f64(a[lo:hi], dtype), to_f64(b[lo:hi], dtype)
        ca, cb = coefficients(exact_dot(x, y, dtype), exact_dot(x, x, dtype), exact_dot(y, y, dtype))
        ref[lo:hi] = ca * x + cb * y
        bound[lo:hi] = 4 * U_W[dtype] * (np.abs(ca * x) + np.abs(cb * y)) + U_S[dtype] * np.abs(ref[lo:hi])
    return ref, bound


def within_bound(out, ref, bound, dtype):
    return bool(np.all(np.abs(to_f64(out, dtype) - ref) <= bound))
