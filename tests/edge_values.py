"""Edge-value inputs for the sum, fold, scale and cast kernels, their plain references, and numpy
restatements of plausible kernel errors ("wrong models"). numpy only, seeded; a helper module for
test_edge_values_cpu.py (which proves that the inputs reach every result class and tell every
wrong model from the reference) and test_gpu_edge_values.py (which runs them on the device).

Arrays travel in the storage types of gpu_util.NPDT: float16 / float32 / float64 arrays, uint16
bit patterns for BF16. The references are independent of oracle/: numpy's own IEEE arithmetic, and
scaled_util's definition (fp32 working type for f16 / bf16, one rounding to the storage type).
"""
import functools

import numpy as np

import scaled_util
from gpu_util import BF16, F16, F32, F64, I32, I64, NPDT, bits

FLOAT_DTYPES = [F32, F64, F16, BF16]
# (unsigned type of the bits, exponent bits, mantissa bits)
FMT = {F32: (np.uint32, 8, 23), F64: (np.uint64, 11, 52), F16: (np.uint16, 5, 10), BF16: (np.uint16, 8, 7)}
FACTORS = [(1.0 / 3.0, 0.7), (1e-30, 1e30), (1e30, 1e-30), (0.0, 1.0), (-1.0, 1.0), (1.0, -0.5)]
NTUPLE = 8192


def rng_for(*key):
    return np.random.default_rng([20261020] + [int(k) for k in key])


def from_bits(u, dtype):
    """Bit patterns (any integer array) -> the dtype's storage array."""
    U = FMT[dtype][0]
    u = np.ascontiguousarray(u).astype(U)
    return u if dtype == BF16 else u.view(NPDT[dtype])


def to_bits(a, dtype):
    return np.ascontiguousarray(a).view(FMT[dtype][0])


def _fields(dtype):
    U, e, m = FMT[dtype]
    return U, e, m, (1 << e) - 1, U(1) << U(e + m)  # ..., the all-ones exponent field, the sign bit


# ---------------------------------------------------------------------------
# classes of a value

def is_nan(a, dtype):
    U, e, m, emax, sign = _fields(dtype)
    b = to_bits(a, dtype)
    return (b & ~sign) > (U(emax) << U(m))


def is_inf(a, dtype):
    U, e, m, emax, sign = _fields(dtype)
    return (to_bits(a, dtype) & ~sign) == (U(emax) << U(m))


def is_subnormal(a, dtype):
    U, e, m, emax, sign = _fields(dtype)
    b = to_bits(a, dtype) & ~sign
    return (b != 0) & (b < (U(1) << U(m)))


def is_finite(a, dtype):
    return ~(is_nan(a, dtype) | is_inf(a, dtype))


def same_cast(got, exp):
    """The rule for cast outputs (float32 arrays): NaN where NaN, the same bits elsewhere."""
    gn, en = np.isnan(got), np.isnan(exp)
    return np.array_equal(gn, en) and np.array_equal(bits(got)[~gn], bits(exp)[~en])


def differing(x, y, dtype):
    """Indices at which two results differ under gpu_util.same_bits's rule (any NaN = any NaN)."""
    if dtype in (I32, I64):
        return np.nonzero(x != y)[0]
    xn, yn = is_nan(x, dtype), is_nan(y, dtype)
    return np.nonzero((xn != yn) | (~xn & ~yn & (to_bits(x, dtype) != to_bits(y, dtype))))[0]


# ---------------------------------------------------------------------------
# inputs

def special_bits(dtype):
    U, e, m, emax, sign = _fields(dtype)
    one, inf = ((1 << (e - 1)) - 1) << m, emax << m
    pos = [0, 1, 2, (1 << m) - 1,                     # 0; the subnormals 1, 2 and largest
           1 << m, (1 << m) + 1,                      # smallest normal and its successor
           one - 1, one, one + 1, one | 1 << (m - 1),  # 1 - ulp, 1, 1 + ulp, 1.5
           inf - 1, (emax - 1) << m,                  # largest finite, largest power of two
           inf, inf | 1 << (m - 1), inf | 1, inf | ((1 << m) - 1)]  # inf; quiet, signalling (payload 1), all-ones NaN
    return np.array(pos + [p | int(sign) for p in pos], dtype=U)


def specials(dtype):
    """The 32 special values of a float dtype (16, with both signs)."""
    return from_bits(special_bits(dtype), dtype)


def int_specials(dtype):
    i = np.iinfo(NPDT[dtype])
    return np.array([i.min, i.min + 1, -1, 0, 1, i.max - 1, i.max], dtype=NPDT[dtype])


def random_bits(dtype, n, rng):
    U = FMT[dtype][0]
    return rng.integers(0, np.iinfo(U).max, size=n, dtype=U, endpoint=True)


def near_exponent_bits(abits, dtype, rng):
    """Random sign and mantissa, the exponent field within +-(mantissa bits + 3) of abits' (kept
    finite): operands that meet in one add - ties, cancellation, one-ulp carries."""
    U, e, m, emax, sign = _fields(dtype)
    ea = ((abits >> U(m)) & U(emax)).astype(np.int64)
    eb = np.clip(ea + rng.integers(-(m + 3), m + 3, size=abits.size, endpoint=True), 0, emax - 1).astype(U)
    r = random_bits(dtype, abits.size, rng)
    return (r & (sign | U((1 << m) - 1))) | (eb << U(m))


def low_exponent_bits(dtype, n, rng):
    """Random finite values, half of them with an exponent field of at most mantissa bits + 3: where
    a cancellation lands among the subnormals."""
    U, e, m, emax, sign = _fields(dtype)
    r = random_bits(dtype, n, rng)
    ex = rng.integers(0, emax - 1, size=n, endpoint=True)
    ex[::2] = rng.integers(0, m + 3, size=(n + 1) // 2, endpoint=True)
    return (r & (sign | U((1 << m) - 1))) | (ex.astype(U) << U(m))


def pairs(dtype, rng):
    """(a, b) for the 2-input sum: specials x specials (1024), uniformly random bit patterns (4096),
    near-exponent pairs (4096), exact and near cancellations (512 each, half of them low enough to
    land among the subnormals), (-0) + (-0) (64), (+0) + (+0) (32), inf - inf (32), finite + finite =
    +-inf (64).
    Integers: the extremes squared and 4096 random pairs."""
    if dtype in (I32, I64):
        sp = int_specials(dtype)
        info = np.iinfo(NPDT[dtype])
        r = [rng.integers(info.min, info.max, size=4096, dtype=NPDT[dtype], endpoint=True) for _ in range(2)]
        return np.concatenate([np.repeat(sp, len(sp)), r[0]]), np.concatenate([np.tile(sp, len(sp)), r[1]])
    U, e, m, emax, sign = _fields(dtype)
    sp = special_bits(dtype)
    a = [np.repeat(sp, len(sp))]
    b = [np.tile(sp, len(sp))]
    a.append(random_bits(dtype, 4096, rng))
    b.append(random_bits(dtype, 4096, rng))
    a.append(random_bits(dtype, 4096, rng))
    b.append(near_exponent_bits(a[-1], dtype, rng))
    c = low_exponent_bits(dtype, 512, rng)
    a.append(c)
    b.append(c ^ sign)  # b = -a
    c = low_exponent_bits(dtype, 512, rng)
    nb = c ^ sign
    nb[1::2] += U(1)    # and one ulp beside it
    a.append(c)
    b.append(nb)
    z = np.concatenate([np.full(64, sign, dtype=U), np.zeros(32, dtype=U)])  # (-0) + (-0), and (+0) + (+0)
    a.append(z)
    b.append(z.copy())
    inf = np.where(np.arange(32) % 2 == 1, sign, U(0)).astype(U) | (U(emax) << U(m))  # inf - inf, either order
    a.append(inf)
    b.append(inf ^ sign)
    # finite + finite = +-inf: both operands in the top binade, the sign alternating
    top = [(random_bits(dtype, 64, rng) & U((1 << m) - 1)) | U((emax - 1) << m) for _ in range(2)]
    s = np.where(np.arange(64) % 2 == 1, sign, U(0)).astype(U)
    a.append(top[0] | s)
    b.append(top[1] | s)
    return from_bits(np.concatenate(a), dtype), from_bits(np.concatenate(b), dtype)


NSTRUCT = 576  # the fold's structured elements (structured_bits)


def structured_bits(dtype, rng):
    """Sources 0, 1, 2 and (the last array) every further source of the fold's structured elements:
    the further sources are -0 (+0 where all are +0), which changes no sum (x + -0 = x, +0 + -0 =
    +0), so the classes survive any number of sources:
    128 cancellations and near cancellations low enough for subnormal results; 64 of all -0; 64 of
    all +0; 64 of inf - inf; 64 of subnormal + subnormal; 128 exact ties (source 1 is half an ulp of
    source 0); 32 of finite + finite = +-inf; and, for the 16-bit types, 32 triples at which one ulp of the fp32 working value
    decides the rounding under the factors (1/3, 0.7): picked from 2^20 random near-exponent
    triples as those where a fused multiply-add changes the result (random triples almost never are:
    the rounding to 16 bits hides an fp32 ulp)."""
    U, e, m, emax, sign = _fields(dtype)
    neg0 = lambda n: np.full(n, sign, dtype=U)
    s = [[], [], [], []]

    def add(x0, x1, x2=None, rest=None):
        s[0].append(x0), s[1].append(x1), s[2].append(neg0(x0.size) if x2 is None else x2)
        s[3].append(neg0(x0.size) if rest is None else rest)

    c = low_exponent_bits(dtype, 128, rng)
    c[::2] = (c[::2] & ~(U(emax) << U(m))) | (rng.integers(0, m + 3, size=64, endpoint=True).astype(U) << U(m))
    nb = c ^ sign
    nb[1::2] += U(1)
    add(c, nb)
    add(neg0(64), neg0(64))
    add(*[np.zeros(64, dtype=U) for _ in range(4)])
    inf = np.where(np.arange(64) % 2 == 1, sign, U(0)).astype(U) | (U(emax) << U(m))
    add(inf, inf ^ sign)
    add(*[random_bits(dtype, 64, rng) & (sign | U((1 << m) - 1)) for _ in range(2)])
    e0 = rng.integers(m + 2, emax - 2, size=128, endpoint=True).astype(U)
    x0 = (random_bits(dtype, 128, rng) & (sign | U((1 << m) - 1))) | (e0 << U(m))
    add(x0, (random_bits(dtype, 128, rng) & sign) | ((e0 - U(m + 1)) << U(m)))
    top = [(random_bits(dtype, 32, rng) & U((1 << m) - 1)) | U((emax - 1) << m) for _ in range(2)]
    sg = np.where(np.arange(32) % 2 == 1, sign, U(0)).astype(U)
    add(top[0] | sg, top[1] | sg)
    if dtype in (F16, BF16):
        t0 = random_bits(dtype, 1 << 20, rng)
        t = [t0, near_exponent_bits(t0, dtype, rng), near_exponent_bits(t0, dtype, rng)]
        st = [from_bits(x, dtype) for x in t]
        ref = fold_ref(st, dtype, *FACTORS[0])
        fused = scaled_util.from_work(_fold_work(st, dtype, *FACTORS[0], fused=True), dtype)
        pick = differing(ref, fused, dtype)[:32]
        assert pick.size == 32
        add(*[x[pick] for x in t])
    else:
        add(*[random_bits(dtype, 32, rng) for _ in range(3)])
    out = [np.concatenate(x) for x in s]
    assert out[0].size == NSTRUCT
    return out


def tuples(dtype, k, rng):
    """k sources of NTUPLE elements for the fold: 2048 drawn from the specials; 256 of
    big, big, -big, 0, ... (bf16: big, u, -u with u half an ulp of big; every other element negated),
    finite through an fp32 accumulator and inf through a 16-bit one;
    NSTRUCT structured elements (structured_bits); the rest random bits, sources 1.. near-exponent to
    source 0 at every other element. Integers: the extremes and random values."""
    n = NTUPLE
    if dtype in (I32, I64):
        info = np.iinfo(NPDT[dtype])
        sp = int_specials(dtype)
        out = []
        for _ in range(k):
            x = rng.integers(info.min, info.max, size=n, dtype=NPDT[dtype], endpoint=True)
            x[:2048] = sp[rng.integers(0, len(sp), size=2048)]
            out.append(x)
        return out
    U, e, m, emax, sign = _fields(dtype)
    sp = special_bits(dtype)
    big = U((emax << m) - 1)
    # bf16 has fp32's exponent range, so big + big is inf in the fp32 accumulator too: there the second
    # and third sources are +-half an ulp of big (a tie that a bf16 accumulator rounds up to inf)
    second = U((emax - 1 - (m + 1)) << m) if dtype == BF16 else big
    flip = np.zeros(256, dtype=U)
    flip[1::2] = sign
    struct = structured_bits(dtype, rng)
    out = []
    for j in range(k):
        x = random_bits(dtype, n, rng)
        if j > 0:
            near = near_exponent_bits(out[0], dtype, rng)
            x[::2] = near[::2]
        x[:2048] = sp[rng.integers(0, len(sp), size=2048)]
        x[2048:2304] = (np.full(256, big if j == 0 else second if j == 1 else second | sign if j == 2 else 0, dtype=U)
                        ^ (flip if j < 3 else U(0)))
        x[2304:2304 + NSTRUCT] = struct[min(j, 3)]
        out.append(x)
    return [from_bits(x, dtype) for x in out]


def f32_cast_inputs(wire, rng):
    """float32 inputs of the casts to `wire` (F16 or BF16): the f32 specials; around every wire
    special and 2048 random wire values w the value halfway between w and its successor and its
    two f32 neighbours (the tie at the overflow threshold and the one at half the smallest
    subnormal among them); 0x7f800001, 0x7fffffff, 0xff80ffff, 0x7fc00000 and 64 more NaNs of the two
    kinds a wrong narrowing loses; 64 finite values that underflow to +-0 and 64 that overflow to
    +-inf; random bit patterns."""
    w = np.concatenate([special_bits(wire), random_bits(wire, 2048, rng)])
    U, e, m, emax, sign = _fields(wire)
    w = w[(w & ~sign) < (U(emax) << U(m))]  # finite: its successor in magnitude exists (inf, for the largest)
    lo = widen(from_bits(w, wire), wire).astype(np.float64)
    hi = widen(from_bits(w + U(1), wire), wire).astype(np.float64)
    big = np.float64(2.0) ** (1 << (e - 1))  # the successor of the largest finite value, were there one
    hi = np.where(np.isinf(hi), np.copysign(big, lo), hi)
    mid = ((lo + hi) / 2).astype(np.float32)  # exact: the wire type's precision plus one bit
    assert np.array_equal(mid.astype(np.float64), (lo + hi) / 2)
    mb = mid.view(np.uint32)
    r = random_bits(F32, 64, rng)
    nans = np.concatenate([np.array([0x7f800001, 0x7fffffff, 0xff80ffff, 0x7fc00000], dtype=np.uint32),
                           (r[:32] & np.uint32(0x8000ffff)) | np.uint32(0x7f800001),   # payload in the dropped bits only
                           r[32:] | np.uint32(0x7fff8000)])                           # rounding up would carry out of it
    # finite values that every correct narrowing turns into +-0 (at most half the smallest wire
    # subnormal) and into +-inf (from the overflow tie up), 32 of each sign
    half_tiny = int(np.float32(widen(from_bits([1], wire), wire)[0] / 2).view(np.uint32))
    tie = int(np.float32((widen(from_bits([(emax << m) - 1], wire), wire).astype(np.float64)[0] + big) / 2).view(np.uint32))
    sgn = np.where(np.arange(64) % 2 == 1, np.uint32(1 << 31), np.uint32(0)).astype(np.uint32)
    under = rng.integers(1, half_tiny, size=64, dtype=np.uint32, endpoint=True) | sgn
    over = rng.integers(tie, 0x7f7fffff, size=64, dtype=np.uint32, endpoint=True) | sgn
    parts = [special_bits(F32), mb, mb + np.uint32(1), mb - np.uint32(1), nans, under, over, random_bits(F32, 4096, rng)]
    return np.concatenate(parts).view(np.float32)


# ---------------------------------------------------------------------------
# plain references

def to_f64(a, dtype):
    with np.errstate(invalid="ignore"):  # (signalling NaNs)
        return scaled_util.to_work(a, dtype).astype(np.float64)


def sum2_ref(a, b, dtype):
    with np.errstate(all="ignore"):
        if dtype in (F32, F64, I32, I64):
            return a + b  # (integers: numpy's wrapping add)
        if dtype == F16:  # exact in float64, so one rounding: the correctly rounded half add
            return (a.astype(np.float64) + b.astype(np.float64)).astype(np.float16)
        return scaled_util.bf16_round(scaled_util.to_work(a, BF16) + scaled_util.to_work(b, BF16))


def fold_ref(srcs, dtype, pre=1.0, post=1.0):
    """The fold, plain (factors 1) or scaled: scaled_util's definition; integers wrap."""
    if dtype in (I32, I64):
        acc = srcs[0].copy()
        for s in srcs[1:]:
            acc = acc + s
        return acc
    return scaled_util.scaled_sum(list(srcs), [True] * len(srcs), pre, post, dtype)


def narrow(x, wire):
    """float32 -> wire storage (round to nearest even)."""
    with np.errstate(all="ignore"):
        return x.astype(np.float16) if wire == F16 else scaled_util.bf16_round(x)


def widen(h, wire):
    """wire storage -> float32, exact."""
    return h.astype(np.float32) if wire == F16 else scaled_util.to_work(h, BF16)


def cast_ref(x, wire):
    return widen(narrow(x, wire), wire)


# ---------------------------------------------------------------------------
# wrong models: what a kernel with one plausible error would compute

def flush(a, dtype):
    """Subnormals replaced by zeros of their sign."""
    U, e, m, emax, sign = _fields(dtype)
    b = to_bits(a, dtype)
    return from_bits(np.where(is_subnormal(a, dtype), b & sign, b), dtype)


def bf16_truncate(w):
    return (np.ascontiguousarray(w, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_ties_away(w):
    x = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (x & 0x7fffffff) > 0x7f800000
    return np.where(nan, (x >> 16) | 0x40, (x + 0x8000) >> 16).astype(np.uint16)


def bf16_naive_nan(w):
    x = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((x + 0x7fff + ((x >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


BF16_ROUNDINGS = {"bf16 truncation": bf16_truncate, "bf16 ties away": bf16_ties_away, "bf16 naive on NaN": bf16_naive_nan}


def _fold_work(srcs, dtype, pre, post, fused=False, early_post=False):
    """scaled_sum's arithmetic in the working type, not yet rounded to the storage type; `fused`
    contracts the first multiply into the first add (fma(s1, f, s0 * f), float32 working type only),
    `early_post` multiplies the partial sum by post before the last add instead of after it."""
    W = scaled_util.work_type(dtype)
    pre_w, post_w = W(pre), W(post)
    with np.errstate(all="ignore"):
        acc = scaled_util.to_work(srcs[0], dtype) * pre_w
        for j, s in enumerate(srcs[1:], 1):
            if early_post and j == len(srcs) - 1:
                acc = acc * post_w
            if fused and j == 1:
                assert W is np.float32
                acc = (scaled_util.to_work(s, dtype).astype(np.float64) * np.float64(pre_w)
                       + acc.astype(np.float64)).astype(np.float32)
            else:
                acc = acc + scaled_util.to_work(s, dtype) * pre_w
        return acc if early_post else acc * post_w


def ftz_fold(srcs, dtype, pre, post):
    """The fold with fp32 denormals flushed to zero at every operation's inputs and result (what the
    hardware's fp32 flush mode does; the 16-bit conversions keep their subnormals)."""
    fz = lambda x: flush(x, F32)
    pre_w, post_w = np.float32(pre), np.float32(post)
    with np.errstate(all="ignore"):
        acc = fz(fz(scaled_util.to_work(srcs[0], dtype)) * pre_w)
        for s in srcs[1:]:
            acc = fz(acc + fz(fz(scaled_util.to_work(s, dtype)) * pre_w))
        return scaled_util.from_work(fz(acc * post_w), dtype)


def narrow_fold(srcs, dtype):
    """Rounding to the storage type at every step (a 16-bit accumulator)."""
    acc = srcs[0]
    for s in srcs[1:]:
        acc = sum2_ref(acc, s, dtype)
    return acc


def wrong_models(srcs, dtype, pre=1.0, post=1.0):
    """{name: result} of every wrong model that applies to the sum or fold of `srcs` (float dtypes)
    with these factors. test_edge_values_cpu.py asserts which of them the inputs tell from the
    reference; the GPU test names the one a wrong device output equals."""
    ref = fold_ref(srcs, dtype, pre, post)
    out = {"subnormal inputs flushed": fold_ref([flush(s, dtype) for s in srcs], dtype, pre, post),
           "subnormal results flushed": flush(ref, dtype)}
    if dtype != F64:
        out["fp32 flush-to-zero mode"] = ftz_fold(srcs, dtype, pre, post)
    if dtype in (F16, BF16) and len(srcs) > 2 and pre == 1.0 and post == 1.0:
        out["narrow accumulator"] = narrow_fold(srcs, dtype)
    if dtype == BF16:
        w = _fold_work(srcs, dtype, pre, post)
        for name, fn in BF16_ROUNDINGS.items():
            out[name] = fn(w)
    if (pre != 1.0 or post != 1.0) and len(srcs) > 1:
        if dtype != F64:
            out["fused multiply-add"] = scaled_util.from_work(_fold_work(srcs, dtype, pre, post, fused=True), dtype)
        out["post-scale before the last add"] = scaled_util.from_work(
            _fold_work(srcs, dtype, pre, post, early_post=True), dtype)
    return out


def cast_wrong_models(x, wire):
    """{name: widened result} of the wrong narrowings of float32 `x` to `wire`."""
    out = {"subnormal results flushed": widen(flush(narrow(x, wire), wire), wire)}
    if wire == BF16:
        out["subnormal inputs flushed"] = cast_ref(flush(x, F32), wire)
        for name, fn in BF16_ROUNDINGS.items():
            out[name] = widen(fn(x), wire)
    return out


def matching_model(got, models, dtype):
    """The names of the wrong models `got` equals exactly (for a failure report)."""
    return [name for name, m in models.items() if differing(got, m, dtype).size == 0]


# ---------------------------------------------------------------------------
# the sets, built once and shared read-only

def _frozen(arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


@functools.lru_cache(maxsize=None)
def pair_set(dtype):
    return tuple(_frozen(list(pairs(dtype, rng_for(1, dtype)))))


@functools.lru_cache(maxsize=None)
def tuple_set(dtype):
    """16 sources; a fold of k takes the first k."""
    return tuple(_frozen(tuples(dtype, 16, rng_for(2, dtype))))


@functools.lru_cache(maxsize=None)
def cast_set(wire):
    return _frozen([f32_cast_inputs(wire, rng_for(3, wire))])[0]
