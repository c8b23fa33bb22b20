"""The edge-value sets of tests/edge_values.py, checked on the CPU: the oracle agrees with the plain
numpy references on every set, the expected results reach every class of result the dtype has
(subnormal, +-0, +-inf from finite operands, NaN from inf - inf, NaN propagated, for the 16-bit
types inexact results and exact ties) at 16 or more elements, and every wrong model of
edge_values.py differs from the reference at 16 or more elements of the sets it applies to. These
are conditions on the inputs: what test_gpu_edge_values.py then finds on the device is decisive.

Which wrong model applies where (the others cannot differ, by the arithmetic):
- "narrow accumulator": 16-bit folds of 3 or more sources (with 2, the one fp32 add rounded once is
  the correctly rounded 16-bit add).
- "bf16 naive on NaN": the casts only. A bf16 operand widened to fp32 has zero low bits, a NaN that
  an fp32 add or multiply propagates keeps them, and the NaN it generates is 0x7fc00000 with either
  sign: adding 0x7fff to such a NaN never carries out of the payload, so sums, folds and scaled forms
  cannot tell the NaN branch from its absence. The casts' 0x7f800001 and 0x7fffffff can.
- "fp32 flush-to-zero mode" (every fp32 operation's subnormal inputs and results flushed): float32
  and bf16. The half sum is a half instruction and a half fold's fp32 values are multiples of 2^-24.
- "fused multiply-add", "post-scale before the last add": the scaled forms at (1/3, 0.7).
"""
import numpy as np
import pytest

import edge_values as ev
import scaled_util
from gpu_util import ALL_DTYPES, BF16, F16, F32, F64, I32, I64, same_bits

MIN = 16
FOLD_KS = [2, 3, 8, 16]


def count(mask):
    return int(np.count_nonzero(mask))


def result_classes(res, srcs, dtype, work=None):
    """{class: count} of a float result; `work` is the working-type value before the one rounding to
    a 16-bit storage type."""
    nan_in = np.zeros(res.shape, bool)
    fin_in = np.ones(res.shape, bool)
    inf_in = np.zeros(res.shape, bool)
    for s in srcs:
        nan_in |= ev.is_nan(s, dtype)
        fin_in &= ev.is_finite(s, dtype)
        inf_in |= ev.is_inf(s, dtype)
    b = ev.to_bits(res, dtype)
    U, e, m, emax, sign = ev._fields(dtype)
    inf = ev.is_inf(res, dtype)
    neg = (b & sign) != 0
    c = {"subnormal": count(ev.is_subnormal(res, dtype)),
         "+0": count(b == 0), "-0": count(b == sign),
         "+inf from finite": count(inf & ~neg & fin_in), "-inf from finite": count(inf & neg & fin_in),
         "NaN from inf - inf": count(ev.is_nan(res, dtype) & ~nan_in & inf_in),
         "NaN propagated": count(ev.is_nan(res, dtype) & nan_in)}
    if work is not None:
        c.update(rounding_classes(work, res, dtype))
    return c


def rounding_classes(work, res, dtype):
    """Inexact roundings and exact ties of float32 `work` rounded to 16-bit `res`."""
    work = np.ascontiguousarray(work, dtype=np.float32)
    fin = np.isfinite(work) & ev.is_finite(res, dtype)
    if dtype == BF16:
        low = work.view(np.uint32) & 0xffff
        return {"inexact": count(fin & (low != 0)), "tie": count(fin & (low == 0x8000))}
    with np.errstate(all="ignore"):
        x, r = work.astype(np.float64), res.astype(np.float64)
        other = np.nextafter(res, np.where(x > r, np.inf, -np.inf).astype(np.float16)).astype(np.float64)
        tie = fin & (x != r) & np.isfinite(other) & (np.abs(x - r) == np.abs(other - x))
    return {"inexact": count(fin & (x != r)), "tie": count(tie)}


def require(counts, what, skip=()):
    print(what, counts)
    low = {k: v for k, v in counts.items() if v < MIN and k not in skip}
    assert not low, "%s: fewer than %d elements of %s" % (what, MIN, low)


def separated(models, ref, dtype, what, names):
    got = {name: ev.differing(models[name], ref, dtype).size for name in names}
    print(what, got)
    low = {k: v for k, v in got.items() if v < MIN}
    assert not low, "%s: the inputs do not tell these wrong models from the reference: %s" % (what, low)


# ---------------------------------------------------------------------------
# generators

@pytest.mark.parametrize("dtype", ev.FLOAT_DTYPES)
def test_specials(dtype):
    sp = ev.specials(dtype)
    assert sp.size == 32 and np.unique(ev.to_bits(sp, dtype)).size == 32
    assert count(ev.is_nan(sp, dtype)) == 6 and count(ev.is_inf(sp, dtype)) == 2
    assert count(ev.is_subnormal(sp, dtype)) == 6
    w = ev.to_f64(sp, dtype)
    eps = 2.0 ** -ev.FMT[dtype][2]
    assert [w[6], w[7], w[8], w[9]] == [1 - eps / 2, 1.0, 1 + eps, 1.5] and w[16 + 7] == -1.0
    if dtype != BF16:
        fi = np.finfo(sp.dtype)
        assert w[10] == float(fi.max) and w[4] == float(fi.tiny) and w[3] == float(fi.tiny) - float(fi.smallest_subnormal)


def test_sets_are_seeded_and_sized():
    for dtype in ev.FLOAT_DTYPES:
        a, b = ev.pairs(dtype, ev.rng_for(1, dtype))
        assert a.size == b.size == 1024 + 4096 + 4096 + 1024 + 96 + 32 + 64
        assert np.array_equal(ev.to_bits(a, dtype), ev.to_bits(ev.pair_set(dtype)[0], dtype))
        assert all(s.size == ev.NTUPLE for s in ev.tuple_set(dtype)) and len(ev.tuple_set(dtype)) == 16
    for dtype in (I32, I64):
        a, b = ev.pair_set(dtype)
        assert a.size == b.size == 49 + 4096
    for wire in (F16, BF16):
        x = ev.cast_set(wire)
        assert x.dtype == np.float32 and x.size > 32 + 3 * 1900 + 68 + 128 + 4096
        for nan in (0x7f800001, 0x7fffffff, 0xff80ffff, 0x7fc00000):
            assert nan in x.view(np.uint32)


# ---------------------------------------------------------------------------
# the 2-input sum

@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_sum_oracle_equals_the_plain_reference(oracle, dtype):
    a, b = ev.pair_set(dtype)
    ref = ev.sum2_ref(a, b, dtype)
    assert same_bits(oracle.sum2(a, b, code=dtype), ref, dtype)
    if dtype in (I32, I64):
        info = np.iinfo(a.dtype)
        exact = a.astype(object) + b.astype(object)  # (python integers)
        wrapped = (exact - info.min) % (1 << info.bits) + info.min
        assert np.array_equal(ref.astype(object), wrapped) and count(exact != wrapped) >= MIN


@pytest.mark.parametrize("dtype", ev.FLOAT_DTYPES)
def test_sum_inputs_reach_every_class_and_tell_the_wrong_models_apart(dtype):
    a, b = ev.pair_set(dtype)
    ref = ev.sum2_ref(a, b, dtype)
    work = ev._fold_work([a, b], dtype, 1.0, 1.0) if dtype in (F16, BF16) else None
    require(result_classes(ref, [a, b], dtype, work), "sum, dtype %d" % dtype)
    models = ev.wrong_models([a, b], dtype)
    names = ["subnormal inputs flushed", "subnormal results flushed"]
    if dtype in (F32, BF16):  # (the half sum is a half instruction, a half fold never meets an fp32 subnormal)
        names.append("fp32 flush-to-zero mode")
    if dtype == BF16:
        names += ["bf16 truncation", "bf16 ties away"]
    separated(models, ref, dtype, "sum, dtype %d" % dtype, names)
    # x + (-x) = +0 and (-0) + (-0) = -0, both there
    bits_a, bits_b = ev.to_bits(a, dtype), ev.to_bits(b, dtype)
    sign = ev._fields(dtype)[4]
    cancel = (bits_a == bits_b ^ sign) & ev.is_finite(a, dtype) & ((bits_a & ~sign) != 0)
    assert count(cancel) >= 512 and (ev.to_bits(ref, dtype)[cancel] == 0).all()
    both_neg_zero = (bits_a == sign) & (bits_b == sign)
    assert count(both_neg_zero) >= 64 and (ev.to_bits(ref, dtype)[both_neg_zero] == sign).all()


# ---------------------------------------------------------------------------
# the fold

@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_fold_oracle_equals_the_plain_reference(oracle, dtype):
    srcs = ev.tuple_set(dtype)
    for k in (range(2, 17) if dtype in (F16, BF16) else (2, 3, 4, 5, 8, 16)):
        assert same_bits(oracle.fold(srcs[:k], code=dtype, wide_acc=True), ev.fold_ref(srcs[:k], dtype), dtype), k


@pytest.mark.parametrize("k", FOLD_KS)
@pytest.mark.parametrize("dtype", ev.FLOAT_DTYPES)
def test_fold_inputs_reach_every_class_and_tell_the_wrong_models_apart(dtype, k):
    srcs = ev.tuple_set(dtype)[:k]
    ref = ev.fold_ref(srcs, dtype)
    work = ev._fold_work(srcs, dtype, 1.0, 1.0) if dtype in (F16, BF16) else None
    what = "fold of %d, dtype %d" % (k, dtype)
    require(result_classes(ref, srcs, dtype, work), what)
    models = ev.wrong_models(srcs, dtype)
    names = ["subnormal inputs flushed", "subnormal results flushed"]
    if dtype in (F32, BF16):
        names.append("fp32 flush-to-zero mode")
    if dtype in (F16, BF16) and k > 2:
        names.append("narrow accumulator")
        # big + big - big: finite through the fp32 accumulator, inf through a 16-bit one
        blk = slice(2048, 2304)
        assert ev.is_finite(ref[blk], dtype).all() and ev.is_inf(models["narrow accumulator"][blk], dtype).all()
    if dtype == BF16:
        names += ["bf16 truncation", "bf16 ties away"]
    separated(models, ref, dtype, what, names)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_schedule_references_agree(oracle, dtype):
    """The ring's oracle against the closed form in numpy, on the 3-source edge set."""
    ins = list(ev.tuple_set(dtype)[:3])
    exp = scaled_util.ring_closed_form(ins, dtype, 1.0, 1.0)
    for out in oracle.ring(ins, code=dtype):
        assert same_bits(out, exp, dtype)


# ---------------------------------------------------------------------------
# the scaled forms

@pytest.mark.parametrize("what", ["pairs", "tuples of 3", "tuples of 8", "one source"])
@pytest.mark.parametrize("dtype", ev.FLOAT_DTYPES)
def test_scaled_inputs_reach_the_factor_cases(dtype, what):
    """What edge_values.FACTORS are for, counted on the sets the scaled kernels get: a product that
    underflows to a subnormal of the working type and comes back, a product and a post-scale that
    overflow, 0 x inf, a negative factor against +-0; and (1/3, 0.7) tells a fused multiply-add and a
    misplaced post-scale from the definition. Not reachable, and not required: half's products with
    1e-30 and 1e30 (all normal floats)."""
    W = scaled_util.work_type(dtype)
    wd = F64 if dtype == F64 else F32
    srcs = {"pairs": list(ev.pair_set(dtype)), "tuples of 3": list(ev.tuple_set(dtype)[:3]),
            "tuples of 8": list(ev.tuple_set(dtype)[:8]),
            "one source": [ev.pair_set(dtype)[0]]}[what]
    sign = ev._fields(dtype)[4]
    fin = np.all([ev.is_finite(s, dtype) for s in srcs], axis=0)
    nan_in = np.any([ev.is_nan(s, dtype) for s in srcs], axis=0)
    if len(srcs) > 1:
        ref = ev.fold_ref(srcs, dtype, 1.0 / 3.0, 0.7)
        separated(ev.wrong_models(srcs, dtype, 1.0 / 3.0, 0.7), ref, dtype, "scaled %s, dtype %d" % (what, dtype),
                  (["fused multiply-add"] if dtype != F64 else []) + ["post-scale before the last add"])
    got = {}
    with np.errstate(all="ignore"):
        work = [scaled_util.to_work(s, dtype) for s in srcs]
        res = ev.fold_ref(srcs, dtype, 1e-30, 1e30)
        sub = np.any([ev.is_subnormal(w * W(1e-30), wd) for w in work], axis=0)
        got["subnormal product, nonzero result"] = count(sub & fin & ((ev.to_bits(res, dtype) & ~sign) != 0))
        got["overflowing product"] = count(np.any([np.isinf(w * W(1e30)) for w in work], axis=0) & fin)
        acc = ev._fold_work(srcs, dtype, 1e-30, 1.0)
        got["overflowing post-scale"] = count(np.isfinite(acc) & np.isinf(acc * W(1e30)) & fin)
    got["0 x inf"] = count(ev.is_nan(ev.fold_ref(srcs, dtype, 0.0, 1.0), dtype) & ~nan_in)
    plain = ev.to_bits(ev.fold_ref(srcs, dtype, 1.0, 1.0), dtype)
    flipped = ev.to_bits(ev.fold_ref(srcs, dtype, -1.0, 1.0), dtype)
    got["+0 to -0"] = count((plain == 0) & (flipped == sign))
    got["-0 to +0"] = count((plain == sign) & (flipped == 0))
    skip = set()
    if dtype == F16:
        skip |= {"subnormal product, nonzero result", "overflowing product", "overflowing post-scale"}
    if what != "pairs":
        skip.add("overflowing post-scale")
    require(got, "scaled %s, dtype %d" % (what, dtype), skip)


# ---------------------------------------------------------------------------
# the casts

@pytest.mark.parametrize("wire", [F16, BF16])
def test_cast_oracle_equals_the_plain_reference(oracle, wire):
    x = ev.cast_set(wire)
    h = ev.narrow(x, wire)
    assert same_bits(oracle.cast_to16(x, wire).view(h.dtype), h, wire)
    assert ev.same_cast(oracle.cast_from16(ev.to_bits(h, wire), wire), ev.widen(h, wire))
    every = np.arange(65536, dtype=np.uint16)  # widening is exact: every wire value, and back
    wide = oracle.cast_from16(every, wire)
    assert ev.same_cast(wide, ev.widen(ev.from_bits(every, wire), wire))
    assert same_bits(ev.narrow(wide, wire), ev.from_bits(every, wire), wire)
    # the allreduce of f32 inputs over a 16-bit wire: cast, fold in fp32, one rounding, cast back
    ins = [x, x[::-1].copy(), np.roll(x, 1)]
    exp = ev.widen(ev.fold_ref([ev.narrow(v, wire) for v in ins], wire), wire)
    assert ev.same_cast(oracle.compressed_fold(ins, wire), exp)


def cast_differing(x, y):
    return count(~((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))))


@pytest.mark.parametrize("wire", [F16, BF16])
def test_cast_inputs_reach_every_class_and_tell_the_wrong_models_apart(wire):
    x = ev.cast_set(wire)
    h = ev.narrow(x, wire)
    ref = ev.widen(h, wire)
    fin, nan = np.isfinite(x), np.isnan(x)
    hb, sign = ev.to_bits(h, wire), ev._fields(wire)[4]
    c = {"subnormal": count(ev.is_subnormal(h, wire)),
         "+0 from nonzero": count((hb == 0) & (x != 0)), "-0 from nonzero": count((hb == sign) & (x != 0)),
         "+0 kept": count((hb == 0) & (x.view(np.uint32) == 0)), "-0 kept": count((hb == sign) & (x.view(np.uint32) == 1 << 31)),
         "+inf from finite": count(ev.is_inf(h, wire) & fin & (hb & sign == 0)),
         "-inf from finite": count(ev.is_inf(h, wire) & fin & (hb & sign != 0)),
         "NaN propagated": count(ev.is_nan(h, wire) & nan)}
    c.update(rounding_classes(x, h, wire))
    assert count(nan) == c["NaN propagated"]
    require(c, "cast to %d" % wire, skip=("+0 kept", "-0 kept"))
    assert c["+0 kept"] >= 1 and c["-0 kept"] >= 1
    # the tie at the overflow threshold (to inf) and its neighbour below (to the largest finite value);
    # half the smallest subnormal (to zero: the even one) and its neighbour above (to the subnormal)
    big, tiny = ev.widen(ev.specials(wire)[10:11], wire).astype(np.float64)[0], ev.widen(ev.specials(wire)[1:2], wire)[0]
    top = np.float32(big + (big - float(ev.widen(ev.from_bits(ev.special_bits(wire)[10:11] - 1, wire), wire)[0])) / 2)
    for v, want in ((top, np.inf), (np.nextafter(top, np.float32(0)), np.float32(big)), (tiny / 2, 0.0),
                    (np.nextafter(np.float32(tiny / 2), np.float32(1)), tiny)):
        for sgn in (1, -1):
            i = np.nonzero(x == np.float32(sgn * v))[0]
            assert i.size >= 1 and (ref[i] == np.float32(sgn * want)).all(), (v, want)
    models = ev.cast_wrong_models(x, wire)
    got = {name: cast_differing(ref, m) for name, m in models.items()}
    print("cast to %d" % wire, got)
    low = {k: v for k, v in got.items() if v < MIN}
    assert not low, low
    # the NaNs that name a wrong narrowing: truncation turns 0x7f800001 into inf, add-and-shift 0x7fffffff into -0
    for pattern, model in ((0x7f800001, "bf16 truncation"), (0xff80ffff, "bf16 truncation"), (0x7fffffff, "bf16 naive on NaN")):
        i = np.nonzero(x.view(np.uint32) == pattern)[0]
        assert i.size >= 1 and np.isnan(ref[i]).all()
        if wire == BF16:
            assert not np.isnan(models[model][i]).any()
