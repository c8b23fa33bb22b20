"""The numpy definition of the MAX / MIN reductions (DESIGN.md §MAX and MIN) and the inputs their tests share.

result[i] = the largest (smallest) of the sources' element i, in the storage type, exact. Integers
compare signed. Floats follow IEEE 754-2019 maximum / minimum: a NaN in any source gives a NaN (the
payload is not part of the contract), -0 < +0, subnormals are kept, the infinities order as values.
For the floats the reference never does floating-point arithmetic: the bits are mapped to a key
whose unsigned order is the total order of the values (sign set -> ~u, else u | sign bit), the keys
are compared, and the winner is mapped back. The result does not depend on the operands' order, so
one reference serves every schedule.
"""
import numpy as np

import edge_values as ev
from gpu_util import ALL_DTYPES, BF16, F16, F32, F64, I32, I64, NPDT, rand, with_specials  # noqa: F401

MAX, MIN = 1, 2  # TIPS_OP_MAX, TIPS_OP_MIN
OPS = [MAX, MIN]
INT_DTYPES = [I32, I64]


def _key(u, sign):
    return np.where((u & sign) != 0, ~u, u | sign)


def _unkey(k, sign):
    return np.where((k & sign) != 0, k & ~sign, ~k)


def ref(srcs, dtype, op):
    """MAX or MIN over the sources (arrays of the dtype's storage type), elementwise."""
    assert op in (MAX, MIN) and len(srcs) >= 1
    pick = np.maximum if op == MAX else np.minimum
    if dtype in INT_DTYPES:
        out = np.array(srcs[0], dtype=NPDT[dtype])
        for s in srcs[1:]:
            out = pick(out, s)
        return out
    U, sign = ev.FMT[dtype][0], ev._fields(dtype)[4]
    key = _key(ev.to_bits(srcs[0], dtype), sign)
    nan = ev.is_nan(srcs[0], dtype)
    for s in srcs[1:]:
        key = pick(key, _key(ev.to_bits(s, dtype), sign))
        nan = nan | ev.is_nan(s, dtype)
    out = _unkey(key, sign).astype(U)
    out[nan] = ev.special_bits(dtype)[13]  # the quiet NaN
    return ev.from_bits(out, dtype)


def same(got, exp, dtype):
    """The bits where exp is not a NaN, NaN-ness where it is; on a difference, where and what."""
    got, exp = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(exp).reshape(-1)
    if got.shape != exp.shape:
        print("shapes differ: %s, %s" % (got.shape, exp.shape))
        return False
    if dtype in INT_DTYPES:
        bad = got != exp
    else:
        gn, en = ev.is_nan(got, dtype), ev.is_nan(exp, dtype)
        bad = (gn != en) | (~en & (ev.to_bits(got, dtype) != ev.to_bits(exp, dtype)))
    idx = np.nonzero(bad)[0]
    if idx.size == 0:
        return True
    u = "u%d" % got.itemsize
    print("%d of %d elements differ; first at %s: got %s, expected %s" % (
        idx.size, got.size, idx[:6].tolist(), [hex(int(v)) for v in got.view(u)[idx[:6]]],
        [hex(int(v)) for v in exp.view(u)[idx[:6]]]))
    return False


def specials(dtype):
    return ev.int_specials(dtype) if dtype in INT_DTYPES else ev.specials(dtype)


def crossed_specials(dtype):
    """(a, b): every special value against every special value, in both operand positions."""
    sp = specials(dtype)
    return np.repeat(sp, sp.size), np.tile(sp, sp.size)


def pair_inputs(dtype, n, seed):
    """Two operands of n elements: random values, gpu_util's specials in the first, and the crossed
    specials block at the start and - so that it lands in the scalar tail - at the end."""
    rng = np.random.default_rng(seed)
    a, b = with_specials(rand(dtype, n, rng), dtype), rand(dtype, n, rng)
    ca, cb = crossed_specials(dtype)
    k = min(n, ca.size)
    a[:k], b[:k] = ca[:k], cb[:k]
    a[n - k:], b[n - k:] = ca[ca.size - k:], cb[cb.size - k:]
    return a, b


def planted(srcs, dtype):
    """Copies of the sources with, for each source position j, a NaN in source j alone at element
    3 + 2 j and a -0 in source j against +0 in every other source at element 4 + 2 j (floats; elements
    past the end are skipped). Integers: the type's minimum and maximum, likewise."""
    out = [np.array(s) for s in srcs]
    n = out[0].size
    if dtype in INT_DTYPES:
        lo, hi = np.iinfo(NPDT[dtype]).min, np.iinfo(NPDT[dtype]).max
        for j in range(len(out)):
            if 3 + 2 * j < n:
                out[j][3 + 2 * j] = lo
            if 4 + 2 * j < n:
                out[j][4 + 2 * j] = hi
        return out
    sb = ev.special_bits(dtype)
    qnan, pzero, nzero = (ev.from_bits(sb[i:i + 1], dtype)[0] for i in (13, 0, 16))
    for j in range(len(out)):
        if 3 + 2 * j < n:
            out[j][3 + 2 * j] = qnan
        if 4 + 2 * j < n:
            for k in range(len(out)):
                out[k][4 + 2 * j] = nzero if k == j else pzero
    return out


def rank_inputs(dtype, n, seed, p):
    """The p ranks' inputs of an allreduce case: rand(dtype, n, default_rng(seed + r)) with the
    specials block at a rank-dependent offset (rotated by r as well), so that NaN, the zeros and the
    other specials of one element arrive from different ranks."""
    sp = specials(dtype)
    ins = []
    for r in range(p):
        x = rand(dtype, n, np.random.default_rng(seed + r))
        blk = np.roll(sp, r)
        off = (5 * r) % max(1, n)
        k = min(blk.size, n - off)
        x[off:off + k] = blk[:k]
        ins.append(x)
    return ins


def finite_nonzero_inputs(dtype, n, seed, p):
    """Inputs without NaN and zero (the RCCL comparison point's own treatment of them is not ours)."""
    return [rand(dtype, n, np.random.default_rng(seed + r), "positive") for r in range(p)]
