"""Adasum without a GPU: the numpy restatement the GPU tests compare against
(tests/adasum_util.py) - inside the definition's bound of an order-free reference, exact where the
definition is exact (a == b, disjoint supports, zero norms), its tree against nested pair calls -
and, through the loaded library, the new C-ABI symbols, the workspace formula, the argument errors
that need no device, and the Python surface's ValueErrors, raised before anything is initialised."""
import os
import subprocess

import numpy as np
import pytest

from adasum_util import (ES, LANES, VECS, _tree256, chunk_elems, chunk_partials, coefficients, fold_chunks, free_ref,
                         long_count, long_pair, pair_intermediates, pair_ref, seeded_pair, segment_dots, segments, to_f64,
                         tree_ref, within_bound, workspace_bytes)
from conftest import REPO
from gpu_util import BF16, F16, F32, F64, I32, I64, NPDT, bits, rand, same_bits

FLOATS = [F32, F64, F16, BF16]
NEW = ("tips_adasum_workspace", "tips_adasum_pair", "tips_allreduce_adasum", "tips_fused_allreduce_adasum_flat")
LIST = [1, 5, 0, 4099, 70001, 3]


def zeros(dtype, n):
    return np.zeros(n, NPDT[dtype])


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("counts", [[1], [63], [64], [65], [4099], [262147], LIST])
def test_restatement_inside_the_bound_of_the_order_free_reference(dtype, counts):
    """|out - ref| <= 4 u_W (|ca a| + |cb b|) + u_S |ref| for seeded normal inputs: the bound the GPU
    tests hold the kernels to holds for the restatement itself."""
    rng = np.random.default_rng(100 * dtype + len(counts) + counts[0] % 7)
    n = sum(counts)
    a, b = rand(dtype, n, rng), rand(dtype, n, rng)
    out = pair_ref(a, b, counts, dtype)
    ref, bound = free_ref(a, b, counts, dtype)
    assert within_bound(out, ref, bound, dtype)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_order_is_a_real_one(dtype):
    """The chunked lane order is not the left-to-right fold: on a long segment the two f64 sums
    differ in their last bits (and both sit within a few ulps of the exact sum). (16-bit products
    have so few bits that either order adds them exactly.)"""
    rng = np.random.default_rng(7)
    n = 3 * chunk_elems(dtype) + 17
    a, b = rand(dtype, n, rng), rand(dtype, n, rng)
    d, na, nb = segment_dots(a, b, dtype)
    x, y = to_f64(a, dtype), to_f64(b, dtype)
    fold = 0.0
    for v in (x * x).tolist():
        fold += v
    assert na != fold
    assert abs(na - fold) <= 1e-12 * fold


def _reference_dots(a, b, dtype):
    """segment_dots as it stood before chunk_partials was split out of it, kept to pin the bits."""
    E, K = 16 // ES[dtype], chunk_elems(dtype)
    n = len(a)
    m = -(-n // K)
    if m == 0:
        return 0.0, 0.0, 0.0
    x = np.zeros(m * K, np.float64)
    y = np.zeros(m * K, np.float64)
    x[:n], y[:n] = to_f64(a, dtype), to_f64(b, dtype)
    x, y = x.reshape(m, VECS, LANES, E), y.reshape(m, VECS, LANES, E)
    acc = np.zeros((3, m, LANES), np.float64)
    for u in range(VECS):
        for j in range(E):
            xs, ys = x[:, u, :, j], y[:, u, :, j]
            acc[0] = acc[0] + xs * ys
            acc[1] = acc[1] + xs * xs
            acc[2] = acc[2] + ys * ys
    c = _tree256(acc)
    rows = -(-m // LANES)
    cp = np.zeros((3, rows * LANES), np.float64)
    cp[:, :m] = c
    cp = cp.reshape(3, rows, LANES)
    lane = np.zeros((3, LANES), np.float64)
    for r in range(rows):
        lane = lane + cp[:, r, :]
    return tuple(float(v) for v in _tree256(lane))


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("counts", [[1], [63], [64], [65], [4099], [262147], LIST])
def test_segment_dots_is_built_on_chunk_partials_bit_for_bit(dtype, counts):
    """The split changed no bit: per segment, segment_dots = fold_chunks(chunk_partials) = the
    unsplit computation; pair_intermediates holds the same chunk sums in global chunk order and the
    coefficients pair_ref uses."""
    rng = np.random.default_rng(100 * dtype + len(counts) + counts[0] % 7)
    a, b = rand(dtype, sum(counts), rng), rand(dtype, sum(counts), rng)
    parts, coef = pair_intermediates(a, b, counts, dtype)
    K = chunk_elems(dtype)
    assert parts.shape == (sum(-(-c // K) for c in counts), 3) and coef.shape == (len(counts), 2)
    c0 = 0
    for s, (lo, hi) in enumerate(segments(counts)):
        dots = segment_dots(a[lo:hi], b[lo:hi], dtype)
        assert np.array_equal(bits(np.array(dots)), bits(np.array(_reference_dots(a[lo:hi], b[lo:hi], dtype))))
        c = chunk_partials(a[lo:hi], b[lo:hi], dtype)
        assert c.shape == (-(-(hi - lo) // K), 3) and c.dtype == np.float64
        assert np.array_equal(bits(np.array(fold_chunks(c))), bits(np.array(dots)))
        assert np.array_equal(bits(parts[c0:c0 + len(c)]), bits(c))
        assert np.array_equal(bits(coef[s]), bits(np.array(coefficients(*dots))))
        c0 += len(c)
    assert c0 == len(parts)
    assert np.array_equal(coef[[c == 0 for c in counts]], np.ones((counts.count(0), 2)))


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("chunks", [257, 300])
def test_second_row_of_the_coefficient_pass_inside_the_bound(dtype, chunks):
    """More than 256 chunks: lane t of the coefficient pass adds a second chunk sum (rows = 2 in
    fold_chunks). The restatement stays inside the order-free reference's bound there.
    Independent operands, as in every use of that bound: it takes the coefficients as exact to one
    rounding, which holds while they are near 1, and the store as a relative error, which holds
    above the subnormals. The launch-shape cases' operands (long_pair: b near 2 a, so ca is an
    exact difference near 4e-5 whose relative error is that of d / na times 1e5, and 0.75 b_i lands
    among f16's subnormals) are made to show the dots' last ulp in ca; the bound says nothing there."""
    n = (chunks - 1) * chunk_elems(dtype) + 16 // ES[dtype] + 1
    assert chunks != 257 or n == long_count(dtype)
    a, b = seeded_pair(dtype, [n])
    assert len(chunk_partials(a[:1], b[:1], dtype)) == 1 and len(chunk_partials(a, b, dtype)) == chunks
    ref, bound = free_ref(a, b, [n], dtype)
    assert within_bound(pair_ref(a, b, [n], dtype), ref, bound, dtype)


def _tree256_low(v):
    """A wrong wave tree: folded from the low half (x[l] += x[l + 1] first, x[l] += x[l + 32] last)."""
    v = v.reshape(v.shape[:-1] + (4, 64))
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _dots_chunks_left_to_right(a, b, dtype):
    """A wrong coefficient pass: the chunk sums added c_0 + c_1 + ... in one accumulator."""
    acc = np.zeros(3, np.float64)
    for c in chunk_partials(a, b, dtype):
        acc = acc + c
    return tuple(acc)


def _dots_low_tree(a, b, dtype):
    return fold_chunks(chunk_partials(a, b, dtype, tree=_tree256_low), tree=_tree256_low)


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("wrong", [_dots_chunks_left_to_right, _dots_low_tree], ids=["chunks_left_to_right", "low_half_tree"])
def test_order_is_visible_in_the_coefficients_at_257_chunks(dtype, wrong):
    """The operands test_gpu_adasum_shapes.py runs at 257 chunks tell the kernels' order from two
    other plausible ones in the f64 bits of (d, na, nb) and - what the device test can read, the
    workspace keeping no segment sums - in those of (ca, cb), so the device comparison of the
    coefficients can fail; all of them agree to a few ulps. (b is near 2 a there: see
    adasum_util.LONG_SALT. With independent operands the dots differ as well, and the coefficients,
    near 1, round the difference away.)"""
    n = long_count(dtype)
    a, b = long_pair(dtype, n)
    right, other = np.array(segment_dots(a, b, dtype)), np.array(wrong(a, b, dtype))
    assert not np.array_equal(bits(right), bits(other))
    assert np.all(np.abs(right - other) <= 1e-12 * np.abs(right[1:]).max())
    assert not np.array_equal(bits(np.array(coefficients(*right))), bits(np.array(coefficients(*other))))


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("counts", [[1], [65], [4099], LIST])
def test_equal_operands_give_the_operand(dtype, counts):
    """a == b: d = na = nb, ca = cb = 0.5 exactly, 0.5 a + 0.5 a = a - in every storage type."""
    rng = np.random.default_rng(3)
    a = rand(dtype, sum(counts), rng)
    assert np.array_equal(bits(pair_ref(a, a.copy(), counts, dtype)), bits(a))


@pytest.mark.parametrize("dtype", FLOATS)
def test_disjoint_supports_give_the_sum(dtype):
    """d = 0: both coefficients are 1 and every element is x + 0."""
    rng = np.random.default_rng(4)
    counts = LIST
    n = sum(counts)
    a, b = rand(dtype, n, rng), rand(dtype, n, rng)
    a[1::2] = zeros(dtype, 1)[0]
    b[0::2] = zeros(dtype, 1)[0]
    exp = a.copy()
    exp[1::2] = b[1::2]
    assert np.array_equal(bits(pair_ref(a, b, counts, dtype)), bits(exp))


@pytest.mark.parametrize("dtype", FLOATS)
def test_zero_norm_operands(dtype):
    """A zero operand has no direction: its coefficient is 1 (not 0 / 0), the other's too (d = 0)."""
    rng = np.random.default_rng(5)
    a = rand(dtype, 300, rng)
    z = zeros(dtype, 300)
    assert coefficients(0.0, 0.0, 5.0) == (1.0, 1.0)
    assert np.array_equal(bits(pair_ref(a, z, [300], dtype)), bits(a))
    assert np.array_equal(bits(pair_ref(z, a, [300], dtype)), bits(a))
    assert np.array_equal(bits(pair_ref(z, z, [100, 200], dtype)), bits(z))


def test_nan_stays_in_its_segment():
    rng = np.random.default_rng(6)
    counts = [40, 50, 60]
    a, b = rand(F32, 150, rng), rand(F32, 150, rng)
    clean = pair_ref(a, b, counts, F32)
    a[45] = np.nan
    out = pair_ref(a, b, counts, F32)
    assert np.isnan(out[40:90]).all()
    assert np.array_equal(bits(out[:40]), bits(clean[:40])) and np.array_equal(bits(out[90:]), bits(clean[90:]))


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("p", [2, 4, 8])
def test_tree_is_nested_pairs(dtype, p):
    rng = np.random.default_rng(p)
    counts = [5, 0, 700, 1]
    vals = [rand(dtype, sum(counts), rng) for _ in range(p)]

    def nest(lo, hi):  # the subtree over ranks [lo, hi): pair(low half, high half)
        if hi - lo == 1:
            return vals[lo]
        mid = (lo + hi) // 2
        return pair_ref(nest(lo, mid), nest(mid, hi), counts, dtype)

    exp = nest(0, p)
    got = tree_ref(vals, counts, dtype)
    assert len(got) == p
    for g in got:
        assert same_bits(g, exp, dtype)
    assert same_bits(tree_ref(vals[:1], counts, dtype)[0], vals[0], dtype)  # p = 1: the copy


# ---------------------------------------------------------------------------
# through the loaded library, no device


def test_new_symbols_declared_exported_and_bound():
    from test_abi import header_functions
    from tips_amd import _lib
    names = header_functions()
    declared = {n for n, _, _ in _lib._SIGNATURES}
    L = _lib.lib()
    for n in NEW:
        assert n in names, n
        assert n in declared, n
        assert hasattr(L, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(REPO, "tips_amd", "lib", "libtips_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported
    assert not set(NEW) & {n for n, _, _ in _lib._DEV_SIGNATURES}


@pytest.mark.parametrize("count,nseg", [(0, 0), (1, 1), (4095, 1), (4096, 1), (262147, 1), (74109, 6), (1 << 33, 1000)])
def test_workspace_formula(count, nseg):
    """3 doubles per chunk (at most count / 4096 + nseg chunks, whatever the float dtype) and 2 per
    segment, rounded up to 256 B - and enough for every dtype's real chunk count."""
    from tips_amd import _lib
    got = _lib.lib().tips_adasum_workspace(count, nseg)
    assert got == workspace_bytes(count, nseg) and got % 256 == 0
    if nseg:
        per = [count // nseg + (1 if i < count % nseg else 0) for i in range(nseg)]
        for dt in FLOATS:
            chunks = sum(-(-c // chunk_elems(dt)) for c in per)
            assert 8 * (3 * chunks + 2 * nseg) <= got


def test_workspace_rejects_negative_sizes():
    from tips_amd import _lib
    L = _lib.lib()
    assert L.tips_adasum_workspace(-1, 1) == -1
    assert L.tips_adasum_workspace(1, -1) == -1


def _pair(L, counts=(8,), dtype=F32, ws_bytes=1 << 20):
    from tips_amd import _lib
    cp, _keep = _lib.i64_array(list(counts))
    return L.tips_adasum_pair(None, None, None, cp, len(counts), dtype, None, ws_bytes, None)


def test_argument_errors_need_no_device():
    from tips_amd import _lib
    L = _lib.lib()
    INVALID, NOT_INIT, UNSUPPORTED = -1, -2, -5
    for dt in (I32, I64):
        assert _pair(L, dtype=dt) == UNSUPPORTED and b"float dtypes only" in L.tips_last_error()
        assert L.tips_allreduce_adasum(None, None, 8, dt, None) == UNSUPPORTED
        assert L.tips_fused_allreduce_adasum_flat(None, None, 0, dt, None, None) == UNSUPPORTED
    assert _pair(L, dtype=99) == INVALID
    assert _pair(L, counts=(4, -1, 3)) == INVALID and b"negative" in L.tips_last_error()
    assert L.tips_adasum_pair(None, None, None, None, -1, F32, None, 0, None) == INVALID
    assert L.tips_adasum_pair(None, None, None, None, 2, F32, None, 0, None) == INVALID  # (no counts)
    assert _pair(L, ws_bytes=-1) == INVALID
    # nothing to do: TIPS_OK with nothing launched, whatever the pointers
    assert _pair(L, counts=()) == 0 and _pair(L, counts=(0, 0, 0), ws_bytes=0) == 0
    # a workspace that is too small, by one byte
    need = L.tips_adasum_workspace(70000, 3)
    assert _pair(L, counts=(1, 69990, 9), ws_bytes=need - 1) == INVALID and b"too small" in L.tips_last_error()
    # the collectives' own argument errors come before the lifecycle check; then: not initialised
    assert L.tips_allreduce_adasum(None, None, -1, F32, None) == INVALID
    assert L.tips_allreduce_adasum(None, None, 0, F32, None) == NOT_INIT
    cp, _keep = _lib.i64_array([3, -2])
    assert L.tips_fused_allreduce_adasum_flat(None, cp, 2, F32, None, None) == INVALID
    assert L.tips_fused_allreduce_adasum_flat(None, None, 0, F32, None, None) == NOT_INIT


def test_python_value_errors_come_before_init():
    import torch
    import tips_amd as tips
    assert tips.Adasum == "Adasum"
    for name in ("Adasum", "adasum_op", "fused_adasum_flat"):
        assert name in tips.__all__ and hasattr(tips, name)
    host = torch.zeros(8)
    with pytest.raises(ValueError, match="device tensors only"):
        tips.allreduce(host, op=tips.Adasum)
    with pytest.raises(ValueError, match="device tensors only"):
        tips.allreduce(np.zeros(8, np.float32), op=tips.Adasum)
    with pytest.raises(ValueError, match="device tensors only"):
        tips.adasum_op(host)
    with pytest.raises(ValueError, match="device tensors only"):
        tips.fused_adasum_flat([host])
    for kw in ({"prescale_factor": 0.5}, {"postscale_factor": 2.0}):
        with pytest.raises(ValueError, match="no scaled Adasum"):
            tips.allreduce(host, op=tips.Adasum, **kw)
    with pytest.raises(ValueError, match="takes no name"):
        tips.allreduce(host, op=tips.Adasum, name="g0")
    with pytest.raises(ValueError, match="sparse"):
        tips.allreduce(tips.IndexedSlices(torch.zeros(2, 3), torch.tensor([0, 1]), (4, 3)), op=tips.Adasum)
    with pytest.raises(ValueError, match="sparse"):
        tips.allreduce(torch.sparse_coo_tensor(torch.tensor([[0, 1]]), torch.ones(2), (4,)), op=tips.Adasum)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1)
    with pytest.raises(ValueError, match="allreduce_grads"):
        tips.DistributedOptimizer(opt, op=tips.Adasum)
    tips.DistributedGradientTape(op=tips.Adasum)  # accepted: it reduces through allreduce_grads
    with pytest.raises(ValueError, match="gradient_predivide_factor"):
        tips.allreduce_grads([host], op=tips.Adasum, gradient_predivide_factor=2.0)
    ints = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="float dtypes only"):
        tips.allreduce(ints, op=tips.Adasum)
    with pytest.raises(ValueError, match="float dtypes only"):
        tips.adasum_op(torch.zeros(4, dtype=torch.int64))
    assert not tips.is_initialized()
