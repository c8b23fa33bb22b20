"""-m gpu: the Adasum pair on the device (tips_adasum_pair) against the numpy
restatement (tests/adasum_util.py), bit for bit, for every float dtype - single segments around a
wave, a vector and a chunk, and a list with a segment below a wave, an empty one and one spanning
several chunks - and inside the definition's bound of the order-free reference. Then what holds
without any restatement: a == b returns a, disjoint supports return tips_bucket_sum's bits, in place
equals out of place, an unaligned view equals its aligned copy, a list equals its segments one by
one, two runs agree; edge values; and, at one rank, the collectives' copy and lifecycle.

Everything here stays within one round of XCD stripes (at most 65 chunks) and judges the output alone.
Shapes beyond that - more than 128 chunks (the striped chunk map), more than 256 (the coefficient
pass's second row), lists on the vector path, mixed alignment - with the workspace's partial sums and
f64 coefficients compared too, further edge values and the layout cache: test_gpu_adasum_shapes.py."""
import numpy as np
import pytest

from adasum_util import free_ref, pair_ref, within_bound
from gpu_util import BF16, F16, F32, F64, NPDT, bits, from_dev, rand, same_bits, stream, to_dev

pytestmark = pytest.mark.gpu

FLOATS = [F32, F64, F16, BF16]
SINGLES = [[1], [63], [64], [65], [4099], [262147]]
LIST = [1, 5, 0, 4099, 70001, 3]
_REF = {}  # (dtype, counts) -> (a, b, restatement, free reference, bound): computed once, never written


def case(dtype, counts):
    key = (dtype, tuple(counts))
    if key not in _REF:
        rng = np.random.default_rng(1000 * dtype + sum(counts) % 997)
        n = sum(counts)
        a, b = rand(dtype, n, rng), rand(dtype, n, rng)
        ref, bound = free_ref(a, b, counts, dtype)
        exp = pair_ref(a, b, counts, dtype)
        for x in (a, b, exp, ref, bound):
            x.setflags(write=False)
        _REF[key] = (a, b, exp, ref, bound)
    return _REF[key]


def pair_dev(da, db, counts, dtype, dst=None, off=0):
    """tips_adasum_pair on device tensors (elements [off, off + sum(counts)) of each); returns dst."""
    import torch
    from tips_amd import _lib
    n = sum(counts)
    if dst is None:
        dst = torch.empty_like(da)
    es = da.element_size()
    need = _lib.lib().tips_adasum_workspace(n, len(counts))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
    cp, _keep = _lib.i64_array(list(counts))
    _lib.call("tips_adasum_pair", dst.data_ptr() + off * es, da.data_ptr() + off * es, db.data_ptr() + off * es, cp,
              len(counts), dtype, ws.data_ptr(), need, stream())
    torch.cuda.synchronize()
    return dst


def pair_np(a, b, counts, dtype):
    return from_dev(pair_dev(to_dev(a), to_dev(b), counts, dtype), dtype)


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("counts", SINGLES + [LIST], ids=lambda c: "x".join(map(str, c)))
def test_bit_exact_and_inside_the_bound(gpu, dtype, counts):
    a, b, exp, ref, bound = case(dtype, counts)
    got = pair_np(a, b, counts, dtype)
    assert same_bits(got, exp, dtype)
    assert within_bound(got, ref, bound, dtype)


@pytest.mark.parametrize("dtype", FLOATS)
def test_equal_operands_return_the_operand(gpu, dtype):
    a = case(dtype, LIST)[0]
    assert np.array_equal(bits(pair_np(a, a.copy(), LIST, dtype)), bits(a))


@pytest.mark.parametrize("dtype", FLOATS)
def test_disjoint_supports_return_the_bucket_sum(gpu, dtype):
    import torch
    from tips_amd import _lib
    a, b = case(dtype, LIST)[0].copy(), case(dtype, LIST)[1].copy()
    a[1::2] = 0
    b[0::2] = 0
    da, db = to_dev(a), to_dev(b)
    dc = torch.empty_like(da)
    _lib.call("tips_bucket_sum", dc.data_ptr(), da.data_ptr(), db.data_ptr(), len(a), dtype, stream())
    got = from_dev(pair_dev(da, db, LIST, dtype), dtype)
    assert np.array_equal(bits(got), bits(from_dev(dc, dtype)))


@pytest.mark.parametrize("dtype", FLOATS)
def test_in_place_equals_out_of_place(gpu, dtype):
    a, b, exp = case(dtype, LIST)[:3]
    for which in (0, 1):
        da, db = to_dev(a), to_dev(b)
        got = from_dev(pair_dev(da, db, LIST, dtype, dst=(da, db)[which]), dtype)
        assert same_bits(got, exp, dtype), which


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("counts", [[4099], [70001], LIST], ids=lambda c: "x".join(map(str, c)))
def test_unaligned_view_returns_the_aligned_bits(gpu, dtype, counts):
    """One element past a 16-B boundary every load is an element load: the same lanes, the same order."""
    import torch
    a, b, exp = case(dtype, counts)[:3]
    pad = np.zeros(1, NPDT[dtype])
    da, db = to_dev(np.concatenate([pad, a])), to_dev(np.concatenate([pad, b]))
    assert da.data_ptr() % 16 == 0
    dst = torch.zeros_like(da)
    got = from_dev(pair_dev(da, db, counts, dtype, dst=dst, off=1), dtype)
    assert same_bits(got[1:], exp, dtype) and got[0] == 0


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_list_equals_its_segments_one_by_one(gpu, dtype):
    a, b = case(dtype, LIST)[:2]
    whole = pair_np(a, b, LIST, dtype)
    o = 0
    for c in LIST:
        if c:
            assert np.array_equal(bits(pair_np(a[o:o + c], b[o:o + c], [c], dtype)), bits(whole[o:o + c])), c
        o += c


@pytest.mark.parametrize("dtype", [F32, F16])
def test_two_runs_return_the_same_bits(gpu, dtype):
    a, b = case(dtype, [262147])[:2]
    assert np.array_equal(bits(pair_np(a, b, [262147], dtype)), bits(pair_np(a, b, [262147], dtype)))


@pytest.mark.parametrize("dtype", FLOATS)
def test_nan_stays_in_its_segment(gpu, dtype):
    a, b, exp = case(dtype, LIST)[:3]
    a = a.copy()
    lo = 1 + 5  # the 4099-element segment
    a[lo + 77] = 0x7fc0 if dtype == BF16 else np.nan
    got = pair_np(a, b, LIST, dtype)
    f = (got.astype(np.uint32) << 16).view(np.float32) if dtype == BF16 else got
    assert np.isnan(f[lo:lo + 4099]).all()
    keep = np.r_[0:lo, lo + 4099:len(a)]
    assert np.array_equal(bits(got)[keep], bits(exp)[keep])
    assert same_bits(got, pair_ref(a, b, LIST, dtype), dtype)


@pytest.mark.parametrize("dtype", FLOATS)
def test_zero_operand(gpu, dtype):
    a = case(dtype, LIST)[0]
    z = np.zeros_like(a)
    assert np.array_equal(bits(pair_np(a, z, LIST, dtype)), bits(a))
    assert np.array_equal(bits(pair_np(z, a, LIST, dtype)), bits(a))
    assert np.array_equal(bits(pair_np(z, z, LIST, dtype)), bits(z))


def test_subnormal_only_segments_keep_their_norms(gpu):
    """f32 subnormals squared are far below f32's range and well inside f64's: the norms are kept, so
    the coefficients are those of the directions, not 1."""
    rng = np.random.default_rng(11)
    counts = [70, 4099]
    n = sum(counts)
    a = rng.integers(1, 1 << 23, size=n, dtype=np.uint32).view(np.float32)
    b = a.copy()
    b[::3] = rng.integers(1, 1 << 23, size=len(b[::3]), dtype=np.uint32).view(np.float32)
    got = pair_np(a, b, counts, F32)
    assert same_bits(got, pair_ref(a, b, counts, F32), F32)
    assert not np.array_equal(bits(got), bits(a + b))  # (coefficients of 1 would give the sum)
    # a == b: ca = cb = 0.5 exactly (d = na = nb, none of them flushed), so every element is
    # fl(0.5 a) + fl(0.5 a) - a itself where halving a subnormal is exact, its even neighbour otherwise
    half = a * np.float32(0.5)
    assert np.array_equal(bits(pair_np(a, a.copy(), counts, F32)), bits(half + half))


def test_one_rank_is_the_copy_and_the_lifecycle(gpu):
    """p = 1: tips_allreduce_adasum copies, the list call packs; after shutdown / init again."""
    import torch
    import tips_amd
    for _ in range(2):
        tips_amd.init()
        for n in (1, 4099, 70001):  # (the scratch, were it used, would grow across sizes)
            t = torch.randn(n, device="cuda")
            out = tips_amd.adasum_op(t)
            assert out.data_ptr() != t.data_ptr() and torch.equal(out, t)
            assert torch.equal(tips_amd.allreduce(t, op=tips_amd.Adasum), t)
            h = t.to(torch.bfloat16)
            assert torch.equal(tips_amd.allreduce(h, op=tips_amd.Adasum), h)
        ts = [torch.randn(s, device="cuda") for s in ((1,), (3, 5), (0,), (4099,))]
        outs = tips_amd.fused_adasum_flat(ts)
        assert all(torch.equal(o, t) and o.shape == t.shape for o, t in zip(outs, ts))
        grads = [ts[0], None, ts[3]]
        red = tips_amd.allreduce_grads(grads, op=tips_amd.Adasum)
        assert red[1] is None and torch.equal(red[0], ts[0]) and torch.equal(red[2], ts[3])
        with pytest.raises(ValueError, match="float dtypes only"):
            tips_amd.allreduce(torch.zeros(4, dtype=torch.int32, device="cuda"), op=tips_amd.Adasum)
        torch.cuda.synchronize()
        tips_amd.shutdown()
    tips_amd.init()
