"""MAX / MIN without a GPU: the numpy reference (tests/minmax_util.py) against hand-written cases and
against np.maximum / np.minimum, the argument checks of tips_bucket_reduce / tips_multi_reduce /
tips_allreduce_op (none of them reaches a launch), and the Python surface's constants and refusals."""
import ctypes

import numpy as np
import pytest

import edge_values as ev
import minmax_util as mm
from gpu_util import ALL_DTYPES, BF16, F16, F32, F64, I32, I64, NPDT, rand
from minmax_util import MAX, MIN

FLOATS = [F32, F64, F16, BF16]


def fb(dtype, *patterns):
    """Values of a float dtype from (sign, exponent field, mantissa field) triples."""
    U, e, m = ev.FMT[dtype]
    return ev.from_bits(np.array([(s << (e + m)) | (x << m) | f for s, x, f in patterns], dtype=U), dtype)


@pytest.mark.parametrize("dtype", FLOATS)
def test_reference_on_hand_written_float_cases(dtype):
    U, e, m = ev.FMT[dtype]
    emax, top = (1 << e) - 1, (1 << m) - 1
    pz, nz = (0, 0, 0), (1, 0, 0)
    pinf, ninf = (0, emax, 0), (1, emax, 0)
    qnan, snan = (0, emax, 1 << (m - 1)), (0, emax, 1)
    one, mone = (0, (1 << (e - 1)) - 1, 0), (1, (1 << (e - 1)) - 1, 0)
    big, small = (0, 0, top), (0, 0, 1)           # the largest and the smallest subnormal
    nbig, nsmall = (1, 0, top), (1, 0, 1)
    #        a      b      MAX    MIN   (None: a NaN)
    rows = [(pz, nz, pz, nz), (nz, pz, pz, nz),
            (qnan, one, None, None), (one, qnan, None, None), (snan, one, None, None), (ninf, snan, None, None),
            (qnan, pinf, None, None), (qnan, qnan, None, None),
            (pinf, one, pinf, one), (one, ninf, one, ninf), (pinf, ninf, pinf, ninf),
            (big, pz, big, pz), (small, pz, small, pz), (nbig, pz, pz, nbig), (nsmall, nz, nz, nsmall),
            (big, small, big, small), (small, big, big, small), (nbig, nsmall, nsmall, nbig), (small, nsmall, small, nsmall),
            (one, mone, one, mone)]
    a, b = fb(dtype, *[r[0] for r in rows]), fb(dtype, *[r[1] for r in rows])
    for op, col in ((MAX, 2), (MIN, 3)):
        for x, y in ((a, b), (b, a)):  # the order of the operands changes nothing
            got = mm.ref([x, y], dtype, op)
            for i, r in enumerate(rows):
                if r[col] is None:
                    assert ev.is_nan(got[i:i + 1], dtype)[0], (op, i)
                else:
                    assert ev.to_bits(got[i:i + 1], dtype)[0] == ev.to_bits(fb(dtype, r[col]), dtype)[0], (op, i)


@pytest.mark.parametrize("dtype", [I32, I64])
def test_reference_on_hand_written_int_cases(dtype):
    i = np.iinfo(NPDT[dtype])
    a = np.array([i.min, i.max, -1, -1, 0, -5, i.min], dtype=NPDT[dtype])
    b = np.array([i.max, i.min, 0, 1, 0, -7, -1], dtype=NPDT[dtype])
    assert mm.ref([a, b], dtype, MAX).tolist() == [i.max, i.max, 0, 1, 0, -5, -1]
    assert mm.ref([a, b], dtype, MIN).tolist() == [i.min, i.min, -1, -1, 0, -7, i.min]
    assert mm.ref([b, a], dtype, MAX).tolist() == [i.max, i.max, 0, 1, 0, -5, -1]
    assert mm.ref([a], dtype, MIN).tolist() == a.tolist()


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("nsrc", [2, 5])
def test_reference_matches_numpy_on_ordinary_data(dtype, nsrc):
    rng = np.random.default_rng(11 + dtype)
    srcs = [rand(dtype, 5003, rng) for _ in range(nsrc)]  # N(0, 3): no NaN, no zero
    if dtype == BF16:
        vals = [(s.astype(np.uint32) << 16).view(np.float32) for s in srcs]
    else:
        vals = srcs
    for op, f in ((MAX, np.maximum), (MIN, np.minimum)):
        exp = vals[0]
        for v in vals[1:]:
            exp = f(exp, v)
        got = mm.ref(srcs, dtype, op)
        if dtype == BF16:
            got = (got.astype(np.uint32) << 16).view(np.float32)
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_same_and_the_shared_inputs(dtype):
    a, b = mm.pair_inputs(dtype, 4099, 5)
    exp = mm.ref([a, b], dtype, MAX)
    assert mm.same(exp, exp, dtype) and mm.same(mm.ref([b, a], dtype, MAX), exp, dtype)
    wrong = exp.copy()
    i = int(np.nonzero(~ev.is_nan(exp, dtype))[0][-1]) if dtype in FLOATS else exp.size - 1
    wrong.view("u%d" % wrong.itemsize)[i] ^= 1  # one bit of one number
    assert not mm.same(wrong, exp, dtype)
    if dtype in FLOATS:  # a NaN's payload is free, a NaN in the place of a number is not
        sp = ev.specials(dtype)
        assert mm.same(sp[13:14], sp[15:16], dtype) and not mm.same(sp[13:14], sp[12:13], dtype)
        ca, cb = mm.crossed_specials(dtype)
        assert ca.size == 32 * 32 and ev.is_nan(mm.ref([ca, cb], dtype, MIN), dtype).sum() == 32 * 32 - 26 * 26
    srcs = mm.planted([rand(dtype, 64, np.random.default_rng(r)) for r in range(3)], dtype)
    got = mm.ref(srcs, dtype, MAX)
    if dtype in FLOATS:
        assert ev.is_nan(got, dtype).tolist() == [i in (3, 5, 7) for i in range(64)]
        assert all(ev.to_bits(got, dtype)[i] == 0 for i in (4, 6, 8))
        assert all(ev.to_bits(mm.ref(srcs, dtype, MIN), dtype)[i] == ev._fields(dtype)[4] for i in (4, 6, 8))


def test_error_codes_without_a_gpu():
    from tips_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    srcs, _keep = _lib.ptr_array([p, p])
    for op in (3, -1, 99):  # a bad op: INVALID_ARG from all three
        assert L.tips_bucket_reduce(p, p, p, 4, _lib.FLOAT32, op, None) == -1
        assert b"op" in L.tips_last_error()
        assert L.tips_multi_reduce(p, srcs, 2, 4, _lib.FLOAT32, op, None) == -1
        assert L.tips_allreduce_op(p, p, 4, _lib.FLOAT32, op, None) == -1
    for op in (_lib.OP_SUM, _lib.OP_MAX, _lib.OP_MIN):
        assert L.tips_bucket_reduce(p, p, p, 4, 99, op, None) == -1  # bad dtype
        assert L.tips_multi_reduce(p, srcs, 2, 4, 99, op, None) == -1
        assert L.tips_allreduce_op(p, p, 4, -1, op, None) == -1
        assert L.tips_bucket_reduce(p, p, p, -1, _lib.FLOAT32, op, None) == -1  # negative count
        assert L.tips_multi_reduce(p, srcs, 2, -1, _lib.FLOAT32, op, None) == -1
        assert L.tips_allreduce_op(p, p, -1, _lib.FLOAT32, op, None) == -1
        assert L.tips_bucket_reduce(None, None, None, 0, _lib.FLOAT32, op, None) == 0  # empty: nothing to do
        assert L.tips_multi_reduce(None, None, 99, 0, _lib.FLOAT32, op, None) == 0
        assert L.tips_bucket_reduce(p, None, p, 4, _lib.FLOAT32, op, None) == -1  # null pointers
        assert L.tips_multi_reduce(None, srcs, 2, 4, _lib.FLOAT32, op, None) == -1
        assert L.tips_multi_reduce(p, None, 2, 4, _lib.FLOAT32, op, None) == -1
        for nsrc in (0, 17, -3):
            assert L.tips_multi_reduce(p, srcs, nsrc, 4, _lib.FLOAT32, op, None) == -1
            assert b"nsrc" in L.tips_last_error()
    # the bad dtype is reported before the bad op
    assert L.tips_bucket_reduce(p, p, p, 4, 99, 7, None) == -1 and b"dtype" in L.tips_last_error()
    # tips_allreduce keeps answering MAX / MIN as before
    assert L.tips_allreduce(None, None, 10, _lib.FLOAT32, _lib.OP_MAX, None) == -5
    assert L.tips_allreduce(None, None, 10, _lib.FLOAT32, _lib.OP_MIN, None) == -5


def test_python_surface_refuses_without_initialising():
    import torch
    import tips_amd as tips
    from tips_amd import _lib
    before = bool(_lib.lib().tips_is_initialize())
    assert tips.Max == "Max" and tips.Min == "Min" and {"Min", "Max", "allreduce_reduce_op"} <= set(tips.__all__)
    x = np.ones(4, dtype=np.float32)
    for op in (tips.Max, tips.Min):
        with pytest.raises(ValueError, match="prescale_factor"):
            tips.allreduce(x, op=op, prescale_factor=0.5)
        with pytest.raises(ValueError, match="postscale_factor"):
            tips.allreduce(x, op=op, postscale_factor=2.0)
        with pytest.raises(ValueError, match="sparse"):
            tips.allreduce(tips.IndexedSlices(x.reshape(2, 2), np.array([0, 1])), op=op)
        with pytest.raises(ValueError, match="sparse"):
            tips.allreduce(torch.sparse_coo_tensor(torch.tensor([[0, 1]]), torch.ones(2), (4,)), op=op)
        with pytest.raises(ValueError, match="name"):
            tips.allreduce(x, op=op, name="grad_0")
        with pytest.raises(ValueError, match="name"):
            tips.allreduce_reduce_op(x, op, name="grad_0")
        with pytest.raises(ValueError, match="SUM only"):
            tips.allreduce_grads([x], op=op)
        with pytest.raises(ValueError, match="SUM only"):
            tips.DistributedOptimizer(torch.optim.SGD([torch.nn.Parameter(torch.ones(2))], lr=0.1), op=op)
        with pytest.raises(ValueError, match="SUM only"):
            tips.DistributedGradientTape(op=op)
    with pytest.raises(ValueError, match="op must be"):
        tips.allreduce_reduce_op(x, "Product")
    assert bool(_lib.lib().tips_is_initialize()) == before  # (the checks come before basics.init())
