"""-m gpu: the ordered row-sum kernels (tips_rows_sum) and the Python surface at one rank, bit-exact
against the numpy definition of tests/sparse_util.py.

Every dtype; row lengths that take the 16-B vector form (several rows per wave, one row per wave,
rows longer than a wave's 1 KiB) and the element form (lengths that are no multiple of 16 B, and
`values` / `dst` one element past a 16-B boundary); entry counts around a wave's 64 lanes, more than
one workgroup, and 5000 entries on one row (the O(n^2 / lanes) ordering must still finish); 1, 2 and
1000 dense rows; unique, equal, ascending, descending and Zipf-like indices; factors 1/3 and 0.7
(powers of two would hide a misplaced factor). dst is pre-filled with a NaN pattern: every row must
be overwritten, the rows nothing names with +0."""
import ctypes

import numpy as np
import pytest

from gpu_util import ALL_DTYPES, BF16, F16, F32, F64, I32, I64, NPDT, bits, same_bits
from sparse_util import FLOATS, PATTERNS, make_indices, rows_sum_ref

pytestmark = pytest.mark.gpu

PRE, POST = 1.0 / 3, 0.7
DS = [1, 3, 4, 7, 64, 129, 1028]
NS = [0, 1, 63, 64, 65, 257, 5000]
RS = [1, 2, 1000]


def tdtype(dtype):
    import torch
    return {F32: torch.float32, F64: torch.float64, I32: torch.int32, I64: torch.int64, F16: torch.float16,
            BF16: torch.int16}[dtype]


def rand_values(dtype, n, D, rng):
    """Values whose sums round: normal floats of mixed magnitude, full-range integers."""
    if dtype in (I32, I64):
        info = np.iinfo(NPDT[dtype])
        return rng.integers(info.min, info.max, size=(n, D), dtype=NPDT[dtype], endpoint=True)
    x = (rng.standard_normal((n, D)) * np.exp2(rng.integers(-6, 7, size=(n, D)))).astype(np.float32)
    if dtype == BF16:
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    return x.astype(NPDT[dtype])


def device_rows_sum(values, idx, rows, dtype, pre=1.0, post=1.0, offset=False, stream=None):
    """tips_rows_sum on device copies of (values [n, D], idx [n]); `offset`: values and dst start one
    element past a 16-B boundary. dst is pre-filled with 0xFF bytes (a NaN pattern for the floats)."""
    import torch
    from tips_amd import _lib
    n, D = values.shape
    off = 1 if offset else 0
    host = np.zeros(n * D + off, NPDT[dtype])
    host[off:] = values.reshape(-1)
    dv = torch.from_numpy(host.view(np.int16) if dtype == BF16 else host).cuda()[off:]
    di = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
    es = np.dtype(NPDT[dtype]).itemsize
    raw = torch.full(((rows * D + off) * es,), 0xFF, dtype=torch.uint8, device="cuda")
    dst = raw.view(tdtype(dtype))[off:]
    assert (n == 0 or dv.data_ptr() % 16 == off * es % 16) and dst.data_ptr() % 16 == off * es % 16
    need = _lib.lib().tips_rows_sum_workspace(rows, n)
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _lib.call("tips_rows_sum", dst.data_ptr(), rows, D, dv.data_ptr() if n else None, di.data_ptr() if n else None, n,
              dtype, pre, post, ws.data_ptr(), need, sp)
    torch.cuda.synchronize()
    return dst.cpu().numpy().view(NPDT[dtype]).reshape(rows, D).copy()


def check(values, idx, rows, dtype, pre=1.0, post=1.0, offset=False, what=""):
    got = device_rows_sum(values, idx, rows, dtype, pre, post, offset)
    exp = rows_sum_ref(values, idx, rows, dtype, pre, post)
    assert same_bits(got, exp, dtype), "%s dtype %d n %d D %d rows %d offset %s: %d elements differ" % (
        what, dtype, values.shape[0], values.shape[1], rows, offset, int((bits(got) != bits(exp)).sum()))
    return got


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_rows_sum_sizes(gpu, dtype, D):
    """Every n x rows for one dtype and row length; the pattern, the alignment and the factors cycle
    so that each meets every n and every row count somewhere in the D's."""
    rng = np.random.default_rng(1000 * dtype + D)
    k = DS.index(D)
    for n in NS:
        for rows in RS:
            k += 1
            pattern = PATTERNS[k % len(PATTERNS)]
            scaled = dtype in FLOATS and (k // len(PATTERNS)) % 2 == 1
            offset = (k // 2) % 2 == 1
            idx = make_indices(pattern, n, rows, rng)
            values = rand_values(dtype, n, D, rng)
            got = check(values, idx, rows, dtype, PRE if scaled else 1.0, POST if scaled else 1.0, offset, pattern)
            if dtype in FLOATS:  # finite inputs: a NaN left in dst is a row that was not written
                f = got if dtype != BF16 else (got.astype(np.uint32) << 16).view(np.float32)
                assert not np.isnan(f).any()
            named = np.zeros(rows, bool)
            named[idx] = True
            assert not bits(got)[~named].any()  # rows nothing names: +0


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_rows_sum_index_patterns(gpu, dtype, pattern):
    """Each index pattern at n = 257 and n = 5000 into 1000 rows - "same" puts all 5000 on one row,
    the worst case of the ordering pass - through the vector form (D = 4 or 8: 16 B per row) and the
    element form (D = 7, and the offset bases), plain and scaled."""
    rng = np.random.default_rng(77 * dtype + len(pattern))
    es = np.dtype(NPDT[dtype]).itemsize
    for n in (257, 5000):
        idx = make_indices(pattern, n, 1000, rng)
        for D, offset in ((16 // es, False), (7, False), (16 // es, True)):
            values = rand_values(dtype, n, D, rng)
            check(values, idx, 1000, dtype, offset=offset, what=pattern)
            if dtype in FLOATS:
                check(values, idx, 1000, dtype, PRE, POST, offset, what=pattern + " scaled")


@pytest.mark.parametrize("rows", [8191, 8192, 100003])
def test_rows_sum_many_rows(gpu, rows):
    """The prefix sum over rows + 1 counters runs in one workgroup up to 8192 of them and as parallel
    tiles of 2048 above: both sides of that threshold, and a count that ends inside a tile. The
    tiled form borrows the first cursors for its carries and must hand them back zeroed."""
    rng = np.random.default_rng(rows)
    for dtype, D, n, pattern in ((F32, 4, 5000, "zipf"), (I64, 3, 5000, "permutation"), (BF16, 8, 257, "descending"),
                                 (F32, 4, 0, "zipf")):
        idx = make_indices(pattern, n, rows, rng)
        if n:
            idx[:3] = [0, rows - 1, rows - 1]  # the first and the last row are named
        check(rand_values(dtype, n, D, rng), idx, rows, dtype, what="many rows")


def _enc(x, dtype):
    x = np.asarray(x)
    if dtype == BF16:
        return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return x.astype(NPDT[dtype])


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("dtype", FLOATS)
def test_rows_sum_edge_rows(gpu, dtype, offset):
    """Row 0: a lone -0 (stays -0). Row 1: inf + -inf (NaN). Row 2: two finite values whose sum
    overflows f16 at the store (and only there: the third entry brings an f16 sum back in range when
    the partial sum is kept in fp32). Row 3: small, big, -big at positions far apart, which a fold in
    another order does not reproduce. Row 4: subnormals whose sum is subnormal. Row 5: nothing."""
    tiny = {F32: np.float32(1e-45), F64: np.float64(5e-324), F16: np.float16(6e-8), BF16: np.float32(9.2e-41)}[dtype]
    big, small = {F32: (1e8, 1.0), F64: (1e17, 1.0), F16: (65504.0, 0.001), BF16: (1e8, 1.0)}[dtype]
    D = 8
    rows_of = [0, 3, 1, 2, 4, 3, 1, 2, 4, 3, 2, 6]
    lead = [-0.0, small, np.inf, 60000.0, 3 * tiny, big, -np.inf, 60000.0, 5 * tiny, -big, -60000.0, 2.5]
    with np.errstate(over="ignore"):
        values = np.stack([_enc(np.full(D, v, np.float64), dtype) for v in lead])
    idx = np.array(rows_of, np.int64)
    for pre, post in ((1.0, 1.0), (PRE, POST)):
        got = check(values, idx, 7, dtype, pre, post, offset, what="edge rows")
        if (pre, post) == (1.0, 1.0):
            assert (bits(got)[0] == bits(_enc([-0.0], dtype))[0]).all()
            assert not bits(got)[5].any()
            exp3 = rows_sum_ref(values, idx, 7, dtype)[3]
            rev3 = rows_sum_ref(values, idx, 7, dtype, reverse=True)[3]
            assert (bits(exp3) != bits(rev3)).all()  # the row is order-sensitive, and the device took the defined order
            assert bits(got)[4].all()  # the subnormal sum is not flushed
    # f16: 60000 + 60000 alone overflows at the store
    if dtype == F16:
        got = check(values[[3, 7]], np.array([0, 0]), 1, dtype, offset=offset)
        assert np.isinf(got).all()


@pytest.mark.parametrize("dtype", [F32, BF16, I64])
def test_out_of_range_indices_are_skipped_and_counted(gpu, dtype):
    import tips_amd
    rng = np.random.default_rng(5 + dtype)
    n, rows, D = 1000, 50, 12
    idx = make_indices("zipf", n, rows, rng)
    bad_at = rng.permutation(n)[:90]
    idx[bad_at[:30]] = -1
    idx[bad_at[30:60]] = rows
    idx[bad_at[60:]] = 1 << 40
    values = rand_values(dtype, n, D, rng)
    calls0, entries0, bad0 = tips_amd.sparse_stats()
    got = check(values, idx, rows, dtype, what="out of range")
    keep = (idx >= 0) & (idx < rows)
    assert same_bits(got, rows_sum_ref(values[keep], idx[keep], rows, dtype), dtype)
    calls1, entries1, bad1 = tips_amd.sparse_stats()
    assert (calls1 - calls0, entries1 - entries0, bad1 - bad0) == (1, n, 90)
    # every index out of range: a table of zeros; and the process goes on
    got = device_rows_sum(values, np.full(n, rows + 5, np.int64), rows, dtype)
    assert not bits(got).any()
    assert tips_amd.sparse_stats()[2] - bad1 == n
    check(values, make_indices("permutation", n, rows, rng), rows, dtype, what="after bad indices")


@pytest.mark.parametrize("dtype", [F32, F16])
def test_same_call_twice_gives_the_same_bits(gpu, dtype):
    rng = np.random.default_rng(9)
    n, rows, D = 5000, 300, 36
    idx = make_indices("zipf", n, rows, rng)
    values = rand_values(dtype, n, D, rng)
    a = device_rows_sum(values, idx, rows, dtype, PRE, POST)
    b = device_rows_sum(values, idx, rows, dtype, PRE, POST)
    assert np.array_equal(bits(a), bits(b))
    # one holder of all entries and three holders in rank order are the same gathered arrays:
    # the definition has no other input (the multi-process test checks the exchange)
    assert same_bits(a, rows_sum_ref(values, idx, rows, dtype, PRE, POST), dtype)


def test_rows_sum_refuses_host_pointers_and_small_workspaces(gpu):
    import torch
    from tips_amd import _lib
    L = _lib.lib()
    rows, D, n = 8, 4, 3
    need = L.tips_rows_sum_workspace(rows, n)
    dst = torch.zeros(rows * D, device="cuda")
    vals = torch.ones(n * D, device="cuda")
    idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    ws = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    hvals = np.ones(n * D, np.float32)
    sp = torch.cuda.current_stream().cuda_stream
    assert L.tips_rows_sum(dst.data_ptr(), rows, D, hvals.ctypes.data, idx.data_ptr(), n, F32, 1.0, 1.0, ws.data_ptr(),
                           need, sp) == -5
    assert b"host memory" in L.tips_last_error()
    assert L.tips_rows_sum(dst.data_ptr(), rows, D, vals.data_ptr(), idx.data_ptr(), n, F32, 1.0, 1.0, ws.data_ptr(),
                           need - 8, sp) == -1
    assert L.tips_rows_sum(dst.data_ptr(), rows, D, vals.data_ptr(), idx.data_ptr(), n, F32, 1.0, 1.0, ws.data_ptr(),
                           need, sp) == 0
    torch.cuda.synchronize()
    assert dst.view(rows, D)[0].eq(3).all() and dst.view(rows, D)[1:].eq(0).all()


# ---------------------------------------------------------------- the Python surface at one rank

@pytest.fixture(scope="module")
def no_negotiation(gpu):
    """tips_sparse_allreduce is refused while a negotiation runs, and in a process that runs the
    whole suite an earlier test's named request has started one: shut down and initialise again
    (what a job does between its phases), which stops it."""
    gpu.shutdown()
    gpu.init()
    return gpu


def test_sparse_allreduce_is_refused_while_a_negotiation_runs(gpu):
    """After the first named request the negotiation thread runs: the call returns
    TIPS_ERR_UNSUPPORTED with a message (named sparse requests are out of scope), tips_rows_sum is
    unaffected, and after shutdown / init the call works again."""
    import torch
    from tips_amd import _lib
    values, idx, sl = _slices(gpu, F32, 50, 9, 4, 2)
    t = torch.ones(8, device="cuda")
    assert torch.equal(gpu.synchronize(gpu.allreduce_async(t, "sparse.negotiation.started")), t)
    with pytest.raises(_lib.TipsError) as ei:
        gpu.sparse_allreduce(sl)
    assert ei.value.code == -5 and "negotiation" in str(ei.value)
    check(values, idx, 9, F32, what="rows_sum beside a negotiation")
    gpu.shutdown()
    gpu.init()
    assert same_bits(gpu.sparse_allreduce(sl).cpu().numpy(), rows_sum_ref(values, idx, 9, F32), F32)


def _slices(gpu, dtype, n, rows, D, seed, pattern="zipf"):
    import torch
    rng = np.random.default_rng(seed)
    idx = make_indices(pattern, n, rows, rng)
    values = rand_values(dtype, n, D, rng)
    tv = torch.from_numpy(values.view(np.int16) if dtype == BF16 else values).cuda()
    if dtype == BF16:
        tv = tv.view(torch.bfloat16)
    return values, idx, gpu.IndexedSlices(tv, torch.from_numpy(idx).cuda(), (rows, D))


def _np(t, dtype):
    import torch
    if dtype == BF16:
        t = t.view(torch.int16)
    return t.cpu().numpy().view(NPDT[dtype])


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_sparse_allreduce_dense_and_coalesced(gpu, no_negotiation, dtype):
    import torch
    values, idx, sl = _slices(gpu, dtype, 700, 90, 10, 31 + dtype)
    dense = gpu.sparse_allreduce(sl)
    exp = rows_sum_ref(values, idx, 90, dtype)
    assert tuple(dense.shape) == (90, 10) and same_bits(_np(dense, dtype), exp, dtype)
    co = gpu.sparse_allreduce(sl, coalesced=True)
    uniq = np.unique(idx)
    assert np.array_equal(co.indices.cpu().numpy(), uniq) and tuple(co.dense_shape) == (90, 10)
    assert same_bits(_np(co.values, dtype), exp[uniq], dtype)
    if dtype in FLOATS:  # op=Average at one rank divides by 1; the factors reach the kernel
        sc = gpu.sparse_allreduce(sl, op=gpu.Average, prescale_factor=PRE, postscale_factor=POST)
        assert same_bits(_np(sc, dtype), rows_sum_ref(values, idx, 90, dtype, PRE, POST), dtype)
    # no entries at all: zeros
    empty = gpu.IndexedSlices(sl.values[:0], sl.indices[:0], (90, 10))
    assert not bits(_np(gpu.sparse_allreduce(empty), dtype)).any()
    torch.cuda.synchronize()


def test_sparse_allreduce_coo_and_trailing_dims(gpu, no_negotiation):
    import torch
    rng = np.random.default_rng(3)
    n, rows = 400, 33
    idx = make_indices("zipf", n, rows, rng)
    values = rand_values(F32, n, 6, rng)
    coo = torch.sparse_coo_tensor(torch.from_numpy(idx).cuda()[None, :], torch.from_numpy(values).cuda().view(n, 2, 3),
                                  (rows, 2, 3))
    dense = gpu.sparse_allreduce(coo)
    assert tuple(dense.shape) == (rows, 2, 3)
    assert same_bits(dense.cpu().numpy().reshape(rows, 6), rows_sum_ref(values, idx, rows, F32), F32)
    # a coalesced zero-row result keeps its shape
    co = gpu.sparse_allreduce(coo, coalesced=True)
    assert tuple(co.values.shape) == (len(np.unique(idx)), 2, 3)


def test_consistency_check_raises_on_bad_indices(gpu, no_negotiation):
    import torch
    values, idx, sl = _slices(gpu, F32, 100, 20, 4, 8)
    bad = gpu.IndexedSlices(sl.values, sl.indices.clone(), sl.dense_shape)
    bad.indices[5] = 20
    gpu.set_consistency_check(True)
    try:
        gpu.sparse_allreduce(sl)
        with pytest.raises(ValueError, match="outside"):
            gpu.sparse_allreduce(bad)
    finally:
        gpu.set_consistency_check(False)
    idx2 = idx.copy()
    idx2[5] = 20
    assert same_bits(gpu.sparse_allreduce(bad).cpu().numpy(), rows_sum_ref(values, idx2, 20, F32), F32)  # off: skipped
    torch.cuda.synchronize()


def test_allreduce_grads_switch(gpu, no_negotiation):
    """sparse_as_dense=True with the switch off is today's route (torch.index_add_); on, the device
    sparse gradients go through sparse_allreduce. On integer-valued data both are exact, so they
    agree; dense gradients and None pass through either way."""
    import torch
    rng = np.random.default_rng(12)
    n, rows, D = 600, 40, 9
    idx = torch.from_numpy(make_indices("zipf", n, rows, rng)).cuda()
    vals = torch.from_numpy(rng.integers(-8, 9, size=(n, D)).astype(np.float32)).cuda()
    dense_g = torch.randn(17, device="cuda")
    coo = torch.sparse_coo_tensor(idx[None, :], vals, (rows, D))
    grads = [gpu.IndexedSlices(vals, idx, (rows, D)), None, dense_g, coo]
    off = gpu.allreduce_grads(grads, sparse_as_dense=True)
    calls0 = gpu.sparse_stats()[0]
    gpu.set_sparse_reduce(True)
    try:
        on = gpu.allreduce_grads(grads, sparse_as_dense=True)
        assert gpu.sparse_stats()[0] - calls0 == 2
        kept = gpu.allreduce_grads(grads, sparse_as_dense=False)  # not asked to densify: nothing changes
        assert kept[0] is grads[0] and kept[3] is grads[3]
    finally:
        gpu.set_sparse_reduce(False)
    assert gpu.sparse_stats()[0] - calls0 == 2
    assert off[1] is None and on[1] is None and on[2] is dense_g and off[2] is dense_g
    for i in (0, 3):
        assert not on[i].is_sparse and torch.equal(on[i], off[i])
    ref = torch.zeros(rows, D, device="cuda").index_add_(0, idx, vals)
    assert torch.equal(on[0], ref)
