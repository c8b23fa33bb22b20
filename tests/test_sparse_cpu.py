"""The sparse row sum without a GPU: the new C-ABI symbols are declared, exported
and bound; the workspace formula; the argument errors of tips_rows_sum that need no device; the
Python surface's ValueErrors, raised before anything is initialised; and the numpy definition the
GPU tests compare against (tests/sparse_util.py) - it agrees with np.add.at where sums are exact,
and it pins a real order: an order-sensitive triple folds differently from the other end."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from gpu_util import ALL_DTYPES, BF16, F16, F32, F64, I32, I64, NPDT, bits
from sparse_util import PATTERNS, make_indices, rows_sum_ref

NEW = ("tips_rows_sum_workspace", "tips_rows_sum", "tips_sparse_allreduce", "tips_sparse_stats")


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
    # the development header keeps its own list: none of the new names is in it
    assert not set(NEW) & {n for n, _, _ in _lib._DEV_SIGNATURES}


@pytest.mark.parametrize("rows,n", [(0, 0), (1, 0), (1, 1), (1000, 5000), (1 << 20, 1 << 16), (3, 1 << 33)])
def test_workspace_formula(rows, n):
    """offset[rows + 1] and cursor[rows + 1] of 8 B, then two id arrays of 8 B per entry."""
    from tips_amd import _lib
    assert _lib.lib().tips_rows_sum_workspace(rows, n) == 8 * (2 * rows + 2) + 16 * n


def test_workspace_rejects_negative_sizes():
    from tips_amd import _lib
    L = _lib.lib()
    assert L.tips_rows_sum_workspace(-1, 0) == -1
    assert L.tips_rows_sum_workspace(0, -1) == -1


def _rows_sum(L, rows=4, row_elems=3, n=0, dtype=F32, pre=1.0, post=1.0, ws_bytes=1 << 20):
    return L.tips_rows_sum(None, rows, row_elems, None, None, n, dtype, pre, post, None, ws_bytes, None)


def test_rows_sum_argument_errors_need_no_device():
    from tips_amd import _lib
    L = _lib.lib()
    INVALID, UNSUPPORTED = -1, -5
    assert _rows_sum(L, rows=-1) == INVALID and b"negative" in L.tips_last_error()
    assert _rows_sum(L, row_elems=-1) == INVALID
    assert _rows_sum(L, n=-1) == INVALID
    assert _rows_sum(L, ws_bytes=-1) == INVALID
    assert _rows_sum(L, dtype=99) == INVALID
    for dt in (I32, I64):
        assert _rows_sum(L, dtype=dt, pre=0.5) == UNSUPPORTED
        assert _rows_sum(L, dtype=dt, post=1.0 / 3) == UNSUPPORTED
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert _rows_sum(L, pre=bad) == INVALID
        assert _rows_sum(L, post=bad) == INVALID
        assert _rows_sum(L, dtype=I32, pre=bad) == INVALID  # (not finite comes before not supported)
    # nothing to write: TIPS_OK with nothing launched, whatever the pointers
    assert _rows_sum(L, rows=0) == 0 and _rows_sum(L, row_elems=0) == 0
    # a workspace that is too small, by one byte
    need = L.tips_rows_sum_workspace(4, 10)
    assert _rows_sum(L, n=10, ws_bytes=need - 1) == INVALID and b"too small" in L.tips_last_error()
    # the collective's own argument errors come before the lifecycle check; then: not initialised
    assert L.tips_sparse_allreduce(None, None, -1, 4, 3, F32, 1.0, 1.0, None, None) == INVALID
    assert L.tips_sparse_allreduce(None, None, 0, 4, 3, I64, 2.0, 1.0, None, None) == UNSUPPORTED
    assert L.tips_sparse_allreduce(None, None, 0, 4, 3, F32, 1.0, 1.0, None, None) == -2
    # no row sum was launched: the counters read zero without touching a device
    v = [ctypes.c_int64(-1) for _ in range(3)]
    assert L.tips_sparse_stats(*[ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [0, 0, 0]


def test_python_value_errors_come_before_init():
    import torch
    import tips_amd as tips
    S = tips.IndexedSlices
    host = S(np.zeros((2, 3), np.float32), np.array([0, 1]), (4, 3))
    with pytest.raises(ValueError, match="allgather branch"):
        tips.sparse_allreduce(host)
    with pytest.raises(ValueError, match="allgather branch"):
        tips.sparse_allreduce(S(torch.zeros(2, 3), torch.tensor([0, 1]), (4, 3)))
    for op in (tips.Max, tips.Min):
        with pytest.raises(ValueError, match="not defined for sparse"):
            tips.sparse_allreduce(host, op=op)
    ints = S(torch.zeros(2, 3, dtype=torch.int32), torch.tensor([0, 1]), (4, 3))
    for kw in ({"prescale_factor": 0.5}, {"postscale_factor": 2.0}, {"op": tips.Average}):
        with pytest.raises(ValueError, match="integer values"):
            tips.sparse_allreduce(ints, **kw)
    with pytest.raises(ValueError, match="dense_shape"):
        tips.sparse_allreduce(S(torch.zeros(2, 3), torch.tensor([0, 1])))
    coo2 = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 2]]), torch.ones(2), (4, 3))
    with pytest.raises(ValueError, match="one sparse dimension"):
        tips.sparse_allreduce(coo2)
    with pytest.raises(ValueError, match="IndexedSlices or a torch sparse"):
        tips.sparse_allreduce(torch.zeros(4, 3))
    assert not tips.is_initialized()
    for name in ("sparse_allreduce", "set_sparse_reduce", "sparse_stats"):
        assert name in tips.__all__ and hasattr(tips, name)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_reference_agrees_with_add_at_where_sums_are_exact(dtype, pattern):
    """Integers wrap, and small integer-valued floats add exactly in any order: there the fold's
    order cannot matter and np.add.at is a second opinion on which rows meet."""
    rng = np.random.default_rng(3 * dtype + len(pattern))
    n, rows, D = 300, 37, 5
    idx = make_indices(pattern, n, rows, rng)
    idx[::17] = [-1, rows, 1 << 40][dtype % 3]  # skipped entries
    if dtype in (I32, I64):
        info = np.iinfo(NPDT[dtype])
        vals = rng.integers(info.min, info.max, size=(n, D), dtype=NPDT[dtype], endpoint=True)
        exp = np.zeros((rows, D), NPDT[dtype])
    else:
        # |sum| <= 1200 < 2^11: exact in f16's 11-bit significand; bf16 has 8 bits: -1 / 0 / 1, |sum| <= 300
        # only if every entry of a row agreed in sign (the seeded walks stay far inside 2^8)
        small = rng.integers(-4, 5, size=(n, D)).astype(np.float32)
        if dtype == BF16:
            small = np.sign(small)
            vals = (small.view(np.uint32) >> 16).astype(np.uint16)
        else:
            vals = small.astype(NPDT[dtype])
        exp = np.zeros((rows, D), np.float64)
    ok = (idx >= 0) & (idx < rows)
    with np.errstate(over="ignore"):
        np.add.at(exp, idx[ok], vals[ok] if dtype != BF16 else small[ok])
    got = rows_sum_ref(vals, idx, rows, dtype)
    if dtype == BF16:
        assert np.abs(exp).max() <= 256
        got = (got.astype(np.uint32) << 16).view(np.float32)
    assert np.array_equal(got.astype(exp.dtype), exp)


@pytest.mark.parametrize("dtype,big,small", [(F32, 1e8, 1.0), (F64, 1e17, 1.0), (F16, 65504.0, 0.001), (BF16, 1e8, 1.0)])
def test_reference_pins_an_order(dtype, big, small):
    """(small + big) - big loses `small` in the working type; (-big + big) + small, the same entries
    folded from the other end, keeps it: the reference's order is a real one."""
    if dtype == BF16:
        enc = lambda x: (np.array(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)
    else:
        enc = lambda x: np.array(x, NPDT[dtype])
    vals = enc([[small], [7.0], [big], [-big]])
    idx = np.array([2, 0, 2, 2])
    fwd = rows_sum_ref(vals, idx, 3, dtype)
    rev = rows_sum_ref(vals, idx, 3, dtype, reverse=True)
    assert bits(fwd)[2, 0] != bits(rev)[2, 0]
    assert bits(fwd)[0, 0] == bits(rev)[0, 0] == bits(enc([[7.0]]))[0, 0]
    assert bits(fwd)[1, 0] == 0  # a row nothing names is +0
    # and the factors sit where the definition puts them: post * (pre * a + pre * b), separately rounded
    if dtype == F32:
        a, b = np.float32(1.1), np.float32(2.3)
        pre, post = np.float32(1.0 / 3), np.float32(0.7)
        exp = ((a * pre) + (b * pre)) * post
        got = rows_sum_ref(np.array([[a], [b]], np.float32), np.array([0, 0]), 1, F32, 1.0 / 3, 0.7)
        assert got[0, 0] == exp


def test_reference_edge_rows():
    """A lone -0 stays -0 (the fold starts from the first row, not from zero); inf + -inf is NaN;
    f16 overflows at the store, not before."""
    vals = np.array([[-0.0], [np.inf], [-np.inf], [60000.0], [60000.0], [-60000.0]], np.float16)
    idx = np.array([0, 1, 1, 2, 2, 2])
    got = rows_sum_ref(vals, idx, 4, F16)
    assert bits(got)[0, 0] == 0x8000
    assert np.isnan(got[1, 0])
    assert got[2, 0] == np.float16(60000.0)  # 120000 in fp32 on the way, no inf
    assert bits(got)[3, 0] == 0
    got = rows_sum_ref(vals[3:5], np.array([0, 0]), 1, F16)
    assert np.isinf(got[0, 0])
