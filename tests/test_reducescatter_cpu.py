"""The reduce-scatter without a device: the two pure-host layout calls against the numpy
restatement (tests/reducescatter_util.py), the argument refusals of the three device entries that
return before anything touches the device, and the Python ValueErrors raised before any init."""
import ctypes
import math

import numpy as np
import pytest

import reducescatter_util as ru
from gpu_util import ALL_DTYPES, F32, I32, NPDT
from tips_amd import _lib

INVALID, NOT_INIT, UNSUPPORTED = -1, -2, -5
RANKS = [1, 2, 3, 8, 16]


def rows_cases(p):
    return sorted({0, 1, max(p - 1, 0), p, p + 1, 4099, 2**40 + 3})


def c_rows(rows, p, q):
    begin = ctypes.c_int64(-1)
    own = _lib.lib().tips_reducescatter_rows(rows, p, q, ctypes.byref(begin))
    return begin.value, own


@pytest.mark.parametrize("p", RANKS)
def test_rows_match_the_restatement_and_tile_the_tensor(p):
    L = _lib.lib()
    for rows in rows_cases(p):
        nxt, prev = 0, None
        for q in range(p):
            b, k = c_rows(rows, p, q)
            assert (b, k) == ru.rows_of(rows, p, q), (rows, p, q)
            assert b == nxt and k >= 0  # in order, nothing skipped
            assert prev is None or prev - 1 <= k <= prev  # never more than the rank before, by at most 1
            nxt, prev = b + k, k
            assert L.tips_reducescatter_rows(rows, p, q, None) == k  # begin may be null
        assert nxt == rows
        assert c_rows(rows, p, 0)[1] - c_rows(rows, p, p - 1)[1] <= 1


def test_rows_refusals():
    L = _lib.lib()
    for rows, p, q in [(-1, 2, 0), (4, 0, 0), (4, 2, 2), (4, 2, -1)]:
        assert L.tips_reducescatter_rows(rows, p, q, None) == INVALID


LIST_ROWS = [0, 5, 1, 4099, 0, 17, 2, 64, 3]
LIST_ELEMS = [33, 1, 128, 33, 1, 128, 1, 33, 0]


def c_layout(rows, elems, dtype, p, q, want_offsets=True):
    pr, _k1 = _lib.i64_array(rows)
    pe, _k2 = _lib.i64_array(elems)
    offs = np.full(len(rows), -1, dtype=np.int64)
    total = _lib.lib().tips_reducescatter_layout(pr, pe, len(rows), dtype, p, q,
                                                 offs.ctypes.data_as(_lib._c_i64_p) if want_offsets else None)
    return offs.tolist(), total


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("p", RANKS)
def test_layout_matches_the_restatement(dtype, p):
    es = np.dtype(NPDT[dtype]).itemsize
    sizes = []
    for q in range(p):
        offs, total = c_layout(LIST_ROWS, LIST_ELEMS, dtype, p, q)
        eoffs, etotal = ru.layout(LIST_ROWS, LIST_ELEMS, es, p, q)
        assert (offs, total) == (eoffs, etotal), (p, q)
        assert c_layout(LIST_ROWS, LIST_ELEMS, dtype, p, q, want_offsets=False)[1] == total
        assert all(o % 256 == 0 for o in offs)
        end = 0
        for i, (r, e) in enumerate(zip(LIST_ROWS, LIST_ELEMS)):
            b = ru.rows_of(r, p, q)[1] * e * es
            if b == 0:
                continue  # takes no space: the next non-empty slice starts where this one would have
            assert offs[i] == -(-end // 256) * 256
            end = offs[i] + b
        assert total == end
        sizes.append(total)
    assert sizes[0] == max(sizes)  # region 0 is the largest: it sizes the staged slots


def test_layout_refusals():
    L = _lib.lib()
    pr, _k1 = _lib.i64_array([4, 4])
    pe, _k2 = _lib.i64_array([1, 1])
    neg, _k3 = _lib.i64_array([4, -4])
    assert L.tips_reducescatter_layout(None, pe, 2, F32, 2, 0, None) == INVALID
    assert L.tips_reducescatter_layout(pr, None, 2, F32, 2, 0, None) == INVALID
    assert L.tips_reducescatter_layout(neg, pe, 2, F32, 2, 0, None) == INVALID
    assert L.tips_reducescatter_layout(pr, neg, 2, F32, 2, 0, None) == INVALID
    assert L.tips_reducescatter_layout(pr, pe, 2, 99, 2, 0, None) == INVALID
    assert L.tips_reducescatter_layout(pr, pe, 2, F32, 2, 2, None) == INVALID
    assert L.tips_reducescatter_layout(pr, pe, 2, F32, 0, 0, None) == INVALID
    assert L.tips_reducescatter_layout(pr, pe, 0, F32, 2, 0, None) == 0


def fold_rc(n=2, nsrc=2, own_pos=0, dtype=F32, op=0, pre=1.0, post=1.0, offsets=(0, 256), counts=(4, 4), outs=True,
            own=True, stages=True):
    """tips_reducescatter_fold with made-up, never dereferenced addresses."""
    po, _k1 = _lib.ptr_array([0x10000, 0x20000][:n] or [0])
    pw, _k2 = _lib.ptr_array([0x30000, 0x40000][:n] or [0])
    pc, _k3 = _lib.i64_array(list(counts))
    pf, _k4 = _lib.i64_array(list(offsets))
    ps, _k5 = _lib.ptr_array([0x50000 + 0x1000 * j for j in range(max(nsrc, 1))])
    return _lib.lib().tips_reducescatter_fold(po if outs else None, pw if own else None, pc, pf, n, ps if stages else None,
                                              nsrc, own_pos, dtype, op, pre, post, None)


def test_fold_refusals_before_the_device():
    assert fold_rc(outs=False) == INVALID
    assert fold_rc(own=False) == INVALID
    assert fold_rc(stages=False) == INVALID
    assert fold_rc(counts=(4, -4)) == INVALID
    assert fold_rc(n=-1) == INVALID
    assert fold_rc(nsrc=0) == INVALID and "nsrc" in _lib.last_error()
    assert fold_rc(nsrc=17) == INVALID and "nsrc" in _lib.last_error()
    assert fold_rc(own_pos=2) == INVALID and "own_pos" in _lib.last_error()
    assert fold_rc(own_pos=-1) == INVALID
    assert fold_rc(offsets=(0, 128)) == INVALID and "multiple" in _lib.last_error()
    assert fold_rc(offsets=(256, 0)) == INVALID  # do not ascend
    assert fold_rc(offsets=(0, 0)) == INVALID    # overlap
    assert fold_rc(op=3) == INVALID
    assert fold_rc(dtype=42) == INVALID
    assert fold_rc(dtype=I32, pre=0.5) == UNSUPPORTED
    assert fold_rc(pre=math.nan) == INVALID
    assert fold_rc(post=math.inf) == INVALID
    assert fold_rc(op=1, post=0.5) == INVALID  # no scaled MAX
    assert fold_rc(counts=(0, 0)) == 0  # nothing to do: returns before any pointer is looked at


def collective_rcs(rows=(4,), elems=(1,), dtype=F32, op=0, pre=1.0, post=1.0, ins=True, outs=True):
    """Both collectives with made-up addresses, in a process that never called tips_init."""
    L = _lib.lib()
    n = len(rows)
    pi, _k1 = _lib.ptr_array([0x10000 + 0x1000 * i for i in range(n)])
    po, _k2 = _lib.ptr_array([0x80000 + 0x1000 * i for i in range(n)])
    pr, _k3 = _lib.i64_array(list(rows))
    pe, _k4 = _lib.i64_array(list(elems))
    rcs = [L.tips_grouped_reducescatter(pi if ins else None, po if outs else None, pr, pe, n, dtype, op, pre, post, None)]
    if n == 1 and ins and outs:
        rcs.append(L.tips_reducescatter(0x10000, 0x80000, rows[0], elems[0], dtype, op, pre, post, None))
    return rcs


def test_collective_refusals_before_the_device():
    assert not _lib.lib().tips_is_initialize()
    assert set(collective_rcs(ins=False)) == {INVALID}
    assert set(collective_rcs(outs=False)) == {INVALID}
    assert set(collective_rcs(rows=(-4,))) == {INVALID}
    assert set(collective_rcs(elems=(-1,))) == {INVALID}
    assert set(collective_rcs(op=3)) == {INVALID}
    assert set(collective_rcs(dtype=17)) == {INVALID}
    assert set(collective_rcs(dtype=I32, post=0.5)) == {UNSUPPORTED}
    assert set(collective_rcs(pre=math.nan)) == {INVALID}
    assert set(collective_rcs(op=2, pre=2.0)) == {INVALID}
    L = _lib.lib()
    pe, _k = _lib.i64_array([1, 1])
    assert L.tips_grouped_reducescatter(None, None, None, pe, 2, F32, 0, 1.0, 1.0, None) == INVALID  # null rows
    assert set(collective_rcs()) == {NOT_INIT}  # nothing to refuse: the call needs tips_init
    assert "tips_init" in _lib.last_error()


def test_python_value_errors_before_init():
    import torch

    import tips_amd as tips
    assert "reducescatter" in tips.__all__ and "grouped_reducescatter" in tips.__all__
    host = torch.zeros(4, 3)
    meta_f = torch.zeros(4, 3, device="meta")  # (is_cuda is False: refused as a host tensor, nothing is touched)
    for bad in [torch.zeros(()), host, meta_f, host.to_sparse(), np.zeros((4, 3), np.float32)]:
        with pytest.raises(ValueError):
            tips.reducescatter(bad, op=tips.Sum)
        with pytest.raises(ValueError):
            tips.grouped_reducescatter([None, bad], op=tips.Sum)

    # the checks on op, factors and name come before any tensor is looked at or anything is initialised
    t = host
    for kw in [dict(op=tips.Adasum), dict(op="Product"), dict(op=tips.Max, prescale_factor=2.0),
               dict(op=tips.Min, postscale_factor=0.5), dict(op=tips.Sum, name="grad")]:
        with pytest.raises(ValueError):
            tips.reducescatter(t, **kw)
        with pytest.raises(ValueError):
            tips.grouped_reducescatter([t], **kw)
    assert not tips.is_initialized()


def test_python_integer_refusals_before_init():
    """An integer tensor with Average or a factor: refused by its dtype, before the tensor's place is looked at."""
    import torch

    import tips_amd as tips
    ints = torch.zeros(4, 3, dtype=torch.int32)
    for kw in [dict(op=tips.Average), dict(), dict(op=tips.Sum, prescale_factor=0.5), dict(op=tips.Sum, postscale_factor=2.0)]:
        with pytest.raises(ValueError, match="integer"):
            tips.reducescatter(ints, **kw)
        with pytest.raises(ValueError, match="integer"):
            tips.grouped_reducescatter([ints.to(torch.int64), None], **kw)
    with pytest.raises(ValueError, match="device"):  # the plain integer sum passes that check and is refused as a host tensor
        tips.reducescatter(ints, op=tips.Sum)
    assert not tips.is_initialized()
