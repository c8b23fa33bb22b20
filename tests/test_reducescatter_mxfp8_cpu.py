"""The MXFP8 reduce-scatter without a device: tips_reducescatter_mxfp8_layout against the
restatement (tests/reducescatter_mxfp8_util.py), the argument refusals of the four entries that return
before anything touches the device, the Python ValueErrors raised before any init, and the
definition's error bound and its advantage over the slice of the MXFP8 allreduce, on the restatement."""
import math

import numpy as np
import pytest

import mxfp8_util as mx
import reducescatter_mxfp8_util as rmx
import reducescatter_util as ru
from tips_amd import _lib

INVALID, NOT_INIT, UNSUPPORTED = -1, -2, -5
RANKS = [1, 2, 3, 8, 16]


def c_layout(rows, elems, p, q, want_offsets=True):
    pr, _k1 = _lib.i64_array(rows)
    pe, _k2 = _lib.i64_array(elems)
    offs = np.full(len(rows), -1, dtype=np.int64)
    total = _lib.lib().tips_reducescatter_mxfp8_layout(pr, pe, len(rows), p, q,
                                                       offs.ctypes.data_as(_lib._c_i64_p) if want_offsets else None)
    return offs.tolist(), total


def check_region(rows, elems, p, q):
    offs, total = c_layout(rows, elems, p, q)
    eoffs, etotal = rmx.layout(rows, elems, p, q)
    assert (offs, total) == (eoffs, etotal), (rows, elems, p, q)
    assert c_layout(rows, elems, p, q, want_offsets=False)[1] == total
    # what the definition promises of it: non-empty slices in list order on multiples of 64 elements,
    # none overlapping, all inside E; empty slices take no space
    end = 0
    for o, c in zip(offs, rmx.slice_counts(rows, elems, p, q)):
        if c == 0:
            assert o == 0
            continue
        assert o % 64 == 0 and o == -(-end // 64) * 64
        end = o + c
    assert total >= end and total % 64 == 0 and (end > 0 or total == 0)
    return total


@pytest.mark.parametrize("p", RANKS)
def test_layout_single_tensors(p):
    for rows in sorted({0, 1, p - 1, p, p + 1, 4099}):
        for e in (1, 33, 64):
            sizes = [check_region([rows], [e], p, q) for q in range(p)]
            assert sizes[0] == max(sizes)
            own = [ru.rows_of(rows, p, q)[1] * e for q in range(p)]
            assert [s == 0 for s in sizes] == [c == 0 for c in own]


LIST_ROWS = [0, 5, 1, 4099, 0, 17, 2, 64, 3, 1]
LIST_ELEMS = [33, 1, 128, 33, 1, 128, 1, 33, 0, 7]


@pytest.mark.parametrize("p", RANKS)
def test_layout_lists_with_empty_slices(p):
    for q in range(p):
        check_region(LIST_ROWS, LIST_ELEMS, p, q)
        check_region([p - 1, 1, 0], [7, 5, 3], p, q)  # the last ranks own nothing of any tensor
    if p > 1:
        assert c_layout([p - 1, 1, 0], [7, 5, 3], p, p - 1) == ([0, 0, 0], 0)


def test_layout_refusals():
    L = _lib.lib()
    pr, _k1 = _lib.i64_array([4, 4])
    pe, _k2 = _lib.i64_array([1, 1])
    neg, _k3 = _lib.i64_array([4, -4])
    assert L.tips_reducescatter_mxfp8_layout(None, pe, 2, 2, 0, None) == INVALID
    assert L.tips_reducescatter_mxfp8_layout(pr, None, 2, 2, 0, None) == INVALID
    assert L.tips_reducescatter_mxfp8_layout(neg, pe, 2, 2, 0, None) == INVALID
    assert L.tips_reducescatter_mxfp8_layout(pr, neg, 2, 2, 0, None) == INVALID
    assert L.tips_reducescatter_mxfp8_layout(pr, pe, 2, 2, 2, None) == INVALID
    assert L.tips_reducescatter_mxfp8_layout(pr, pe, 2, 2, -1, None) == INVALID
    assert L.tips_reducescatter_mxfp8_layout(pr, pe, 2, 0, 0, None) == INVALID
    assert L.tips_reducescatter_mxfp8_layout(pr, pe, -1, 2, 0, None) == INVALID
    assert L.tips_reducescatter_mxfp8_layout(pr, pe, 0, 2, 0, None) == 0


def fold_rc(n=2, nsrc=2, own_pos=0, factor=1.0, counts=(4, 4), outs=(0x10000, 0x20000), own=(0x30000, 0x40000),
            wires=(0x50000, 0x60000)):
    """tips_reducescatter_mxfp8_fold with made-up, never dereferenced addresses."""
    po, _k1 = _lib.ptr_array(list(outs)) if outs is not None else (None, None)
    pw, _k2 = _lib.ptr_array(list(own)) if own is not None else (None, None)
    pc, _k3 = _lib.i64_array(list(counts))
    ps, _k4 = _lib.ptr_array(list(wires)) if wires is not None else (None, None)
    return _lib.lib().tips_reducescatter_mxfp8_fold(po, pw, pc, n, ps, nsrc, own_pos, factor, None)


def test_fold_refusals_before_the_device():
    assert not _lib.lib().tips_is_initialize()
    assert fold_rc(nsrc=0) == INVALID and "nsrc" in _lib.last_error()
    assert fold_rc(nsrc=17, wires=tuple(0x50000 + 0x1000 * j for j in range(17))) == INVALID and "nsrc" in _lib.last_error()
    assert fold_rc(own_pos=2) == INVALID and "own_pos" in _lib.last_error()
    assert fold_rc(own_pos=-1) == INVALID
    assert fold_rc(counts=(4, -4)) == INVALID
    assert fold_rc(n=-1) == INVALID
    assert fold_rc(outs=None) == INVALID
    assert fold_rc(own=None) == INVALID
    assert fold_rc(wires=None) == INVALID
    assert fold_rc(outs=(0x10000, 0)) == INVALID          # a null pointer of a non-empty tensor
    assert fold_rc(own=(0, 0x40000)) == INVALID
    assert fold_rc(outs=(0x10002, 0x20000)) == INVALID and "4-B" in _lib.last_error()
    assert fold_rc(own=(0x30000, 0x40001)) == INVALID
    assert fold_rc(wires=(0, 0x60008)) == INVALID and "16-B" in _lib.last_error()
    assert fold_rc(wires=(0, 0)) == INVALID               # a null wire that is not the own position's
    assert fold_rc(factor=math.nan) == INVALID and "factor" in _lib.last_error()
    assert fold_rc(factor=math.inf) == INVALID
    assert fold_rc(factor=1e300) == INVALID               # finite, but no finite float
    assert fold_rc(counts=(0, 0)) == 0                    # nothing to do: returns before any pointer is looked at
    assert fold_rc(counts=(0, 0), outs=(0, 0), own=(0, 0)) == 0  # an empty tensor's pointer may be null
    assert fold_rc(n=0, nsrc=1, wires=None, counts=(0,)) == 0


def collective_rcs(rows=(4,), elems=(1,), factor=1.0, ins=True, outs=True):
    """Both collectives with made-up addresses, in a process that never called tips_init."""
    L = _lib.lib()
    n = len(rows)
    pi, _k1 = _lib.ptr_array([0x10000 + 0x1000 * i for i in range(n)])
    po, _k2 = _lib.ptr_array([0x80000 + 0x1000 * i for i in range(n)])
    pr, _k3 = _lib.i64_array(list(rows))
    pe, _k4 = _lib.i64_array(list(elems))
    rcs = [L.tips_grouped_reducescatter_mxfp8(pi if ins else None, po if outs else None, pr, pe, n, factor, None)]
    if n == 1 and ins and outs:
        rcs.append(L.tips_reducescatter_mxfp8(0x10000, 0x80000, rows[0], elems[0], factor, None))
    return rcs


def test_collective_refusals_before_the_device():
    assert not _lib.lib().tips_is_initialize()
    assert set(collective_rcs(ins=False)) == {INVALID}
    assert set(collective_rcs(outs=False)) == {INVALID}
    assert set(collective_rcs(rows=(-4,))) == {INVALID}
    assert set(collective_rcs(elems=(-1,))) == {INVALID}
    assert set(collective_rcs(rows=(2**40,), elems=(2**40,))) == {INVALID}
    assert set(collective_rcs(factor=math.nan)) == {INVALID}
    assert set(collective_rcs(factor=-math.inf)) == {INVALID}
    L = _lib.lib()
    pe, _k = _lib.i64_array([1, 1])
    assert L.tips_grouped_reducescatter_mxfp8(None, None, None, pe, 2, 1.0, None) == INVALID  # null rows
    assert set(collective_rcs()) == {NOT_INIT}  # nothing to refuse: the call needs tips_init
    assert "tips_init" in _lib.last_error()


def test_python_value_errors_before_init():
    import torch

    import tips_amd as tips
    assert "reducescatter_mxfp8_layout" in tips.__all__ and "mxfp8_fold_segs" in tips.__all__
    t = torch.zeros(4, 3)
    fp8 = tips.Compression.fp8
    for kw in [dict(op=tips.Max, compression=fp8), dict(op=tips.Min, compression=fp8),
               dict(op=tips.Sum, compression=fp8.error_feedback()), dict(op=tips.Average, compression=tips.MXFP8ErrorFeedback()),
               dict(op=tips.Adasum, compression=fp8), dict(op=tips.Sum, compression=fp8, name="grad"),
               dict(op=tips.Sum, compression=tips.Compression.fp16, name="grad")]:
        with pytest.raises(ValueError):
            tips.reducescatter(t, **kw)
        with pytest.raises(ValueError):
            tips.grouped_reducescatter([t, None], **kw)
    with pytest.raises(ValueError, match="feedback"):
        tips.reducescatter(t, compression=fp8.error_feedback())
    for comp in (fp8, tips.Compression.fp16, tips.Compression.none):  # a host tensor stays refused under every compressor
        with pytest.raises(ValueError):
            tips.reducescatter(t, op=tips.Sum, compression=comp)
        with pytest.raises(ValueError):
            tips.reducescatter(torch.zeros(()), op=tips.Sum, compression=comp)
    assert tips.reducescatter_mxfp8_layout([5, 0, 3], [7, 4, 64], 2, 1) == tuple(reversed(rmx.layout([5, 0, 3], [7, 4, 64], 2, 1)))
    assert not tips.is_initialized()


# ---- the definition's accuracy, on the restatement ----

# A row is a multiple of the block, so the blocks of a slice are blocks of the whole tensor. Both tests
# below look at a maximum over a shard, which settles only over many blocks per magnitude: with 5p + 1
# rows of 6144 elements a shard holds 960 blocks and more, and the restatement's worst error reaches
# 0.93 - 0.94 of the bound, the figure the definition was checked at (0.93 - 0.96). At 96 elements a
# row (15 blocks a shard) it reaches 0.90 - 0.94 and the second test's comparison is decided by single
# elements: see its docstring.
ROW = 6144


def spread_inputs(p, seed):
    """p ranks' tensors [5p + 1, 6144] whose per-block magnitudes are spread over 2^-20 ... 2^20."""
    n = (5 * p + 1) * ROW
    return [mx.spread_blocks(n, np.random.default_rng([19, seed, p, r]), lo=-20, hi=20) for r in range(p)]


@pytest.mark.parametrize("p", [2, 3, 8, 16])
def test_error_bound(p):
    """|out - SUM x_r| <= SUM_{r != q} amax_{r,b} / 16 + (p - 1) 2^-24 SUM_r (|x_r| + [r != q] amax_{r,b} / 16): the scaled
    block maximum lies in (224, 448], so a code is within amax / 16 of its value, and the fold adds p - 1 f32 roundings."""
    worst = 0.0
    for seed in range(3):
        xs = spread_inputs(p, seed)
        x64 = np.stack(xs).astype(np.float64)
        amax = np.repeat(np.abs(x64).reshape(p, -1, mx.BLOCK).max(axis=2), mx.BLOCK, axis=1)
        for q in range(p):
            out = rmx.shards([[x] for x in xs], [ROW], q)[0].astype(np.float64)
            sl = lambda a: ru.slice_of(a, ROW, p, q)  # noqa: E731
            peers = [r for r in range(p) if r != q]
            exact = sum(sl(x64[r]) for r in range(p))
            quant = sum(sl(amax[r]) for r in peers) / 16.0
            bound = quant + (p - 1) * 2.0 ** -24 * (sum(np.abs(sl(x64[r])) for r in range(p)) + quant)
            err = np.abs(out - exact)
            assert (err <= bound).all(), (p, seed, q, float((err / bound).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("p %d: worst error / bound %.4f" % (p, worst))


@pytest.mark.parametrize("p", [2, 3, 8, 16])
def test_never_further_from_the_sum_than_the_allreduce_slice(p):
    """The maximum error over every shard is at most that of the same rows of mxfp8_util.collective (every
    value quantised twice, the owner's included). Every (seed, shard) that misses is reported.

    It is a statement about maxima, not a theorem about every input: the maximum over a shard is one
    element's error, and the allreduce's second quantisation sometimes cancels part of the first. On
    these inputs (seeds 0 - 2, shards of 960 blocks and more) it holds for every shard, the ratio of the
    two maxima having mean 0.60 - 0.67. On shorter shards it misses now and then and was seen to: rows
    of 96 elements (15 blocks a shard) miss for p 3 (seeds 1, 2; ratio up to 1.02), p 8 (seeds 0, 1, 2;
    up to 1.18) and p 16 (seed 1; 1.09), e.g. p 8 seed 1 shard 1: 34649.9 against 30469.8; rows of 1536
    elements miss once in seeds 0 - 2 (p 16, seed 0, shard 12: ratio 1.05)."""
    from tips_amd import ops
    missed, ratios = [], []
    for seed in range(3):
        xs = spread_inputs(p, seed)
        n = xs[0].size
        elems, offs = ops.mxfp8_flat_elems([n])
        whole = mx.collective([mx.flat_of([x], offs, elems) for x in xs])[offs[0]:offs[0] + n].astype(np.float64)
        exact = np.stack(xs).astype(np.float64).sum(axis=0)
        for q in range(p):
            out = rmx.shards([[x] for x in xs], [ROW], q)[0].astype(np.float64)
            mine = float(np.abs(out - ru.slice_of(exact, ROW, p, q)).max())
            theirs = float(np.abs(ru.slice_of(whole, ROW, p, q) - ru.slice_of(exact, ROW, p, q)).max())
            ratios.append(mine / theirs)
            if mine > theirs:
                missed.append("seed %d, shard %d: %.6g against the allreduce slice's %.6g" % (seed, q, mine, theirs))
    print("p %d: own error / allreduce slice's error: mean %.3f, largest %.3f" % (p, float(np.mean(ratios)), max(ratios)))
    assert not missed, "p %d: %s" % (p, "; ".join(missed))
