"""numpy restatement of the MXFP8 reduce-scatter (include/tips_hip.h, "MXFP8 reduce-scatter"; DESIGN.md
§19), built from mxfp8_util (quantize, dequantize_blocks, canonical) and reducescatter_util (rows_of,
slice_of).

- layout():  region q of a list - tips_fused_layout over the slices' element counts as FLOAT32 (the
             definition names that call; the counts come from the row split restated here).
- wire_of(): wire q of one rank - mxfp8_util.quantize of its slices q under that layout.
- fold():    the owner's result over flat positions: own values raw, every peer wire dequantised,
             ((y_0 + y_1) + ...) as numpy float32 adds, then one multiply by float32(factor) when it is not 1.
- shards():  rank q's outputs of a list, from all ranks' inputs.
"""
import numpy as np

import mxfp8_util as mx
import reducescatter_util as ru

F32 = 0


def slice_counts(rows, row_elems, p, q):
    return [ru.rows_of(r, p, q)[1] * e for r, e in zip(rows, row_elems)]


def layout(rows, row_elems, p, q):
    """(offsets, E) of region q in flat elements; an empty slice has offset 0."""
    from tips_amd import ops
    counts = slice_counts(rows, row_elems, p, q)
    if sum(counts) == 0:
        return [0] * len(counts), 0
    elems, offs = ops.mxfp8_flat_elems(counts)
    return [o if c else 0 for o, c in zip(offs, counts)], elems


def wire_of(ins, row_elems, p, q):
    """Wire q of a rank whose flat tensors are `ins`: the bytes tips_mxfp8_quantize gives for its slices q."""
    rows = [x.size // e if e else 0 for x, e in zip(ins, row_elems)]
    offs, elems = layout(rows, row_elems, p, q)
    return mx.quantize(mx.flat_of([ru.slice_of(x, e, p, q) for x, e in zip(ins, row_elems)], offs, elems))


def dequantized(wire, elems):
    """Every flat position of a wire buffer, factor 1, NaNs as they come (canonical at the end of fold)."""
    so = mx.scales_offset(elems)
    nb = -(-elems // mx.BLOCK)
    codes = np.zeros(nb * mx.BLOCK, np.uint8)
    codes[:min(so, nb * mx.BLOCK)] = wire[:min(so, nb * mx.BLOCK)]
    return mx.dequantize_blocks(codes.reshape(-1, mx.BLOCK), wire[so:so + nb]).reshape(-1)[:elems]


def fold(own, offs, wires, own_pos, elems, factor=1.0):
    """The outputs of the fold over a layout: own[i] (flat f32) at offs[i]; wires[j] a wire buffer for
    j != own_pos (wires[own_pos] is not looked at). One source: reducescatter_util's one-source fold."""
    return fold_dequantized(own, offs, [None if j == own_pos else dequantized(w, elems) for j, w in enumerate(wires)],
                            own_pos, factor)


def fold_dequantized(own, offs, ys, own_pos, factor=1.0):
    """fold() over the peers' dequantised flat arrays ys[j] (ys[own_pos] is not looked at)."""
    nsrc = len(ys)
    if nsrc == 1:
        return [ru.fold([np.ascontiguousarray(x, np.float32)], F32, ru.SUM, 1.0, float(factor)) for x in own]
    outs = []
    with np.errstate(all="ignore"):
        for x, o in zip(own, offs):
            x = np.ascontiguousarray(x, np.float32).reshape(-1)
            acc = None
            for j in range(nsrc):
                y = x if j == own_pos else ys[j][o:o + x.size]
                acc = y.copy() if acc is None else (acc + y).astype(np.float32)
            if float(np.float32(factor)) != 1.0:
                acc = (acc * np.float32(factor)).astype(np.float32)
            outs.append(mx.canonical(acc))
    return outs


def shards(ins_per_rank, row_elems, q, factor=1.0):
    """Rank q's outputs: ins_per_rank[r][i] is rank r's flat f32 tensor i."""
    p = len(ins_per_rank)
    rows = [x.size // e if e else 0 for x, e in zip(ins_per_rank[0], row_elems)]
    offs, elems = layout(rows, row_elems, p, q)
    own = [ru.slice_of(x, e, p, q) for x, e in zip(ins_per_rank[q], row_elems)]
    wires = [None if r == q else wire_of(ins_per_rank[r], row_elems, p, q) for r in range(p)]
    return fold(own, offs, wires, q, elems, factor)
