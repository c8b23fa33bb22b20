"""numpy restatement of the MXFP8 wire's error feedback (include/tips_hip.h, "MXFP8 error feedback";
DESIGN.md §17): quantise with feedback, fold with feedback and the collective, over the plain wire's
restatement (tests/mxfp8_util.py: quantize_blocks, dequantize_blocks, fold_acc, dequantize). The add
c = x + r and the subtract r' = c - y are numpy float32 operations (IEEE, one rounding each). No
dependency on the library: a list's offsets and the rank count are arguments."""
import numpy as np

import mxfp8_util as mx

BLOCK = mx.BLOCK


def chunk_of(nblocks, p, q, align=8):
    """Blocks [b, e) of chunk q of p: per = round_up(ceil(nblocks / p), align) blocks each, the last ones shorter or empty."""
    per = mx.round_up(-(-nblocks // p), align)
    b = min(q * per, nblocks)
    return b, min(b + per, nblocks)


def ef_elems(elems, p):
    """f32 elements of the state: the sender residual, then the owner residual of the largest chunk (chunk 0)."""
    b, e = chunk_of(-(-elems // BLOCK), p, 0)
    return mx.scales_offset(elems) + (BLOCK * (e - b) if p > 1 else 0)


def ef_bytes(elems, p):
    return 4 * ef_elems(elems, p)


def mask_of(counts, offsets, elems):
    """bool [round_up(E, 256)]: the flat positions that hold a tensor element."""
    m = np.zeros(mx.scales_offset(elems), bool)
    for n, o in zip(counts, offsets):
        m[o:o + n] = True
    return m


def quantize_blocks_ef(x, r, mask):
    """x, r: f32 [nblocks, 32]; mask: bool [nblocks, 32], the positions that hold a tensor element.
    -> (codes, scale bytes, the new residual): c = x + r where mask, +0 elsewhere; c quantised;
    r' = c - y where mask (+0 over a poisoned block), r untouched elsewhere."""
    x = np.ascontiguousarray(x, np.float32)
    r = np.ascontiguousarray(r, np.float32)
    with np.errstate(all="ignore"):
        c = np.where(mask, (x + r).astype(np.float32), np.float32(0)).astype(np.float32)
        codes, sb = mx.quantize_blocks(c)
        y = mx.dequantize_blocks(codes, sb)
        rn = (c - y).astype(np.float32)
    rn[sb == 0xFF] = np.float32(0)
    return codes, sb, np.where(mask, rn, r).astype(np.float32)


def quantize_ef(flat, mask, residual):
    """flat f32 [E], mask bool [round_up(E, 256)], residual f32 [round_up(E, 256)] -> (the wire buffer, the new residual)."""
    elems = flat.size
    so = mx.scales_offset(elems)
    x = np.zeros(so, np.float32)
    x[:elems] = flat
    codes, sb, rn = quantize_blocks_ef(x.reshape(-1, BLOCK), np.asarray(residual, np.float32)[:so].reshape(-1, BLOCK),
                                       np.asarray(mask, bool)[:so].reshape(-1, BLOCK))
    wire = np.zeros(mx.wire_bytes(elems), np.uint8)
    wire[:so] = codes.reshape(-1)
    wire[so:so + sb.size] = sb
    return wire, rn.reshape(-1)


def fold_ef(dst, wires, elems, begin, count, residual):
    """dst (copied) with blocks [begin, begin + count) = quantise(fold of the wires + residual), and the
    new residual f32 [32 * count]: every position of a block alike."""
    out = dst.copy()
    o = np.asarray(residual, np.float32)[:BLOCK * count].copy()
    if count:
        so = mx.scales_offset(elems)
        with np.errstate(all="ignore"):
            c = (mx.fold_acc(wires, elems, begin, count) + o.reshape(-1, BLOCK)).astype(np.float32)
            codes, sb = mx.quantize_blocks(c)
            on = (c - mx.dequantize_blocks(codes, sb)).astype(np.float32)
        on[sb == 0xFF] = np.float32(0)
        out[begin * BLOCK:(begin + count) * BLOCK] = codes.reshape(-1)
        out[so + begin:so + begin + count] = sb
        o = on.reshape(-1)
    return out, o


def collective_ef(flats, states, factor=1.0, mask=None):
    """One step over ranks 0 ... p-1. flats: f32 [E] per rank; states: f32 [ef_elems(E, p)] per rank
    (sender residual, then the rank's owner residual); mask: the tensor positions (default: all of
    [0, E)). -> (the output, flat f32 [E], the same on every rank; the new states)."""
    p, elems = len(flats), flats[0].size
    so = mx.scales_offset(elems)
    if mask is None:
        mask = np.arange(so) < elems
    new = [np.asarray(s, np.float32).copy() for s in states]
    wires = []
    for r in range(p):
        assert new[r].size == ef_elems(elems, p)
        w, new[r][:so] = quantize_ef(flats[r], mask, new[r][:so])
        wires.append(w)
    if p == 1:
        return mx.dequantize(wires[0], elems, factor), new
    nb = -(-elems // BLOCK)
    reduced = np.zeros(mx.wire_bytes(elems), np.uint8)
    for q in range(p):  # rank q owns chunk q; an empty chunk leaves its owner residual alone
        b, e = chunk_of(nb, p, q)
        if e > b:
            reduced, new[q][so:so + BLOCK * (e - b)] = fold_ef(reduced, wires, elems, b, e - b, new[q][so:so + BLOCK * (e - b)])
    return mx.dequantize(reduced, elems, factor), new
