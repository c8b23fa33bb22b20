"""The reduce-scatter's definitions in numpy, for the CPU and GPU tests.

- rows_of():   the row split - rank q of p owns base + (q < rem) rows from row q * base + min(q, rem).
- layout():    region q of a list - every tensor's slice q in list order, each non-empty slice at the
               next multiple of 256 bytes, empty slices taking no space.
- fold():      the result of a segment from its sources in rank order: edge_values.fold_ref /
               scaled_util's definition for SUM (plain or with factors), minmax_util.ref for MAX / MIN;
               one plain source is the copy.
- shards():    every rank's result of a list, from all ranks' inputs.
"""
import hashlib

import numpy as np

import edge_values as ev
import minmax_util as mm
from gpu_util import NPDT

SUM, MAX, MIN = 0, 1, 2
ALIGN = 256


def rows_of(rows, p, q):
    """(first row, rows) of rank q."""
    base, rem = divmod(rows, p)
    return q * base + min(q, rem), base + (1 if q < rem else 0)


def layout(rows, row_elems, es, p, q):
    """(offsets, bytes) of region q: offsets[i] is where tensor i's slice starts (for an empty slice:
    where the next one will), bytes reaches to the last slice's last byte."""
    offs, nxt, end = [], 0, 0
    for r, e in zip(rows, row_elems):
        b = rows_of(r, p, q)[1] * e * es
        offs.append(nxt)
        if b > 0:
            end = nxt + b
            nxt = -(-end // ALIGN) * ALIGN
    return offs, end


def fold(srcs, dtype, op=SUM, pre=1.0, post=1.0):
    if len(srcs) == 1 and pre == 1.0 and post == 1.0:
        return np.array(srcs[0], copy=True)  # one source, nothing to scale: the copy (MAX / MIN alike)
    if op == SUM:
        return ev.fold_ref(list(srcs), dtype, pre, post)
    return mm.ref(list(srcs), dtype, op)


def same(got, exp, dtype):
    """The project's bit rule (gpu_util.same_bits): the same bits, any NaN matching any NaN."""
    got, exp = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(exp).reshape(-1)
    return got.shape == exp.shape and ev.differing(got, exp, dtype).size == 0


def slice_of(x, row_elems, p, q):
    """Rank q's slice of the flat array x of a [rows, row_elems] tensor."""
    rows = x.size // row_elems if row_elems else 0
    b, k = rows_of(rows, p, q)
    return x[b * row_elems:(b + k) * row_elems]


def shards(ins, row_elems, dtype, q, op=SUM, pre=1.0, post=1.0):
    """Rank q's outputs: ins[r][i] is rank r's flat tensor i."""
    p = len(ins)
    return [fold([slice_of(ins[r][i], e, p, q) for r in range(p)], dtype, op, pre, post) for i, e in enumerate(row_elems)]


def sha1_of(arrays, dtype):
    """One digest of a list of results; every NaN counts as the quiet NaN (payloads are no part of the contract)."""
    h = hashlib.sha1()
    for a in arrays:
        a = np.array(a, copy=True).reshape(-1)
        if dtype in ev.FLOAT_DTYPES:
            b = ev.to_bits(a, dtype)
            b[ev.is_nan(a, dtype)] = ev.special_bits(dtype)[13]
        h.update(a.tobytes())
    return h.hexdigest()


def inputs(dtype, n, seed, r):
    """Rank r's flat input of n elements for a case seed: random bits, NaN patterns included."""
    if dtype in ev.FLOAT_DTYPES:
        return ev.from_bits(ev.random_bits(dtype, n, ev.rng_for(77, seed, r)), dtype)
    info = np.iinfo(NPDT[dtype])
    return ev.rng_for(77, seed, r).integers(info.min, info.max, size=n, dtype=NPDT[dtype], endpoint=True)
