"""The sparse row sum's definition in numpy, for the CPU and GPU tests.

    dense[j][:] = post * (e(x1) + e(x2) + ... + e(xk)),   e(x) = pre * x

x1 ... xk are the rows values[i][:] with indices[i] == j, in ascending position i (a stable argsort
by index; for p ranks the concatenation in rank order), folded left to right starting from the first
row itself, in the working type - float32 for F32 / F16 / BF16, float64 for F64, the integer type
for I32 / I64 - with every multiply and add a separate numpy operation (numpy's ufuncs round each
result: no fused multiply-add) and one rounding to the storage type at the end. With pre == post ==
1 nothing is multiplied. A row no entry names is +0; entries whose index is outside [0, rows) are
skipped. The rounding helpers are scaled_util's (bf16_round = kernels_device.h bf16_round_bits).
"""
import numpy as np

from gpu_util import BF16, F16, F32, F64, I32, I64, NPDT
from scaled_util import from_work, to_work, work_type

FLOATS = (F32, F64, F16, BF16)


def _work(values, dtype):
    if dtype in (I32, I64):
        return values.astype(NPDT[dtype])
    return to_work(values, dtype)


def rows_sum_ref(values, indices, rows, dtype, pre=1.0, post=1.0, reverse=False):
    """values [n, D] in the storage type (BF16 as uint16 bit patterns), indices [n] int64 ->
    dense [rows, D] in the storage type. reverse=True folds each row's entries from the last to
    the first (a different, equally deterministic order: what the definition is NOT)."""
    values = np.asarray(values)
    indices = np.asarray(indices, dtype=np.int64)
    n, D = values.shape
    assert indices.shape == (n,)
    scaled = not (pre == 1.0 and post == 1.0)
    assert not (scaled and dtype in (I32, I64))
    W = NPDT[dtype] if dtype in (I32, I64) else work_type(dtype)
    ids = np.nonzero((indices >= 0) & (indices < rows))[0]
    ids = ids[np.argsort(indices[ids], kind="stable")]
    row = indices[ids]
    acc = np.zeros((rows, D), dtype=W)
    if len(ids):
        start = np.r_[0, np.nonzero(row[1:] != row[:-1])[0] + 1]          # first position of each segment
        length = np.diff(np.r_[start, len(ids)])
        pos = np.arange(len(ids)) - np.repeat(start, length)               # position inside the segment
        if reverse:
            pos = np.repeat(length, length) - 1 - pos
        with np.errstate(all="ignore"):
            for k in range(int(length.max())):
                sel = pos == k
                x = _work(values[ids[sel]], dtype)
                if scaled:
                    x = x * W(pre)
                if k == 0:
                    acc[row[sel]] = x
                else:
                    acc[row[sel]] = acc[row[sel]] + x
            if scaled:
                named = row[start]
                acc[named] = acc[named] * W(post)
    if dtype in (I32, I64):
        return acc
    return from_work(acc, dtype)


def concat_ranks(parts):
    """[(values_r, indices_r)] in rank order -> the gathered (values, indices)."""
    return np.concatenate([v for v, _ in parts]), np.concatenate([i for _, i in parts])


def make_indices(pattern, n, rows, rng):
    """The index patterns the tests use; values in [0, rows)."""
    if n == 0:
        return np.zeros(0, np.int64)
    if pattern == "permutation":  # all unique while n <= rows, then wrapping round
        return (rng.permutation(max(n, rows))[:n] % rows).astype(np.int64)
    if pattern == "same":
        return np.full(n, min(7, rows - 1), np.int64)
    if pattern == "ascending":
        return np.sort(rng.integers(0, rows, n)).astype(np.int64)
    if pattern == "descending":
        return np.sort(rng.integers(0, rows, n))[::-1].astype(np.int64).copy()
    if pattern == "zipf":
        return ((rng.zipf(1.3, n) - 1) % rows).astype(np.int64)
    raise KeyError(pattern)


PATTERNS = ("permutation", "same", "ascending", "descending", "zipf")
