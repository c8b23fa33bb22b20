"""The scaled allreduce's definition in numpy (Scaled allreduce), for the CPU and GPU tests.

result = post * SUM_r (pre * x_r). Everything runs in the working type W - float32 for F32, F16
and BF16, float64 for F64 - into which the factors are converted once; every multiply and every
add is a separate numpy operation (numpy's ufuncs round each result: no fused multiply-add), and
a sum rounds to the storage type once, when it stores.

- scaled_sum():  one sum kernel: sources in order, raw ones multiplied by pre, the sum by post.
- interpret():   plan_util.interpret with that arithmetic. The plan dump does not say which sources
  are raw or which sum is the last, so every buffer carries, per element, how many ranks' inputs
  it has absorbed: an input element counts 1, a transfer carries the count along, a sum's output
  counts the sum of its sources'. A source is raw at count 1; a sum is finished at count p.
- ring_closed_form() / fold_closed_form(): what the schedules must compute, written without plans.
"""
import numpy as np

from gpu_util import BF16, F16, F32, F64, NPDT
from plan_util import IN, STG

FLOAT_DTYPES = [F32, F64, F16, BF16]


def work_type(dtype):
    return np.float64 if dtype == F64 else np.float32


def to_work(a, dtype):
    if dtype == BF16:
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(work_type(dtype))


def bf16_round(w):
    """kernels_device.h bf16_round_bits on a float32 array (round to nearest even, NaNs kept quiet)."""
    x = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (x & 0x7fffffff) > 0x7f800000
    r = (x + 0x7fff + ((x >> 16) & 1)) >> 16
    return np.where(nan, (x >> 16) | 0x40, r).astype(np.uint16)


def from_work(w, dtype):
    """The one rounding to the storage type."""
    if dtype == BF16:
        return bf16_round(w)
    with np.errstate(over="ignore"):
        return w.astype(NPDT[dtype])


def scaled_sum(srcs, raws, pre, post, dtype):
    """((s0 * f0) + (s1 * f1) + ...) * post in W, rounded once; fj = pre for a raw source, else 1."""
    W = work_type(dtype)
    pre_w, post_w, one = W(pre), W(post), W(1)
    with np.errstate(all="ignore"):
        acc = to_work(srcs[0], dtype) * (pre_w if raws[0] else one)
        for s, raw in zip(srcs[1:], raws[1:]):
            x = to_work(s, dtype) * (pre_w if raw else one)
            acc = acc + x
        acc = acc * post_w
    return from_work(acc, dtype)


def interpret(plans, ins, dtype, pre, post, inplace=False):
    """p ranks' plans on host buffers with the scaled arithmetic; returns the p outputs."""
    p = len(plans)
    ins = [np.ascontiguousarray(x).copy() for x in ins]
    es = ins[0].itemsize
    n = ins[0].size
    outs = ins if inplace else [np.zeros_like(x) for x in ins]
    stg = [np.zeros(max(1, pl["staging"]), np.uint8) for pl in plans]
    # ranks absorbed, per byte of every buffer (bytes, because transfers and staging are addressed in bytes)
    cin = [np.ones(n * es, np.int32) for _ in range(p)]
    cout = cin if inplace else [np.zeros(n * es, np.int32) for _ in range(p)]
    cstg = [np.zeros(max(1, pl["staging"]), np.int32) for pl in plans]

    def raw(r, buf):
        if buf == STG:
            return stg[r], cstg[r]
        if buf == IN:
            return ins[r].view(np.uint8), cin[r]
        return outs[r].view(np.uint8), cout[r]

    for i in range(len(plans[0]["steps"])):
        moves = []
        for r in range(p):
            nth = {}
            for x in plans[r]["steps"][i]["xfers"]:
                if not x["send"]:
                    continue
                q = x["peer"]
                k = nth.get(q, 0)
                nth[q] = k + 1
                rv = [y for y in plans[q]["steps"][i]["xfers"] if not y["send"] and y["peer"] == r][k]
                data, cnt = raw(r, x["buf"])
                sl = slice(x["off"], x["off"] + x["bytes"])
                moves.append((data[sl].copy(), cnt[sl].copy(), q, rv))
        for data, cnt, q, rv in moves:
            d, c = raw(q, rv["buf"])
            sl = slice(rv["off"], rv["off"] + rv["bytes"])
            d[sl] = data
            c[sl] = cnt
        for r in range(p):
            for u in plans[r]["steps"][i]["sums"]:
                srcs, raws, total = [], [], 0
                for b, o in u["srcs"]:
                    d, c = raw(r, b)
                    sl = slice(o, o + u["count"] * es)
                    k = int(c[o])
                    assert (c[sl] == k).all() and k >= 1, "a sum's source mixes partial sums of different depth"
                    srcs.append(d[sl].view(ins[0].dtype).copy())
                    raws.append(k == 1)
                    total += k
                assert total <= p, "a rank's input was added twice"
                res = scaled_sum(srcs, raws, pre, post if total == p else 1.0, dtype)
                d, c = raw(r, u["dst"][0])
                sl = slice(u["dst"][1], u["dst"][1] + u["count"] * es)
                d[sl] = res.view(np.uint8)
                c[sl] = total
    for r in range(p):
        assert (cout[r] == p).all(), "rank %d's output holds elements that are not sums over all ranks" % r
    return outs


def chunk_bounds(n, p, es, c):
    """rt.h chunk_of: chunks of ceil(n / p) elements rounded up to 256 bytes."""
    align = 256 // es
    per = -(-(-(-n // p)) // align) * align
    b = min(c * per, n)
    return b, min(b + per, n)


def ring_closed_form(ins, dtype, pre, post):
    """Chunk c folds ranks c, c+1, ..., c-1 (mod p): each reduce-scatter step adds one rank's raw
    chunk (times pre) to the partial sum received (the first step's partner is raw too), rounds to
    the storage type, and the last step multiplies by post before it rounds."""
    p, n = len(ins), ins[0].size
    out = np.zeros_like(ins[0])
    for c in range(p):
        b, e = chunk_bounds(n, p, ins[0].itemsize, c)
        if e <= b:
            continue
        acc = scaled_sum([ins[(c + 1) % p][b:e], ins[c][b:e]], [True, True], pre, post if p == 2 else 1.0, dtype)
        for k in range(2, p):
            acc = scaled_sum([ins[(c + k) % p][b:e], acc], [True, False], pre, post if k == p - 1 else 1.0, dtype)
        out[b:e] = acc
    return out


def fold_closed_form(ins, dtype, pre, post):
    """Direct and one-shot: the rank-order fold of the raw inputs in W, then post, one rounding."""
    return scaled_sum(list(ins), [True] * len(ins), pre, post, dtype)
