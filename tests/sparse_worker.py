"""One rank of a multi-process sparse-allreduce test job (tests/test_gpu_sparse_procs.py).

Run as: python sparse_worker.py RANK SIZE CASES_JSON, with the RCCL environment of
tests/test_gpu_rccl_procs.py (rccl_env): every process is its own RCCL rank on the one GPU, named as
its own host (NCCL_HOSTID) so RCCL joins them over its socket transport. Each case is run through
tips_amd.sparse_allreduce (or, for the mismatch and refused cases, tips_sparse_allreduce itself) and compared bit
for bit with tests/sparse_util.py on the concatenation of every rank's entries in rank order - every
rank generates all ranks' inputs from the case's seed. Prints one JSON line: {"rank", "results"}.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def rank_inputs(c, r, size):
    """Rank r's (values [n_r, D], indices [n_r]) of case c."""
    import numpy as np
    from sparse_util import make_indices
    from test_gpu_sparse import rand_values
    rng = np.random.default_rng(1000 * c["seed"] + r)
    n, rows, D = c["ns"][r], c["rows"], c["D"]
    if c["sets"] == "disjoint":  # rank r names only rows congruent to r modulo size
        idx = (make_indices("zipf", n, max(1, rows // size), rng) * size + r) % rows if n else np.zeros(0, np.int64)
        idx = idx.astype(np.int64)
    else:
        idx = make_indices(c.get("pattern", "zipf"), n, rows, rng)
    return rand_values(c["dtype"], n, D, rng), idx


def main():
    rank, size, cases = int(sys.argv[1]), int(sys.argv[2]), json.loads(sys.argv[3])
    import faulthandler
    import signal
    faulthandler.register(signal.SIGUSR1, all_threads=True)

    import numpy as np
    import torch

    from gpu_util import BF16, NPDT, same_bits
    from sparse_util import concat_ranks, rows_sum_ref
    import tips_amd
    from tips_amd import _lib

    torch.cuda.set_device(0)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(size), LOCAL_RANK="0", NCCL_HOSTID="tips-rank-%d" % rank)
    tips_amd.init()
    assert tips_amd.size() == size and tips_amd.rank() == rank
    L = _lib.lib()
    sp = torch.cuda.current_stream().cuda_stream

    def sum_still_works():
        t = torch.full((1000,), float(rank + 1), device="cuda")
        out = tips_amd.allreduce(t)
        torch.cuda.synchronize()
        return bool(torch.all(out == size * (size + 1) / 2).item())

    results = []
    for c in cases:
        dtype, rows, D = c["dtype"], c["rows"], c["D"]
        parts = [rank_inputs(c, r, size) for r in range(size)]
        values, idx = parts[rank]
        tv = torch.from_numpy(values.view(np.int16) if dtype == BF16 else values).cuda()
        ti = torch.from_numpy(idx).cuda()
        res = {"case": c}
        if c.get("mismatch"):  # rank 1 brings rows of another length: refused on every rank, before any exchange of entries
            d = D + 1 if rank == 1 else D
            out = torch.empty(rows * d, dtype=tv.dtype, device="cuda")
            rc = L.tips_sparse_allreduce(tv.data_ptr(), ti.data_ptr(), len(idx) if rank != 1 else 0, rows, d, dtype, 1.0, 1.0,
                                         out.data_ptr(), sp)
            res.update(rc=int(rc), error=_lib.last_error())
            res["ok"] = rc == -7 and "Mismatched sparse allreduce" in res["error"] and sum_still_works()
            results.append(res)
            continue
        if c.get("refused"):  # rank 1's dense_out is host memory: its own error there, "refused" on the others, nobody waits
            host_out = np.empty(rows * D, values.dtype)
            out = torch.empty(rows * D, dtype=tv.dtype, device="cuda")
            rc = L.tips_sparse_allreduce(tv.data_ptr(), ti.data_ptr(), len(idx), rows, D, dtype, 1.0, 1.0,
                                         host_out.ctypes.data if rank == 1 else out.data_ptr(), sp)
            res.update(rc=int(rc), error=_lib.last_error())
            want = (-5, "host memory") if rank == 1 else (-7, "refused its arguments")
            res["ok"] = rc == want[0] and want[1] in res["error"] and sum_still_works()
            results.append(res)
            continue
        if dtype == BF16:
            tv = tv.view(torch.bfloat16)
        f = c.get("predivide", 1.0)
        kw = {}
        pre = post = 1.0
        if c.get("average"):  # op=Average with a gradient predivision factor f: prescale 1/f, postscale f / size
            kw = dict(op=tips_amd.Average, prescale_factor=1.0 / f, postscale_factor=f)
            pre, post = 1.0 / f, f / size
        dense = tips_amd.sparse_allreduce(tips_amd.IndexedSlices(tv, ti, (rows, D)), **kw)
        torch.cuda.synchronize()
        got = (dense.view(torch.int16) if dtype == BF16 else dense).cpu().numpy().view(NPDT[dtype])
        g_values, g_idx = concat_ranks(parts)
        exp = rows_sum_ref(g_values, g_idx, rows, dtype, pre, post)
        res["ok"] = bool(same_bits(got, exp, dtype))
        res["sha1"] = hashlib.sha1(got.tobytes()).hexdigest()
        res["entries"] = int(len(g_idx))
        if c.get("coalesced"):
            co = tips_amd.sparse_allreduce(tips_amd.IndexedSlices(tv, ti, (rows, D)), coalesced=True, **kw)
            uniq = np.unique(g_idx)
            cv = (co.values.view(torch.int16) if dtype == BF16 else co.values).cpu().numpy().view(NPDT[dtype])
            res["ok"] = res["ok"] and np.array_equal(co.indices.cpu().numpy(), uniq) and bool(same_bits(cv, exp[uniq], dtype))
        results.append(res)
    tips_amd.shutdown()
    print(json.dumps({"rank": rank, "results": results}), flush=True)


if __name__ == "__main__":
    main()
