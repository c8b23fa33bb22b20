"""One rank of a multi-process Adasum test job (tests/test_gpu_adasum_procs.py).

Run as: python adasum_worker.py RANK SIZE CASES_JSON, with the RCCL environment of
tests/test_gpu_rccl_procs.py (rccl_env): every process is its own RCCL rank on the one GPU. Every
rank generates all ranks' inputs from the case's seed and compares its own result bit for bit with
the restatement's tree (tests/adasum_util.py). Prints one JSON line: {"rank", "results"}.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    rank, size, cases = int(sys.argv[1]), int(sys.argv[2]), json.loads(sys.argv[3])
    import faulthandler
    import signal
    faulthandler.register(signal.SIGUSR1, all_threads=True)

    import numpy as np
    import torch

    from adasum_util import tree_ref
    from gpu_util import BF16, F32, NPDT, from_dev, rand, same_bits, to_dev
    import tips_amd
    from tips_amd import _lib

    torch.cuda.set_device(0)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(size), LOCAL_RANK="0", NCCL_HOSTID="tips-rank-%d" % rank)
    tips_amd.init()
    assert tips_amd.size() == size and tips_amd.rank() == rank
    L = _lib.lib()
    sp = torch.cuda.current_stream().cuda_stream
    pow2 = size & (size - 1) == 0

    def dev(x, dtype):
        t = to_dev(x)
        return t.view(torch.bfloat16) if dtype == BF16 else t

    def host(t, dtype):
        return from_dev(t.view(torch.int16) if dtype == BF16 else t, dtype)

    def sum_still_works():
        t = torch.full((1000,), float(rank + 1), device="cuda")
        out = tips_amd.allreduce(t)
        torch.cuda.synchronize()
        return bool(torch.all(out == size * (size + 1) / 2).item())

    results = []
    for c in cases:
        dtype, counts, kind = c["dtype"], c["counts"], c["kind"]
        n = sum(counts)
        vals = [rand(dtype, n, np.random.default_rng(1000 * c["seed"] + r)) for r in range(size)]
        res = {"case": c}
        if kind == "mismatch":  # rank 1 brings another count list of the same total
            mine = list(counts)
            if rank == 1:
                mine[0], mine[1] = mine[0] + 1, mine[1] - 1
            o, ts = 0, []
            for k in mine:
                ts.append(dev(vals[rank][o:o + k], dtype))
                o += k
            pp, _k1 = _lib.ptr_array([t.data_ptr() for t in ts])
            cp, _k2 = _lib.i64_array(mine)
            flat = torch.empty(_lib.lib().tips_fused_layout(cp, len(mine), dtype, None), dtype=torch.uint8, device="cuda")
            rc = L.tips_fused_allreduce_adasum_flat(pp, cp, len(mine), dtype, flat.data_ptr(), sp)
            res.update(rc=int(rc), error=_lib.last_error())
            res["ok"] = rc == -7 and "Mismatched Adasum" in _lib.last_error() and sum_still_works()
            results.append(res)
            continue
        if kind == "refused":  # rank 1's `in` is host memory: its own error there, "refused" on the others, nobody waits
            t = dev(vals[rank], dtype)
            out = torch.empty_like(t)
            rc = L.tips_allreduce_adasum(vals[rank].ctypes.data if rank == 1 else t.data_ptr(), out.data_ptr(), n, dtype, sp)
            res.update(rc=int(rc), error=_lib.last_error())
            want = (-5, "host memory") if rank == 1 else (-7, "refused its arguments")
            res["ok"] = rc == want[0] and want[1] in res["error"] and sum_still_works()
            results.append(res)
            continue
        if not pow2:  # refused on every rank before any exchange; the job goes on
            t = dev(vals[rank], dtype)
            out = torch.empty_like(t)
            rc = L.tips_allreduce_adasum(t.data_ptr(), out.data_ptr(), n, dtype, sp)
            cp, _k2 = _lib.i64_array([n])
            pp, _k1 = _lib.ptr_array([t.data_ptr()])
            rc2 = L.tips_fused_allreduce_adasum_flat(pp, cp, 1, dtype, out.data_ptr(), sp)
            res.update(rc=int(rc), rc2=int(rc2), error=_lib.last_error())
            res["ok"] = rc == -5 and rc2 == -5 and "power-of-two" in _lib.last_error() and sum_still_works()
            results.append(res)
            continue
        exp = tree_ref(vals, counts, dtype)[rank]
        if kind == "single":
            t = dev(vals[rank], dtype)
            if c.get("inplace"):
                _lib.call("tips_allreduce_adasum", t.data_ptr(), t.data_ptr(), n, dtype, sp)
                got = host(t, dtype)
            else:
                got = host(tips_amd.adasum_op(t), dtype)
        elif kind == "python":  # allreduce(op=Adasum)
            got = host(tips_amd.allreduce(dev(vals[rank], dtype), op=tips_amd.Adasum), dtype)
        else:  # "flat" (fused_adasum_flat), "grads" / "grads_unfused" (allreduce_grads): one segment per tensor
            o, ts = 0, []
            for k in counts:
                ts.append(dev(vals[rank][o:o + k], dtype))
                o += k
            if kind == "flat":
                outs = tips_amd.fused_adasum_flat(ts)
            else:
                grads = ts[:2] + [None] + ts[2:]
                outs = tips_amd.allreduce_grads(grads, op=tips_amd.Adasum, fused=kind == "grads")
                assert outs[2] is None
                outs = outs[:2] + outs[3:]
            torch.cuda.synchronize()
            got = np.concatenate([host(x.reshape(-1), dtype) for x in outs]) if outs else np.zeros(0, NPDT[dtype])
            res["inputs_kept"] = all(np.array_equal(host(t, dtype), vals[rank][a:a + k]) for t, a, k in
                                     zip(ts, np.cumsum([0] + counts[:-1]), counts))
        torch.cuda.synchronize()
        res["ok"] = bool(same_bits(got, exp, dtype)) and res.get("inputs_kept", True)
        res["sha1"] = hashlib.sha1(got.tobytes()).hexdigest()
        results.append(res)
    tips_amd.shutdown()
    print(json.dumps({"rank": rank, "results": results}), flush=True)


if __name__ == "__main__":
    main()
