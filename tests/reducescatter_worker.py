"""One rank of a multi-process reduce-scatter test job (tests/test_gpu_reducescatter_procs.py).

Run as: python reducescatter_worker.py RANK SIZE CASES_JSON, with the RCCL environment of
tests/test_gpu_rccl_procs.py (rccl_env): every process is its own RCCL rank on the one GPU. Every
rank generates all ranks' inputs from the case's seed and compares its own shards with the numpy
definition (tests/reducescatter_util.py) under the project's bit rule. Prints one JSON line:
{"rank", "results"}.
"""
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

    import reducescatter_util as ru
    import tips_amd
    from gpu_util import BF16, NPDT
    from tips_amd import _lib

    torch.cuda.set_device(0)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(size), LOCAL_RANK="0", NCCL_HOSTID="tips-rank-%d" % rank)
    tips_amd.init()
    assert tips_amd.size() == size and tips_amd.rank() == rank
    L = _lib.lib()
    sp = torch.cuda.current_stream().cuda_stream
    TORCH = {0: torch.float32, 1: torch.float64, 2: torch.int32, 3: torch.int64, 4: torch.float16, 5: torch.bfloat16}
    OPS = {"sum": (ru.SUM, tips_amd.Sum), "scaled": (ru.SUM, tips_amd.Sum), "average": (ru.SUM, tips_amd.Average),
           "max": (ru.MAX, tips_amd.Max), "min": (ru.MIN, tips_amd.Min)}

    def dev(a, dtype, shape):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy((a.view(np.int16) if dtype == BF16 else a).copy()).cuda()
        return (t.view(torch.bfloat16) if dtype == BF16 else t).reshape(shape)

    def host(t, dtype):
        t = t.detach().contiguous().reshape(-1)
        return (t.view(torch.int16) if dtype == BF16 else t).cpu().numpy().view(NPDT[dtype])

    def sum_still_works():
        t = torch.full((1000,), float(rank + 1), device="cuda")
        out = tips_amd.allreduce(t)
        torch.cuda.synchronize()
        return bool(torch.all(out == size * (size + 1) / 2).item())

    results = []
    for c in cases:
        kind, dtype, seed = c["kind"], c.get("dtype", 0), c["seed"]
        shapes = [tuple(s) for s in c["shapes"]]
        elems = [int(np.prod(s[1:])) for s in shapes]
        ins = [[ru.inputs(dtype, int(np.prod(s)), seed * 100 + i, r) for i, s in enumerate(shapes)] for r in range(size)]
        res = {"case": c}
        if kind == "mismatch":  # rank 1 brings another rows list of the same total
            rows = [s[0] for s in shapes]
            if rank == 1:
                rows[0], rows[1] = rows[0] + 1, rows[1] - 1
            ts = [torch.zeros(r * e, device="cuda") for r, e in zip(rows, elems)]
            outs = [torch.zeros(r * e + 1, device="cuda") for r, e in zip(rows, elems)]
            pi, _k1 = _lib.ptr_array([t.data_ptr() for t in ts])
            po, _k2 = _lib.ptr_array([t.data_ptr() for t in outs])
            pr, _k3 = _lib.i64_array(rows)
            pe, _k4 = _lib.i64_array(elems)
            rc = L.tips_grouped_reducescatter(pi, po, pr, pe, len(rows), 0, 0, 1.0, 1.0, sp)
            res.update(rc=int(rc), error=_lib.last_error())
            res["ok"] = rc == -7 and res["error"].startswith("Mismatched reduce-scatter") and sum_still_works()
            results.append(res)
            continue
        if kind == "refused":  # rank 1's input is host memory: its own error there, "refused" on the others, nobody waits
            a = np.ascontiguousarray(ins[rank][0])
            t = dev(a, dtype, shapes[0])
            out = torch.zeros(a.size + 1, device="cuda")
            rc = L.tips_reducescatter(a.ctypes.data if rank == 1 else t.data_ptr(), out.data_ptr(), shapes[0][0], elems[0], dtype,
                                      0, 1.0, 1.0, sp)
            res.update(rc=int(rc), error=_lib.last_error())
            want = (-5, "host memory") if rank == 1 else (-7, "refused its arguments")
            res["ok"] = rc == want[0] and want[1] in res["error"] and sum_still_works()
            results.append(res)
            continue
        if kind == "consistency":  # allgather(reducescatter(x)) against the direct allreduce of x
            op = c["op"]
            x = dev(ins[rank][0], dtype, shapes[0])
            whole = tips_amd.allgather_op(tips_amd.reducescatter(x, op=OPS[op][1]))
            prev = tips_amd.set_algorithm("direct")
            ref = torch.empty_like(x)
            if op == "sum":
                _lib.call("tips_allreduce", x.data_ptr(), ref.data_ptr(), x.numel(), dtype, 0, sp)
            else:
                _lib.call("tips_allreduce_op", x.data_ptr(), ref.data_ptr(), x.numel(), dtype, OPS[op][0], sp)
            tips_amd.set_algorithm(prev)
            torch.cuda.synchronize()
            got = host(whole, dtype)
            res["ok"] = bool(whole.shape == x.shape and ru.same(got, host(ref, dtype), dtype))
            res["sha1"] = ru.sha1_of([got], dtype)
            results.append(res)
            continue
        op = c.get("op", "sum")
        pre, post = (c.get("pre", 1.0), c.get("post", 1.0)) if op == "scaled" else (1.0, 1.0 / size if op == "average" else 1.0)
        exp_all = [ru.shards(ins, elems, dtype, q, OPS[op][0], pre, post) for q in range(size)]
        ts = [dev(ins[rank][i], dtype, s) for i, s in enumerate(shapes)]
        if kind == "grouped":  # through Python, a None entry in between
            outs = tips_amd.grouped_reducescatter(ts[:1] + [None] + ts[1:], op=OPS[op][1], prescale_factor=pre if op == "scaled" else 1.0,
                                                  postscale_factor=post if op == "scaled" else 1.0)
            assert outs[1] is None
            outs = outs[:1] + outs[2:]
        elif op == "average":  # through Python
            outs = [tips_amd.reducescatter(ts[0], op=tips_amd.Average)]
        else:  # the C entry
            own_rows = ru.rows_of(shapes[0][0], size, rank)[1]
            out = torch.empty((own_rows,) + shapes[0][1:], dtype=TORCH[dtype], device="cuda")
            _lib.call("tips_reducescatter", ts[0].data_ptr(), out.data_ptr(), shapes[0][0], elems[0], dtype, OPS[op][0],
                      float(pre), float(post), sp)
            outs = [out]
        torch.cuda.synchronize()
        got = [host(o, dtype) for o in outs]
        ok = all(tuple(o.shape) == (ru.rows_of(s[0], size, rank)[1],) + s[1:] for o, s in zip(outs, shapes))
        ok = ok and all(ru.same(g, e, dtype) for g, e in zip(got, exp_all[rank]))
        ok = ok and all(ru.same(host(t, dtype), a, dtype) and np.array_equal(host(t, dtype).view(np.uint8), np.ascontiguousarray(a).view(np.uint8))
                        for t, a in zip(ts, ins[rank]))  # inputs untouched
        res["ok"] = bool(ok)
        # one digest of this rank's shards beside the restatement's (every NaN counted as the quiet NaN)
        res["sha1"] = ru.sha1_of(got, dtype)
        res["sha1_ref"] = ru.sha1_of(exp_all[rank], dtype)
        results.append(res)
    tips_amd.shutdown()
    print(json.dumps({"rank": rank, "results": results}), flush=True)


if __name__ == "__main__":
    main()
