"""One rank of a multi-process MXFP8 reduce-scatter test job (tests/test_gpu_reducescatter_mxfp8_procs.py).

Run as: python reducescatter_mxfp8_worker.py RANK SIZE CASES_JSON, with the RCCL environment of
tests/test_gpu_rccl_procs.py (rccl_env): every process is its own RCCL rank on the one GPU. Every
rank generates all ranks' seeded inputs and compares its own shards, bit for bit, with the numpy
restatement (tests/reducescatter_mxfp8_util.py). Prints one JSON line: {"rank", "results"}.
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

    import mxfp8_util as mx
    import reducescatter_mxfp8_util as rmx
    import reducescatter_util as ru
    import tips_amd
    from gpu_util import BF16, F32
    from tips_amd import _lib

    torch.cuda.set_device(0)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(size), LOCAL_RANK="0", NCCL_HOSTID="tips-rank-%d" % rank)
    tips_amd.init()
    assert tips_amd.size() == size and tips_amd.rank() == rank
    L = _lib.lib()
    sp = torch.cuda.current_stream().cuda_stream
    fp8 = tips_amd.Compression.fp8

    def inputs(n, seed, i, r):
        return mx.spread_blocks(n, np.random.default_rng([77, seed, i, r]), lo=-20, hi=20)

    def same_bits(got, exp):
        got, exp = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(exp).reshape(-1)
        return got.shape == exp.shape and np.array_equal(got.view(np.uint32), exp.view(np.uint32))

    def host(t):
        return t.detach().contiguous().reshape(-1).cpu().numpy()

    def bf16_host(t):
        return t.detach().contiguous().reshape(-1).view(torch.int16).cpu().numpy().view(np.uint16)

    def plain_works():
        t = torch.from_numpy(inputs(300, 999, 0, rank)).cuda()
        out = tips_amd.reducescatter(t, op=tips_amd.Sum, compression=fp8)
        torch.cuda.synchronize()
        exp = rmx.shards([[inputs(300, 999, 0, r)] for r in range(size)], [1], rank)[0]
        return same_bits(host(out), exp)

    results = []
    for c in cases:
        kind, seed = c["kind"], c["seed"]
        shapes = [tuple(s) for s in c["shapes"]]
        elems = [int(np.prod(s[1:])) for s in shapes]
        ins = [[inputs(int(np.prod(s)), seed, i, r) for i, s in enumerate(shapes)] for r in range(size)]
        res = {"case": c}
        if kind == "mismatch":  # rank 1 calls the plain grouped reduce-scatter, the others the MXFP8 form
            rows = [s[0] for s in shapes]
            ts = [torch.from_numpy(a).cuda() for a in ins[rank]]
            outs = [torch.zeros(a.size + 1, device="cuda") for a in ins[rank]]
            pi, _k1 = _lib.ptr_array([t.data_ptr() for t in ts])
            po, _k2 = _lib.ptr_array([t.data_ptr() for t in outs])
            pr, _k3 = _lib.i64_array(rows)
            pe, _k4 = _lib.i64_array(elems)
            if rank == 1:
                rc = L.tips_grouped_reducescatter(pi, po, pr, pe, len(rows), F32, 0, 1.0, 1.0, sp)
            else:
                rc = L.tips_grouped_reducescatter_mxfp8(pi, po, pr, pe, len(rows), 1.0, sp)
            res.update(rc=int(rc), error=_lib.last_error())
            res["ok"] = rc == -7 and res["error"].startswith("Mismatched reduce-scatter" if rank == 1 else "Mismatched MXFP8 reduce-scatter")
            results.append(res)
            continue
        if kind == "refused":  # rank 1's input is host memory: its own error there, "refused" on the others, nobody waits
            a = np.ascontiguousarray(ins[rank][0])
            t = torch.from_numpy(a).cuda()
            out = torch.zeros(a.size + 1, device="cuda")
            rc = L.tips_reducescatter_mxfp8(a.ctypes.data if rank == 1 else t.data_ptr(), out.data_ptr(), shapes[0][0], elems[0], 1.0, sp)
            res.update(rc=int(rc), error=_lib.last_error())
            want = (-5, "host memory") if rank == 1 else (-7, "refused its arguments")
            res["ok"] = rc == want[0] and want[1] in res["error"]
            results.append(res)
            continue
        if kind == "after":  # after the error cases a plain MXFP8 reduce-scatter still works
            res["ok"] = bool(plain_works())
            results.append(res)
            continue
        if kind == "mixed":  # f32 and bf16 tensors in one list: the bf16 group travels uncompressed
            b16 = [[ru.inputs(BF16, int(np.prod(s)), seed * 100 + i, r) for i, s in enumerate(shapes)] for r in range(size)]
            # (finite bf16 values only: keep the sign, clear the top exponent bit)
            b16 = [[(a.view(np.uint16) & 0xBFFF).astype(np.uint16) for a in per] for per in b16]
            tf = [torch.from_numpy(a).cuda().reshape(s) for a, s in zip(ins[rank], shapes)]
            tb = [torch.from_numpy(a.view(np.int16).copy()).cuda().view(torch.bfloat16).reshape(s) for a, s in zip(b16[rank], shapes)]
            mixed = [x for pair in zip(tf, tb) for x in pair]
            outs = tips_amd.grouped_reducescatter(mixed, op=tips_amd.Sum, compression=fp8)
            plain = tips_amd.grouped_reducescatter(tb, op=tips_amd.Sum)
            torch.cuda.synchronize()
            exp = rmx.shards(ins, elems, rank)
            ok = all(same_bits(host(o), e) for o, e in zip(outs[0::2], exp))
            ok = ok and all(o.dtype == torch.bfloat16 and np.array_equal(bf16_host(o), bf16_host(q)) for o, q in zip(outs[1::2], plain))
            expb = ru.shards([[a.view(np.uint16) for a in per] for per in b16], elems, BF16, rank)
            ok = ok and all(ru.same(bf16_host(o), e, BF16) for o, e in zip(outs[1::2], expb))
            res["ok"] = bool(ok)
            results.append(res)
            continue
        op = c.get("op", "sum")
        factor = {"sum": 1.0, "average": 1.0 / size, "factor": c.get("factor", 1.0)}[op]
        exp = rmx.shards(ins, elems, rank, factor)
        ts = [torch.from_numpy(a).cuda().reshape(s) for a, s in zip(ins[rank], shapes)]
        if kind == "grouped":  # through Python, a None entry in between
            outs = tips_amd.grouped_reducescatter(ts[:1] + [None] + ts[1:], op=tips_amd.Average if op == "average" else tips_amd.Sum,
                                                  postscale_factor=factor if op == "factor" else 1.0, compression=fp8)
            assert outs[1] is None
            outs = outs[:1] + outs[2:]
        elif op == "average":  # through Python
            outs = [tips_amd.reducescatter(ts[0], op=tips_amd.Average, compression=fp8)]
        else:  # the C entry
            own_rows = ru.rows_of(shapes[0][0], size, rank)[1]
            out = torch.empty((own_rows,) + shapes[0][1:], dtype=torch.float32, device="cuda")
            _lib.call("tips_reducescatter_mxfp8", ts[0].data_ptr(), out.data_ptr(), shapes[0][0], elems[0], float(factor), sp)
            outs = [out]
        torch.cuda.synchronize()
        got = [host(o) for o in outs]
        ok = all(tuple(o.shape) == (ru.rows_of(s[0], size, rank)[1],) + s[1:] for o, s in zip(outs, shapes))
        ok = ok and all(same_bits(g, e) for g, e in zip(got, exp))
        ok = ok and all(same_bits(host(t), a) for t, a in zip(ts, ins[rank]))  # inputs untouched
        res["ok"] = bool(ok)
        # one digest of this rank's shards beside the restatement's
        res["sha1"] = ru.sha1_of(got, F32)
        res["sha1_ref"] = ru.sha1_of(exp, F32)
        results.append(res)
    tips_amd.shutdown()
    print(json.dumps({"rank": rank, "results": results}), flush=True)


if __name__ == "__main__":
    main()
