"""One rank of a multi-process MXFP8 test job (tests/test_gpu_mxfp8_procs.py).

Run as: python mxfp8_worker.py RANK SIZE CASES_JSON, with the RCCL environment of
tests/test_gpu_rccl_procs.py (rccl_env): every process is its own RCCL rank on the one GPU. Every
rank generates all ranks' inputs from the case's seed and compares its own result bit for bit with
the restatement's collective (tests/mxfp8_util.py). Prints one JSON line: {"rank", "results"}.
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

    import mxfp8_util as mx
    import tips_amd
    from tips_amd import Compression, _lib, ops

    torch.cuda.set_device(0)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(size), LOCAL_RANK="0", NCCL_HOSTID="tips-rank-%d" % rank)
    tips_amd.init()
    assert tips_amd.size() == size and tips_amd.rank() == rank
    L = _lib.lib()
    sp = torch.cuda.current_stream().cuda_stream

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def split(a, counts):
        return [a[o:o + k] for o, k in zip(np.cumsum([0] + counts[:-1]), counts)]

    def bits(t):
        return t.detach().cpu().contiguous().view(-1).numpy().view(np.uint32)

    def sum_still_works():
        t = torch.full((1000,), float(rank + 1), device="cuda")
        out = tips_amd.allreduce(t)
        torch.cuda.synchronize()
        return bool(torch.all(out == size * (size + 1) / 2).item())

    results = []
    for c in cases:
        counts, kind = c["counts"], c["kind"]
        factor = c.get("factor", 1.0)
        n = sum(counts)
        vals = [mx.spread_blocks(n, np.random.default_rng(1000 * c["seed"] + r), -20, 20) for r in range(size)]
        res = {"case": c}
        if kind == "mismatch":  # rank 1 brings another count list of the same total
            mine = list(counts)
            if rank == 1:
                mine[0], mine[1] = mine[0] + 1, mine[1] - 1
            ts = [dev(a) for a in split(vals[rank], mine)]
            pp, _k1 = _lib.ptr_array([t.data_ptr() for t in ts])
            cp, _k2 = _lib.i64_array(mine)
            flat = torch.empty(L.tips_fused_layout(cp, len(mine), 0, None), dtype=torch.uint8, device="cuda")
            rc = L.tips_fused_allreduce_mxfp8_flat(pp, cp, len(mine), flat.data_ptr(), 1.0, sp)
            res.update(rc=int(rc), error=_lib.last_error())
            res["ok"] = rc == -7 and "Mismatched MXFP8" in _lib.last_error() and sum_still_works()
            results.append(res)
            continue
        if kind == "refused":  # rank 1's input is host memory: its own error there, "refused" on the others, nobody waits
            a = np.ascontiguousarray(vals[rank])
            t = dev(a)
            out = torch.empty_like(t)
            rc = L.tips_allreduce_mxfp8(a.ctypes.data if rank == 1 else t.data_ptr(), out.data_ptr(), n, 1.0, sp)
            res.update(rc=int(rc), error=_lib.last_error())
            want = (-5, "host memory") if rank == 1 else (-7, "refused its arguments")
            res["ok"] = rc == want[0] and want[1] in res["error"] and sum_still_works()
            results.append(res)
            continue
        elems, offs = ops.mxfp8_flat_elems(counts)
        if kind == "mixed":  # f32 device, bf16 device and host numpy members in one list
            f32s = split(vals[rank], counts)
            grads = [dev(f32s[0]), dev(f32s[1]).to(torch.bfloat16), f32s[2].copy(), None, dev(f32s[3])]
            outs = tips_amd.allreduce_grads(grads, compression=Compression.fp8)
            plain = tips_amd.allreduce_grads(grads, compression=Compression.none)
            torch.cuda.synchronize()
            ok = outs[3] is None and outs[1].dtype == torch.bfloat16 and isinstance(outs[2], np.ndarray)
            ok = ok and torch.equal(outs[1].view(torch.int16), plain[1].view(torch.int16))
            ok = ok and np.array_equal(outs[2].view(np.uint32), np.asarray(plain[2]).view(np.uint32))
            sub = [0, 3]  # the float32 device members form their own MXFP8 list
            sc = [counts[i] for i in sub]
            se, so = ops.mxfp8_flat_elems(sc)
            exp = mx.collective([mx.flat_of([split(v, counts)[i] for i in sub], so, se) for v in vals])
            got = np.concatenate([bits(outs[0]), bits(outs[4])])
            want = np.concatenate([exp[o:o + k] for o, k in zip(so, sc)]).view(np.uint32)
            res["ok"] = bool(ok and np.array_equal(got, want))
            res["sha1"] = hashlib.sha1(got.tobytes()).hexdigest()
            results.append(res)
            continue
        if kind == "grads_avg":
            factor = 1.0 / size
        flat_exp = mx.collective([mx.flat_of(split(v, counts), offs, elems) for v in vals], factor)
        exp = np.concatenate([flat_exp[o:o + k] for o, k in zip(offs, counts)]).view(np.uint32)
        if kind == "single":
            t = dev(vals[rank])
            if c.get("inplace"):
                _lib.call("tips_allreduce_mxfp8", t.data_ptr(), t.data_ptr(), n, factor, sp)
                got = bits(t)
            else:
                got = bits(tips_amd.allreduce_mxfp8(t, factor))
        elif kind == "python":  # allreduce(compression=Compression.fp8)
            got = bits(tips_amd.allreduce(dev(vals[rank]), compression=Compression.fp8))
        else:  # "flat" (fused_allreduce_mxfp8), "grads" / "grads_unfused" / "grads_avg" (allreduce_grads)
            ts = [dev(a) for a in split(vals[rank], counts)]
            if kind == "flat":
                outs = tips_amd.fused_allreduce_mxfp8(ts, factor)
            else:
                if kind == "grads_avg":
                    tips_amd.set_op_scaling(True)
                grads = ts[:2] + [None] + ts[2:]
                outs = tips_amd.allreduce_grads(grads, compression=Compression.fp8, fused=kind != "grads_unfused",
                                                op=tips_amd.Average if kind == "grads_avg" else None)
                tips_amd.set_op_scaling(False)
                assert outs[2] is None
                outs = outs[:2] + outs[3:]
            torch.cuda.synchronize()
            if kind == "grads_unfused":  # one collective per tensor: each tensor is its own list
                exp = np.concatenate([
                    mx.collective([mx.flat_of([split(v, counts)[i]], [0], ops.mxfp8_flat_elems([k])[0]) for v in vals],
                                  factor)[:k] for i, k in enumerate(counts)]).view(np.uint32)
            got = np.concatenate([bits(x) for x in outs]) if outs else np.zeros(0, np.uint32)
            res["inputs_kept"] = all(np.array_equal(bits(t), a.view(np.uint32)) for t, a in zip(ts, split(vals[rank], counts)))
        torch.cuda.synchronize()
        res["ok"] = bool(np.array_equal(got, exp)) and res.get("inputs_kept", True)
        res["sha1"] = hashlib.sha1(got.tobytes()).hexdigest()
        results.append(res)
    tips_amd.shutdown()
    print(json.dumps({"rank": rank, "results": results}), flush=True)


if __name__ == "__main__":
    main()
