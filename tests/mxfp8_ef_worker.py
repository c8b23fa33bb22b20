"""One rank of a multi-process MXFP8 error-feedback job (tests/test_gpu_mxfp8_ef_procs.py).

Run as: python mxfp8_ef_worker.py RANK SIZE CASES_JSON, with the RCCL environment of
tests/test_gpu_rccl_procs.py (rccl_env): every process is its own RCCL rank on the one GPU. Every
rank generates all ranks' inputs of every step from the case's seed, runs the restatement's
collective_ef (tests/mxfp8_ef_util.py) over all ranks' states, and compares its own outputs and its
own state bit for bit after each step. Prints one JSON line: {"rank", "results"}.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

STEPS = 3


def main():
    rank, size, cases = int(sys.argv[1]), int(sys.argv[2]), json.loads(sys.argv[3])
    import faulthandler
    import signal
    faulthandler.register(signal.SIGUSR1, all_threads=True)

    import numpy as np
    import torch

    import mxfp8_ef_util as ef
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
        res = {"case": c}
        elems, offs = ops.mxfp8_flat_elems(counts)
        need = ops.mxfp8_ef_bytes(elems, size)
        assert need == ef.ef_bytes(elems, size)
        if kind in ("kind_mismatch", "short_state"):
            x = mx.spread_blocks(n, np.random.default_rng(1000 * c["seed"] + rank), -20, 20)
            t = dev(x)
            out = torch.empty_like(t)
            state = torch.full((need // 4,), 0.25, device="cuda")
            if kind == "kind_mismatch" and rank != 0:  # rank 0 brings the feedback call, every other rank the plain one
                rc = L.tips_allreduce_mxfp8(t.data_ptr(), out.data_ptr(), n, 1.0, sp)
            else:  # "short_state": rank 1's state is 4 bytes short
                short = 4 if (kind == "short_state" and rank == 1) else 0
                rc = L.tips_allreduce_mxfp8_ef(t.data_ptr(), out.data_ptr(), n, 1.0, state.data_ptr(), need - short, sp)
            torch.cuda.synchronize()
            res.update(rc=int(rc), error=_lib.last_error())
            res["ok"] = rc == -7 and bool(torch.all(state == 0.25).item()) and sum_still_works()
            results.append(res)
            continue
        mask = ef.mask_of(counts, offs, elems)
        host_states = [np.zeros(ef.ef_elems(elems, size), np.float32) for _ in range(size)]
        comp = Compression.fp8.error_feedback()
        state = torch.zeros(need // 4, device="cuda")
        ok, sha = True, hashlib.sha1()
        for step in range(STEPS):
            seed = 1000 * c["seed"] + 100 * min(step, c.get("new_inputs", STEPS))  # (new_inputs = 1: steps 1 and 2 repeat step 1's)
            vals = [mx.spread_blocks(n, np.random.default_rng(seed + r), -20, 20) for r in range(size)]
            flat_exp, host_states = ef.collective_ef([mx.flat_of(split(v, counts), offs, elems) for v in vals], host_states,
                                                     factor, mask)
            exp = np.concatenate([flat_exp[o:o + k] for o, k in zip(offs, counts)]).view(np.uint32)
            if kind == "single":
                t = dev(vals[rank])
                if c.get("inplace"):
                    _lib.call("tips_allreduce_mxfp8_ef", t.data_ptr(), t.data_ptr(), n, factor, state.data_ptr(), need, sp)
                    got = bits(t)
                else:
                    got = bits(tips_amd.allreduce_mxfp8_ef(t, state, factor))
            elif kind == "flat":
                outs = tips_amd.fused_allreduce_mxfp8_ef([dev(a) for a in split(vals[rank], counts)], state, factor)
                got = np.concatenate([bits(x) for x in outs])
            else:  # "grads": allreduce_grads(compression=<MXFP8ErrorFeedback>), the object keeps the state
                ts = [dev(a) for a in split(vals[rank], counts)]
                outs = tips_amd.allreduce_grads(ts[:2] + [None] + ts[2:], compression=comp)
                assert outs[2] is None
                got = np.concatenate([bits(x) for x in outs[:2] + outs[3:]])
                sd = comp.state_dict()
                assert list(sd) == [("list", "cuda:0", tuple(counts), size)], list(sd)
                state = sd[("list", "cuda:0", tuple(counts), size)]
            torch.cuda.synchronize()
            ok = ok and bool(np.array_equal(got, exp)) and bool(np.array_equal(bits(state), host_states[rank].view(np.uint32)))
            sha.update(got.tobytes())
        res["ok"] = ok
        res["sha1"] = sha.hexdigest()
        res["state_nonzero"] = bool(host_states[rank].any())
        results.append(res)
    tips_amd.shutdown()
    print(json.dumps({"rank": rank, "results": results}), flush=True)


if __name__ == "__main__":
    main()
