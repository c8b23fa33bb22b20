"""One RCCL rank of a MAX / MIN allreduce test job (tests/test_gpu_minmax.py), modelled on
tests/scaled_worker.py: every rank of the job runs on the test box's one GPU, names its own host
(NCCL_HOSTID) so that RCCL joins them over its socket transport, and initialises through tips_init's
TCP bootstrap.

argv: rank size out_dir cases(json). A case is {"dtype", "n", "seed", "algo", "op", "inplace"?,
"inputs"?: "finite", "where"?: "host" | "python", "expect"?: rc}: tips_allreduce_op on the rank's
seeded input (minmax_util.rank_inputs, or finite_nonzero_inputs) under the named schedule - through
device pointers, host (numpy) pointers, or tips_amd.allreduce(t, op=...). The rank's output is saved
to out_dir/case<i>_rank<r>.npy and the parent test compares it with the numpy reference. With
"expect" the call must return that status instead (the peer schedule's refusal) and nothing is saved.
Prints one JSON line {"rank", "results": [{"case", "ok", "rc", "error"}]}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

ALGO_NAMES = {"auto": -1, "ring": 0, "direct": 1, "rccl": 2, "oneshot": 3, "peer": 4}


def main():
    rank, size, out_dir, cases = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], json.loads(sys.argv[4])
    import faulthandler
    import signal
    faulthandler.register(signal.SIGUSR1, all_threads=True)  # the launcher's timeout: where every thread stands

    import numpy as np
    import torch
    import minmax_util as mm
    from gpu_util import from_dev, to_dev
    from tips_amd import _lib

    L = _lib.lib()
    torch.cuda.set_device(0)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(size), LOCAL_RANK="0", NCCL_HOSTID="tips-rank-%d" % rank)
    L.tips_init()
    if not L.tips_is_initialize():
        print(json.dumps({"rank": rank, "results": [{"case": "init", "ok": False, "error": _lib.last_error()}]}))
        return
    sp = torch.cuda.current_stream().cuda_stream
    results = []
    for i, c in enumerate(cases):
        dtype, n, op = c["dtype"], c["n"], c["op"]
        make = mm.finite_nonzero_inputs if c.get("inputs") == "finite" else mm.rank_inputs
        mine = make(dtype, n, c["seed"], size)[rank]
        _lib.call("tips_set_algorithm", ALGO_NAMES[c["algo"]])
        rc, out = 0, None
        if c.get("where") == "python":
            import tips_amd
            t = to_dev(mine)
            if dtype == mm.BF16:
                t = t.view(torch.bfloat16)
            res = tips_amd.allreduce(t, op={mm.MAX: tips_amd.Max, mm.MIN: tips_amd.Min}[op])
            torch.cuda.synchronize()
            out = from_dev(res.view(torch.int16) if dtype == mm.BF16 else res, dtype)
        elif c.get("where") == "host":
            x = mine.copy()
            y = x if c.get("inplace") else np.empty_like(x)
            rc = L.tips_allreduce_op(x.ctypes.data, y.ctypes.data, n, dtype, op, None)
            out = y
        else:
            x = to_dev(mine)
            y = x if c.get("inplace") else torch.empty_like(x)
            rc = L.tips_allreduce_op(x.data_ptr(), y.data_ptr(), n, dtype, op, sp)
            torch.cuda.synchronize()
            out = from_dev(y, dtype) if rc == 0 else None
        want = c.get("expect", 0)
        res = {"case": c, "rc": int(rc), "ok": rc == want, "error": "" if rc == 0 else _lib.last_error()}
        if rc == 0 and want == 0:
            np.save(os.path.join(out_dir, "case%d_rank%d.npy" % (i, rank)), out)
        results.append(res)
    _lib.call("tips_set_algorithm", ALGO_NAMES["auto"])
    L.tips_shutdown()
    print(json.dumps({"rank": rank, "results": results}), flush=True)


if __name__ == "__main__":
    main()
