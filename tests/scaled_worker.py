"""One RCCL rank of a scaled-allreduce test job (tests/test_gpu_scaled.py), modelled on
tests/peer_worker.py: every rank of the job runs on the test box's one GPU, names its own host
(NCCL_HOSTID) so that RCCL joins them over its socket transport, and initialises through tips_init's
TCP bootstrap.

argv: rank size out_dir cases(json). Two kinds of case:
- {"dtype", "n", "seed", "algo", "pre", "post", "inplace"?, "kind"?}: tips_allreduce_scaled on
  seeded inputs under the named schedule; the rank's output is saved to out_dir/case<i>_rank<r>.npy
  and the parent test compares it (bit-exact against the scaled plan interpreter).
- {"op": "grads" | "optimizer", ...}: the Python surface with set_op_scaling(True), checked here.
Prints one JSON line {"rank", "results": [{"case", "ok", "rc", "error", ...}]}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

ALGO_NAMES = {"auto": -1, "ring": 0, "direct": 1, "rccl": 2, "oneshot": 3}


def inputs(c, size):
    import numpy as np
    from gpu_util import rand
    return [rand(c["dtype"], c["n"], np.random.default_rng(c["seed"] + r), c.get("kind", "normal")) for r in range(size)]


def grads_case(c, rank, size):
    """allreduce_grads(op=Average) on config 5's gradient list (214 float32 tensors) under the
    default schedule (one-shot for small buckets, direct otherwise at p > 2: both the rank-order
    fold): bit-exact against the fold in fp32 times fp32(1 / size), rounded once."""
    import numpy as np
    import torch
    import bench
    import scaled_util
    import tips_amd
    from gpu_util import F32
    sizes = bench.resnet50_grad_sizes()
    g = torch.Generator(device="cuda")

    def flat(r):
        g.manual_seed(c["seed"] * 100 + r)
        return torch.empty(sum(sizes), dtype=torch.float32, device="cuda").uniform_(-1.0, 1.0, generator=g)

    mine = flat(rank)
    before = mine.clone()
    got = tips_amd.allreduce_grads(list(torch.split(mine, sizes)), op=tips_amd.Average)
    torch.cuda.synchronize()
    exp = scaled_util.fold_closed_form([flat(r).cpu().numpy() for r in range(size)], F32, 1.0, 1.0 / size)
    got = torch.cat([t.reshape(-1) for t in got]).cpu().numpy()
    ok = np.array_equal(got.view(np.uint32), exp.view(np.uint32)) and torch.equal(mine, before)
    return {"case": c, "rc": 0, "ok": bool(ok), "error": "" if ok else "%d of %d elements differ" % (
        int((got.view(np.uint32) != exp.view(np.uint32)).sum()), got.size)}


def optimizer_case(c, rank, size):
    """DistributedOptimizer(op=Average, gradient_predivide_factor=f).step() over SGD: the update is
    p - lr * mean_r grad_r. The reference is recomputed in float64 from every rank's gradients; the
    bound per element is lr * (size + 2) * 2^-24 * mean|grad| for the scaled sum (one multiply per
    input, size - 1 adds, one multiply, and the two factors' conversion to fp32, all relative to
    the terms' magnitudes) plus 3 * 2^-24 * (|p| + lr * |mean|) for SGD's own multiply and subtract."""
    import torch
    import tips_amd

    def model():
        torch.manual_seed(c["seed"])
        return torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Tanh(), torch.nn.Linear(32, 4)).cuda()

    def backward(m, r):
        g = torch.Generator().manual_seed(c["seed"] * 100 + r)
        m(torch.randn(8, 16, generator=g).cuda()).pow(2).sum().backward()
        return [p.grad.detach().double() for p in m.parameters()]

    all_g = [backward(model(), r) for r in range(size)]
    m = model()
    backward(m, rank)
    lr, eps = 0.05, 2.0 ** -24
    exp, tol = [], []
    for i, p in enumerate(m.parameters()):
        mean = sum(all_g[r][i] for r in range(size)) / size
        mean_abs = sum(all_g[r][i].abs() for r in range(size)) / size
        exp.append(p.detach().double() - lr * mean)
        tol.append(lr * (size + 2) * eps * mean_abs + 3 * eps * (p.detach().double().abs() + lr * mean.abs()))
    opt = tips_amd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=lr), op=tips_amd.Average,
                                        gradient_predivide_factor=c["f"])
    opt.step()
    torch.cuda.synchronize()
    worst = max(float(((p.detach().double() - e).abs() / t).max()) for p, e, t in zip(m.parameters(), exp, tol))
    plain = max(float((p.detach().double() - e).abs().max()) for p, e in zip(m.parameters(), exp))
    ok = worst <= 1.0
    return {"case": c, "rc": 0, "ok": bool(ok), "worst_error_over_bound": worst, "max_abs_error": plain,
            "error": "" if ok else "the update is not p - lr * mean(grad)"}


def main():
    rank, size, out_dir, cases = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], json.loads(sys.argv[4])
    import faulthandler
    import signal
    faulthandler.register(signal.SIGUSR1, all_threads=True)  # the launcher's timeout: where every thread stands

    import numpy as np
    import torch
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
        if c.get("op"):
            import tips_amd
            _lib.call("tips_set_algorithm", ALGO_NAMES["auto"])
            tips_amd.set_op_scaling(True)
            results.append((grads_case if c["op"] == "grads" else optimizer_case)(c, rank, size))
            tips_amd.set_op_scaling(False)
            continue
        _lib.call("tips_set_algorithm", ALGO_NAMES[c["algo"]])
        x = to_dev(inputs(c, size)[rank])
        y = x if c.get("inplace") else torch.empty_like(x)
        rc = L.tips_allreduce_scaled(x.data_ptr(), y.data_ptr(), c["n"], c["dtype"], c["pre"], c["post"], sp)
        torch.cuda.synchronize()
        res = {"case": c, "rc": int(rc), "ok": rc == 0, "error": "" if rc == 0 else _lib.last_error()}
        if rc == 0:
            np.save(os.path.join(out_dir, "case%d_rank%d.npy" % (i, rank)), from_dev(y, c["dtype"]))
        results.append(res)
    L.tips_shutdown()
    print(json.dumps({"rank": rank, "results": results}), flush=True)


if __name__ == "__main__":
    main()
