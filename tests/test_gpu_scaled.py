"""-m gpu: the scaled forms of the sum, fold and copy kernels and the scaled allreduce, bit-exact
against the numpy definition (tests/scaled_util.py): result = post * SUM_r (pre * x_r), every
multiply and add a separate IEEE operation in fp32 (f64 for float64), one rounding per kernel.

The factors are not powers of two (1/3, 0.7): with 1/3 a fused multiply-add changes about 29 % of
N(0,3) float32 elements and a factor applied after the add instead of before it about 38 %
(test_scaled_cpu.py checks that the cases tell them apart), so bit-exactness here means separate
operations in the defined places.

tips_bucket_sum_scaled marks both operands raw (mask 3) and behaves as mask 0 with prescale 1;
mask 1 (only the local operand raw) is what a ring step after the first runs, covered by the p = 3
ring cases below. No entry point of the C-ABI reaches mask 2 (only the second operand raw).
"""
import functools
import json
import os
import signal
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

import plan_util
import scaled_util
from gpu_util import BF16, F16, F32, F64, I32, from_dev, rand, same_bits, stream, to_dev, with_specials
from scaled_util import FLOAT_DTYPES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [1, 3, 4099, 300007, 3 * (1 << 20) + 5]  # the last crosses a full round of XCD stripes
FACTORS = [(1.0 / 3.0, 0.7), (1.0, 1.0 / 3.0), (1.0 / 3.0, 1.0)]
MAXSRC = 16


def same(got, exp, dtype):
    """same_bits, and on a difference where and what (the first few elements), for the failure report."""
    if same_bits(got, exp, dtype):
        return True
    g, e = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(exp).reshape(-1)
    gb, eb = g.view("u%d" % g.itemsize), e.view("u%d" % e.itemsize)
    idx = np.nonzero(gb != eb)[0]
    print("%d of %d elements differ; first at %s: got %s (%s), expected %s (%s)" % (
        idx.size, g.size, idx[:6].tolist(), g[idx[:6]].tolist(), [hex(int(v)) for v in gb[idx[:6]]],
        e[idx[:6]].tolist(), [hex(int(v)) for v in eb[idx[:6]]]))
    return False


@functools.lru_cache(maxsize=2)
def pool(dtype, n):
    """16 seeded inputs of one (dtype, n), the first with specials; shared by the cases (read only)."""
    rng = np.random.default_rng(77 + 31 * dtype + n % 1009)
    ins = [rand(dtype, n, rng) for _ in range(MAXSRC)]
    ins[0] = with_specials(ins[0], dtype)
    for x in ins:
        x.setflags(write=False)
    return ins


@pytest.mark.parametrize("pre,post", FACTORS)
@pytest.mark.parametrize("dtype", FLOAT_DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_bucket_sum_scaled_matches_the_definition(gpu, n, dtype, pre, post):
    import torch
    from tips_amd import _lib
    a, b = pool(dtype, n)[:2]
    exp = scaled_util.scaled_sum([a, b], [True, True], pre, post, dtype)
    da, db = to_dev(a), to_dev(b)
    dc = torch.empty_like(da)
    _lib.call("tips_bucket_sum_scaled", dc.data_ptr(), da.data_ptr(), db.data_ptr(), n, dtype, pre, post, stream())
    torch.cuda.synchronize()
    assert same(from_dev(dc, dtype), exp, dtype)
    # in place into either operand
    _lib.call("tips_bucket_sum_scaled", da.data_ptr(), da.data_ptr(), db.data_ptr(), n, dtype, pre, post, stream())
    torch.cuda.synchronize()
    assert same(from_dev(da, dtype), exp, dtype)
    da = to_dev(a)
    _lib.call("tips_bucket_sum_scaled", db.data_ptr(), da.data_ptr(), db.data_ptr(), n, dtype, pre, post, stream())
    torch.cuda.synchronize()
    assert same(from_dev(db, dtype), exp, dtype)
    if n > 1:  # pointers offset by one element: not 16-B aligned, the scalar fallback
        da, db = to_dev(a), to_dev(b)
        dc = torch.zeros_like(da)
        _lib.call("tips_bucket_sum_scaled", dc[1:].data_ptr(), da[1:].data_ptr(), db[1:].data_ptr(), n - 1, dtype, pre,
                  post, stream())
        torch.cuda.synchronize()
        got = from_dev(dc, dtype)
        assert same(got[1:], exp[1:], dtype) and got.view(np.uint8)[:a.itemsize].max() == 0


@pytest.mark.parametrize("nsrc", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("dtype", FLOAT_DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_multi_sum_scaled_matches_the_definition(gpu, n, dtype, nsrc):
    import torch
    from tips_amd import _lib
    ins = pool(dtype, n)[:nsrc]
    devs = [to_dev(x) for x in ins]
    out = torch.empty_like(devs[0])
    pp, _keep = _lib.ptr_array([d.data_ptr() for d in devs])
    for pre, post in (FACTORS if n == 4099 else FACTORS[:1]):
        exp = scaled_util.scaled_sum(ins, [True] * nsrc, pre, post, dtype)
        _lib.call("tips_multi_sum_scaled", out.data_ptr(), pp, nsrc, n, dtype, pre, post, stream())
        torch.cuda.synchronize()
        assert same(from_dev(out, dtype), exp, dtype), (pre, post)
    pre, post = FACTORS[0]
    if n > 1:  # in place into the last source, through views offset by one element (the scalar fallback)
        pp, _keep = _lib.ptr_array([d[1:].data_ptr() for d in devs])
        _lib.call("tips_multi_sum_scaled", devs[-1][1:].data_ptr(), pp, nsrc, n - 1, dtype, pre, post, stream())
        torch.cuda.synchronize()
        exp = scaled_util.scaled_sum([x[1:] for x in ins], [True] * nsrc, pre, post, dtype)
        got = from_dev(devs[-1], dtype)
        assert same(got[1:], exp, dtype) and same(got[:1], ins[-1][:1], dtype)
    else:  # in place, aligned
        _lib.call("tips_multi_sum_scaled", devs[-1].data_ptr(), pp, nsrc, n, dtype, pre, post, stream())
        torch.cuda.synchronize()
        assert same(from_dev(devs[-1], dtype), scaled_util.scaled_sum(ins, [True] * nsrc, pre, post, dtype), dtype)


@pytest.mark.parametrize("dtype", FLOAT_DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_scale_matches_the_definition(gpu, n, dtype):
    import torch
    from tips_amd import _lib
    a = pool(dtype, n)[0]
    f = 1.0 / 3.0
    exp = scaled_util.scaled_sum([a], [True], f, 1.0, dtype)
    da = to_dev(a)
    dc = torch.empty_like(da)
    _lib.call("tips_scale", dc.data_ptr(), da.data_ptr(), n, dtype, f, stream())
    torch.cuda.synchronize()
    assert same(from_dev(dc, dtype), exp, dtype)
    _lib.call("tips_scale", da.data_ptr(), da.data_ptr(), n, dtype, f, stream())  # in place
    torch.cuda.synchronize()
    assert same(from_dev(da, dtype), exp, dtype)
    if n > 1:  # offset by one element: the scalar fallback
        da = to_dev(a)
        dc = torch.zeros_like(da)
        _lib.call("tips_scale", dc[1:].data_ptr(), da[1:].data_ptr(), n - 1, dtype, f, stream())
        torch.cuda.synchronize()
        got = from_dev(dc, dtype)
        assert same(got[1:], exp[1:], dtype) and got.view(np.uint8)[:a.itemsize].max() == 0


@pytest.mark.parametrize("dtype", FLOAT_DTYPES + [I32])
def test_factors_of_one_are_the_plain_kernels(gpu, dtype):
    """(1, 1) dispatches to the unscaled launchers: the bits of tips_bucket_sum / tips_multi_sum
    (integer dtypes included: nothing to scale is not an error)."""
    import torch
    from tips_amd import _lib
    n = 300007
    rng = np.random.default_rng(3 + dtype)
    ins = [with_specials(rand(dtype, n, rng), dtype)] + [rand(dtype, n, rng) for _ in range(4)]
    devs = [to_dev(x) for x in ins]
    plain, scaled = torch.empty_like(devs[0]), torch.empty_like(devs[0])
    _lib.call("tips_bucket_sum", plain.data_ptr(), devs[0].data_ptr(), devs[1].data_ptr(), n, dtype, stream())
    _lib.call("tips_bucket_sum_scaled", scaled.data_ptr(), devs[0].data_ptr(), devs[1].data_ptr(), n, dtype, 1.0, 1.0,
              stream())
    torch.cuda.synchronize()
    assert same(from_dev(scaled, dtype), from_dev(plain, dtype), dtype)
    for nsrc in (2, 3, 5):
        pp, _keep = _lib.ptr_array([d.data_ptr() for d in devs[:nsrc]])
        _lib.call("tips_multi_sum", plain.data_ptr(), pp, nsrc, n, dtype, stream())
        _lib.call("tips_multi_sum_scaled", scaled.data_ptr(), pp, nsrc, n, dtype, 1.0, 1.0, stream())
        torch.cuda.synchronize()
        assert same(from_dev(scaled, dtype), from_dev(plain, dtype), dtype)
    if dtype in FLOAT_DTYPES:  # and the definition with factors 1 is that fold (`scaled` holds the 5-source one)
        assert same(from_dev(scaled, dtype), scaled_util.scaled_sum(ins[:5], [True] * 5, 1.0, 1.0, dtype), dtype)


@pytest.mark.parametrize("dtype", FLOAT_DTYPES)
def test_allreduce_scaled_at_one_rank(gpu, dtype):
    """One rank: the scaled copy - device pointers out of place and in place, host pointers (the
    staged path, and the pipelined pieces for a buffer above TIPS_HOST_PIECE_BYTES)."""
    import torch
    from tips_amd import _lib
    pre, post = FACTORS[0]
    n = 300007
    a = pool(dtype, n)[0]
    exp = scaled_util.scaled_sum([a], [True], pre, post, dtype)
    da = to_dev(a)
    dc = torch.empty_like(da)
    _lib.call("tips_allreduce_scaled", da.data_ptr(), dc.data_ptr(), n, dtype, pre, post, stream())
    _lib.call("tips_allreduce_scaled", da.data_ptr(), da.data_ptr(), n, dtype, pre, post, stream())
    torch.cuda.synchronize()
    assert same(from_dev(dc, dtype), exp, dtype) and same(from_dev(da, dtype), exp, dtype)
    x = a.copy()
    y = np.empty_like(x)
    _lib.call("tips_allreduce_scaled", x.ctypes.data, y.ctypes.data, n, dtype, pre, post, None)
    assert same(y, exp, dtype)
    _lib.call("tips_allreduce_scaled", x.ctypes.data, x.ctypes.data, n, dtype, pre, post, None)  # host, in place
    assert same(x, exp, dtype)
    os.environ["TIPS_HOST_PIECE_BYTES"] = str(256 << 10)  # (read per call) several pipelined pieces
    try:
        x = a.copy()
        _lib.call("tips_allreduce_scaled", x.ctypes.data, y.ctypes.data, n, dtype, pre, post, None)
    finally:
        del os.environ["TIPS_HOST_PIECE_BYTES"]
    assert same(y, exp, dtype)


def test_fused_flat_scaled_at_one_rank(gpu):
    """40 tensors of mixed counts, two of them below 16 bytes: the pack, then one in-place scale of
    the flat buffer - every tensor at its layout offset is (x * pre) * post."""
    import ctypes
    import torch
    from tips_amd import _lib
    pre, post = FACTORS[0]
    rng = np.random.default_rng(40)
    counts = [1, 3] + [int(c) for c in rng.integers(5, 70000, size=38)]
    ins = [rand(F32, c, rng) for c in counts]
    devs = [to_dev(x) for x in ins]
    cp, _k1 = _lib.i64_array(counts)
    offs = (ctypes.c_int64 * len(counts))()
    total = _lib.call("tips_fused_layout", cp, len(counts), F32, offs)
    flat = torch.zeros(total // 4, dtype=torch.float32, device="cuda")
    pp, _k2 = _lib.ptr_array([d.data_ptr() for d in devs])
    _lib.call("tips_fused_allreduce_flat_scaled", pp, cp, len(counts), F32, flat.data_ptr(), pre, post, stream())
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    for x, o, d in zip(ins, offs, devs):
        exp = scaled_util.scaled_sum([x], [True], pre, post, F32)
        assert same(got[o // 4:o // 4 + x.size], exp, F32)
        assert same(from_dev(d, F32), x, F32)  # inputs unchanged


def test_python_allreduce_average_follows_the_switch(gpu):
    import torch
    x = torch.from_numpy(pool(F32, 4099)[1].copy()).cuda()
    gpu.set_op_scaling(False)
    assert torch.equal(gpu.allreduce(x, op=gpu.Average, prescale_factor=1.0 / 3.0), x)
    gpu.set_op_scaling(True)
    try:
        got = gpu.allreduce(x, op=gpu.Average, prescale_factor=1.0 / 3.0)
        torch.cuda.synchronize()
        exp = scaled_util.scaled_sum([x.cpu().numpy()], [True], 1.0 / 3.0, 1.0, F32)
        assert same(got.cpu().numpy(), exp, F32)
        assert same(gpu.allreduce_scaled(x, 1.0 / 3.0, 0.7).cpu().numpy(),
                         scaled_util.scaled_sum([x.cpu().numpy()], [True], 1.0 / 3.0, 0.7, F32), F32)
        with pytest.raises(ValueError):
            gpu.allreduce(torch.ones(4, dtype=torch.int32, device="cuda"), op=gpu.Average)
    finally:
        gpu.set_op_scaling(False)


@pytest.mark.parametrize("p", [2, 3, 8, 16])
def test_derived_error_bound(gpu, p):
    """fp32, inputs U[0.5, 1.5): one multiply per input, p - 1 adds, one multiply, and the factors'
    conversion to fp32 - the result is within (p + 2) * 2^-24 of the float64 value, relatively."""
    import torch
    from tips_amd import _lib
    pre, post = FACTORS[0]
    n = 4099
    rng = np.random.default_rng(p)
    ins = [rand(F32, n, rng, "positive") for _ in range(p)]
    devs = [to_dev(x) for x in ins]
    out = torch.empty_like(devs[0])
    pp, _keep = _lib.ptr_array([d.data_ptr() for d in devs])
    _lib.call("tips_multi_sum_scaled", out.data_ptr(), pp, p, n, F32, pre, post, stream())
    torch.cuda.synchronize()
    ref = post * sum(pre * x.astype(np.float64) for x in ins)
    err = np.abs(from_dev(out, F32).astype(np.float64) - ref) / ref
    print("p = %d: max relative error %.3g, bound %.3g" % (p, err.max(), (p + 2) * 2.0 ** -24))
    assert err.max() <= (p + 2) * 2.0 ** -24


# ---------------------------------------------------------------------------
# over RCCL ranks (one process per rank on this one GPU, socket transport)

def run_scaled_job(p, cases, out_dir, timeout=240, **extra_env):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, TIPS_NO_RCCL="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               TIPS_BOOTSTRAP_PORT=str(port), NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1", TIPS_VERBOSE="1")
    env.update(extra_env)
    t0 = time.time()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "scaled_worker.py"), str(r), str(p), str(out_dir),
                               json.dumps(cases)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for r in range(p)]
    outs = []
    try:
        for pr in procs:
            o, e = pr.communicate(timeout=timeout)
            outs.append((pr.returncode, o, e))
    except subprocess.TimeoutExpired:
        for pr in procs:  # a hang: every worker still running dumps its threads' stacks (faulthandler)
            if pr.poll() is None:
                pr.send_signal(signal.SIGUSR1)
        time.sleep(2)
        tails = []
        for r, pr in enumerate(procs):
            pr.kill()
            o, e = pr.communicate()
            tails.append("rank %d (rc %s):\n%s\n--- stdout:\n%s" % (r, pr.returncode, e[-4000:], o[-2000:]))
        raise AssertionError("job timed out after %d s\n%s" % (timeout, "\n".join(tails)))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    results = []
    for r, (rc, o, e) in enumerate(outs):
        assert rc == 0, "rank %d exited %d:\n%s\n--- stdout:\n%s" % (r, rc, e[-3000:], o[-3000:])
        results.append(json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1]))
    print("scaled job p = %d, %d cases: %.1f s" % (p, len(cases), time.time() - t0))
    bad = ["rank %d: %r" % (res["rank"], c) for res in results for c in res["results"] if not c["ok"]]
    assert not bad, "\n".join(bad[:12])
    return results


@pytest.mark.parametrize("p", [2, 3])
def test_scaled_schedules_over_rccl(gpu, p, tmp_path):
    """tips_allreduce_scaled under ring, direct and one-shot over p RCCL ranks: every rank's output
    bit-exact against the scaled plan interpreter (which derives, from how many ranks each element
    has absorbed, where pre and post belong); one case under TIPS_ALGO_RCCL, where the factors are
    applied unfused around ncclAllReduce, within (p + 2) ulp of the definition."""
    pre, post = FACTORS[0]
    cases = []
    for algo in ("ring", "direct", "oneshot"):
        for dtype in FLOAT_DTYPES:
            for n in (1, 4099, 300007):
                cases.append({"dtype": dtype, "n": n, "seed": 50 * dtype + n % 17, "algo": algo, "pre": pre, "post": post})
        cases.append({"dtype": F32, "n": 262147, "seed": 5, "algo": algo, "pre": pre, "post": post, "inplace": True})
    cases.append({"dtype": F32, "n": 70001, "seed": 9, "algo": "rccl", "pre": pre, "post": post, "kind": "positive"})
    run_scaled_job(p, cases, tmp_path)
    algos = {"ring": plan_util.RING, "direct": plan_util.DIRECT, "oneshot": plan_util.ONESHOT}
    for i, c in enumerate(cases):
        dtype, n = c["dtype"], c["n"]
        ins = [rand(dtype, n, np.random.default_rng(c["seed"] + r), c.get("kind", "normal")) for r in range(p)]
        got = [np.load(os.path.join(tmp_path, "case%d_rank%d.npy" % (i, r))) for r in range(p)]
        if c["algo"] == "rccl":
            ref = post * sum(pre * x.astype(np.float64) for x in ins)
            for g in got:
                ulps = np.abs(g.astype(np.float64) - ref) / np.spacing(ref.astype(np.float32)).astype(np.float64)
                print("rccl, p = %d: max error %.2f ulp" % (p, ulps.max()))
                assert ulps.max() <= p + 2
            continue
        plans = [plan_util.dump(algos[c["algo"]], p, r, n, dtype) for r in range(p)]
        exp = scaled_util.interpret(plans, ins, dtype, pre, post, inplace=bool(c.get("inplace")))
        for r in range(p):
            assert same(got[r], exp[r], dtype), (c, r)


def test_average_through_the_python_surface_over_rccl(gpu, tmp_path):
    """set_op_scaling(True) over 3 RCCL ranks: allreduce_grads(op=Average) on config 5's gradient
    list, bit-exact against the fold times 1/3; DistributedOptimizer(op=Average,
    gradient_predivide_factor=2).step() against the average recomputed in float64."""
    cases = [{"op": "grads", "seed": 4}, {"op": "optimizer", "seed": 7, "f": 2.0}]
    results = run_scaled_job(3, cases, tmp_path)
    for res in results:
        print("rank %d: optimizer worst error / bound %.3g (max abs %.3g)" % (
            res["rank"], res["results"][1]["worst_error_over_bound"], res["results"][1]["max_abs_error"]))
