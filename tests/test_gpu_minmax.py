"""-m gpu: MAX and MIN through tips_bucket_reduce, tips_multi_reduce and tips_allreduce_op, against the
numpy definition of tests/minmax_util.py: exact in the storage type, integers signed, floats by
IEEE 754-2019 maximum / minimum (a NaN in any operand gives a NaN, -0 < +0, subnormals kept). The
result does not depend on the operands' order, so the one reference serves the 2-input launch, every
launch shape of the fold, the scalar kernels and the ring, direct and one-shot schedules alike: the
bits where the reference is a number, NaN-ness where it is a NaN.
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

import minmax_util as mm
from gpu_util import ALL_DTYPES, BF16, F16, F32, F64, I32, I64, NPDT, from_dev, rand, stream, to_dev
from minmax_util import MAX, MIN, OPS, same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [1, 3, 4099, 300007, 3 * (1 << 20) + 5]  # the last crosses a full round of XCD stripes
NSRCS = [1, 2, 3, 4, 8, 16]
SUM = 0


# ---------------------------------------------------------------------------
# tips_bucket_reduce

@functools.lru_cache(maxsize=2)
def pair_case(dtype, n):
    """The two operands of one (dtype, n) and both ops' references; shared by the cases (read only)."""
    a, b = mm.pair_inputs(dtype, n, 300 + 7 * dtype + n % 1009)
    exp = {op: mm.ref([a, b], dtype, op) for op in OPS}
    for x in (a, b, exp[MAX], exp[MIN]):
        x.setflags(write=False)
    return a, b, exp


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_bucket_reduce_matches_the_definition(gpu, op, dtype, n):
    import torch
    from tips_amd import _lib
    a, b, exps = pair_case(dtype, n)
    exp = exps[op]
    da, db = to_dev(a), to_dev(b)
    dc = torch.empty_like(da)
    _lib.call("tips_bucket_reduce", dc.data_ptr(), da.data_ptr(), db.data_ptr(), n, dtype, op, stream())
    torch.cuda.synchronize()
    assert same(from_dev(dc, dtype), exp, dtype)
    # in place into either operand
    _lib.call("tips_bucket_reduce", da.data_ptr(), da.data_ptr(), db.data_ptr(), n, dtype, op, stream())
    torch.cuda.synchronize()
    assert same(from_dev(da, dtype), exp, dtype)
    da = to_dev(a)
    _lib.call("tips_bucket_reduce", db.data_ptr(), da.data_ptr(), db.data_ptr(), n, dtype, op, stream())
    torch.cuda.synchronize()
    assert same(from_dev(db, dtype), exp, dtype)
    if n > 1:  # pointers offset by one element: not 16-B aligned, the scalar kernel
        db = to_dev(b)
        dc = torch.zeros_like(da)
        _lib.call("tips_bucket_reduce", dc[1:].data_ptr(), da[1:].data_ptr(), db[1:].data_ptr(), n - 1, dtype, op, stream())
        torch.cuda.synchronize()
        got = from_dev(dc, dtype)
        assert same(got[1:], exp[1:], dtype) and got.view(np.uint8)[:a.itemsize].max() == 0


# ---------------------------------------------------------------------------
# tips_multi_reduce: sizes in bytes, so that every dtype reaches the same launch shapes of run_multi

def fold_counts(dtype):
    """Element counts: 4099 (256 lanes x 1 vector); for the 32-bit types 4 MiB (4 vectors per lane
    beyond 4 sources); just over 12 MiB (the capped 128-lane launch from 4 sources on)."""
    es = np.dtype(NPDT[dtype]).itemsize
    counts = [4099, (3 * (1 << 20) + 5) * 4 // es]
    if es == 4:
        counts.insert(1, 1 << 20)
    return counts


FOLD_CASES = [(dtype, n) for dtype in ALL_DTYPES for n in fold_counts(dtype)]


@functools.lru_cache(maxsize=1)
def fold_sources(dtype, n):
    """16 sources of one (dtype, n): four seeded random arrays and rotations of them (a rotation by
    a few elements meets other values at every index), the crossed specials at the start of the
    first two. Read only."""
    rng = np.random.default_rng(900 + 13 * dtype + n % 1013)
    base = [rand(dtype, n, rng) for _ in range(4)]
    srcs = [np.roll(base[j % 4], 17 * (j // 4)) for j in range(16)]
    ca, cb = mm.crossed_specials(dtype)
    k = min(n, ca.size)
    srcs[0][:k], srcs[1][:k] = ca[:k], cb[:k]
    for x in srcs:
        x.setflags(write=False)
    return srcs


@pytest.mark.parametrize("nsrc", NSRCS)
@pytest.mark.parametrize("dtype,n", FOLD_CASES)
def test_multi_reduce_matches_the_definition(gpu, dtype, n, nsrc):
    import torch
    from tips_amd import _lib
    # a NaN in exactly one source, and a -0 against +0 in the others, for each source position
    ins = mm.planted(fold_sources(dtype, n)[:nsrc], dtype)
    devs = [to_dev(x) for x in ins]
    out = torch.empty_like(devs[0])
    pp, _keep = _lib.ptr_array([d.data_ptr() for d in devs])
    exps = {op: mm.ref(ins, dtype, op) for op in OPS}
    for op in OPS:
        _lib.call("tips_multi_reduce", out.data_ptr(), pp, nsrc, n, dtype, op, stream())
        torch.cuda.synchronize()
        assert same(from_dev(out, dtype), exps[op], dtype), op
    if n == 4099:  # one unaligned case per (dtype, nsrc): every pointer offset by one element, the scalar kernel
        out.zero_()
        po, _keep2 = _lib.ptr_array([d[1:].data_ptr() for d in devs])
        _lib.call("tips_multi_reduce", out[1:].data_ptr(), po, nsrc, n - 1, dtype, MIN, stream())
        torch.cuda.synchronize()
        got = from_dev(out, dtype)
        assert same(got[1:], exps[MIN][1:], dtype) and got.view(np.uint8)[:got.itemsize].max() == 0
    # in place into source 0
    _lib.call("tips_multi_reduce", devs[0].data_ptr(), pp, nsrc, n, dtype, MAX, stream())
    torch.cuda.synchronize()
    assert same(from_dev(devs[0], dtype), exps[MAX], dtype)
    for j in range(1, nsrc):  # the other sources are only read
        if j in (1, nsrc - 1):
            assert np.array_equal(from_dev(devs[j], dtype).view(np.uint8), ins[j].view(np.uint8))


# ---------------------------------------------------------------------------
# op = SUM is the plain twin; one rank; the Python surface

@pytest.mark.parametrize("dtype", [F32, I32])
def test_sum_through_the_new_calls_is_the_plain_twin(gpu, dtype):
    import torch
    from tips_amd import _lib
    n = 300007
    ins = fold_sources(dtype, n)[:5]
    devs = [to_dev(x) for x in ins]
    plain, new = torch.empty_like(devs[0]), torch.empty_like(devs[0])
    bits = lambda t: from_dev(t, dtype).view(np.uint8)  # noqa: E731
    _lib.call("tips_bucket_sum", plain.data_ptr(), devs[0].data_ptr(), devs[1].data_ptr(), n, dtype, stream())
    _lib.call("tips_bucket_reduce", new.data_ptr(), devs[0].data_ptr(), devs[1].data_ptr(), n, dtype, SUM, stream())
    torch.cuda.synchronize()
    assert np.array_equal(bits(new), bits(plain))
    for nsrc in (1, 2, 3, 5):
        pp, _keep = _lib.ptr_array([d.data_ptr() for d in devs[:nsrc]])
        _lib.call("tips_multi_sum", plain.data_ptr(), pp, nsrc, n, dtype, stream())
        _lib.call("tips_multi_reduce", new.data_ptr(), pp, nsrc, n, dtype, SUM, stream())
        torch.cuda.synchronize()
        assert np.array_equal(bits(new), bits(plain)), nsrc
    _lib.call("tips_allreduce", devs[2].data_ptr(), plain.data_ptr(), n, dtype, SUM, stream())
    _lib.call("tips_allreduce_op", devs[2].data_ptr(), new.data_ptr(), n, dtype, SUM, stream())
    torch.cuda.synchronize()
    assert np.array_equal(bits(new), bits(plain)) and np.array_equal(bits(new), ins[2].view(np.uint8))


@pytest.mark.parametrize("dtype", ALL_DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_allreduce_op_at_one_rank(gpu, op, dtype):
    """One rank: the copy, or nothing in place - device pointers and host (numpy) pointers."""
    import torch
    from tips_amd import _lib
    n = 300007
    a = fold_sources(dtype, n)[0]
    da = to_dev(a)
    dc = torch.zeros_like(da)
    _lib.call("tips_allreduce_op", da.data_ptr(), dc.data_ptr(), n, dtype, op, stream())
    _lib.call("tips_allreduce_op", da.data_ptr(), da.data_ptr(), n, dtype, op, stream())
    torch.cuda.synchronize()
    assert same(from_dev(dc, dtype), a, dtype) and same(from_dev(da, dtype), a, dtype)
    x = a.copy()
    y = np.zeros_like(x)
    _lib.call("tips_allreduce_op", x.ctypes.data, y.ctypes.data, n, dtype, op, None)
    assert same(y, a, dtype)
    _lib.call("tips_allreduce_op", x.ctypes.data, x.ctypes.data, n, dtype, op, None)  # host, in place
    assert same(x, a, dtype)


def test_python_allreduce_max_min_at_one_rank(gpu):
    import torch
    a = fold_sources(F32, 4099)[0]
    t = torch.from_numpy(a.copy()).cuda()
    for op in (gpu.Max, gpu.Min):
        got = gpu.allreduce(t, op=op)
        torch.cuda.synchronize()
        assert got is not t and same(got.cpu().numpy(), a, F32)
        got = gpu.allreduce(a, op=op)  # numpy: the host path
        assert isinstance(got, np.ndarray) and got is not a and same(got, a, F32)
    gpu.set_op_scaling(True)  # whatever the switch says
    try:
        assert same(gpu.allreduce(t, op=gpu.Max).cpu().numpy(), a, F32)
    finally:
        gpu.set_op_scaling(False)
    h = torch.from_numpy(fold_sources(F16, 4099)[2].copy()).cuda()  # Compression composes: compress, reduce, decompress
    got = gpu.allreduce(h.float(), op=gpu.Min, compression=gpu.Compression.fp16)
    assert got.dtype == torch.float32 and same(got.half().cpu().numpy(), h.cpu().numpy(), F16)


# ---------------------------------------------------------------------------
# over RCCL ranks (one process per rank on this one GPU, socket transport)

def run_minmax_job(p, cases, out_dir, timeout=240, **extra_env):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, TIPS_NO_RCCL="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               TIPS_BOOTSTRAP_PORT=str(port), NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1", TIPS_VERBOSE="1")
    env.update(extra_env)
    t0 = time.time()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "minmax_worker.py"), str(r), str(p), str(out_dir),
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
    print("minmax job p = %d, %d cases: %.1f s" % (p, len(cases), time.time() - t0))
    bad = ["rank %d: %r" % (res["rank"], c) for res in results for c in res["results"] if not c["ok"]]
    assert not bad, "\n".join(bad[:12])
    return results


@pytest.mark.parametrize("p", [2, 3])
def test_minmax_schedules_over_rccl(gpu, p, tmp_path):
    """tips_allreduce_op under ring, direct and one-shot over p RCCL ranks, the specials arriving
    from different ranks: every rank's output against the numpy reference over the p inputs. And in
    the same job: ncclMax under TIPS_ALGO_RCCL on finite, zero-free data (bit-exact: a compare
    rounds nothing); host buffers; the peer schedule's refusal on every rank (TIPS_ERR_UNSUPPORTED,
    and the job goes on); at p = 3 the Python surface, tips.allreduce(t, op=tips.Max)."""
    cases = []
    for algo in ("ring", "direct", "oneshot"):
        for op in OPS:
            for dtype in (F32, BF16, I64):
                for n in (1, 4099, 300007):
                    cases.append({"dtype": dtype, "n": n, "seed": 60 * dtype + n % 19 + op, "algo": algo, "op": op})
            for dtype in (F64, I32, F16):
                cases.append({"dtype": dtype, "n": 4099, "seed": 7 * dtype + op, "algo": algo, "op": op})
        cases.append({"dtype": F32, "n": 262147, "seed": 5, "algo": algo, "op": MIN if algo == "direct" else MAX, "inplace": True})
    cases.append({"dtype": F32, "n": 70001, "seed": 9, "algo": "rccl", "op": MAX, "inputs": "finite"})
    cases.append({"dtype": F16, "n": 70001, "seed": 12, "algo": "auto", "op": MIN, "where": "host"})
    cases.append({"dtype": F32, "n": 4099, "seed": 3, "algo": "peer", "op": MAX, "expect": -5})
    cases.append({"dtype": I32, "n": 4099, "seed": 4, "algo": "ring", "op": MIN})  # (the job goes on after the refusal)
    if p == 3:
        cases.append({"dtype": BF16, "n": 70001, "seed": 21, "algo": "auto", "op": MAX, "where": "python"})
    results = run_minmax_job(p, cases, tmp_path)
    for res in results:
        peer = [c for c in res["results"] if c["case"]["algo"] == "peer"][0]
        assert peer["rc"] == -5 and "PEER" in peer["error"], peer
    for i, c in enumerate(cases):
        if c.get("expect"):
            continue
        dtype, n = c["dtype"], c["n"]
        make = mm.finite_nonzero_inputs if c.get("inputs") == "finite" else mm.rank_inputs
        exp = mm.ref(make(dtype, n, c["seed"], p), dtype, c["op"])
        for r in range(p):
            got = np.load(os.path.join(tmp_path, "case%d_rank%d.npy" % (i, r)))
            assert same(got, exp, dtype), (c, r)
