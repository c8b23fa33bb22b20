"""The scaled allreduce (result = post * SUM_r (pre * x_r)) on a host without a GPU: the C-ABI's
declarations and argument checks, the Python switch, and the schedules' plans interpreted with the
scaled arithmetic (tests/scaled_util.py) against closed forms of what each schedule must compute.

The factors are not powers of two: 1/2, 1/4, 1/8 are exact and would hide a factor applied in the
wrong place or twice; with 1/3, a*s + b*s and (a + b)*s differ in the last bit on about a third of
random float32 elements, and so does a fused multiply-add.
"""
import inspect
import os
import re

import numpy as np
import pytest

import plan_util
import scaled_util
from gpu_util import BF16, F16, F32, F64, I32, I64, rand, same_bits, with_specials
from scaled_util import FLOAT_DTYPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALED = ["tips_scale", "tips_bucket_sum_scaled", "tips_multi_sum_scaled", "tips_allreduce_scaled",
          "tips_fused_allreduce_flat_scaled"]
PRE, POST = 1.0 / 3.0, 0.7


def test_header_exports_and_binding_agree():
    from tips_amd import _lib
    with open(os.path.join(REPO, "include", "tips_hip.h")) as f:
        header = f.read()
    L = _lib.lib()
    sigs = {n: (r, a) for n, r, a in _lib._SIGNATURES}
    for name in SCALED:
        m = re.search(r"TIPS_API\s+int\s+%s\(([^;]*)\);" % name, header)
        assert m, "%s is not declared in include/tips_hip.h" % name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert hasattr(L, name), "%s is not exported" % name
        res, args = sigs[name]
        assert len(args) == len(params), (name, params)
        for p, a in zip(params, args):  # every double in the header is a c_double in the binding, and only those
            assert (p.startswith("double ")) == (a.__name__ == "c_double"), (name, p, a)
    with open(os.path.join(REPO, "include", "tips_hip_dev.h")) as f:
        assert "scaled" not in f.read()  # the development header gains nothing


def _ptr(a):
    return a.ctypes.data


def test_argument_errors_before_init():
    """Refused on their arguments alone - no device, no tips_init."""
    from tips_amd import _lib
    L = _lib.lib()
    INVALID, UNSUPPORTED = -1, -5
    x = np.ones(8, np.float64)
    pp, _k = _lib.ptr_array([_ptr(x), _ptr(x)])
    cp, _k2 = _lib.i64_array([8, 8])
    for dtype in (I32, I64):  # an integer dtype with a factor
        assert L.tips_scale(_ptr(x), _ptr(x), 2, dtype, PRE, None) == UNSUPPORTED
        assert L.tips_bucket_sum_scaled(_ptr(x), _ptr(x), _ptr(x), 2, dtype, PRE, 1.0, None) == UNSUPPORTED
        assert L.tips_multi_sum_scaled(_ptr(x), pp, 2, 2, dtype, 1.0, POST, None) == UNSUPPORTED
        assert L.tips_allreduce_scaled(_ptr(x), _ptr(x), 2, dtype, PRE, POST, None) == UNSUPPORTED
        assert L.tips_fused_allreduce_flat_scaled(pp, cp, 2, dtype, _ptr(x), PRE, POST, None) == UNSUPPORTED
        assert "float" in _lib.last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):  # a factor that is not finite
        assert L.tips_scale(_ptr(x), _ptr(x), 2, F32, bad, None) == INVALID
        assert L.tips_bucket_sum_scaled(_ptr(x), _ptr(x), _ptr(x), 2, F32, bad, 1.0, None) == INVALID
        assert L.tips_multi_sum_scaled(_ptr(x), pp, 2, 2, F64, 1.0, bad, None) == INVALID
        assert L.tips_allreduce_scaled(_ptr(x), _ptr(x), 2, F32, 1.0, bad, None) == INVALID
        assert L.tips_fused_allreduce_flat_scaled(pp, cp, 2, F32, _ptr(x), bad, POST, None) == INVALID
        assert "finite" in _lib.last_error()
    assert L.tips_scale(_ptr(x), _ptr(x), -1, F32, PRE, None) == INVALID  # a negative count
    assert L.tips_bucket_sum_scaled(_ptr(x), _ptr(x), _ptr(x), -1, F32, PRE, POST, None) == INVALID
    assert L.tips_multi_sum_scaled(_ptr(x), pp, 2, -1, F32, PRE, POST, None) == INVALID
    assert L.tips_allreduce_scaled(_ptr(x), _ptr(x), -1, F32, PRE, POST, None) == INVALID
    neg, _k3 = _lib.i64_array([8, -8])
    assert L.tips_fused_allreduce_flat_scaled(pp, neg, 2, F32, _ptr(x), PRE, POST, None) == INVALID
    assert L.tips_multi_sum_scaled(_ptr(x), pp, 17, 2, F32, PRE, POST, None) == INVALID
    assert L.tips_scale(_ptr(x), _ptr(x), 2, 9, PRE, None) == INVALID  # an unknown dtype
    assert L.tips_allreduce(_ptr(x), _ptr(x), 2, F32, _lib.OP_MAX, None) == UNSUPPORTED  # (MAX / MIN stay unsupported)


def test_switch_defaults_off_and_signatures_are_unchanged(monkeypatch):
    import tips_amd
    from tips_amd import ops
    if os.environ.get("TIPS_OP_SCALING", "0") != "1":
        assert ops.op_scaling() is False
    assert list(inspect.signature(tips_amd.allreduce).parameters) == [
        "tensor", "average", "device_dense", "device_sparse", "compression", "op", "prescale_factor",
        "postscale_factor", "name"]
    assert list(inspect.signature(tips_amd.allreduce_scaled).parameters) == [
        "tensor", "prescale_factor", "postscale_factor", "name"]
    monkeypatch.setattr(ops, "_op_scaling", False)
    tips_amd.set_op_scaling(True)
    assert ops.op_scaling() is True
    tips_amd.set_op_scaling(0)
    assert ops.op_scaling() is False
    # the environment variable sets the initial value (a fresh interpreter reads it)
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", "from tips_amd import ops; print(ops.op_scaling())"], cwd=REPO,
                       env=dict(os.environ, TIPS_OP_SCALING="1"), capture_output=True, text=True, timeout=120)
    assert r.stdout.strip() == "True", r.stdout + r.stderr


def _toy_model():
    import torch
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Tanh(), torch.nn.Linear(3, 2))


@pytest.mark.parametrize("f", [1.0, 2.0])
def test_distributed_optimizer_average_follows_the_switch(monkeypatch, f):
    """Two fake ranks holding the same gradient (test_python_api.py's harness). Off: op=Average still
    sums (the update is twice the local one). On: every gradient is reduced with prescale = 1/f and
    postscale = f/size, here through tips_amd.allreduce_scaled (host gradients), which the fake
    answers with post * (pre * g + pre * g)."""
    import torch
    import tips_amd
    from tips_amd import ops
    from test_python_api import _fake_two_ranks
    _fake_two_ranks(monkeypatch)
    summed, scaled = [], []
    monkeypatch.setattr(tips_amd, "allreduce", lambda t, **kw: summed.append(1) or t * 2)

    def fake_scaled(t, prescale_factor=1.0, postscale_factor=1.0, name=None):
        scaled.append((prescale_factor, postscale_factor))
        return (t * prescale_factor + t * prescale_factor) * postscale_factor

    monkeypatch.setattr(tips_amd, "allreduce_scaled", fake_scaled)
    lr = 0.1
    x = torch.randn(5, 4)
    for on in (False, True):
        monkeypatch.setattr(ops, "_op_scaling", on)
        del summed[:], scaled[:]
        ref, dist_m = _toy_model(), _toy_model()
        for m in (ref, dist_m):
            m(x).pow(2).sum().backward()
        opt = tips_amd.DistributedOptimizer(torch.optim.SGD(dist_m.parameters(), lr=lr), op=tips_amd.Average,
                                            gradient_predivide_factor=f)
        with torch.no_grad():
            exp = [p - lr * (1 if on else 2) * p.grad for p in ref.parameters()]
        opt.step()
        for p, e in zip(dist_m.parameters(), exp):
            assert torch.allclose(p, e, atol=1e-6)
        if on:
            assert not summed and len(scaled) == 4
            assert all(pre == 1.0 / f and post == f / 2 for pre, post in scaled), scaled
        else:
            assert not scaled and len(summed) == 4


def test_allreduce_honours_the_factors_only_when_switched_on(monkeypatch):
    import torch
    import tips_amd
    from tips_amd import ops
    monkeypatch.setattr(tips_amd, "size", lambda: 4)
    calls = []
    monkeypatch.setattr(tips_amd, "allreduce_op", lambda t, name=None: calls.append("sum") or t)
    monkeypatch.setattr(tips_amd, "allreduce_scaled",
                        lambda t, pre, post, name=None: calls.append((pre, post, name)) or t)
    x = torch.ones(3)
    monkeypatch.setattr(ops, "_op_scaling", False)
    tips_amd.allreduce(x, op=tips_amd.Average, prescale_factor=PRE, postscale_factor=POST)
    assert calls == ["sum"]
    monkeypatch.setattr(ops, "_op_scaling", True)
    del calls[:]
    tips_amd.allreduce(x, op=tips_amd.Average, prescale_factor=PRE, postscale_factor=POST, name="g")
    tips_amd.allreduce(x, op=tips_amd.Sum, prescale_factor=PRE)
    tips_amd.allreduce(x, postscale_factor=POST)
    tips_amd.allreduce(x, op=tips_amd.Sum)  # nothing to scale: the plain SUM
    assert calls == [(PRE, POST / 4, "g"), (PRE, 1.0, None), (1.0, POST, None), "sum"]
    with pytest.raises(ValueError, match="integer"):
        tips_amd.allreduce(torch.ones(3, dtype=torch.int32), op=tips_amd.Average)
    with pytest.raises(ValueError, match="integer"):
        tips_amd.allreduce_grads([np.ones(3, np.int64)], op=tips_amd.Average)


# ---------------------------------------------------------------------------
# the plans, interpreted

ALGOS = {"ring": plan_util.RING, "direct": plan_util.DIRECT, "oneshot": plan_util.ONESHOT}
SIZES = [1, 4099, 70001]


def _inputs(dtype, n, p, seed):
    rng = np.random.default_rng(seed)
    ins = [rand(dtype, n, rng) for _ in range(p)]
    ins[0] = with_specials(ins[0], dtype)
    return ins


@pytest.mark.parametrize("dtype", FLOAT_DTYPES)
@pytest.mark.parametrize("p", [2, 3, 4, 5])
@pytest.mark.parametrize("algo", sorted(ALGOS))
def test_scaled_plans_match_the_closed_forms(oracle, algo, p, dtype):
    for K in (1, 2):
        for n in SIZES:
            ins = _inputs(dtype, n, p, 1000 * p + n % 97 + dtype)
            plans = [plan_util.dump(ALGOS[algo], p, r, n, dtype, depth=K) for r in range(p)]
            # factors 1: the scaled interpreter is the plain one
            plain = plan_util.interpret(plans, ins, dtype)
            for got, exp in zip(scaled_util.interpret(plans, ins, dtype, 1.0, 1.0), plain):
                assert same_bits(got, exp, dtype), (algo, p, K, n, "factors 1")
            closed = (scaled_util.ring_closed_form if algo == "ring" else scaled_util.fold_closed_form)(ins, dtype, PRE, POST)
            for inplace in (False, True):
                for got in scaled_util.interpret(plans, ins, dtype, PRE, POST, inplace=inplace):
                    assert same_bits(got, closed, dtype), (algo, p, K, n, inplace)


def test_the_cases_tell_a_misplaced_factor_and_an_fma_apart():
    """What the factors are chosen for: on N(0,3) float32 at n = 4099, prescale 1/3 applied after the add
    instead of before it, or fused into it, changes a large share of the elements."""
    rng = np.random.default_rng(5)
    a, b = rand(F32, 4099, rng), rand(F32, 4099, rng)
    s = np.float32(PRE)
    right = a * s + b * s
    late = (a + b) * s
    fused = (a.astype(np.float64) * np.float64(s) + (b * s).astype(np.float64)).astype(np.float32)  # fma(a, s, b*s)
    assert np.mean(right != late) > 0.25
    assert np.mean(right != fused) > 0.15
    assert same_bits(scaled_util.scaled_sum([a, b], [True, True], PRE, 1.0, F32), right, F32)


def test_bf16_rounding_is_the_oracles(oracle):
    rng = np.random.default_rng(9)
    w = with_specials((rng.standard_normal(5000) * 3).astype(np.float32), F32)
    import torch
    exp = torch.from_numpy(w).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert same_bits(scaled_util.bf16_round(w), exp, BF16)
