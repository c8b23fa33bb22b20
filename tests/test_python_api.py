"""The tips_amd Python surface on CPU: it mirrors tips.tensorflow's names and
signatures, maps dtypes like the reference (plus f16/bf16), and fails loudly
when the HIP library is missing (no CPU fallback)."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO


def test_reference_names_exist():
    import tips_amd
    # tips/tensorflow/__init__.py:8,17-18 and ops.py/basics.py names used on the allreduce path
    for name in ("allreduce", "allreduce_op", "size", "rank", "shutdown", "size_op", "rank_op", "Compression",
                 "Average", "Sum", "TipsBasics"):
        assert hasattr(tips_amd, name), name
    assert tips_amd.Average == 'Average' and tips_amd.Sum == 'Sum'


def test_allreduce_signature_matches_reference():
    import tips_amd
    params = list(inspect.signature(tips_amd.allreduce).parameters)
    # tips/tensorflow/__init__.py:20-28
    assert params == ["tensor", "average", "device_dense", "device_sparse", "compression", "op", "prescale_factor",
                      "postscale_factor", "name"]
    assert list(inspect.signature(tips_amd.allreduce_op).parameters) == ["tensor", "name"]  # ops.py:61


def test_dtype_codes():
    import torch
    from tips_amd import tensors
    assert tensors.dtype_code(np.zeros(1, np.float32)) == 0
    assert tensors.dtype_code(np.zeros(1, np.float64)) == 1
    assert tensors.dtype_code(np.zeros(1, np.int32)) == 2
    assert tensors.dtype_code(np.zeros(1, np.int64)) == 3
    assert tensors.dtype_code(np.zeros(1, np.float16)) == 4
    assert tensors.dtype_code(torch.zeros(1, dtype=torch.bfloat16)) == 5
    assert tensors.dtype_code(torch.zeros(1, dtype=torch.float32)) == 0
    for bad in (np.zeros(1, np.uint8), torch.zeros(1, dtype=torch.bool), np.zeros(1, np.complex64)):
        with pytest.raises(TypeError, match="Not supported dtype found"):
            tensors.dtype_code(bad)


def test_compression_round_trip():
    import torch
    from tips_amd import Compression
    x = np.linspace(-3, 3, 17).astype(np.float32)
    c, ctx = Compression.fp16.compress(x)
    assert c.dtype == np.float16
    assert Compression.fp16.decompress(c, ctx).dtype == np.float32
    t = torch.linspace(-3, 3, 17)
    c, ctx = Compression.fp16.compress(t)
    assert c.dtype == torch.float16 and Compression.fp16.decompress(c, ctx).dtype == torch.float32
    i = np.arange(5, dtype=np.int32)
    c, ctx = Compression.fp16.compress(i)
    assert c is i  # integers are not compressed (compression.py:55-57)
    assert Compression.none.compress(x) == (x, None)


def test_missing_library_fails_loudly():
    code = ("import tips_amd, numpy as np\n"
            "try:\n"
            "    tips_amd.allreduce(np.ones(3, np.float32))\n"
            "except tips_amd.TipsLibraryError as e:\n"
            "    print('LOUD', e)\n")
    env = dict(os.environ, TIPS_HIP_LIB="/nonexistent/libtips_hip.so")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, env=env, timeout=300)
    assert "LOUD" in r.stdout and "no CPU fallback" in r.stdout, r.stdout + r.stderr


def test_allreduce_without_gpu_raises_not_computes():
    """On a host with no HIP device the op must raise (init fails), never return a host-computed sum."""
    code = ("import tips_amd, numpy as np\n"
            "try:\n"
            "    out = tips_amd.allreduce(np.ones(3, np.float32))\n"
            "    print('COMPUTED', out)\n"
            "except tips_amd.TipsError as e:\n"
            "    print('RAISED', e.code)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, timeout=300)
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    assert "RAISED" in r.stdout, r.stdout + r.stderr


def _fake_two_ranks(monkeypatch):
    """allgather over two ranks that hold the same tensor, without a GPU: the host logic of the sparse
    branch (__init__.py:59-74 of the reference) is what is under test here."""
    import torch
    import tips_amd

    def gather(t, name=None):
        return torch.cat([t, t]) if isinstance(t, torch.Tensor) else np.concatenate([t, t])

    monkeypatch.setattr(tips_amd, "allgather_op", gather)
    monkeypatch.setattr(tips_amd, "size", lambda: 2)
    # dense host gradients go through the fused host path at N > 1: here each through the (faked)
    # tips_amd.allreduce, so the tests below see one reduction per gradient
    monkeypatch.setattr(tips_amd._ops, "fused_allreduce_host_flat", lambda ts: [tips_amd.allreduce(t) for t in ts])
    # (a remembered plan calls the library directly: none here, so every call takes the fake)
    monkeypatch.setattr(tips_amd, "_remember_plan", lambda grads, groups: None)


def test_indexed_slices_take_the_allgather_branch(monkeypatch):
    import tips_amd
    _fake_two_ranks(monkeypatch)
    vals = np.arange(6, dtype=np.float32).reshape(3, 2)
    idx = np.array([4, 0, 4], dtype=np.int64)
    s = tips_amd.allreduce(tips_amd.IndexedSlices(vals, idx, dense_shape=(5, 2)))
    assert isinstance(s, tips_amd.IndexedSlices) and s.dense_shape == (5, 2)
    assert np.array_equal(s.values, np.concatenate([vals, vals])) and np.array_equal(s.indices, np.tile(idx, 2))
    a = tips_amd.allreduce(tips_amd.IndexedSlices(vals, idx, dense_shape=(5, 2)), op=tips_amd.Average)
    assert np.array_equal(a.values, np.concatenate([vals, vals]) / 2)  # the reference divides here


def test_torch_sparse_allreduce_represents_the_sum(monkeypatch):
    import torch
    import tips_amd
    _fake_two_ranks(monkeypatch)
    dense = torch.zeros(6, 3)
    dense[1, 2] = 1.5
    dense[4, 0] = -2.0
    sp = dense.to_sparse()
    out = tips_amd.allreduce(sp)
    assert out.is_sparse and out.shape == dense.shape
    assert torch.equal(out.to_dense(), 2 * dense)
    assert torch.equal(tips_amd.allreduce(sp, op=tips_amd.Average).to_dense(), dense)


def test_allreduce_grads_routes_sparse_to_allgather(monkeypatch):
    import torch
    import tips_amd
    _fake_two_ranks(monkeypatch)
    dense = torch.zeros(4, 2)
    dense[2, 1] = 3.0
    sl = tips_amd.IndexedSlices(np.ones((1, 2), np.float32), np.array([3]), dense_shape=(4, 2))
    out = tips_amd.allreduce_grads([None, dense.to_sparse(), sl])
    assert out[0] is None
    assert torch.equal(out[1].to_dense(), 2 * dense)
    assert np.array_equal(out[2].indices, [3, 3])


def test_allreduce_grads_sparse_as_dense(monkeypatch):
    """sparse_as_dense (reference __init__.py:205-210): IndexedSlices (numpy or torch) and torch sparse
    gradients are densified (repeated rows summed) and then take the dense allreduce."""
    import torch
    import tips_amd
    _fake_two_ranks(monkeypatch)
    monkeypatch.setattr(tips_amd, "allreduce", lambda t, **kw: t * 2)
    sl = tips_amd.IndexedSlices(np.ones((3, 2), np.float32), np.array([1, 3, 1]), dense_shape=(4, 2))
    tsl = tips_amd.IndexedSlices(torch.ones(2, 2), torch.tensor([0, 0]), dense_shape=(3, 2))
    dense = torch.zeros(4, 2)
    dense[2, 1] = 3.0
    out = tips_amd.allreduce_grads([sl, tsl, dense.to_sparse(), None], sparse_as_dense=True, fused=False)
    exp0 = np.zeros((4, 2), np.float32)
    exp0[1] = 2.0
    exp0[3] = 1.0
    assert isinstance(out[0], np.ndarray) and np.array_equal(out[0], 2 * exp0)
    assert torch.equal(out[1], 2 * torch.tensor([[2.0, 2.0], [0.0, 0.0], [0.0, 0.0]]))
    assert not out[2].is_sparse and torch.equal(out[2], 2 * dense)
    assert out[3] is None


def _toy_model():
    import torch
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Tanh(), torch.nn.Linear(3, 2))


def test_distributed_optimizer_sums_gradients_before_step(monkeypatch):
    """DistributedOptimizer (reference __init__.py:252-456) over torch.optim: step() allreduces every
    .grad first; as in the reference the reduction is a SUM even for op=Average (two fake ranks
    holding the same gradient: the update is twice the local one)."""
    import torch
    import tips_amd
    _fake_two_ranks(monkeypatch)
    monkeypatch.setattr(tips_amd, "allreduce", lambda t, **kw: t * 2)
    ref, dist_m = _toy_model(), _toy_model()
    x = torch.randn(5, 4)
    for m in (ref, dist_m):
        m(x).pow(2).sum().backward()
    lr = 0.1
    opt = tips_amd.DistributedOptimizer(torch.optim.SGD(dist_m.parameters(), lr=lr))
    with torch.no_grad():
        exp = [p - lr * 2 * p.grad for p in ref.parameters()]
    opt.step()
    for p, e in zip(dist_m.parameters(), exp):
        assert torch.allclose(p, e, atol=1e-7)


def test_distributed_optimizer_backward_passes_and_validation(monkeypatch):
    import torch
    import tips_amd
    _fake_two_ranks(monkeypatch)
    calls = []
    monkeypatch.setattr(tips_amd, "allreduce", lambda t, **kw: calls.append(1) or t)
    m = _toy_model()
    x = torch.randn(5, 4)
    opt = tips_amd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=0.1), backward_passes_per_step=2,
                                        average_aggregated_gradients=True)
    before = [p.detach().clone() for p in m.parameters()]
    m(x).sum().backward()
    g1 = [p.grad.clone() for p in m.parameters()]
    opt.step()  # first pass: accumulate only
    assert not calls and all(torch.equal(p, b) for p, b in zip(m.parameters(), before))
    m(x).sum().backward()  # .grad now holds both passes
    opt.step()
    assert len(calls) == len(before)
    for p, b, g in zip(m.parameters(), before, g1):  # averaged over the 2 passes: (g + g) / 2 = g
        assert torch.allclose(p, b - 0.1 * g, atol=1e-6)
    with pytest.raises(ValueError, match="gradient_predivide_factor not supported"):
        tips_amd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=0.1), op="Sum", gradient_predivide_factor=2.0)
    with pytest.raises(ValueError, match="groups should be a non-negative integer"):
        tips_amd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=0.1), groups=-1)
    with pytest.raises(ValueError, match="doesn't inherit"):
        tips_amd.DistributedOptimizer(object())


def test_distributed_optimizer_synchronize_then_step(monkeypatch):
    """step() skips its own reduction only after a synchronize() of this very pass with no backward
    after it (the clip-gradients pattern). A synchronize() followed by another backward without a
    step (evaluation), or one in an earlier accumulation pass, does not excuse step(): it reduces
    again, with a warning; a second synchronize() without a backward in between warns too."""
    import warnings
    import torch
    import tips_amd
    _fake_two_ranks(monkeypatch)
    calls = []
    monkeypatch.setattr(tips_amd, "allreduce", lambda t, **kw: calls.append(1) or t)
    m = _toy_model()
    x = torch.randn(5, 4)
    n = len(list(m.parameters()))
    opt = tips_amd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=0.0))
    m(x).sum().backward()
    opt.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        opt.step()  # the clip pattern: reduced once, in synchronize()
    assert len(calls) == n
    opt.zero_grad()
    m(x).sum().backward()
    opt.synchronize()  # e.g. an evaluation that never steps
    opt.zero_grad()
    m(x).sum().backward()
    with pytest.warns(UserWarning, match="before a later backward"):
        opt.step()
    assert len(calls) == 3 * n
    opt.synchronize()
    with pytest.warns(UserWarning, match="called again with no backward"):
        opt.synchronize()
    assert len(calls) == 5 * n
    calls.clear()
    acc = tips_amd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=0.0), backward_passes_per_step=2)
    opt.zero_grad()
    m(x).sum().backward()
    acc.synchronize()  # in the first (accumulation) pass
    acc.step()
    m(x).sum().backward()
    with pytest.warns(UserWarning, match="earlier accumulation pass"):
        acc.step()
    assert len(calls) == 2 * n


def test_distributed_gradient_tape(monkeypatch):
    """DistributedGradientTape (reference __init__.py:460-569): gradient() differentiates, then sums
    the gradients over the ranks (a SUM for op=Average too); an unused source stays None; a single
    source gives a single gradient; a wrapped tape object supplies the gradients; the reference's
    argument validation."""
    import torch
    import tips_amd
    _fake_two_ranks(monkeypatch)
    monkeypatch.setattr(tips_amd, "allreduce", lambda t, **kw: t * 2)
    w = torch.randn(3, requires_grad=True)
    unused = torch.randn(2, requires_grad=True)
    x = torch.randn(3)
    tape = tips_amd.DistributedGradientTape()
    gw, gu = tape.gradient((w * x).sum(), [w, unused])
    assert torch.equal(gw, 2 * x) and gu is None
    assert torch.equal(tape.gradient((w * w).sum(), w), 4 * w.detach())

    class Tape(object):
        def gradient(self, target, sources, output_gradients=None):
            return [torch.ones_like(s) for s in sources]
    assert torch.equal(tips_amd.DistributedGradientTape(Tape()).gradient(None, [w])[0], 2 * torch.ones(3))
    with pytest.raises(ValueError, match="gradient_predivide_factor not supported"):
        tips_amd.DistributedGradientTape(op="Sum", gradient_predivide_factor=2.0)
    with pytest.raises(ValueError, match="groups should be a non-negative integer"):
        tips_amd.DistributedGradientTape(groups=0)
    with pytest.warns(DeprecationWarning):
        tips_amd.DistributedGradientTape(num_groups=2)
    with pytest.raises(ValueError, match="gradient"):
        tips_amd.DistributedGradientTape(object())


def test_fast_list_helper_reads_pointers_counts_and_shapes():
    """tips_amd._fast (the list helper allreduce_grads' device path uses) on CPU tensors: data
    pointers and counts as torch reports them, one hash per shape list, None for a list it must not
    take (another dtype, a strided view, a non-tensor), and max_refcount as sys.getrefcount - 1."""
    import ctypes
    import sys
    import torch
    from tips_amd import _fast
    flat = torch.zeros(4096)
    ts = [flat[0:10].view(2, 5), flat[64:64 + 7], flat[128:128 + 300].view(3, 10, 10), torch.zeros(0)]
    n = len(ts)
    pa, na = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
    a, b = ctypes.addressof(pa), ctypes.addressof(na)
    st, dev, h = _fast.dev_list(ts, a, b, 0)
    assert st == 6 and dev == -1  # c10::ScalarType::Float, CPU
    assert list(pa) == [t.data_ptr() for t in ts] and list(na) == [t.numel() for t in ts]
    # the hash follows the shapes, not only the counts
    ts2 = [flat[0:10].view(5, 2)] + ts[1:]
    assert _fast.dev_list(ts2, a, b, 0)[2] != h
    assert _fast.dev_list(list(ts), a, b, 0)[2] == h
    # lists it leaves to the general path
    assert _fast.dev_list(ts, a, b, 1) is None                       # not device tensors
    assert _fast.dev_list(ts[:2] + [torch.zeros(3, dtype=torch.float64)], a, b, 0) is None
    assert _fast.dev_list([flat[::2]], a, b, 0) is None              # not contiguous
    assert _fast.dev_list([flat[:4], None], a, b, 0) is None
    assert _fast.dev_list([torch.zeros(3).to_sparse()], a, b, 0) is None
    assert _fast.dev_list([torch.empty(3, device="meta")], a, b, 0) is None  # neither CPU nor device
    # cap: the arrays hold n entries; a sequence of any other length is refused before any write
    pa[0] = na[0] = -7
    assert _fast.dev_list(ts + [flat[:1]], a, b, 0, n) is None
    assert pa[0] == -7 and na[0] == -7
    assert _fast.dev_list(ts, a, b, 0, n)[2] == h
    x = torch.zeros(3)
    assert _fast.max_refcount([x]) == sys.getrefcount(x) - 1
    keep = [x, x]
    assert _fast.max_refcount([x]) == sys.getrefcount(x) - 1 and len(keep) == 2
    assert _fast.max_refcount([]) == 0


def test_flat_output_sets_are_not_handed_out_twice():
    """_FlatOutputs.take (allreduce_grads' output sets) returns the views in a new list, made before
    the library call releases the GIL: while one call's outputs are referenced, a second take()
    gets another set; once they are dropped, the first set comes back. (CPU tensors stand in for
    device ones; tips_fused_layout is host-only.)"""
    import gc
    import torch
    from tips_amd import _lib
    from tips_amd.ops import _FlatOutputs
    shapes = (torch.Size([3, 5]), torch.Size([7]), torch.Size([2, 2, 2]))
    fo = _FlatOutputs(shapes, [15, 7, 8], _lib.FLOAT32, torch.float32, torch.device("cpu"))
    f1, v1 = fo.take()
    assert [v.shape for v in v1] == list(shapes)
    f2, v2 = fo.take()
    assert f2.data_ptr() != f1.data_ptr()  # set 1's views are still held
    p1 = f1.data_ptr()
    del v1, f1
    gc.collect()
    f3, v3 = fo.take()
    assert f3.data_ptr() == p1 and v3[0].data_ptr() == p1
    held = v3[1]
    del v3, f3
    f4, v4 = fo.take()
    assert f4.data_ptr() != p1  # one view of set 1 is still held by the caller
    del held


def test_host_output_pool_reuses_only_released_outputs(monkeypatch):
    """allreduce_op's host outputs of >= 1 MiB come from _HostOutPool: a released output is handed
    out again (page-locked once, no fresh pages per call); one still referenced - directly, through
    a numpy view, or through torch's .numpy() on its storage - is not; small outputs are fresh.
    (tips_host_register is stubbed: no GPU here.)"""
    import numpy as np
    import torch
    import tips_amd.ops as ops

    class Stub:
        def tips_host_register(self, p, n):
            return 0
    monkeypatch.setattr(ops._lib, "lib", lambda: Stub())
    pool = ops._HostOutPool()
    src = np.zeros(1 << 19, dtype=np.float32)  # 2 MiB
    a = pool.take(src)
    b = pool.take(src)
    assert a is not b and a.shape == src.shape and a.dtype == src.dtype
    pa = a.ctypes.data
    del a
    c = pool.take(src)
    assert c.ctypes.data == pa
    view = c[::2]
    del c
    assert pool.take(src).ctypes.data != pa and view.size == 1 << 18
    small = np.zeros(100, dtype=np.float32)
    pool.take(small)
    assert (False, "float32", (100,)) not in pool.sets  # (under 1 MiB: a fresh output, not pooled)
    t = torch.zeros(1 << 19)
    x = pool.take(t)
    px = x.data_ptr()
    del x
    y = pool.take(t)
    assert y.data_ptr() == px
    arr = y.numpy()
    del y
    assert pool.take(t).data_ptr() != px and arr.size == 1 << 19


def test_fused_list_refuses_host_tensors():
    """FusedList.allreduce_ reads pointers, counts and dtype in C++ (_fast.dev_list) and falls back
    to the Python checks, with their error text, for a list it does not take: host tensors here."""
    import torch
    from tips_amd.ops import FusedList
    fl = FusedList([3, 4])
    with pytest.raises(ValueError, match="needs device tensors"):
        fl.allreduce_([torch.zeros(3), torch.zeros(4)])
    assert fl.allreduce_([]) == []


def test_evicted_host_flat_sets_unregister_after_last_use(monkeypatch):
    """_HOST_FLAT keeps 16 host list signatures; a set evicted from it stays page-locked only while
    an output of it is alive, and is unregistered once the last one goes (numpy views and
    torch.from_numpy storages both hold the page-locked array). Cycles through 20 signatures.
    (tips_host_register / _unregister are stubbed: no GPU here.)"""
    import gc
    import torch
    import tips_amd.ops as ops

    live = {}

    class Stub:
        def tips_host_register(self, p, n):
            assert p not in live, "address registered twice"
            live[p] = n
            return 0

        def tips_host_unregister(self, p):
            assert p in live
            del live[p]
            return 0

        def tips_fused_layout(self, cp, n, code, offs):
            return ops._lib.lib().tips_fused_layout(cp, n, code, offs)
    real = ops._lib.lib
    monkeypatch.setattr(ops._lib, "lib", lambda: Stub())
    monkeypatch.setattr(ops._lib, "call", lambda name, *a: getattr(Stub(), name)(*a))
    monkeypatch.setattr(Stub, "tips_fused_layout", lambda self, *a: real().tips_fused_layout(*a))
    monkeypatch.setattr(ops, "_HOST_FLAT", {})
    held = []
    for k in range(20):
        srcs = [np.zeros(k + 3, np.float32), np.zeros(7, np.float32)] if k % 2 else \
            [torch.zeros(k + 3), torch.zeros(5)]
        fo = ops._host_flat_outputs(srcs)
        flat, views = fo.take()
        if k == 0:
            held.append(views[1])  # an output of the first (torch) set outlives its eviction
        del flat, views
    gc.collect()
    assert len(ops._HOST_FLAT) == 16
    kept = {tensors_ptr(s[0]) for fo in ops._HOST_FLAT.values() for s in fo.sets}
    # every registration still live belongs to a kept set, or to the output still held
    assert set(live) - kept == {held[0].untyped_storage().data_ptr()}
    del held[:]
    gc.collect()
    assert set(live) == kept


def tensors_ptr(x):
    from tips_amd import tensors
    return tensors.data_ptr(x)


def test_grad_plan_never_matches_a_dead_gradient_or_a_changed_tensor(monkeypatch):
    """_GradPlan (allreduce_grads' remembered split): a gradient that died does not pass for a
    None in the same position, and a None position must stay None; a plan's run() re-checks its
    device groups through the checking reader (here: _dev_list_flat refuses the changed list)."""
    import gc
    import torch
    import tips_amd
    a, b = torch.zeros(3), torch.zeros(4)
    plan = tips_amd._GradPlan([a, None, b], [([0, 2], None, None)])
    assert plan.matches([a, None, b])
    assert not plan.matches([a, b, b]) and not plan.matches([a, None])
    del a
    gc.collect()
    assert plan.dead and not plan.matches([None, None, b])
    c = torch.zeros(2)
    plan2 = tips_amd._GradPlan([c], [([0], None, None)])
    calls = []
    monkeypatch.setattr(tips_amd._ops, "_dev_list_flat", lambda ts: calls.append(ts) or None)
    assert plan2.run([c]) is None and calls == [[c]]


def test_flat_output_keys_follow_the_layout_settings(monkeypatch):
    """A fusion layout depends on TIPS_FUSION_THRESHOLD / TIPS_COPY_TILE_BYTES / TIPS_FUSION_BALANCE
    as well as the counts: the cached flat-output sets are keyed on them, so a changed setting gets
    offsets of its own layout."""
    import torch
    import tips_amd.ops as ops
    monkeypatch.setattr(ops, "_FLAT_OUTPUTS", {})
    ts = [torch.zeros(300 << 10), torch.zeros(300 << 10)]  # 1.2 MiB each
    fo1 = ops._flat_outputs(ts, ops._lib.FLOAT32)
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(1 << 20))
    fo2 = ops._flat_outputs(ts, ops._lib.FLOAT32)
    assert fo2 is not fo1
    monkeypatch.delenv("TIPS_FUSION_THRESHOLD")
    assert ops._flat_outputs(ts, ops._lib.FLOAT32) is fo1


def test_flat_output_take_is_exclusive_across_threads():
    """_FlatOutputs.take from many threads at once: no set is handed to two holders at a time (the
    free check and the hand-out run under the object's lock)."""
    import threading
    import torch
    from tips_amd import _lib
    from tips_amd.ops import _FlatOutputs
    fo = _FlatOutputs((torch.Size([8]), torch.Size([3])), [8, 3], _lib.FLOAT32, torch.float32, torch.device("cpu"))
    owners = {}
    bad = []
    lock = threading.Lock()

    def worker(k):
        for _ in range(300):
            flat, views = fo.take()
            p = flat.data_ptr()
            with lock:
                if owners.get(p) is not None:
                    bad.append((p, owners[p], k))
                owners[p] = k
            with lock:
                owners[p] = None
            del flat, views
    th = [threading.Thread(target=worker, args=(k,)) for k in range(6)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad


@pytest.mark.parametrize("warm", ["0", "1", "2"])
def test_overlap_trial_with_any_warmup(monkeypatch, warm):
    """TIPS_OVERLAP_TRIAL_WARMUP=0 made the last trial step read the end event of a step
    that was never recorded (KeyError inside step() on every rank). The warm-up is clamped to 1;
    the trial then runs to its choice. Events are faked on the CPU: 'during' steps take 5 ms,
    'after' steps 7 ms, so the choice is 'during'."""
    import torch
    import tips_amd.ops
    from tips_amd import basics
    from tips_amd.optim import _OverlapChoice
    monkeypatch.setenv("TIPS_OVERLAP_TRIAL_WARMUP", warm)
    monkeypatch.setenv("TIPS_OVERLAP_TRIAL_STEPS", "2")
    clock = [0.0]

    class Ev(object):
        def record(self, *a):
            self.t = clock[0]

        def synchronize(self):
            pass

        def elapsed_time(self, other):
            return other.t - self.t

    monkeypatch.setattr(torch.cuda, "Event", lambda enable_timing=True: Ev())
    monkeypatch.setattr(tips_amd.ops, "_allgather_i64", lambda v: list(v))
    monkeypatch.setattr(basics, "size", lambda: 1)
    oc = _OverlapChoice("auto")
    assert oc.warm >= 1
    s = 0
    while oc.chosen is None:
        clock[0] += 5.0 if oc.on(s) else 7.0
        oc.stepped(s)
        s += 1
        assert s < 20
    assert oc.chosen is True and oc.report["chosen"] == "during"
    assert s == oc.warm + 4


# --- which C entries a gradient list reaches ---------------------------------------------------
# Every entry point goes through the one funnel tips_amd._lib.call; the spy below logs
# (entry name, list length where the entry takes one, the factors it was given) and returns 0.
_AG = ("tips_allgather_i64",), ("tips_allgatherv",)  # one allgather_op: the first dimensions, then the rows
_REG = ("tips_host_register",)                        # a new host output set is page-locked
_AR = ("tips_allreduce",)
_AR_S = "tips_allreduce_scaled"                       # (prescale, postscale)
_FLAT = "tips_fused_allreduce_flat"                   # (n)
_FLAT_S = "tips_fused_allreduce_flat_scaled"          # (n, prescale, postscale)
_CAST = "tips_fused_allreduce_cast"                   # (n)
_SCALE = "tips_scale"                                 # (factor)
_HOST = "tips_fused_allreduce_host_flat"              # (n)
_MX = "tips_fused_allreduce_mxfp8_flat"               # (n, factor)
_MX1 = "tips_allreduce_mxfp8"                         # (factor)
_EFB = ("tips_mxfp8_ef_bytes",)                       # the size of a list's error-feedback state
_MXEF = "tips_fused_allreduce_mxfp8_ef_flat"          # (n, factor)

# entry -> (position of the list length among its arguments or None, positions of its factors)
_ROUTE_ARGS = {_FLAT: (2, ()), _FLAT_S: (2, (5, 6)), _CAST: (3, ()), _HOST: (2, ()), _MX: (2, (4,)), _MXEF: (2, (4,)),
               _AR_S: (None, (4, 5)), _MX1: (None, (3,)), _SCALE: (None, (4,))}

_INT_DEV = "op=Average is not defined for integer gradients (dtype torch.int32)"
_INT_HOST = "op=Average is not defined for integer gradients (dtype int32)"
_EF_LIST = ("allreduce_grads(fused=False) does not combine with MXFP8 error feedback: the residual state belongs to "
            "the fused list")
_EF_BODY = "fused=False does not combine with MXFP8 error feedback"
_NO_MAX = ("op=Max is not supported for gradient lists: the fused reductions carry SUM only (reduce single tensors "
           "with allreduce(tensor, op=Max))")
_NO_MIN = ("op=Min is not supported for gradient lists: the fused reductions carry SUM only (reduce single tensors "
           "with allreduce(tensor, op=Min))")


def _route_list(which):
    """The lists of the route test. Device members: f32 [5], f32 [4099] as a stride-2 view, f16 [3],
    i32 [4]; host members: numpy f32 [7], CPU torch f64 [2, 3]; a host sparse COO tensor, a host
    IndexedSlices and None."""
    import torch
    import tips_amd

    def dev(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device="cuda")

    def host():
        return [np.zeros(7, np.float32), torch.zeros(2, 3, dtype=torch.float64)]

    def sparse():
        return [torch.sparse_coo_tensor([[0, 2]], [1.0, 2.0], (4,)),
                tips_amd.IndexedSlices(np.zeros((3, 2), np.float32), np.array([4, 0, 4], np.int64), dense_shape=(5, 2)),
                None]
    if which == "fast":       # one dtype of contiguous device tensors: the fast list
        return [dev(5), dev(2, 3), dev(4)]
    if which == "dev2":       # two device dtypes: not a fast list, but a split a plan remembers
        return [dev(5), dev(6), dev(3, dtype=torch.float16)]
    if which == "mixed":      # everything
        return [dev(5), dev(8198)[::2], dev(3, dtype=torch.float16), dev(4, dtype=torch.int32)] + host() + sparse()
    if which == "mixed_float":  # everything that takes a scale (an integer under Average raises)
        return [dev(5), dev(8198)[::2], dev(3, dtype=torch.float16)] + host() + sparse()
    if which == "host":
        return host()
    if which == "host_sparse":
        return host() + sparse()
    if which == "host_int":
        return [np.zeros(4, np.int32), np.zeros(7, np.float32)]
    raise KeyError(which)


def _route_rows():
    """(id, list, compression, op, scaling, fused, gradient_predivide_factor, expected): `expected`
    is the log of each call of the list (calls after the first repeat it with the same tensor
    objects) and how many of the calls ran a remembered plan - or the message of the ValueError.
    At size() == 2 Average is (prescale 1, postscale 0.5), with gradient_predivide_factor 2 it is
    (0.5, 1); the MXFP8 wire and the cast path get the product."""
    A = "Average"
    sparse2 = [*_AG, *_AG, *_AG, *_AG]  # the COO tensor's indices and values, the IndexedSlices' values and indices
    host2 = [_REG, (_HOST, 1), _REG, (_HOST, 1)]  # numpy f32 and torch f64: one host group each, new sets
    rows = [
        # the fast list: three contiguous float32 device tensors
        ("fast-none", "fast", "none", None, False, True, 1, ([[(_FLAT, 3)], [(_FLAT, 3)]], 0)),
        ("fast-none-average-unscaled", "fast", "none", A, False, True, 1, ([[(_FLAT, 3)]], 0)),
        ("fast-none-sum-scaling", "fast", "none", None, True, True, 2, ([[(_FLAT, 3)]], 0)),
        ("fast-none-average", "fast", "none", A, True, True, 1, ([[(_FLAT_S, 3, 1.0, 0.5)], [(_FLAT_S, 3, 1.0, 0.5)]], 0)),
        ("fast-none-average-predivide", "fast", "none", A, True, True, 2, ([[(_FLAT_S, 3, 0.5, 1.0)]], 0)),
        ("fast-none-unfused", "fast", "none", None, False, False, 1, ([[_AR, _AR, _AR]], 0)),
        ("fast-none-average-unfused", "fast", "none", A, True, False, 1,
         ([[(_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)]], 0)),
        ("fast-fp16", "fast", "fp16", None, False, True, 1, ([[(_CAST, 3)], [(_CAST, 3)]], 0)),
        ("fast-fp16-average", "fast", "fp16", A, True, True, 1, ([[(_CAST, 3), (_SCALE, 0.5)]], 0)),
        ("fast-fp16-average-predivide", "fast", "fp16", A, True, True, 2, ([[(_CAST, 3), (_SCALE, 0.5)]], 0)),
        ("fast-fp16-unfused", "fast", "fp16", None, False, False, 1, ([[_AR, _AR, _AR]], 0)),
        ("fast-fp16-average-unfused", "fast", "fp16", A, True, False, 2,
         ([[(_AR_S, 0.5, 1.0), (_AR_S, 0.5, 1.0), (_AR_S, 0.5, 1.0)]], 0)),
        ("fast-fp8", "fast", "fp8", None, False, True, 1, ([[(_MX, 3, 1.0)]], 0)),
        ("fast-fp8-average-predivide", "fast", "fp8", A, True, True, 2, ([[(_MX, 3, 0.5)]], 0)),
        ("fast-fp8-average-unfused", "fast", "fp8", A, True, False, 1, ([[(_MX1, 0.5), (_MX1, 0.5), (_MX1, 0.5)]], 0)),
        ("fast-ef", "fast", "ef", None, False, True, 1, ([[_EFB, (_MXEF, 3, 1.0)], [_EFB, (_MXEF, 3, 1.0)]], 0)),
        ("fast-ef-average", "fast", "ef", A, True, True, 1, ([[_EFB, (_MXEF, 3, 0.5)]], 0)),
        # two device dtypes: the second call runs the remembered plan (unscaled only)
        ("dev2-none", "dev2", "none", None, False, True, 1, ([[(_FLAT, 2), (_FLAT, 1)], [(_FLAT, 2), (_FLAT, 1)]], 1)),
        ("dev2-none-average", "dev2", "none", A, True, True, 1,
         ([[(_FLAT_S, 2, 1.0, 0.5), (_FLAT_S, 1, 1.0, 0.5)], [(_FLAT_S, 2, 1.0, 0.5), (_FLAT_S, 1, 1.0, 0.5)]], 0)),
        # the mixed list: sparse members inside the loop, then device groups (f32 x 2, f16, i32), then
        # cast groups, then host groups
        ("mixed-none", "mixed", "none", None, False, True, 1,
         ([sparse2 + [(_FLAT, 2), (_FLAT, 1), (_FLAT, 1)] + host2], 0)),
        ("mixed-none-average-unscaled", "mixed", "none", A, False, True, 2,
         ([sparse2 + [(_FLAT, 2), (_FLAT, 1), (_FLAT, 1)] + host2], 0)),
        ("mixed-none-unfused", "mixed", "none", None, False, False, 1, ([[_AR, _AR, _AR, _AR, _AR, _AR] + sparse2], 0)),
        ("mixed-fp16", "mixed", "fp16", None, False, True, 1,
         ([sparse2 + [(_FLAT, 1), (_FLAT, 1), (_CAST, 2)] + host2], 0)),
        ("mixed-fp8", "mixed", "fp8", None, False, True, 1,
         ([[(_MX, 2, 1.0)] + sparse2 + [(_FLAT, 1), (_FLAT, 1)] + host2], 0)),
        ("mixed-ef", "mixed", "ef", None, False, True, 1,
         ([[_EFB, (_MXEF, 2, 1.0)] + sparse2 + [(_FLAT, 1), (_FLAT, 1)] + host2], 0)),
        ("mixed-none-average-integer", "mixed", "none", A, True, True, 1, _INT_DEV),
        # under a scale: host members one scaled allreduce each (inside the loop, before the sparse
        # ones that follow them in the list), device groups after the loop
        ("mixed_float-none-average", "mixed_float", "none", A, True, True, 1,
         ([[(_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)] + sparse2 + [(_FLAT_S, 2, 1.0, 0.5), (_FLAT_S, 1, 1.0, 0.5)]], 0)),
        ("mixed_float-none-average-predivide", "mixed_float", "none", A, True, True, 2,
         ([[(_AR_S, 0.5, 1.0), (_AR_S, 0.5, 1.0)] + sparse2 + [(_FLAT_S, 2, 0.5, 1.0), (_FLAT_S, 1, 0.5, 1.0)]], 0)),
        ("mixed_float-fp16-average", "mixed_float", "fp16", A, True, True, 1,
         ([[(_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)] + sparse2 + [(_CAST, 2), (_SCALE, 0.5)]], 0)),
        ("mixed_float-fp8-average", "mixed_float", "fp8", A, True, True, 1,
         ([[(_MX, 2, 0.5), (_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)] + sparse2 + [(_FLAT_S, 1, 1.0, 0.5)]], 0)),
        ("mixed_float-ef-average", "mixed_float", "ef", A, True, True, 1,
         ([[_EFB, (_MXEF, 2, 0.5), (_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)] + sparse2 + [(_FLAT_S, 1, 1.0, 0.5)]], 0)),
        ("mixed_float-none-average-unfused", "mixed_float", "none", A, True, False, 1,
         ([[(_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)] + sparse2], 0)),
        # host members only: no device, so these rows run everywhere
        ("host-none", "host", "none", None, False, True, 1, ([host2, [(_HOST, 1), (_HOST, 1)]], 1)),
        ("host-none-average-unscaled", "host", "none", A, False, True, 1, ([host2], 0)),
        ("host-none-average", "host", "none", A, True, True, 1,
         ([[(_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)], [(_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)]], 0)),
        ("host-none-unfused", "host", "none", None, False, False, 1, ([[_AR, _AR]], 0)),
        ("host-fp16", "host", "fp16", None, False, True, 1, ([host2, [(_HOST, 1), (_HOST, 1)]], 0)),
        ("host-fp16-average", "host", "fp16", A, True, True, 1, ([[(_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)]], 0)),
        ("host-fp8", "host", "fp8", None, False, True, 1, ([host2], 0)),
        ("host-fp8-average-predivide", "host", "fp8", A, True, True, 2, ([[(_AR_S, 0.5, 1.0), (_AR_S, 0.5, 1.0)]], 0)),
        ("host-ef", "host", "ef", None, False, True, 1, ([host2], 0)),
        ("host_sparse-none", "host_sparse", "none", None, False, True, 1, ([sparse2 + host2], 0)),
        ("host_sparse-none-average", "host_sparse", "none", A, True, True, 1,
         ([[(_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)] + sparse2], 0)),
        ("host_sparse-fp16-average-unfused", "host_sparse", "fp16", A, True, False, 1,
         ([[(_AR_S, 1.0, 0.5), (_AR_S, 1.0, 0.5)] + sparse2], 0)),
        # the refusals: nothing reaches the library
        ("host_int-none-average-integer", "host_int", "none", A, True, True, 1, _INT_HOST),
        ("host-ef-unfused", "host", "ef", None, False, False, 1, _EF_LIST),
        ("host-ef-unfused-body", "host", "ef", None, False, False, 1, _EF_BODY),
        ("host-none-max", "host", "none", "Max", False, True, 1, _NO_MAX),
        ("host-none-min-body", "host", "none", "Min", True, True, 1, _NO_MIN),
    ]
    out = []
    for row in rows:
        marks = [] if row[1].startswith("host") else [pytest.mark.gpu]
        out.append(pytest.param(*row[1:], id=row[0], marks=marks))
    return out


@pytest.mark.parametrize("which,compression,op,scaling,fused,predivide,expected", _route_rows())
def test_gradient_list_routes(monkeypatch, request, which, compression, op, scaling, fused, predivide, expected):
    """Which C entries allreduce_grads reaches for a list, in which order, with how many tensors and
    which factors: a route that fell to the unfused path would give the same bits, only slower. Two
    ranks are faked (size() == 2, init a no-op) and tips_amd._lib.call is a spy that logs and returns
    0, so nothing is launched and the outputs are not looked at; tips_fused_layout (pure host, not
    through the funnel) runs for real, and so does _remember_plan. Rows whose id ends in -body call
    _reduce_grads, allreduce_grads' N > 1 body, directly: its checks hold there too."""
    import tips_amd
    ops = tips_amd._ops
    log = []

    def spy(name, *args):
        n_at, factors_at = _ROUTE_ARGS.get(name, (None, ()))
        log.append((name,) + (() if n_at is None else (int(args[n_at]),)) + tuple(float(args[k]) for k in factors_at))
        return 0

    plan_runs = []
    real_run = tips_amd._GradPlan.run

    def counted_run(self, grads):
        plan_runs.append(len(grads))
        return real_run(self, grads)

    monkeypatch.setattr(tips_amd._lib, "call", spy)
    monkeypatch.setattr(tips_amd, "size", lambda: 2)
    monkeypatch.setattr(tips_amd.basics, "size", lambda: 2)  # (the allgather of a sparse member asks there)
    monkeypatch.setattr(tips_amd, "init", lambda: None)
    monkeypatch.setattr(tips_amd.basics, "init", lambda: None)
    monkeypatch.setattr(tips_amd._GradPlan, "run", counted_run)
    monkeypatch.setattr(ops, "_check", False)
    # the spy page-locks nothing, so the host sets made here have nothing to unregister when they go
    # (the real call would leave a HIP error behind for whoever asks the runtime next)
    monkeypatch.setattr(ops, "_unregister", lambda ptr: None)
    for mod, cache, fresh in ((ops, "_FLAT_OUTPUTS", {}), (ops, "_FAST_FLAT", {}), (ops, "_HOST_FLAT", {}),
                              (tips_amd, "_PLANS", [])):
        monkeypatch.setattr(mod, cache, fresh)  # no set or plan of another test, and none of this one left behind
    was = ops.op_scaling()
    tips_amd.set_op_scaling(scaling)
    try:
        grads = _route_list(which)
        comp = {"none": tips_amd.Compression.none, "fp16": tips_amd.Compression.fp16, "fp8": tips_amd.Compression.fp8,
                "ef": tips_amd.Compression.fp8.error_feedback()}[compression]
        body = request.node.callspec.id.endswith("-body")

        def reduce():
            if body:
                return tips_amd._reduce_grads(grads, compression=comp, op=op, fused=fused,
                                              gradient_predivide_factor=predivide)
            return tips_amd.allreduce_grads(grads, compression=comp, op=op, fused=fused,
                                            gradient_predivide_factor=predivide)
        if isinstance(expected, str):
            with pytest.raises(ValueError) as e:
                reduce()
            assert str(e.value) == expected and log == []
            return
        logs, planned = expected
        for want in logs:
            del log[:]
            out = reduce()
            assert len(out) == len(grads) and [o is None for o in out] == [g is None for g in grads]
            del out  # (released: the next call of the list gets the same output sets)
            assert log == want
        assert len(plan_runs) == planned
    finally:
        tips_amd.set_op_scaling(was)
