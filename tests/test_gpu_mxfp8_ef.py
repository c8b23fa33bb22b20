"""-m gpu: the MXFP8 error-feedback kernels and one-rank collectives against the numpy restatement
(tests/mxfp8_ef_util.py; the definition: include/tips_hip.h "MXFP8 error feedback").
Every comparison is bit for bit: payload bytes, scale bytes, residuals and f32 outputs. Wire and
residual buffers sit between guard bytes; residual positions that hold no tensor element carry a
sentinel that must survive."""
import numpy as np
import pytest

import mxfp8_ef_util as ef
import mxfp8_util as mx
import test_gpu_mxfp8 as base
from test_gpu_adasum_procs import LIST20

pytestmark = pytest.mark.gpu

SENTINEL = 0xC1C2C3C4  # (a finite f32 pattern: a padding position's residual is neither read nor written)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def guarded_f32(values):
    """(the guarded byte buffer, its f32 view holding `values`)."""
    import torch
    buf, view = base.guarded(4 * values.size)
    f = view.view(torch.float32)
    f.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)))
    assert f.data_ptr() % 16 == 0
    return buf, f


def start_residual(arrays, offs, elems, rng, rel=1.0 / 16):
    """A non-zero residual of the size a step leaves behind (up to `rel` of each block's largest
    |x|), the sentinel at every position without a tensor element."""
    so = mx.scales_offset(elems)
    flat = mx.flat_of(arrays, offs, elems)
    amax = np.abs(np.concatenate([flat, np.zeros(so - elems, np.float32)])).reshape(-1, 32).max(axis=1)
    amax[~np.isfinite(amax)] = 1.0
    with np.errstate(all="ignore"):
        r = (rng.uniform(-1, 1, so) * np.repeat(amax, 32) * rel).astype(np.float32)
    r[~np.isfinite(r)] = 0
    mask = ef.mask_of([a.size for a in arrays], offs, elems)
    r.view(np.uint32)[~mask] = SENTINEL
    return r, mask


def same_bits(got, exp, what):
    bad = np.flatnonzero(bits(got) != bits(exp))
    assert bad.size == 0, (what, bad[:6], bits(got)[bad[:6]], bits(exp)[bad[:6]])


def quantize_ef_dev(gpu, arrays, r0, shifts=None):
    """tips_mxfp8_quantize_ef on the device: (wire bytes, new residual), guards checked."""
    import torch
    devs = [base.dev_f32(a, (shifts or [0] * len(arrays))[i]) for i, a in enumerate(arrays)]
    elems, _ = base.layout([a.size for a in arrays])
    nbytes = mx.wire_bytes(elems)
    wbuf, wire = base.guarded(nbytes)
    rbuf, res = guarded_f32(r0)
    gpu.mxfp8_quantize_ef(devs, res, wire=wire)
    torch.cuda.synchronize()
    assert base.guards_kept(wbuf, nbytes) and base.guards_kept(rbuf, 4 * r0.size)
    for d, a in zip(devs, arrays):  # the inputs are read only
        assert np.array_equal(bits(d.cpu().numpy()), bits(a))
    return wire.cpu().numpy(), res.cpu().numpy()


def check_quantize_ef(gpu, arrays, r0, mask, shifts=None):
    elems, offs = base.layout([a.size for a in arrays])
    exp_wire, exp_r = ef.quantize_ef(mx.flat_of(arrays, offs, elems), mask, r0)
    got_wire, got_r = quantize_ef_dev(gpu, arrays, r0, shifts)
    base.same_wire(got_wire, exp_wire, elems)
    same_bits(got_r, exp_r, "residual")
    assert (bits(got_r)[~mask] == SENTINEL).all()
    return exp_wire, exp_r


@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 257, 4095, 4096, 4097, 70001])
def test_quantize_ef_sizes_and_alignment(gpu, n):
    """One tensor with a random non-zero starting residual; the tensor 16-B aligned and 4 B past it
    (the element path for x, the vector path for the residual): the same bits."""
    rng = np.random.default_rng(n)
    x = mx.spread_blocks(n, rng, -100, 100)
    elems, offs = base.layout([n])
    r0, mask = start_residual([x], offs, elems, rng)
    for shift in (0, 1):
        check_quantize_ef(gpu, [x], r0, mask, [shift])


def test_quantize_ef_edge_blocks(gpu):
    """The quantiser's edge blocks with a zero residual (the plain bytes, -0 apart), with the residual
    that cancels x to zero, with a small one, and blocks whose x + r overflows."""
    rng = np.random.default_rng(11)
    eb = base.edge_blocks()
    nb = eb.shape[0]
    big = np.full((4, 32), 3.0e38, np.float32) * rng.choice([-1.0, 1.0], size=(4, 32)).astype(np.float32)
    x = np.concatenate([eb, eb, eb, big]).astype(np.float32)
    with np.errstate(all="ignore"):
        small = (np.abs(eb).max(axis=1, keepdims=True) / 32 * rng.uniform(-1, 1, eb.shape)).astype(np.float32)
    small[~np.isfinite(small)] = 0
    r = np.concatenate([np.zeros_like(eb), -eb, small, big]).astype(np.float32)
    r[3 * nb + 1] = r[3 * nb + 1] / 3   # 3e38 + 1e38 overflows too
    r[3 * nb + 2] = -r[3 * nb + 2] / 2  # ... and this sum is finite
    x, r = x.reshape(-1), r.reshape(-1)
    elems, offs = base.layout([x.size])
    r0 = np.zeros(mx.scales_offset(elems), np.float32)
    r0[:r.size] = r
    mask = ef.mask_of([x.size], offs, elems)
    r0.view(np.uint32)[~mask] = SENTINEL
    for shift in (0, 1):
        exp_wire, exp_r = check_quantize_ef(gpu, [x], r0, mask, [shift])
    so = mx.scales_offset(elems)
    sb = exp_wire[so:so + 3 * nb + 4]
    plain = mx.quantize(mx.flat_of([eb.reshape(-1)], [0], eb.size))
    same = (eb.reshape(-1).view(np.uint32) != 0x80000000)
    assert np.array_equal(exp_wire[:eb.size][same], plain[:eb.size][same])  # zero residual: the plain bytes
    assert (exp_wire[nb * 32:2 * nb * 32] == 0).all() and (sb[nb:2 * nb] == 0).all()  # cancelled: +0, scale byte 0
    assert (bits(exp_r)[nb * 32:2 * nb * 32] == 0).all()
    assert list(sb[3 * nb:] == 255) == [True, True, False, True]  # the overflowing sums poison their blocks
    assert (bits(exp_r)[3 * nb * 32:][:64] == 0).all() and np.isfinite(exp_r[mask]).all()


def test_quantize_ef_poison_stays_in_its_block(gpu):
    """A NaN, +Inf and -Inf at each of the 32 positions: that block is 0x7F / 0xFF and its residual +0;
    both neighbours keep their bytes and get the residual of an unpoisoned step."""
    rng = np.random.default_rng(12)
    specials = [np.nan, np.inf, -np.inf]
    x = rng.standard_normal((2 * 96 + 1, 32)).astype(np.float32)
    for k in range(96):
        x[2 * k + 1, k % 32] = specials[k // 32]
    x = x.reshape(-1)
    elems, offs = base.layout([x.size])
    r0, mask = start_residual([x], offs, elems, rng)
    r0[mask & (r0 == 0)] = np.float32(0.01)
    exp_wire, exp_r = check_quantize_ef(gpu, [x], r0, mask)
    so = mx.scales_offset(elems)
    sb = exp_wire[so:so + 2 * 96 + 1]
    assert (sb[1::2] == 255).all() and (sb[0::2] != 255).all()
    rr = bits(exp_r)[:x.size].reshape(-1, 32)
    assert (rr[1::2] == 0).all() and rr[0::2].any(axis=1).all()


LIST50 = [1, 31, 33, 100, 257, 64, 2, 0, 4097, 65] + [3 + 37 * i % 300 for i in range(40)]


def test_quantize_ef_list_of_50(gpu):
    """50 small tensors, an empty one among them, at every 4-B alignment: more segments than one launch
    carries, so two launches. Padding bytes and their scales are zero; the residual's padding
    positions keep the sentinel (check_quantize_ef); a second step from the new residual is exact too."""
    assert len(LIST50) == 50 and 0 in LIST50
    rng = np.random.default_rng(13)
    arrays = [mx.spread_blocks(n, rng, -30, 30) for n in LIST50]
    elems, offs = base.layout(LIST50)
    r0, mask = start_residual(arrays, offs, elems, rng)
    shifts = [i % 4 for i in range(50)]
    exp_wire, exp_r = check_quantize_ef(gpu, arrays, r0, mask, shifts)
    so = mx.scales_offset(elems)
    assert (exp_wire[:so][~mask] == 0).all() and (exp_wire[so + so // 32:] == 0).all()
    check_quantize_ef(gpu, arrays, exp_r, mask, shifts)


@pytest.mark.parametrize("nsrc", [1, 2, 8, 16])
def test_fold_ef(gpu, nsrc):
    """Block ranges at the start, in the middle, at the end and all of a larger buffer, each with a
    random residual of 32 floats per block: wire bytes outside the range keep the guard pattern; a
    poisoned source block and a sum that overflows poison their block and reset its residual."""
    import torch
    elems = 4096 + 64
    nb = elems // 32
    wires = base.fold_sources(nsrc, elems, 60 + nsrc)
    devs = [torch.from_numpy(w).cuda() for w in wires]
    nbytes = mx.wire_bytes(elems)
    so = mx.scales_offset(elems)
    rng = np.random.default_rng(70 + nsrc)
    for begin, count in [(0, 9), (40, 51), (nb - 7, 7), (0, nb)]:
        o0 = (rng.standard_normal(32 * count) * np.exp2(rng.integers(-24, 18, size=32 * count))).astype(np.float32)
        buf, dst = base.guarded(nbytes)
        obuf, o = guarded_f32(o0)
        gpu.mxfp8_fold_ef(dst, devs, elems, begin, count, o)
        torch.cuda.synchronize()
        assert base.guards_kept(buf, nbytes) and base.guards_kept(obuf, 4 * o0.size)
        exp, exp_o = ef.fold_ef(np.full(nbytes, base.PAT, np.uint8), wires, elems, begin, count, o0)
        base.same_wire(dst.cpu().numpy(), exp, elems)
        same_bits(o.cpu().numpy(), exp_o, "owner residual")
        assert np.isfinite(exp_o).all()
        if count == nb and nsrc > 1:
            assert exp[so + 3] == 255 and exp[so + 5] == 255 and (exp[so:so + nb] == 255).sum() == 2
            eo = bits(exp_o).reshape(-1, 32)
            assert (eo[3] == 0).all() and (eo[5] == 0).all() and eo[4].any()
    # dst aliasing source 0
    o0 = (rng.standard_normal(32 * (nb - 3)) / 8).astype(np.float32)
    exp, exp_o = ef.fold_ef(wires[0], wires, elems, 2, nb - 3, o0)
    obuf, o = guarded_f32(o0)
    gpu.mxfp8_fold_ef(devs[0], devs, elems, 2, nb - 3, o)
    torch.cuda.synchronize()
    base.same_wire(devs[0].cpu().numpy(), exp, elems)
    same_bits(o.cpu().numpy(), exp_o, "owner residual (aliased)")
    assert base.guards_kept(obuf, 4 * o0.size)


@pytest.mark.parametrize("nsrc", [1, 2, 16])
@pytest.mark.parametrize("nb", [1, 127, 128, 129])
def test_fold_ef_with_a_zero_residual_is_the_plain_fold(gpu, nb, nsrc):
    """The two fold forms share one body: over an all-zero owner residual mxfp8_fold_ef writes the payload
    and scale bytes mxfp8_fold writes, and its new residual is the restatement's. nb blocks: less than,
    one short of, exactly and one more than the 128 blocks of a workgroup. The sources are random wire
    buffers: scale bytes 0 ... 240 (no product overflows), payload codes drawn from the finite codes
    without 0x80, the two NaN codes then put at one place each - every code but 0x80, so no block sum is -0
    (acc + +0 would turn it into +0) and every byte is compared - and one source block poisoned whole."""
    import torch
    elems = 32 * nb
    nbytes, so = mx.wire_bytes(elems), mx.scales_offset(elems)
    rng = np.random.default_rng(1000 * nb + nsrc)
    finite = np.array([c for c in range(256) if c not in (0x7F, 0x80, 0xFF)], np.uint8)
    wires = []
    for j in range(nsrc):
        w = np.zeros(nbytes, np.uint8)
        w[:elems] = rng.choice(finite, size=elems)
        w[rng.integers(0, elems, size=2)] = (0x7F, 0xFF)
        w[so:so + nb] = rng.integers(0, 241, size=nb)
        wires.append(w)
    bad = nb // 2
    wires[nsrc // 2][so + bad] = 255
    wires[nsrc // 2][bad * 32:(bad + 1) * 32] = 0x7F
    assert not any((w[:elems] == 0x80).any() for w in wires)
    zeros = np.zeros(32 * nb, np.float32)
    exp, exp_o = ef.fold_ef(np.full(nbytes, base.PAT, np.uint8), wires, elems, 0, nb, zeros)
    assert exp[so + bad] == 255 and (nb == 1 or (exp[so:so + nb] != 255).any())
    devs = [torch.from_numpy(w).cuda() for w in wires]
    pbuf, plain = base.guarded(nbytes)
    gpu.mxfp8_fold(plain, devs, elems, 0, nb)
    fbuf, with_ef = base.guarded(nbytes)
    obuf, o = guarded_f32(zeros)
    gpu.mxfp8_fold_ef(with_ef, devs, elems, 0, nb, o)
    torch.cuda.synchronize()
    assert base.guards_kept(pbuf, nbytes) and base.guards_kept(fbuf, nbytes) and base.guards_kept(obuf, 4 * zeros.size)
    assert np.array_equal(with_ef.cpu().numpy(), plain.cpu().numpy())  # every byte: payload, scales, untouched tail
    base.same_wire(with_ef.cpu().numpy(), exp, elems)
    same_bits(o.cpu().numpy(), exp_o, "owner residual")
    assert (bits(exp_o).reshape(-1, 32)[bad] == 0).all() and np.isfinite(exp_o).all()


@pytest.fixture(scope="module")
def no_negotiation(gpu):
    """The collectives refuse to run beside a negotiation, which an earlier test may have started."""
    gpu.shutdown()
    gpu.init()
    return gpu


@pytest.mark.parametrize("n", [100, 4099, 70001])
def test_one_rank_allreduce_ef_three_steps(no_negotiation, n):
    """tips_allreduce_mxfp8_ef at one rank, three steps with the state carried forward: output and state
    bit for bit after each step - out of place, then in place; the third step repeats the second's input."""
    gpu = no_negotiation
    import torch
    from tips_amd import _lib
    elems, offs = base.layout([n])
    assert gpu.mxfp8_ef_bytes(elems, 1) == 4 * mx.scales_offset(elems)
    mask = ef.mask_of([n], offs, elems)
    host_state = [np.zeros(ef.ef_elems(elems, 1), np.float32)]
    host_state[0].view(np.uint32)[~mask] = SENTINEL  # (what the caller zeroes matters at tensor positions only)
    sbuf, state = guarded_f32(host_state[0])
    sp = torch.cuda.current_stream().cuda_stream
    x = None
    for step in range(3):
        if step < 2:
            x = mx.spread_blocks(n, np.random.default_rng(200 + 10 * n + step), -40, 40)
        flat = mx.flat_of([x], [0], elems)
        factor = [1.0, 0.5, 1.0][step]
        exp, host_state = ef.collective_ef([flat], host_state, factor, mask)
        t = base.dev_f32(x)
        if step == 1:
            _lib.call("tips_allreduce_mxfp8_ef", t.data_ptr(), t.data_ptr(), n, factor, state.data_ptr(), 4 * state.numel(), sp)
            out = t
        else:
            out = gpu.allreduce_mxfp8_ef(t, state, factor)
        torch.cuda.synchronize()
        same_bits(out.cpu().numpy(), exp[:n], "output of step %d" % step)
        same_bits(state.cpu().numpy(), host_state[0], "state after step %d" % step)
        assert base.guards_kept(sbuf, 4 * state.numel())
    assert host_state[0][mask].any()


def test_one_rank_fused_flat_ef_three_steps(no_negotiation):
    """tips_fused_allreduce_mxfp8_ef_flat over the 20-tensor list, new gradients every step, factor 0.25."""
    gpu = no_negotiation
    import torch
    elems, offs = base.layout(LIST20)
    mask = ef.mask_of(LIST20, offs, elems)
    host_state = [np.zeros(ef.ef_elems(elems, 1), np.float32)]
    sbuf, state = guarded_f32(host_state[0])
    for step in range(3):
        arrays = base.list20(30 + step)
        exp, host_state = ef.collective_ef([mx.flat_of(arrays, offs, elems)], host_state, 0.25, mask)
        outs = gpu.fused_allreduce_mxfp8_ef([base.dev_f32(a, i % 4) for i, a in enumerate(arrays)], state, 0.25)
        torch.cuda.synchronize()
        for a, o, got in zip(arrays, offs, outs):
            same_bits(got.cpu().numpy(), exp[o:o + a.size], "output of step %d" % step)
        same_bits(state.cpu().numpy(), host_state[0], "state after step %d" % step)
        assert base.guards_kept(sbuf, 4 * state.numel())
    assert not bits(host_state[0])[~mask].any()  # zeros stay zeros where no tensor element lies


def test_allreduce_with_the_compressor_keys_its_state_by_name(no_negotiation):
    """allreduce(t, compression=ef, name=...) at one rank: the named state is carried from call to call,
    another name starts from zeros, state_dict / load_state_dict move it to a new object."""
    gpu = no_negotiation
    import torch
    n = 4099
    elems, offs = base.layout([n])
    mask = ef.mask_of([n], offs, elems)
    comp = gpu.Compression.fp8.error_feedback()
    x = mx.spread_blocks(n, np.random.default_rng(77), -10, 10)
    flat = mx.flat_of([x], [0], elems)
    zeros = [np.zeros(ef.ef_elems(elems, 1), np.float32)]
    exp1, s1 = ef.collective_ef([flat], zeros, 1.0, mask)
    exp2, s2 = ef.collective_ef([flat], s1, 1.0, mask)
    exp3, s3 = ef.collective_ef([flat], s2, 1.0, mask)
    same_bits(gpu.allreduce(base.dev_f32(x), compression=comp, name="w").cpu().numpy(), exp1[:n], "first call")
    same_bits(gpu.allreduce(base.dev_f32(x), compression=comp, name="w").cpu().numpy(), exp2[:n], "second call")
    same_bits(gpu.allreduce(base.dev_f32(x), compression=comp, name="v").cpu().numpy(), exp1[:n], "another name")
    sd = comp.state_dict()
    key = ("tensor", "w", n, str(torch.device("cuda", torch.cuda.current_device())))
    assert set(sd) == {key, ("tensor", "v") + key[2:]}
    same_bits(sd[key].cpu().numpy(), s2[0], "state_dict")
    other = gpu.Compression.fp8.error_feedback()
    other.load_state_dict({k: v.cpu() for k, v in sd.items()})  # (as a checkpoint read on the host)
    same_bits(gpu.allreduce(base.dev_f32(x), compression=other, name="w").cpu().numpy(), exp3[:n], "after load_state_dict")
    comp.reset()
    same_bits(gpu.allreduce(base.dev_f32(x), compression=comp, name="w").cpu().numpy(), exp1[:n], "after reset")


def test_ef_refusals(no_negotiation):
    """A host ef, a misaligned ef, a short ef_bytes and a capturing stream are refused, the state is
    untouched, and the next call works."""
    gpu = no_negotiation
    import torch
    from tips_amd import _lib
    L = _lib.lib()
    n = 64
    elems, _ = base.layout([n])
    need = gpu.mxfp8_ef_bytes(elems, 1)
    assert need == 4 * mx.scales_offset(elems)
    t = torch.ones(n, device="cuda")
    state = torch.full((need // 4 + 4,), 0.125, device="cuda")
    host = np.zeros(need // 4, np.float32)
    wire = torch.zeros(mx.wire_bytes(elems), dtype=torch.uint8, device="cuda")
    one, _k = _lib.i64_array([n])
    dp, _k3 = _lib.ptr_array([t.data_ptr()])
    wp, _k4 = _lib.ptr_array([wire.data_ptr()])
    sp = torch.cuda.current_stream().cuda_stream
    assert L.tips_allreduce_mxfp8_ef(t.data_ptr(), t.data_ptr(), n, 1.0, host.ctypes.data, need, sp) == -5
    assert b"host memory" in L.tips_last_error()
    assert L.tips_allreduce_mxfp8_ef(t.data_ptr(), t.data_ptr(), n, 1.0, state.data_ptr() + 4, need, sp) == -1
    assert b"16-B aligned" in L.tips_last_error()
    assert L.tips_allreduce_mxfp8_ef(t.data_ptr(), t.data_ptr(), n, 1.0, state.data_ptr(), need - 4, sp) == -7
    assert b"ef_bytes" in L.tips_last_error()
    assert L.tips_allreduce_mxfp8_ef(t.data_ptr(), t.data_ptr(), n, 1.0, None, need, sp) == -1
    assert L.tips_allreduce_mxfp8_ef(t.data_ptr(), t.data_ptr(), n, 1.0, t.data_ptr(), need, sp) == -1  # overlaps the tensor
    flat = torch.empty(elems, device="cuda")
    assert L.tips_fused_allreduce_mxfp8_ef_flat(dp, one, 1, flat.data_ptr(), 1.0, host.ctypes.data, need, sp) == -5
    assert L.tips_fused_allreduce_mxfp8_ef_flat(dp, one, 1, flat.data_ptr(), 1.0, state.data_ptr(), 16, sp) == -7
    assert L.tips_mxfp8_quantize_ef(dp, one, 1, wire.data_ptr(), host.ctypes.data, sp) == -5
    assert L.tips_mxfp8_quantize_ef(dp, one, 1, wire.data_ptr(), state.data_ptr() + 4, sp) == -1
    assert L.tips_mxfp8_quantize_ef(dp, one, 1, wire.data_ptr(), t.data_ptr(), sp) == -1   # overlaps the tensor
    assert L.tips_mxfp8_fold_ef(wire.data_ptr(), wp, 1, 64, 0, 2, host.ctypes.data, sp) == -5
    assert L.tips_mxfp8_fold_ef(wire.data_ptr(), wp, 1, 64, 0, 2, state.data_ptr() + 8, sp) == -1
    assert L.tips_mxfp8_fold_ef(wire.data_ptr(), wp, 1, 64, 0, 2, wire.data_ptr(), sp) == -1  # overlaps a wire buffer
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rc = L.tips_allreduce_mxfp8_ef(t.data_ptr(), t.data_ptr(), n, 1.0, state.data_ptr(), need, side.cuda_stream)
            msg = L.tips_last_error()
    assert rc == -5 and b"captur" in msg
    torch.cuda.synchronize()
    assert torch.all(state == 0.125).item() and torch.all(t == 1.0).item()
    state.zero_()
    out = gpu.allreduce_mxfp8_ef(t, state[:need // 4])  # ... and the next call works
    assert torch.equal(out, t)
