"""-m gpu: the MXFP8 wire's kernels and one-rank collectives against the numpy restatement
(tests/mxfp8_util.py; the definition: include/tips_hip.h "MXFP8 wire"). Every
comparison is bit for bit: payload bytes, scale bytes and f32 outputs (a NaN is 0x7FC00000)."""
import numpy as np
import pytest

import mxfp8_util as mx
from test_gpu_adasum_procs import LIST20

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes on either side of a device buffer under test
PAT = 0xA5


def layout(counts):
    from tips_amd import ops
    return ops.mxfp8_flat_elems(counts)


def guarded(nbytes):
    """(whole uint8 device buffer filled with PAT, the 16-B aligned view of nbytes in its middle)."""
    import torch
    buf = torch.full((GUARD + nbytes + GUARD,), PAT, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def guards_kept(buf, nbytes):
    h = buf.cpu().numpy()
    return (h[:GUARD] == PAT).all() and (h[GUARD + nbytes:] == PAT).all()


def dev_f32(a, shift=0):
    """a on the device, `shift` elements past a 16-B boundary."""
    import torch
    base = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
    t = base[shift:shift + a.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    assert a.size == 0 or t.data_ptr() % 16 == 4 * shift  # (an empty tensor's pointer is null)
    return t


def quantize_dev(gpu, tensors):
    import torch
    elems, _ = layout([t.numel() for t in tensors])
    nbytes = mx.wire_bytes(elems)
    buf, wire = guarded(nbytes)
    gpu.mxfp8_quantize(tensors, wire=wire)
    torch.cuda.synchronize()
    assert guards_kept(buf, nbytes)
    return wire.cpu().numpy()


def same_wire(got, exp, elems):
    so = mx.scales_offset(elems)
    bad_p, bad_s = np.flatnonzero(got[:so] != exp[:so]), np.flatnonzero(got[so:] != exp[so:])
    assert bad_p.size == 0 and bad_s.size == 0, (bad_p[:6], got[bad_p[:6]], exp[bad_p[:6]], bad_s[:6],
                                                 got[so:][bad_s[:6]], exp[so:][bad_s[:6]])


def ref_wire(arrays):
    counts = [a.size for a in arrays]
    elems, offs = layout(counts)
    return mx.quantize(mx.flat_of(arrays, offs, elems)), elems, offs


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4099, 70001, (1 << 20) + 5])
def test_quantize_sizes_and_alignment(gpu, n):
    """One tensor, per-block magnitudes over 2^-140 ... 2^127; at element offsets 1, 2 and 3 from a
    16-B boundary (the element-by-element path) the bytes are those of the aligned run."""
    x = mx.spread_blocks(n, np.random.default_rng(n))
    exp, elems, _ = ref_wire([x])
    for shift in range(4):
        same_wire(quantize_dev(gpu, [dev_f32(x, shift)]), exp, elems)


def f32_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def edge_blocks():
    """The edge blocks of the quantiser, [nblocks, 32] f32."""
    rng = np.random.default_rng(5)
    blocks = []
    ev = mx.edge_values()
    ev = np.concatenate([ev, np.zeros(-ev.size % 31, np.float32)]).reshape(-1, 31)
    with np.errstate(all="ignore"):
        for s in (-127, -1, 0, 119):  # 31 edge values and the anchor 448 * 2^s, which fixes the scale at s
            two_s = np.float32(2.0 ** s)
            for k, row in enumerate(ev):
                blocks.append(np.insert((row * two_s).astype(np.float32), k % 32, np.float32(448.0) * two_s))
    for e in (1, 100, 127, 254):  # amax with fr = 0x5FFFFF, 0x600000, 0x600001
        for fr in (0x5FFFFF, 0x600000, 0x600001):
            amax = f32_bits([(e << 23) | fr])[0]
            b = (amax * rng.uniform(-1, 1, 32)).astype(np.float32)
            b[rng.integers(32)] = -amax if fr & 1 else amax
            blocks.append(b)
    sub = f32_bits(rng.integers(0, 0x800000, size=(4, 32)).astype(np.uint32) | (rng.integers(0, 2, size=(4, 32)).astype(np.uint32) << 31))
    blocks += list(sub)
    blocks += [np.zeros(32, np.float32), -np.zeros(32, np.float32), f32_bits(np.where(np.arange(32) % 2, 0x80000000, 0))]
    top = f32_bits([0x7F7FFFFF, 0x7F600001, 0x7F600000, 0x7F5FFFFF, 0x7F000000, 0xFF7FFFFF])  # amax above 448 * 2^119
    for t in top:
        b = (np.float32(3.0e38) * rng.uniform(-1, 1, 32)).astype(np.float32)
        b[rng.integers(32)] = t
        blocks.append(b)
    for pos in range(32):  # the block's maximum at each position
        b = rng.standard_normal(32).astype(np.float32)
        b[pos] = np.float32(-37.5 if pos % 2 else 37.5)
        blocks.append(b)
    return np.stack(blocks).astype(np.float32)


def test_quantize_edge_blocks(gpu):
    x = edge_blocks().reshape(-1)
    exp, elems, _ = ref_wire([x])
    so = mx.scales_offset(elems)
    assert set(exp[so:so + 4 * 33][::1]) >= {0, 126, 127, 246}  # the four anchored scales are what they should be
    same_wire(quantize_dev(gpu, [dev_f32(x)]), exp, elems)
    same_wire(quantize_dev(gpu, [dev_f32(x, 1)]), exp, elems)


def test_quantize_poison_stays_in_its_block(gpu):
    """A NaN, +Inf and -Inf at each of the 32 positions: that block is 0x7F / 0xFF, both neighbours are not."""
    rng = np.random.default_rng(6)
    specials = [np.nan, np.inf, -np.inf]
    x = rng.standard_normal((2 * 96 + 1, 32)).astype(np.float32)
    for k in range(96):
        x[2 * k + 1, k % 32] = specials[k // 32]
    exp, elems, _ = ref_wire([x.reshape(-1)])
    got = quantize_dev(gpu, [dev_f32(x.reshape(-1))])
    same_wire(got, exp, elems)
    so = mx.scales_offset(elems)
    sb = got[so:so + x.shape[0]]
    assert (sb[1::2] == 255).all() and (sb[0::2] != 255).all()
    assert (got[:x.size].reshape(-1, 32)[1::2] == 0x7F).all() and (got[:x.size].reshape(-1, 32)[0::2] != 0x7F).all()


def list20(seed):
    rng = np.random.default_rng(seed)
    return [mx.spread_blocks(n, rng, -30, 30) for n in LIST20]


def test_quantize_list(gpu):
    """The 20-tensor list (an empty and a 1-element tensor, odd sizes, unaligned tensors): padding bytes
    and their scales are zero, the guards are kept (quantize_dev), two runs give the same bytes."""
    arrays = list20(7)
    exp, elems, offs = ref_wire(arrays)
    devs = [dev_f32(a, i % 4) for i, a in enumerate(arrays)]
    got = quantize_dev(gpu, devs)
    same_wire(got, exp, elems)
    covered = np.zeros(mx.scales_offset(elems), bool)
    for a, o in zip(arrays, offs):
        covered[o:o + a.size] = True
    assert (got[:covered.size][~covered] == 0).all()
    so = mx.scales_offset(elems)
    nb = covered.size // 32
    assert (got[so:so + nb][~covered.reshape(-1, 32).any(axis=1)] == 0).all() and (got[so + nb:] == 0).all()
    assert np.array_equal(quantize_dev(gpu, devs), got)


def fold_sources(nsrc, elems, seed):
    rng = np.random.default_rng(seed)
    wires = []
    for j in range(nsrc):
        x = mx.spread_blocks(elems, rng, -20, 20)
        x[3 * 32:4 * 32] = np.float32(3.0e38) * (1 if j < 2 else 0)  # the sum of sources 0 and 1 overflows
        wires.append(mx.quantize(x))
    if nsrc > 1:
        so = mx.scales_offset(elems)
        wires[1][so + 5] = 255  # a poisoned source block
        wires[1][5 * 32:6 * 32] = 0x7F
    return wires


@pytest.mark.parametrize("nsrc", [1, 2, 3, 8, 16])
def test_fold(gpu, nsrc):
    """Block ranges at the start, in the middle, at the end and empty; blocks outside the range keep
    the guard pattern; a poisoned source block and a sum that overflows poison exactly their block."""
    import torch
    elems = 4096 + 64
    nb = elems // 32
    wires = fold_sources(nsrc, elems, 40 + nsrc)
    devs = [torch.from_numpy(w).cuda() for w in wires]
    nbytes = mx.wire_bytes(elems)
    so = mx.scales_offset(elems)
    for begin, count in [(0, 9), (40, 51), (nb - 7, 7), (17, 0), (nb, 0), (0, nb)]:
        buf, dst = guarded(nbytes)
        gpu.mxfp8_fold(dst, devs, elems, begin, count)
        torch.cuda.synchronize()
        assert guards_kept(buf, nbytes)
        exp = mx.fold(np.full(nbytes, PAT, np.uint8), wires, elems, begin, count)
        same_wire(dst.cpu().numpy(), exp, elems)
        if count == nb and nsrc > 1:
            assert exp[so + 3] == 255 and exp[so + 5] == 255 and (exp[so:so + nb] == 255).sum() == 2
    # dst aliasing source 0
    exp = mx.fold(wires[0], wires, elems, 2, nb - 3)
    gpu.mxfp8_fold(devs[0], devs, elems, 2, nb - 3)
    torch.cuda.synchronize()
    same_wire(devs[0].cpu().numpy(), exp, elems)


def test_fold_order_is_left_to_right(gpu):
    """Sources {2^27, 1, -2^27}: (2^27 + 1) - 2^27 = 0 but (2^27 - 2^27) + 1 = 1 in f32."""
    import torch
    elems = 64
    vals = {"big": 2.0 ** 27, "one": 1.0, "neg": -2.0 ** 27}
    w = {k: mx.quantize(np.full(elems, v, np.float32)) for k, v in vals.items()}
    for order, want in [(("big", "one", "neg"), 0.0), (("big", "neg", "one"), 1.0), (("one", "neg", "big"), 0.0)]:
        srcs = [w[k] for k in order]
        exp = mx.fold(srcs[0], srcs, elems, 0, 2)
        assert (mx.dequantize(exp, elems) == np.float32(want)).all()
        dst = torch.zeros(mx.wire_bytes(elems), dtype=torch.uint8, device="cuda")
        gpu.mxfp8_fold(dst, [torch.from_numpy(s).cuda() for s in srcs], elems, 0, 2)
        torch.cuda.synchronize()
        same_wire(dst.cpu().numpy(), exp, elems)


SCALES = [0, 1, 127, 246, 254, 255]


def all_codes_wire():
    """Every code 0 ... 255 under each scale byte of SCALES: 8 blocks per scale byte, one tensor."""
    n = 256 * len(SCALES)
    elems = layout([n])[0]  # (the flat layout rounds the tensor up to a tile)
    wire = np.zeros(mx.wire_bytes(elems), np.uint8)
    wire[:n] = np.tile(np.arange(256, dtype=np.uint8), len(SCALES))
    wire[mx.scales_offset(elems):][:n // 32] = np.repeat(np.array(SCALES, np.uint8), 8)
    return wire, n, elems


@pytest.mark.parametrize("factor", [1.0, 0.125, 1.0 / 3.0])
def test_dequantize_all_codes(gpu, factor):
    import torch
    wire, n, elems = all_codes_wire()
    out = torch.full((n,), 7.0, device="cuda")
    gpu.mxfp8_dequantize(torch.from_numpy(wire).cuda(), [out], factor)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    exp = mx.dequantize(wire, elems, factor)[:n]
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), np.flatnonzero(got.view(np.uint32) != exp.view(np.uint32))[:8]
    if factor == 1.0:  # no multiply: the table decode * 2^(scale - 127), built from f64
        sb = np.repeat(np.array(SCALES), 256)
        with np.errstate(all="ignore"):
            table = np.ldexp(mx.decode_e4m3(wire[:n]).astype(np.float64), sb - 127).astype(np.float32)
        ok = ~np.isnan(table) & (sb != 255)
        assert np.array_equal(got.view(np.uint32)[ok], table.view(np.uint32)[ok])
        assert (got.view(np.uint32)[~ok] == mx.QNAN).all()


def test_dequantize_list_writes_only_the_tensors(gpu):
    """The 20-tensor list into outputs at odd addresses with guard words round every one: partial last
    blocks write nothing past their tensor."""
    import torch
    arrays = list20(8)
    wire, elems, offs = ref_wire(arrays)
    exp = mx.dequantize(wire, elems, 0.5)
    gap = 5
    arena = torch.full((sum(LIST20) + gap * (len(LIST20) + 1),), -777.0, device="cuda")
    outs, pos = [], gap
    for n in LIST20:
        outs.append(arena[pos:pos + n])
        pos += n + gap
    gpu.mxfp8_dequantize(torch.from_numpy(wire).cuda(), outs, 0.5)
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    pos = gap
    for n, o in zip(LIST20, offs):
        assert np.array_equal(host[pos:pos + n].view(np.uint32), exp[o:o + n].view(np.uint32))
        assert (host[pos - gap:pos] == -777.0).all() and (host[pos + n:pos + n + gap] == -777.0).all()
        pos += n + gap


@pytest.fixture(scope="module")
def no_negotiation(gpu):
    """The collectives refuse to run beside a negotiation (named MXFP8 requests are not implemented), and an
    earlier test of the session may have started one with a named request: shutdown / init ends it."""
    gpu.shutdown()
    gpu.init()
    return gpu


def test_collective_is_refused_while_a_negotiation_runs(gpu):
    import torch
    from tips_amd import _lib
    t = torch.ones(64, device="cuda")
    gpu.allreduce(t, name="mxfp8.starts.the.negotiation")
    rc = _lib.lib().tips_allreduce_mxfp8(t.data_ptr(), t.data_ptr(), 64, 1.0, torch.cuda.current_stream().cuda_stream)
    assert rc == -5 and b"negotiation" in _lib.lib().tips_last_error()
    gpu.shutdown()
    gpu.init()


@pytest.mark.parametrize("n", [1, 4099, 70001])
def test_one_rank_allreduce_is_the_round_trip(no_negotiation, n):
    gpu = no_negotiation
    import torch
    from tips_amd import _lib
    x = mx.spread_blocks(n, np.random.default_rng(90 + n), -40, 40)
    elems, _ = layout([n])
    exp = mx.collective([mx.flat_of([x], [0], elems)])[:n]
    t = dev_f32(x)
    out = gpu.allreduce_mxfp8(t)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(t.cpu().numpy().view(np.uint32), x.view(np.uint32))
    sp = torch.cuda.current_stream().cuda_stream
    _lib.call("tips_allreduce_mxfp8", t.data_ptr(), t.data_ptr(), n, 1.0, sp)  # in place
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    half = gpu.allreduce(dev_f32(x), compression=gpu.Compression.fp8)
    assert np.array_equal(half.cpu().numpy().view(np.uint32), exp.view(np.uint32))


def test_one_rank_fused_flat_is_the_round_trip(no_negotiation):
    gpu = no_negotiation
    import torch
    arrays = list20(9)
    _, elems, offs = ref_wire(arrays)
    exp = mx.collective([mx.flat_of(arrays, offs, elems)], 0.25)
    outs = gpu.fused_allreduce_mxfp8([dev_f32(a, i % 4) for i, a in enumerate(arrays)], 0.25)
    torch.cuda.synchronize()
    for a, o, got in zip(arrays, offs, outs):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), exp[o:o + a.size].view(np.uint32))


def test_host_pointers_and_capture_are_refused(no_negotiation):
    gpu = no_negotiation
    import torch
    from tips_amd import _lib
    L = _lib.lib()
    host = np.zeros(64, np.float32)
    t = torch.zeros(64, device="cuda")
    wire = torch.zeros(mx.wire_bytes(64), dtype=torch.uint8, device="cuda")
    one, _k = _lib.i64_array([64])
    hp, _k2 = _lib.ptr_array([host.ctypes.data])
    dp, _k3 = _lib.ptr_array([t.data_ptr()])
    sp = torch.cuda.current_stream().cuda_stream
    assert L.tips_mxfp8_quantize(hp, one, 1, wire.data_ptr(), sp) == -5
    assert b"host memory" in L.tips_last_error()
    assert L.tips_mxfp8_quantize(dp, one, 1, host.ctypes.data, sp) == -5
    assert L.tips_mxfp8_dequantize(hp, one, 1, wire.data_ptr(), 1.0, sp) == -5
    assert L.tips_mxfp8_fold(wire.data_ptr(), hp, 1, 64, 0, 2, sp) == -5
    assert L.tips_allreduce_mxfp8(host.ctypes.data, t.data_ptr(), 64, 1.0, sp) == -5
    assert L.tips_mxfp8_quantize(dp, one, 1, wire.data_ptr() + 4, sp) == -1  # the wire buffer is 16-B aligned
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rc = L.tips_allreduce_mxfp8(t.data_ptr(), t.data_ptr(), 64, 1.0, side.cuda_stream)
            msg = L.tips_last_error()
    assert rc == -5 and b"captur" in msg
    torch.cuda.synchronize()
    out = gpu.allreduce_mxfp8(t)  # ... and the next call works
    assert torch.equal(out, t)
