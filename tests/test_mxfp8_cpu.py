"""The MXFP8 wire without a GPU: the restatement's encoder against torch's CPU
float8_e4m3fn cast, the per-block error bound of the collective on seeded data, the wire-size formula,
the argument refusals that need no device, and the Python surface's marker and ValueErrors."""
import ctypes

import numpy as np
import pytest

import mxfp8_util as mx


def test_encoder_matches_torch_cast():
    """Every grid value, every midpoint and midpoint +- 1 f32 ulp, both signs: the integer encoder
    gives torch's float32 -> float8_e4m3fn bytes."""
    import torch
    v = mx.edge_values()
    assert v.size == 2 * (127 + 3 * 126)
    want = torch.from_numpy(v.copy()).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = mx.encode_e4m3(v)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    # ... and the decoder is the cast back
    codes = np.arange(256, dtype=np.uint8)
    back = torch.from_numpy(codes).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    dec = mx.decode_e4m3(codes)
    nan = np.isnan(back)
    assert np.array_equal(np.isnan(dec), nan) and np.array_equal(dec.view(np.uint32)[~nan], back.view(np.uint32)[~nan])


def test_scale_rule():
    """fr = 0x5FFFFF / 0x600000 keep s = e - 8 (amax * 2^-s <= 448), 0x600001 takes e - 7; zero,
    subnormal and the largest amax clamp; a non-finite element poisons only its block."""
    one = 0x3F800000
    assert list(mx.scale_bytes([one | 0x5FFFFF, one | 0x600000, one | 0x600001])) == [119, 119, 120]
    assert list(mx.scale_bytes([0, 1, 0x007FFFFF, 0x7F7FFFFF])) == [0, 0, 0, 246]
    x = np.ones((3, 32), np.float32)
    x[1, 7] = np.inf
    codes, sb = mx.quantize_blocks(x)
    assert list(sb) == [119, 255, 119] and (codes[1] == 0x7F).all() and (codes[0] == codes[2]).all()
    x[1, 7] = -0.0
    codes, sb = mx.quantize_blocks(x)
    assert codes[1, 7] == 0x80


@pytest.mark.parametrize("p", [2, 8])
def test_collective_error_bound(p):
    """|result - f64 sum| <= (SUM amax_r + amax_fold) / 16 + (p - 1) 2^-24 SUM amax_r per block: each
    quantisation errs by at most amax / 16, each f32 add by at most 2^-24 of the running magnitude."""
    n = 4099
    rng = np.random.default_rng(100 + p)
    elems = mx.round_up(n, 64)
    flats = []
    for _ in range(p):
        x = rng.standard_normal(n)
        out = rng.random(n) < 0.01
        x[out] *= np.exp(rng.uniform(-20, 20, size=int(out.sum())))
        flats.append(mx.flat_of([x.astype(np.float32)], [0], elems))
    got = mx.collective(flats).astype(np.float64)
    exact = np.sum([f.astype(np.float64) for f in flats], axis=0)
    nb = elems // mx.BLOCK
    amax = np.sum([np.abs(f.astype(np.float64)).reshape(nb, 32).max(axis=1) for f in flats], axis=0)
    wires = [mx.quantize(f) for f in flats]
    afold = np.abs(mx.fold_acc(wires, elems, 0, nb).astype(np.float64)).max(axis=1)
    bound = (amax + afold) / 16 + (p - 1) * 2.0 ** -24 * amax
    err = np.abs(got - exact).reshape(nb, 32).max(axis=1)
    print("p = %d: worst error / bound %.3f" % (p, float(np.max(err / np.maximum(bound, 1e-300)))))
    assert (err <= bound).all()
    assert err.max() > 0


@pytest.mark.parametrize("elems", [0, 32, 64, 8192, 1 << 28])
def test_wire_bytes(elems):
    from tips_amd import _lib
    so = ctypes.c_int64(-1)
    total = _lib.lib().tips_mxfp8_wire_bytes(elems, ctypes.byref(so))
    assert so.value == mx.round_up(elems, 256) == mx.scales_offset(elems)
    assert total == mx.round_up(elems, 256) + mx.round_up(elems // 32, 256) == mx.wire_bytes(elems)
    assert _lib.lib().tips_mxfp8_wire_bytes(elems, None) == total
    import tips_amd
    assert tips_amd.mxfp8_wire_bytes(elems) == (total, so.value)


def test_refusals_without_a_device():
    from tips_amd import _lib
    L = _lib.lib()
    one, _k = _lib.i64_array([64])
    neg, _k2 = _lib.i64_array([-1])
    nul, _k3 = _lib.ptr_array([0])
    some, _k4 = _lib.ptr_array([4096])
    assert L.tips_mxfp8_wire_bytes(-1, None) == -1
    for fn in (L.tips_mxfp8_quantize,):
        assert fn(nul, neg, 1, None, None) == -1
        assert fn(None, one, 1, None, None) == -1      # null list
        assert fn(nul, one, 1, None, None) == -1       # null tensor
        assert fn(some, one, 1, None, None) == -1      # null wire
        assert fn(None, None, -1, None, None) == -1
        assert fn(None, None, 0, None, None) == 0      # nothing to do
    assert L.tips_mxfp8_dequantize(nul, neg, 1, None, 1.0, None) == -1
    assert L.tips_mxfp8_dequantize(nul, one, 1, None, 1.0, None) == -1
    assert L.tips_mxfp8_dequantize(some, one, 1, None, 1.0, None) == -1
    assert L.tips_mxfp8_dequantize(some, one, 1, None, float("nan"), None) == -1
    assert L.tips_mxfp8_dequantize(some, one, 1, None, float("inf"), None) == -1
    assert L.tips_mxfp8_dequantize(None, None, 0, None, 1.0, None) == 0
    for nsrc in (0, 17, -3):
        assert L.tips_mxfp8_fold(None, some, nsrc, 64, 0, 1, None) == -1
        assert b"nsrc" in L.tips_last_error()
    assert L.tips_mxfp8_fold(None, some, 1, -64, 0, 1, None) == -1
    assert L.tips_mxfp8_fold(None, some, 1, 64, -1, 1, None) == -1
    assert L.tips_mxfp8_fold(None, some, 1, 64, 0, -1, None) == -1
    assert L.tips_mxfp8_fold(None, some, 1, 64, 1, 2, None) == -1   # 2 blocks in all
    assert L.tips_mxfp8_fold(None, some, 1, 64, 3, 0, None) == -1
    assert L.tips_mxfp8_fold(None, None, 1, 64, 0, 1, None) == -1
    assert L.tips_mxfp8_fold(None, some, 1, 64, 0, 1, None) == -1   # null dst
    assert L.tips_mxfp8_fold(None, some, 1, 64, 2, 0, None) == 0    # an empty range at the end
    assert L.tips_allreduce_mxfp8(None, None, -1, 1.0, None) == -1
    assert L.tips_allreduce_mxfp8(None, None, 10, float("nan"), None) == -1
    assert L.tips_allreduce_mxfp8(None, None, 0, 1.0, None) == -2   # not initialised
    assert L.tips_fused_allreduce_mxfp8_flat(nul, neg, 1, None, 1.0, None) == -1
    assert L.tips_fused_allreduce_mxfp8_flat(some, one, 1, None, 1.0, None) == -1  # null flat


def test_compression_fp8_is_a_marker():
    import tips_amd
    from tips_amd import Compression
    assert Compression.fp8 is tips_amd.MXFP8Compressor and issubclass(Compression.fp8, tips_amd.Compressor)
    x = np.arange(5, dtype=np.float32)
    c, ctx = Compression.fp8.compress(x)
    assert c is x and ctx is None and Compression.fp8.decompress(c, ctx) is x


@pytest.mark.parametrize("op", ["Max", "Min", "Adasum"])
def test_ops_other_than_the_sum_are_refused(op):
    """Before any collective: nothing is initialised by these calls."""
    import tips_amd
    from tips_amd import Compression
    x = np.ones(4, np.float32)
    with pytest.raises(ValueError, match="Compression.fp8"):
        tips_amd.allreduce(x, compression=Compression.fp8, op=op)
    with pytest.raises(ValueError, match="Compression.fp8"):
        tips_amd.allreduce_grads([x], compression=Compression.fp8, op=op)
    assert not tips_amd.is_initialized()


def test_host_tensors_are_not_mxfp8_tensors():
    import torch
    from tips_amd import ops
    assert not ops.is_mxfp8_tensor(np.ones(3, np.float32)) and not ops.is_mxfp8_tensor(torch.ones(3))
    with pytest.raises(ValueError):
        ops.allreduce_mxfp8(torch.ones(3))
    with pytest.raises(ValueError):
        ops.fused_allreduce_mxfp8([torch.ones(3)])
