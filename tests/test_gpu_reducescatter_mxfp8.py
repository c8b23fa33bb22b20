"""-m gpu, one process: the MXFP8 reduce-scatter's fold-dequantise kernel through
tips_reducescatter_mxfp8_fold, and the collectives and the Python surface at one rank.

Everything is bit for bit against the numpy restatement (tests/reducescatter_mxfp8_util.py; a NaN is
0x7FC00000). The peers' wire buffers come from tips.mxfp8_quantize on seeded per-source lists, except
where a test builds them by hand. Guard bytes lie before and after every output and are read back
after the run, and the own slices and the wires are compared with their host copies."""
import functools

import numpy as np
import pytest

import mxfp8_util as mx
import reducescatter_mxfp8_util as rmx
import reducescatter_util as ru

pytestmark = pytest.mark.gpu

F32 = 0
GUARD = 64  # bytes of sentinel kept before and after every output
THIRD = float(np.float32(1.0) / np.float32(3.0))
DIRECTED = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 70001, 0] + [7 + (193 * i) // 39 for i in range(40)]
NSRC_POS = [(1, [0]), (2, [0, 1]), (3, [0, 1, 2]), (8, list(range(8))), (9, [0, 8]), (16, [0, 15])]


def layout(counts):
    from tips_amd import ops
    return ops.mxfp8_flat_elems(counts)


class Arena(object):
    """The device side of one list: `nwires` wire buffers quantised on the device from seeded lists, one
    buffer of own slices and one of outputs, every segment at a 16-B aligned place (+ one element
    when shifted) with guard bytes around it. The tests only read the wires and the own slices."""

    def __init__(self, gpu, counts, seed, nwires=16, wires=None):
        import torch
        self.counts = list(counts)
        self.elems, self.offs = layout(self.counts)
        rng = np.random.default_rng([19, seed])
        if wires is None:
            wires = []
            for _ in range(nwires):
                ts = [torch.from_numpy(mx.spread_blocks(c, rng, lo=-20, hi=20)).cuda() for c in self.counts]
                wires.append(gpu.mxfp8_quantize(ts))
            torch.cuda.synchronize()
        self.wire_dev = wires
        self.wire_host = [w.cpu().numpy() for w in wires]
        assert all(w.size == mx.wire_bytes(self.elems) and d.data_ptr() % 16 == 0 for w, d in zip(self.wire_host, wires))
        self.ys = [rmx.dequantized(w, self.elems) for w in self.wire_host]
        self.place, cur = [], 0  # byte offsets of the aligned variant of every segment in the own / output buffers
        for c in self.counts:
            self.place.append(cur + GUARD)
            cur += GUARD + -(-(c * 4 + 4) // 16) * 16 + GUARD
        self.bytes = cur
        self.own_host = mx.spread_blocks(self.bytes // 4, rng, lo=-20, hi=20)
        self.own_dev = torch.from_numpy(self.own_host.view(np.uint8)).cuda()
        self.out_dev = torch.empty(self.bytes, dtype=torch.uint8, device="cuda")
        assert self.own_dev.data_ptr() % 16 == 0 and self.out_dev.data_ptr() % 16 == 0

    def set_own(self, i, values, shift=0):
        """Overwrite segment i's own slice (at `shift`), host and device."""
        import torch
        b = self.place[i] // 4 + shift
        self.own_host[b:b + self.counts[i]] = values
        self.own_dev.copy_(torch.from_numpy(self.own_host.view(np.uint8)))

    def own_slice(self, i, shift):
        b = self.place[i] // 4 + shift
        return self.own_host[b:b + self.counts[i]]

    def run(self, nsrc, own_pos, factor, own_shift, dst_shift, only=None, entry="mxfp8"):
        import torch
        from tips_amd import _lib
        idx = list(range(len(self.counts))) if only is None else only
        self.out_dev.fill_(0xA5)
        po, _k1 = _lib.ptr_array([self.out_dev.data_ptr() + self.place[i] + dst_shift * 4 if self.counts[i] else 0 for i in idx])
        pw, _k2 = _lib.ptr_array([self.own_dev.data_ptr() + self.place[i] + own_shift * 4 if self.counts[i] else 0 for i in idx])
        pc, _k3 = _lib.i64_array([self.counts[i] for i in idx])
        sp = torch.cuda.current_stream().cuda_stream
        if entry == "mxfp8":
            ps, _k4 = _lib.ptr_array([0 if j == own_pos else self.wire_dev[j].data_ptr() for j in range(nsrc)])
            _lib.call("tips_reducescatter_mxfp8_fold", po, pw, pc, len(idx), ps if nsrc > 1 else None, nsrc, own_pos, factor, sp)
        else:  # the plain fold with one source: what one source of the MXFP8 fold is defined as
            assert nsrc == 1 and only is None
            pf, _k4 = _lib.i64_array([4 * o for o in self.offs])
            _lib.call("tips_reducescatter_fold", po, pw, pc, pf, len(idx), None, 1, 0, F32, ru.SUM, 1.0, factor, sp)
        torch.cuda.synchronize()
        return self.out_dev.cpu().numpy()

    def expected(self, nsrc, own_pos, factor, own_shift, only=None):
        idx = list(range(len(self.counts))) if only is None else only
        outs = rmx.fold_dequantized([self.own_slice(i, own_shift) for i in idx], [self.offs[i] for i in idx], self.ys[:nsrc],
                                    own_pos, factor)
        return dict(zip(idx, outs))

    def check(self, out, exps, dst_shift):
        untouched = np.ones(self.bytes, dtype=bool)
        for i, exp in exps.items():
            b, n = self.place[i] + dst_shift * 4, self.counts[i]
            got = out[b:b + n * 4].view(np.float32)
            bad = np.flatnonzero(got.view(np.uint32) != exp.view(np.uint32))
            assert bad.size == 0, "segment %d (%d elements): %d differ, first at %s: got %s, expected %s" % (
                i, n, bad.size, bad[:4].tolist(), got[bad[:4]].view(np.uint32), exp[bad[:4]].view(np.uint32))
            untouched[b:b + n * 4] = False
        assert (out[untouched] == 0xA5).all(), "bytes outside the outputs were written"

    def inputs_unchanged(self):
        assert np.array_equal(self.own_dev.cpu().numpy(), self.own_host.view(np.uint8))
        for d, h in zip(self.wire_dev, self.wire_host):
            assert np.array_equal(d.cpu().numpy(), h)


@functools.lru_cache(maxsize=None)
def directed(gpu):
    return Arena(gpu, DIRECTED, 0)


@pytest.mark.parametrize("factor", [1.0, 0.125, THIRD])
def test_directed_list(gpu, factor):
    a = directed(gpu)
    assert sorted(a.counts[15:])[0] == 7 and sorted(a.counts[15:])[-1] == 200 and len(a.counts) == 55
    for nsrc, positions in NSRC_POS:
        for own_pos in positions:
            for own_shift in (0, 1):
                exps = a.expected(nsrc, own_pos, factor, own_shift)  # (where the output lies changes no bit of it)
                for dst_shift in (0, 1):
                    a.check(a.run(nsrc, own_pos, factor, own_shift, dst_shift), exps, dst_shift)
    a.inputs_unchanged()


def test_list_longer_than_one_launch(gpu):
    """250 small segments: the records travel in several launches."""
    a = Arena(gpu, [(7 * i) % 45 + (i % 5 == 0) * 300 for i in range(250)], 1, nwires=9)
    for nsrc, own_pos in [(1, 0), (3, 1), (8, 7), (9, 0)]:
        for shift in (0, 1):
            a.check(a.run(nsrc, own_pos, 1.0, shift, shift), a.expected(nsrc, own_pos, 1.0, shift), shift)
    a.inputs_unchanged()


def test_exhaustive_decode(gpu):
    """Every (scale byte, payload code) pair, scale byte 255 and the codes 0x7F / 0xFF included, against
    an own slice of -0.0, for which the add is the identity: the output is canonical(dequantise)."""
    import torch
    n = 65536
    elems, offs = layout([n])
    assert offs == [0] and elems >= n
    wire = np.zeros(mx.wire_bytes(elems), np.uint8)
    wire[:n] = np.arange(n) & 0xFF
    so = mx.scales_offset(elems)
    wire[so:so + n // 32] = np.arange(n // 32) >> 3
    pairs = set(zip(np.repeat(wire[so:so + n // 32], 32).tolist(), wire[:n].tolist()))
    assert len(pairs) == 65536
    exp = mx.dequantize(wire, elems)[:n]
    dev = torch.from_numpy(wire).cuda()
    for own_pos in (0, 1):
        a = Arena(gpu, [n], 2, wires=[dev, dev])
        for shift in (0, 1):
            a.set_own(0, np.float32(-0.0), shift)
            out = a.run(2, own_pos, 1.0, shift, shift)
            a.check(out, {0: exp}, shift)
            a.check(out, a.expected(2, own_pos, 1.0, shift), shift)  # ... and the restatement says the same
        a.inputs_unchanged()


def bits(words):
    return np.asarray(words, dtype=np.uint32).view(np.float32)


def test_edge_values(gpu):
    """One tensor of 8 blocks and 5 elements; wire 1 is quantised from data with a NaN in block 2, wire 2
    is built by hand: +Inf (448 * 2^127) in block 4, scale byte 0 over block 5, -0 over block 6. The
    sources are (own, wire 1, wire 2) with the own slice first, in the middle and last."""
    import torch
    n = 8 * 32 + 5
    elems, offs = layout([n])
    so = mx.scales_offset(elems)
    rng = np.random.default_rng(23)
    peer = mx.spread_blocks(n, rng, lo=-4, hi=4)
    peer[2 * 32 + 7] = np.nan
    peer[3 * 32:4 * 32] = np.float32(3.0e38) * rng.uniform(0.9, 1.0, 32).astype(np.float32)  # block 3: near the largest float
    peer[5 * 32:6 * 32] = 0.0
    peer[6 * 32:7 * 32] = np.float32(-0.0)
    w1 = gpu.mxfp8_quantize([torch.from_numpy(peer).cuda()])
    hand = mx.quantize(mx.flat_of([mx.spread_blocks(n, rng, lo=-4, hi=4)], offs, elems))
    hand[4 * 32:5 * 32] = 0x7E
    hand[so + 4] = 254                      # 448 * 2^127 overflows to +Inf
    hand[5 * 32:6 * 32] = rng.integers(1, 0x40, 32) | (rng.integers(0, 2, 32) << 7)
    hand[so + 5] = 0                        # codes below 2.0 under 2^-127: subnormals
    hand[6 * 32:7 * 32] = 0x80
    hand[so + 6] = 0                        # -0
    hand[3 * 32:4 * 32] = 0
    hand[so + 3] = 0
    w2 = torch.from_numpy(hand).cuda()
    for own_pos in (0, 1, 2):
        wires = [w1, w2]
        wires.insert(own_pos, w1)  # (a placeholder at the own position: never read)
        a = Arena(gpu, [n], 3, wires=wires)
        for shift in (0, 1):
            own = mx.spread_blocks(n, np.random.default_rng(29), lo=-4, hi=4)
            own[1] = np.nan
            own[33] = np.inf
            own[34] = -np.inf
            own[3 * 32:4 * 32] = np.float32(3.0e38)     # the sum with block 3 of wire 1 overflows to +Inf
            own[4 * 32 + 3] = -np.inf                   # against the peer's +Inf: NaN
            own[5 * 32:6 * 32] = 0.0                    # the peer's subnormals survive the add
            own[6 * 32:7 * 32] = np.float32(-0.0)
            a.set_own(0, own, shift)
            out = a.run(3, own_pos, 1.0, shift, shift)
            a.check(out, a.expected(3, own_pos, 1.0, shift), shift)
            got = out[a.place[0] + 4 * shift:][:4 * n].view(np.float32)
            gb = got.view(np.uint32)
            assert (gb[64:96] == mx.QNAN).all()                              # the poisoned block, whole
            assert not np.isnan(got[35:64]).any() and not np.isnan(got[96:128]).any()  # its neighbours are untouched
            assert gb[1] == mx.QNAN and np.isfinite(got[0]) and np.isfinite(got[2])         # own NaN: that element only
            assert got[33] == np.inf and got[34] == -np.inf and np.isfinite(got[35])
            assert (got[96:128] == np.inf).all()                             # the overflowing sum
            assert gb[4 * 32 + 3] == mx.QNAN and (got[4 * 32 + 4:5 * 32] == np.inf).all()   # +Inf - Inf, and +Inf beside it
            sub = got[5 * 32:6 * 32]
            assert (np.abs(sub) < np.float32(2.0 ** -126)).all() and (sub != 0).all()  # subnormals kept
            assert (gb[6 * 32:7 * 32] == 0x80000000).all()                   # -0 on every source
        a.inputs_unchanged()


def test_one_source_is_the_plain_fold(gpu):
    """nsrc = 1: the bytes tips_reducescatter_fold writes with one source and postscale = factor; with
    factor 1 the copy, which keeps a signalling NaN's bits."""
    a = directed(gpu)
    for factor in (1.0, 0.125, THIRD):
        for shift in (0, 1):
            got = a.run(1, 0, factor, shift, shift)
            ref = a.run(1, 0, factor, shift, shift, entry="plain")
            assert np.array_equal(got, ref), (factor, shift)
    b = Arena(gpu, [5, 70], 4, nwires=0)
    snan = bits([0x7F800001, 0xFFA00000, 0x7FC00000, 0x7F800000, 0x80000000])
    for shift in (0, 1):
        b.set_own(0, snan, shift)
        out = b.run(1, 0, 1.0, shift, shift)
        assert np.array_equal(out[b.place[0] + 4 * shift:][:20].view(np.uint32), snan.view(np.uint32))
        b.check(out, {i: b.own_slice(i, shift) for i in (0, 1)}, shift)
    b.inputs_unchanged()


@pytest.fixture(scope="module")
def one_rank(gpu):
    """The collectives refuse to run beside a negotiation an earlier test of the session may have started."""
    gpu.shutdown()
    gpu.init()
    assert gpu.size() == 1
    return gpu


LIST_ROWS = [5, 0, 257, 1, 64, 3]
LIST_ELEMS = [33, 7, 1, 4099, 128, 0]


def test_one_rank_collectives_are_the_scaled_copy(one_rank):
    import torch
    from tips_amd import _lib
    L = _lib.lib()
    sp = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(31)
    hosts = [mx.spread_blocks(r * e, rng, lo=-20, hi=20) for r, e in zip(LIST_ROWS, LIST_ELEMS)]
    devs = [torch.from_numpy(h.copy()).cuda() for h in hosts]
    for factor in (1.0, 0.375):
        outs = [torch.full((h.nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda") for h in hosts]
        pi, _k1 = _lib.ptr_array([d.data_ptr() for d in devs])
        po, _k2 = _lib.ptr_array([o.data_ptr() + 16 for o in outs])
        pr, _k3 = _lib.i64_array(LIST_ROWS)
        pe, _k4 = _lib.i64_array(LIST_ELEMS)
        _lib.call("tips_grouped_reducescatter_mxfp8", pi, po, pr, pe, len(hosts), factor, sp)
        single = torch.full((hosts[0].nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        _lib.call("tips_reducescatter_mxfp8", devs[0].data_ptr(), single.data_ptr() + 16, LIST_ROWS[0], LIST_ELEMS[0], factor, sp)
        torch.cuda.synchronize()
        for h, d, o in zip(hosts + [hosts[0]], devs + [devs[0]], outs + [single]):
            got = o.cpu().numpy()
            exp = ru.fold([h], F32, ru.SUM, 1.0, factor)
            assert np.array_equal(got[16:16 + h.nbytes].view(np.uint32), exp.view(np.uint32)), factor
            assert (got[:16] == 0xA5).all() and (got[16 + h.nbytes:] == 0xA5).all()
            assert np.array_equal(d.cpu().numpy().view(np.uint32), h.view(np.uint32))  # inputs untouched
    assert L.tips_reducescatter_mxfp8(devs[0].data_ptr(), outs[0].data_ptr(), 0, 33, 1.0, sp) == 0  # nothing to do


def test_one_rank_refusals(one_rank):
    import torch
    from tips_amd import _lib
    L = _lib.lib()
    sp = torch.cuda.current_stream().cuda_stream
    t = torch.zeros(64 * 4, device="cuda")
    out = torch.zeros(64 * 4, device="cuda")
    host = np.zeros(64 * 4, np.float32)
    assert L.tips_reducescatter_mxfp8(t.data_ptr(), t.data_ptr() + 128, 64, 4, 1.0, sp) == -1  # an output over an input
    assert b"overlaps" in L.tips_last_error()
    assert L.tips_reducescatter_mxfp8(host.ctypes.data, out.data_ptr(), 64, 4, 1.0, sp) == -5
    assert b"host memory" in L.tips_last_error()
    assert L.tips_reducescatter_mxfp8(t.data_ptr(), host.ctypes.data, 64, 4, 1.0, sp) == -5
    assert L.tips_reducescatter_mxfp8(t.data_ptr() + 2, out.data_ptr(), 8, 4, 1.0, sp) == -1  # not 4-B aligned
    assert L.tips_reducescatter_mxfp8(t.data_ptr(), out.data_ptr(), 64, 4, float("nan"), sp) == -1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rc = L.tips_reducescatter_mxfp8(t.data_ptr(), out.data_ptr(), 64, 4, 1.0, side.cuda_stream)
            msg = L.tips_last_error()
    assert rc == -5 and b"captur" in msg
    torch.cuda.synchronize()
    t.fill_(2.0)  # ... and the next call works
    assert L.tips_reducescatter_mxfp8(t.data_ptr(), out.data_ptr(), 64, 4, 0.5, sp) == 0
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())


def test_python_surface_at_one_rank(one_rank):
    import torch
    tips = one_rank
    fp8, fp16 = tips.Compression.fp8, tips.Compression.fp16
    x = torch.randn(7, 33, device="cuda")
    for op in (tips.Average, tips.Sum):  # one rank: the factor is 1, the copy
        y = tips.reducescatter(x, op=op, compression=fp8)
        assert y.shape == x.shape and y.dtype == x.dtype and y.data_ptr() != x.data_ptr() and torch.equal(y, x)
    y = tips.reducescatter(x, op=tips.Sum, prescale_factor=0.5, postscale_factor=0.75, compression=fp8)
    assert torch.equal(y, x * 0.375)  # one factor, prescale * postscale
    half = torch.randn(9, 5, device="cuda").to(torch.bfloat16)
    for kw in (dict(op=tips.Sum), dict(op=tips.Sum, prescale_factor=0.5, postscale_factor=4.0)):
        assert torch.equal(tips.reducescatter(half, compression=fp8, **kw), tips.reducescatter(half, **kw))
    ints = torch.arange(40, dtype=torch.int64, device="cuda").reshape(10, 2, 2)
    empty = torch.zeros(0, 4, device="cuda")
    outs = tips.grouped_reducescatter([x, None, half, ints, empty], op=tips.Sum, compression=fp8)
    assert outs[1] is None and len(outs) == 5
    for got, src in zip(outs, [x, None, half, ints, empty]):
        if src is not None:
            assert got.shape == src.shape and got.dtype == src.dtype and got.is_contiguous() and torch.equal(got, src)
    # any other compressor composes as for allreduce: compress, reduce-scatter, decompress
    y16 = tips.reducescatter(x, op=tips.Sum, compression=fp16)
    assert y16.dtype == x.dtype and torch.equal(y16, tips.allreduce(x, compression=fp16)) and torch.equal(y16, x.half().float())
    z = torch.randn(3, 5, device="cuda")
    g16 = tips.grouped_reducescatter([x, None, z], op=tips.Sum, compression=fp16)
    assert g16[1] is None and torch.equal(g16[0], y16) and torch.equal(g16[2], z.half().float())
    with pytest.raises(ValueError):
        tips.reducescatter(x, op=tips.Max, compression=fp8)
    with pytest.raises(ValueError):
        tips.reducescatter(x, op=tips.Sum, compression=fp8.error_feedback())
