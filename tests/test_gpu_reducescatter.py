"""-m gpu, one process: the reduce-scatter's kernel through tips_reducescatter_fold with sources made up on
the device, and the collectives and the Python surface at one rank.

One directed segment list serves every dtype - 1, 3, a vector less one element, one vector, 257, an
empty segment, 4099, 70001 (many tiles and a ragged end) and 40 segments of 5 ... 44 elements that share
tiles - with `own` and `dst` 16-B aligned, either shifted by one element, and both; nsrc 1, 2, 3, 8 and
16 with the own slice first, in the middle and last; SUM plain and with the factors 1/3 and 3/8, MAX and
MIN. Every output is compared with the numpy definition (tests/reducescatter_util.py) under the
project's bit rule (the same bits; any NaN matches any NaN), the guard bytes around every output, the
own slices and the stages are unchanged, and the single 70001-element segment equals tips_multi_sum /
tips_multi_sum_scaled / tips_multi_reduce over contiguous copies of the same sources."""
import functools

import numpy as np
import pytest

import edge_values as ev
import reducescatter_util as ru
from gpu_util import ALL_DTYPES, BF16, F16, F32, F64, I32, I64, NPDT  # noqa: F401

pytestmark = pytest.mark.gpu

FLOATS = [F32, F64, F16, BF16]
PRE, POST = float(np.float32(1.0) / np.float32(3.0)), 0.375
OPS = [("sum", ru.SUM, 1.0, 1.0), ("scaled", ru.SUM, PRE, POST), ("max", ru.MAX, 1.0, 1.0), ("min", ru.MIN, 1.0, 1.0)]
NSRC = [1, 2, 3, 8, 16]
GUARD = 64  # bytes of sentinel kept before and after every output


def es_of(dtype):
    return np.dtype(NPDT[dtype]).itemsize


def directed_counts(dtype):
    ve = 16 // es_of(dtype)
    return [1, 3, ve - 1, ve, 257, 0, 4099, 70001] + list(range(5, 45))


def region_offsets(counts, es):
    offs, nxt = [], 0
    for c in counts:
        offs.append(nxt)
        if c:
            nxt = -(-(nxt + c * es) // 256) * 256
    return offs, nxt


class Arena(object):
    """The device side of one dtype's list: 16 staged regions of random bits, one buffer of own slices
    and one of outputs, every segment at a 16-B aligned place (+ one element when shifted) with guard
    bytes around it. Built once per dtype; the tests only read the stages and the own slices."""

    def __init__(self, dtype, counts, seed):
        import torch
        self.dtype, self.counts, self.es = dtype, counts, es_of(dtype)
        self.offs, self.region = region_offsets(counts, self.es)
        rng = ev.rng_for(18, dtype, seed)
        nreg = self.region // self.es
        gen = (lambda n: ev.from_bits(ev.random_bits(dtype, n, rng), dtype)) if dtype in FLOATS else \
            (lambda n: rng.integers(np.iinfo(NPDT[dtype]).min, np.iinfo(NPDT[dtype]).max, size=n, dtype=NPDT[dtype], endpoint=True))
        self.stage_host = [gen(nreg) for _ in range(16)]
        self.stage_dev = [torch.from_numpy(s.view(np.uint8)).cuda() for s in self.stage_host]
        # places of the segments in the own / output buffers: byte offsets of the aligned variant
        self.place, cur = [], 0
        for c in counts:
            self.place.append(cur + GUARD)
            cur += GUARD + -(-(c * self.es + self.es) // 16) * 16 + GUARD
        self.bytes = cur
        self.own_host = gen(self.bytes // self.es)
        self.own_dev = torch.from_numpy(self.own_host.view(np.uint8)).cuda()
        self.out_dev = torch.empty(self.bytes, dtype=torch.uint8, device="cuda")

    def own_slice(self, i, shift):
        b = self.place[i] // self.es + shift
        return self.own_host[b:b + self.counts[i]]

    def stage_slice(self, j, i):
        b = self.offs[i] // self.es
        return self.stage_host[j][b:b + self.counts[i]]

    def sources(self, i, nsrc, own_pos, own_shift):
        return [self.own_slice(i, own_shift) if j == own_pos else self.stage_slice(j, i) for j in range(nsrc)]

    def run(self, nsrc, own_pos, op, pre, post, own_shift, dst_shift, only=None):
        """One tips_reducescatter_fold over the list (or the segments `only`); returns the output buffer's bytes."""
        import torch
        from tips_amd import _lib
        idx = list(range(len(self.counts))) if only is None else only
        self.out_dev.fill_(0xA5)
        po, _k1 = _lib.ptr_array([self.out_dev.data_ptr() + self.place[i] + dst_shift * self.es for i in idx])
        pw, _k2 = _lib.ptr_array([self.own_dev.data_ptr() + self.place[i] + own_shift * self.es for i in idx])
        pc, _k3 = _lib.i64_array([self.counts[i] for i in idx])
        pf, _k4 = _lib.i64_array([self.offs[i] for i in idx])
        ps, _k5 = _lib.ptr_array([0 if j == own_pos else self.stage_dev[j].data_ptr() for j in range(nsrc)])
        _lib.call("tips_reducescatter_fold", po, pw, pc, pf, len(idx), ps, nsrc, own_pos, self.dtype, op, pre, post,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return self.out_dev.cpu().numpy()

    def expected(self, nsrc, own_pos, op, pre, post, own_shift, only=None):
        idx = list(range(len(self.counts))) if only is None else only
        return {i: ru.fold(self.sources(i, nsrc, own_pos, own_shift), self.dtype, op, pre, post) for i in idx}

    def check(self, out, exps, dst_shift):
        untouched = np.ones(self.bytes, dtype=bool)
        for i, exp in exps.items():
            b, n = self.place[i] + dst_shift * self.es, self.counts[i]
            got = out[b:b + n * self.es].view(NPDT[self.dtype])
            bad = ev.differing(got, exp, self.dtype)
            assert bad.size == 0, "segment %d (%d elements): %d differ, first at %s" % (i, n, bad.size, bad[:4].tolist())
            untouched[b:b + n * self.es] = False
        assert (out[untouched] == 0xA5).all(), "bytes outside the outputs were written"

    def inputs_unchanged(self):
        assert np.array_equal(self.own_dev.cpu().numpy(), self.own_host.view(np.uint8))
        for d, h in zip(self.stage_dev, self.stage_host):
            assert np.array_equal(d.cpu().numpy(), h.view(np.uint8))


@functools.lru_cache(maxsize=None)
def arena(dtype):
    return Arena(dtype, directed_counts(dtype), 0)


def ops_for(dtype):
    return [o for o in OPS if dtype in FLOATS or o[0] != "scaled"]


@pytest.mark.parametrize("opname", [o[0] for o in OPS])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_directed_list(gpu, dtype, opname):
    if opname == "scaled" and dtype in (I32, I64):
        from tips_amd import _lib
        a = arena(dtype)
        with pytest.raises(_lib.TipsError) as e:  # integers take no factors
            a.run(2, 0, ru.SUM, PRE, POST, 0, 0)
        assert e.value.code == -5
        return
    _, op, pre, post = [o for o in OPS if o[0] == opname][0]
    a = arena(dtype)
    for nsrc in NSRC:
        for own_pos in sorted({0, nsrc // 2, nsrc - 1}):
            for own_shift in (0, 1):
                exps = a.expected(nsrc, own_pos, op, pre, post, own_shift)  # (where the output lies changes no bit of it)
                for dst_shift in (0, 1):
                    a.check(a.run(nsrc, own_pos, op, pre, post, own_shift, dst_shift), exps, dst_shift)
    a.inputs_unchanged()


@pytest.mark.parametrize("dtype", [F32, BF16, I64])
def test_list_longer_than_one_launch(gpu, dtype):
    """250 small segments: the records travel in several launches, and tiles hold up to 16 segments."""
    a = Arena(dtype, [(7 * i) % 45 + (i % 5 == 0) * 300 for i in range(250)], 1)
    for nsrc, own_pos in [(1, 0), (3, 1), (16, 0)]:
        for shift in (0, 1):
            a.check(a.run(nsrc, own_pos, ru.SUM, 1.0, 1.0, shift, shift), a.expected(nsrc, own_pos, ru.SUM, 1.0, 1.0, shift), shift)
    a.inputs_unchanged()


@pytest.mark.parametrize("dtype", FLOATS)
def test_edge_tuples_through_both_paths(gpu, dtype):
    """edge_values.tuple_set (NaN, Inf, subnormals, signed zeros, 16-bit overflow): one aligned segment
    (the vector path) and the same shifted by one element on both sides (the element path)."""
    import torch
    from tips_amd import _lib
    srcs = ev.tuple_set(dtype)
    n, es = srcs[0].size, es_of(dtype)
    nsrc, own_pos = 8, 3
    stages = [torch.from_numpy(np.ascontiguousarray(s).view(np.uint8).copy()).cuda() for s in srcs[:nsrc]]
    pad = np.zeros(16 // es, dtype=srcs[0].dtype)
    own = torch.from_numpy(np.concatenate([pad, srcs[own_pos], pad]).view(np.uint8)).cuda()
    out = torch.empty(n * es + 64, dtype=torch.uint8, device="cuda")
    for _, op, pre, post in OPS:
        exp = ru.fold(list(srcs[:nsrc]), dtype, op, pre, post)
        for shift in (0, 1):
            out.fill_(0xA5)
            po, _k1 = _lib.ptr_array([out.data_ptr() + 16 + shift * es])
            pw, _k2 = _lib.ptr_array([own.data_ptr() + 16])
            pc, _k3 = _lib.i64_array([n])
            pf, _k4 = _lib.i64_array([0])
            if shift:  # an own slice that is not 16-B aligned: a copy one element further on
                own_s = torch.from_numpy(np.concatenate([pad, pad[:1], srcs[own_pos], pad]).view(np.uint8)).cuda()
                pw, _k2 = _lib.ptr_array([own_s.data_ptr() + 16 + es])
            ps, _k5 = _lib.ptr_array([0 if j == own_pos else stages[j].data_ptr() for j in range(nsrc)])
            _lib.call("tips_reducescatter_fold", po, pw, pc, pf, 1, ps, nsrc, own_pos, dtype, op, pre, post,
                      torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            host = out.cpu().numpy()
            b = 16 + shift * es
            got = host[b:b + n * es].view(NPDT[dtype])
            bad = ev.differing(got, exp, dtype)
            assert bad.size == 0, (op, pre, shift, bad[:4].tolist())
            assert (host[:b] == 0xA5).all() and (host[b + n * es:] == 0xA5).all()


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_long_segment_equals_the_contiguous_fold(gpu, dtype):
    """The 70001-element segment alone against the existing kernels over contiguous copies of its sources."""
    import torch
    from tips_amd import _lib
    a = arena(dtype)
    i = a.counts.index(70001)
    sp = torch.cuda.current_stream().cuda_stream
    for nsrc, own_pos in [(2, 1), (3, 0), (8, 4), (16, 15)]:
        copies = [torch.from_numpy(np.ascontiguousarray(s).view(np.uint8).copy()).cuda() for s in a.sources(i, nsrc, own_pos, 0)]
        ps, _k = _lib.ptr_array([c.data_ptr() for c in copies])
        for name, op, pre, post in ops_for(dtype):
            out = a.run(nsrc, own_pos, op, pre, post, 0, 0, only=[i])
            a.check(out, a.expected(nsrc, own_pos, op, pre, post, 0, only=[i]), 0)
            ref = torch.empty(70001 * a.es, dtype=torch.uint8, device="cuda")
            if name == "sum":
                _lib.call("tips_multi_sum", ref.data_ptr(), ps, nsrc, 70001, dtype, sp)
            elif name == "scaled":
                _lib.call("tips_multi_sum_scaled", ref.data_ptr(), ps, nsrc, 70001, dtype, pre, post, sp)
            else:
                _lib.call("tips_multi_reduce", ref.data_ptr(), ps, nsrc, 70001, dtype, op, sp)
            torch.cuda.synchronize()
            got = out[a.place[i]:a.place[i] + 70001 * a.es].view(NPDT[dtype])
            exp = ref.cpu().numpy().view(NPDT[dtype])
            assert ev.differing(got, exp, dtype).size == 0, (nsrc, name)


@pytest.fixture(scope="module")
def one_rank(gpu):
    """The collectives refuse to run beside a negotiation an earlier test of the session may have started."""
    gpu.shutdown()
    gpu.init()
    assert gpu.size() == 1
    return gpu


LIST_ROWS = [5, 0, 257, 1, 64, 3]
LIST_ELEMS = [33, 7, 1, 4099, 128, 0]


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_one_rank_collectives_are_the_scaled_copy(one_rank, dtype):
    import torch
    from tips_amd import _lib
    L = _lib.lib()
    sp = torch.cuda.current_stream().cuda_stream
    hosts = [ru.inputs(dtype, r * e, 30 + i, 0) for i, (r, e) in enumerate(zip(LIST_ROWS, LIST_ELEMS))]
    devs = [torch.from_numpy(np.ascontiguousarray(h).view(np.uint8).copy()).cuda() for h in hosts]
    for name, op, pre, post in ops_for(dtype):
        outs = [torch.full((h.nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda") for h in hosts]
        pi, _k1 = _lib.ptr_array([d.data_ptr() for d in devs])
        po, _k2 = _lib.ptr_array([o.data_ptr() + 16 for o in outs])
        pr, _k3 = _lib.i64_array(LIST_ROWS)
        pe, _k4 = _lib.i64_array(LIST_ELEMS)
        _lib.call("tips_grouped_reducescatter", pi, po, pr, pe, len(hosts), dtype, op, pre, post, sp)
        single = torch.full((hosts[0].nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        _lib.call("tips_reducescatter", devs[0].data_ptr(), single.data_ptr() + 16, LIST_ROWS[0], LIST_ELEMS[0], dtype, op,
                  pre, post, sp)
        torch.cuda.synchronize()
        for h, d, o in zip(hosts + [hosts[0]], devs + [devs[0]], outs + [single]):
            got = o.cpu().numpy()
            exp = ru.fold([h], dtype, op, pre, post)
            assert ev.differing(got[16:16 + h.nbytes].view(NPDT[dtype]), exp, dtype).size == 0, name
            if name != "scaled":  # the copy moves every bit, a NaN's payload included
                assert np.array_equal(got[16:16 + h.nbytes], np.ascontiguousarray(h).view(np.uint8))
            assert (got[:16] == 0xA5).all() and (got[16 + h.nbytes:] == 0xA5).all()
            assert np.array_equal(d.cpu().numpy(), np.ascontiguousarray(h).view(np.uint8))  # inputs untouched
    assert L.tips_reducescatter(devs[0].data_ptr(), outs[0].data_ptr(), 0, 33, dtype, 0, 1.0, 1.0, sp) == 0  # nothing to do


def test_one_rank_refusals(one_rank):
    import torch
    from tips_amd import _lib
    L = _lib.lib()
    sp = torch.cuda.current_stream().cuda_stream
    t = torch.zeros(64 * 4, device="cuda")
    out = torch.zeros(64 * 4, device="cuda")
    host = np.zeros(64 * 4, np.float32)
    # an output that overlaps an input
    assert L.tips_reducescatter(t.data_ptr(), t.data_ptr() + 128, 64, 4, F32, 0, 1.0, 1.0, sp) == -1
    assert b"overlaps" in L.tips_last_error()
    pi, _k1 = _lib.ptr_array([t.data_ptr(), out.data_ptr()])
    po, _k2 = _lib.ptr_array([out.data_ptr() + 512, t.data_ptr()])
    two, _k3 = _lib.i64_array([8, 8])
    el, _k4 = _lib.i64_array([4, 4])
    assert L.tips_grouped_reducescatter(pi, po, two, el, 2, F32, 0, 1.0, 1.0, sp) == -1  # output 1 lies in input 0
    # host pointers, either side
    assert L.tips_reducescatter(host.ctypes.data, out.data_ptr(), 64, 4, F32, 0, 1.0, 1.0, sp) == -5
    assert b"host memory" in L.tips_last_error()
    assert L.tips_reducescatter(t.data_ptr(), host.ctypes.data, 64, 4, F32, 0, 1.0, 1.0, sp) == -5
    # a pointer that is not aligned to its element
    assert L.tips_reducescatter(t.data_ptr() + 2, out.data_ptr(), 8, 4, F32, 0, 1.0, 1.0, sp) == -1
    # a capturing stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            rc = L.tips_reducescatter(t.data_ptr(), out.data_ptr(), 64, 4, F32, 0, 1.0, 1.0, side.cuda_stream)
            msg = L.tips_last_error()
    assert rc == -5 and b"captur" in msg
    torch.cuda.synchronize()
    # ... and the next call works
    t.fill_(2.0)
    assert L.tips_reducescatter(t.data_ptr(), out.data_ptr(), 64, 4, F32, 0, 1.0, 0.5, sp) == 0
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())


def test_python_surface_at_one_rank(one_rank):
    import torch
    tips = one_rank
    x = torch.randn(7, 33, device="cuda")
    for op in (tips.Average, tips.Sum, tips.Max, tips.Min):  # one rank: every one of them is the input
        y = tips.reducescatter(x, op=op)
        assert y.shape == x.shape and y.dtype == x.dtype and y.data_ptr() != x.data_ptr() and torch.equal(y, x)
    y = tips.reducescatter(x, op=tips.Sum, prescale_factor=0.5, postscale_factor=4.0)
    assert torch.equal(y, (x * 0.5) * 4.0)
    nc = torch.randn(33, 6, device="cuda").t()  # [6, 33], not contiguous
    assert not nc.is_contiguous()
    ints = torch.arange(40, dtype=torch.int64, device="cuda").reshape(10, 2, 2)
    half = torch.randn(5, dtype=torch.float32, device="cuda").to(torch.bfloat16)
    empty = torch.zeros(0, 4, device="cuda")
    outs = tips.grouped_reducescatter([x, None, nc, ints, half, empty], op=tips.Sum)
    assert outs[1] is None and len(outs) == 6
    for got, src in zip(outs, [x, None, nc, ints, half, empty]):
        if src is not None:
            assert got.shape == src.shape and got.dtype == src.dtype and got.is_contiguous() and torch.equal(got, src)
    avg = tips.grouped_reducescatter([x, half], op=tips.Average)
    assert torch.equal(avg[0], x) and torch.equal(avg[1], half)
    with pytest.raises(ValueError):
        tips.reducescatter(ints, op=tips.Average)
    with pytest.raises(ValueError):
        tips.reducescatter(x, op=tips.Sum, name="named")
