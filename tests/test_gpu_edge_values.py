"""-m gpu: the sum, fold, scale and cast kernels on the edge-value sets of tests/edge_values.py -
subnormal operands and results, signed zeros, inf - inf, overflow from finite operands, NaNs of
every payload, exact ties, intermediates that overflow a 16-bit accumulator - bit-exact (any NaN
for any NaN) against the plain numpy references of that module. test_edge_values_cpu.py shows, on
the CPU, that the oracle agrees with those references and that the sets tell every wrong model of
the module from them; here only the device is compared, and nothing is computed from its output.

Every set goes through each position of a kernel that has arithmetic of its own: the 16-byte
vector body with the in-kernel tail (aligned buffers whose length is one less than a whole number
of vectors), the element-wise fallback (the same buffers through views offset by one element), and
calls of less than one vector, where every element is tail.
"""
import functools

import numpy as np
import pytest

import edge_values as ev
from gpu_util import ALL_DTYPES, BF16, F16, F32, F64, I32, I64, NPDT, bits, from_dev, same_bits, simulate, stream, to_dev

pytestmark = pytest.mark.gpu

INTS = (I32, I64)
N3, N12 = 786432 + 3, 3145728 + 5  # test_gpu_kernels.py's: 3 MiB + 12 B and 12 MiB + 20 B of float32
FILL = 0xAB


def ve_of(dtype):
    return 16 // np.dtype(NPDT[dtype]).itemsize


def padded(arrs, dtype):
    """The arrays extended by special values until the length is one less than a whole number of
    16-byte vectors: a full in-kernel tail behind a partial last tile."""
    ve = ve_of(dtype)
    extra = (ve - 1 - arrs[0].size) % ve
    sp = ev.int_specials(dtype) if dtype in INTS else ev.specials(dtype)
    out = [np.concatenate([a, np.resize(np.roll(sp, 5 * j), extra)]) for j, a in enumerate(arrs)]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pair_case(dtype):
    return tuple(padded(ev.pair_set(dtype), dtype))


@functools.lru_cache(maxsize=None)
def tuple_case(dtype):
    return tuple(padded(ev.tuple_set(dtype), dtype))


@functools.lru_cache(maxsize=None)
def fold_expected(dtype, k, pre=1.0, post=1.0):
    exp = ev.fold_ref(tuple_case(dtype)[:k], dtype, pre, post)
    exp.setflags(write=False)
    return exp


def hexes(a, idx):
    return [hex(int(v)) for v in bits(a)[idx]]


def same(got, exp, dtype, operands=(), models=None, what=""):
    """same_bits; on a difference: how many elements, the first few with operand, got and expected
    bits, and the wrong model of edge_values.py that the device output equals, if one does."""
    if same_bits(got, exp, dtype):
        return True
    idx = ev.differing(got, exp, dtype)
    head = idx[:6]
    print("%s: %d of %d elements differ; first at %s" % (what, idx.size, got.size, head.tolist()))
    for j, s in enumerate(operands):
        print("  operand %d: %s" % (j, hexes(s, head)))
    print("  got:       %s\n  expected:  %s" % (hexes(got, head), hexes(exp, head)))
    if models is not None and dtype not in INTS:
        names = ev.matching_model(got, models(), dtype)
        print("  the device output equals the wrong model(s): %s" % (names if names else "none of them"))
    return False


def call_sum(dst, a, b, n, dtype, factors=None):
    from tips_amd import _lib
    if factors is None:
        _lib.call("tips_bucket_sum", dst, a, b, n, dtype, stream())
    else:
        _lib.call("tips_bucket_sum_scaled", dst, a, b, n, dtype, factors[0], factors[1], stream())


def call_fold(dst, srcs, n, dtype, factors=None, remote=False):
    from tips_amd import _lib
    pp, _keep = _lib.ptr_array(srcs)
    if remote:
        _lib.dev_call("tips_multi_sum_remote", dst, pp, len(srcs), n, dtype, stream())
    elif factors is None:
        _lib.call("tips_multi_sum", dst, pp, len(srcs), n, dtype, stream())
    else:
        _lib.call("tips_multi_sum_scaled", dst, pp, len(srcs), n, dtype, factors[0], factors[1], stream())


# ---------------------------------------------------------------------------
# the 2-input sum

def run_sum_positions(dtype, factors):
    """Out of place and in place into a on the aligned buffers (body + tail), then the views offset by
    one element (the element-wise kernel), whose first element must stay as it was."""
    import torch
    a, b = pair_case(dtype)
    n = a.size
    assert n % ve_of(dtype) == ve_of(dtype) - 1
    if factors is None:
        exp = ev.sum2_ref(a, b, dtype)
        models = (lambda: ev.wrong_models([a, b], dtype)) if dtype not in INTS else None
    else:
        exp = ev.fold_ref([a, b], dtype, *factors)
        models = lambda: ev.wrong_models([a, b], dtype, *factors)
    da, db = to_dev(a), to_dev(b)
    dc = torch.empty_like(da)
    assert da.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0 and dc.data_ptr() % 16 == 0
    call_sum(dc.data_ptr(), da.data_ptr(), db.data_ptr(), n, dtype, factors)
    torch.cuda.synchronize()
    ok = same(from_dev(dc, dtype), exp, dtype, (a, b), models, "body + tail")
    call_sum(da.data_ptr(), da.data_ptr(), db.data_ptr(), n, dtype, factors)
    torch.cuda.synchronize()
    ok = same(from_dev(da, dtype), exp, dtype, (a, b), models, "body + tail, in place") and ok
    da = to_dev(a)
    dc = torch.full_like(da.view(torch.uint8), FILL).view(da.dtype)
    call_sum(dc[1:].data_ptr(), da[1:].data_ptr(), db[1:].data_ptr(), n - 1, dtype, factors)
    torch.cuda.synchronize()
    got = from_dev(dc, dtype)
    ok = same(got[1:], exp[1:], dtype, (a[1:], b[1:]), None, "element-wise") and ok
    assert ok and (got[:1].view(np.uint8) == FILL).all()


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_bucket_sum(gpu, dtype):
    run_sum_positions(dtype, None)


@pytest.mark.parametrize("pre,post", ev.FACTORS)
@pytest.mark.parametrize("dtype", ev.FLOAT_DTYPES)
def test_bucket_sum_scaled(gpu, dtype, pre, post):
    run_sum_positions(dtype, (pre, post))


# ---------------------------------------------------------------------------
# the fold

def run_fold_positions(dtype, k, factors=None, remote=False):
    """Body + tail out of place, then in place into the last source through views offset by one
    element (the element-wise kernel). Returns the body + tail output for further comparisons."""
    import torch
    srcs = tuple_case(dtype)[:k]
    n = srcs[0].size
    assert n % ve_of(dtype) == ve_of(dtype) - 1
    exp = fold_expected(dtype, k) if factors is None else fold_expected(dtype, k, *factors)
    models = None if dtype in INTS else (lambda: ev.wrong_models(srcs, dtype, *(factors or (1.0, 1.0))))
    devs = [to_dev(s) for s in srcs]
    out = torch.empty_like(devs[0])
    assert all(d.data_ptr() % 16 == 0 for d in devs + [out])
    call_fold(out.data_ptr(), [d.data_ptr() for d in devs], n, dtype, factors, remote)
    torch.cuda.synchronize()
    first = from_dev(out, dtype)
    ok = same(first, exp, dtype, srcs, models, "body + tail")
    call_fold(devs[-1][1:].data_ptr(), [d[1:].data_ptr() for d in devs], n - 1, dtype, factors, remote)
    torch.cuda.synchronize()
    got = from_dev(devs[-1], dtype)
    ok = same(got[1:], exp[1:], dtype, [s[1:] for s in srcs], None, "element-wise, in place") and ok
    assert ok and np.array_equal(bits(got[:1]), bits(srcs[-1][:1]))
    return first


MULTI_CASES = ([(d, k) for d in (F16, BF16) for k in (2, 3, 8, 16)] + [(d, k) for d in (F32, F64) for k in (3, 8)]
               + [(I32, 3), (I64, 3)])


@pytest.mark.parametrize("dtype,nsrc", MULTI_CASES)
def test_multi_sum(gpu, dtype, nsrc):
    run_fold_positions(dtype, nsrc)


REMOTE_CASES = ([(d, k) for d in (F16, BF16) for k in range(2, 17)]
                + [(d, k) for d in (F32, F64, I32, I64) for k in (2, 3, 4, 5, 16)])


@pytest.mark.parametrize("dtype,nsrc", REMOTE_CASES)
def test_multi_sum_remote(gpu, dtype, nsrc):
    """The peer schedule's pull-fold launch (4 vectors per lane for every source count) through its
    single-GPU entry in the development library; and the same bits as tips_multi_sum on the same
    buffers (any NaN for any NaN, as everywhere)."""
    import torch
    remote = run_fold_positions(dtype, nsrc, remote=True)
    devs = [to_dev(s) for s in tuple_case(dtype)[:nsrc]]
    out = torch.empty_like(devs[0])
    call_fold(out.data_ptr(), [d.data_ptr() for d in devs], devs[0].numel(), dtype)
    torch.cuda.synchronize()
    assert same(remote, from_dev(out, dtype), dtype, what="remote fold against tips_multi_sum")


@pytest.mark.parametrize("pre,post", ev.FACTORS)
@pytest.mark.parametrize("nsrc", [3, 8])
@pytest.mark.parametrize("dtype", ev.FLOAT_DTYPES)
def test_multi_sum_scaled(gpu, dtype, nsrc, pre, post):
    run_fold_positions(dtype, nsrc, (pre, post))


@pytest.mark.parametrize("dtype,nsrc,nbytes", [
    (F16, 5, 4 * N3),    # 4 vectors per lane
    (BF16, 6, 4 * N12),  # 128 lanes, 5 workgroups per CU
    (F32, 4, 4 * N12),   # 128 lanes, 8 workgroups per CU
    (BF16, 2, 4 * N12),  # the two-source fold that does not take the sum's launch
])
def test_fold_launch_shapes(gpu, dtype, nsrc, nbytes):
    """The fold's separately instantiated launch shapes, on the edge set repeated to the size that
    selects them; the expected array is the set's, repeated."""
    import torch
    n = nbytes // np.dtype(NPDT[dtype]).itemsize
    base = ev.tuple_set(dtype)[:nsrc]
    exp8k = ev.fold_ref(base, dtype)

    def repeated(x):
        return np.concatenate([np.tile(x, n // x.size), x[:n % x.size]])

    devs = [to_dev(repeated(s)) for s in base]
    out = torch.empty_like(devs[0])
    call_fold(out.data_ptr(), [d.data_ptr() for d in devs], n, dtype)
    torch.cuda.synchronize()
    got = from_dev(out, dtype)
    if not same_bits(got, repeated(exp8k), dtype):  # the report, on the first repetition that differs
        bad = ev.differing(got, repeated(exp8k), dtype)
        r = int(bad[0]) // exp8k.size * exp8k.size
        m = min(exp8k.size, n - r)
        same(got[r:r + m], exp8k[:m], dtype, [s[:m] for s in base], lambda: ev.wrong_models([s[:m] for s in base], dtype),
             "%d elements differ, first in the repetition at %d" % (bad.size, r))
        pytest.fail("the fold's launch shape at %d x %d bytes differs from the reference" % (nsrc, nbytes))


# ---------------------------------------------------------------------------
# calls of less than one vector: every element goes through the tail code

def special_pairs(dtype):
    if dtype in INTS:
        sp = ev.int_specials(dtype)
    else:
        sp = ev.specials(dtype)
    a, b = np.repeat(sp, len(sp)), np.tile(sp, len(sp))
    return a, b, np.ascontiguousarray(b[::-1])


TAIL_CASES = ([(d, f) for d in ALL_DTYPES for f in ("sum", "fold")]
              + [(d, f) for d in ev.FLOAT_DTYPES for f in ("sum scaled", "fold scaled")])  # (scaling: float dtypes)


@pytest.mark.parametrize("dtype,form", TAIL_CASES)
def test_tails_only(gpu, dtype, form):
    """specials x specials in chunks of one element less than a vector, each chunk a call of its own
    at a 16-byte-aligned offset (no vector: the tail code does everything), enqueued back to back;
    the element after each chunk keeps its fill."""
    import torch
    ve = ve_of(dtype)
    srcs = special_pairs(dtype)[:2 if form.startswith("sum") else 3]
    total = srcs[0].size
    nchunk = -(-total // (ve - 1))
    es = srcs[0].itemsize

    def spread(x):  # chunk i at element i * ve, FILL bytes between
        out = np.full(nchunk * ve * es, FILL, dtype=np.uint8).view(x.dtype)
        for i in range(nchunk):
            part = x[i * (ve - 1):(i + 1) * (ve - 1)]
            out[i * ve:i * ve + part.size] = part
        return out

    for factors in ([None] if "scaled" not in form else ev.FACTORS[:3]):
        if factors is None:
            exp = ev.sum2_ref(srcs[0], srcs[1], dtype) if len(srcs) == 2 else ev.fold_ref(srcs, dtype)
        else:
            exp = ev.fold_ref(srcs, dtype, *factors)
        devs = [to_dev(spread(s)) for s in srcs]
        out = torch.full_like(devs[0].view(torch.uint8), FILL).view(devs[0].dtype)
        base = [d.data_ptr() for d in devs]
        assert all(p % 16 == 0 for p in base + [out.data_ptr()])
        for i in range(nchunk):
            cnt = min(ve - 1, total - i * (ve - 1))
            off = i * ve * es
            if len(srcs) == 2:
                call_sum(out.data_ptr() + off, base[0] + off, base[1] + off, cnt, dtype, factors)
            else:
                call_fold(out.data_ptr() + off, [p + off for p in base], cnt, dtype, factors)
        torch.cuda.synchronize()
        got = from_dev(out, dtype)
        models = None if dtype in INTS else (lambda: ev.wrong_models(list(srcs), dtype, *(factors or (1.0, 1.0))))
        want = spread(exp)
        keep = np.ones(want.size, bool)  # the elements of the chunks
        keep[ve - 1::ve] = False
        keep[(nchunk - 1) * ve + (total - (nchunk - 1) * (ve - 1)):] = False
        packed = got[keep]
        assert packed.size == total
        assert same(packed, exp, dtype, srcs, models, "%s, factors %s" % (form, factors))
        assert (got[~keep].view(np.uint8) == FILL).all(), "a call of %d elements wrote past its end" % (ve - 1)


# ---------------------------------------------------------------------------
# the scaled copy

@pytest.mark.parametrize("dtype", ev.FLOAT_DTYPES)
def test_scale(gpu, dtype):
    """tips_scale with every factor of edge_values.FACTORS (1.0, the plain copy, among them), and the
    pairs through the one-rank tips_allreduce_scaled (the same kernel with both multiplies): body +
    tail out of place and in place, and the element-wise kernel."""
    import torch
    from tips_amd import _lib
    a = pair_case(dtype)[0]
    n = a.size
    da = to_dev(a)
    dc = torch.empty_like(da)
    singles = sorted({f for pair in ev.FACTORS for f in pair})
    for pre, post in [(f, 1.0) for f in singles] + ev.FACTORS:
        exp = ev.fold_ref([a], dtype, pre, post)
        models = lambda: ev.wrong_models([a], dtype, pre, post)

        def run(dst, src, cnt):
            if post == 1.0:
                _lib.call("tips_scale", dst, src, cnt, dtype, pre, stream())
            else:
                _lib.call("tips_allreduce_scaled", src, dst, cnt, dtype, pre, post, stream())
            torch.cuda.synchronize()

        run(dc.data_ptr(), da.data_ptr(), n)
        ok = same(from_dev(dc, dtype), exp, dtype, (a,), models, "body + tail, factors %r" % ((pre, post),))
        db = da.clone()
        run(db.data_ptr(), db.data_ptr(), n)
        ok = same(from_dev(db, dtype), exp, dtype, (a,), models, "in place, factors %r" % ((pre, post),)) and ok
        dd = torch.full_like(da.view(torch.uint8), FILL).view(da.dtype)
        run(dd[1:].data_ptr(), da[1:].data_ptr(), n - 1)
        got = from_dev(dd, dtype)
        ok = same(got[1:], exp[1:], dtype, (a[1:],), None, "element-wise, factors %r" % ((pre, post),)) and ok
        assert ok and (got[:1].view(np.uint8) == FILL).all()


# ---------------------------------------------------------------------------
# the casts

WIRES = {"float16": F16, "bfloat16": BF16}


def check_cast(outs, parts, wire):
    """Every output against widen(narrow(x)); NaN inputs come back NaN, 0x7f800001 and 0x7fffffff
    (which a truncating or an add-and-shift narrowing turns into inf or -0) among them."""
    ok = True
    for k, (o, x) in enumerate(zip(outs, parts)):
        got = o.cpu().numpy()
        exp = ev.cast_ref(x, wire)
        if not ev.same_cast(got, exp):
            ok = False
            idx = np.nonzero(~((bits(got) == bits(exp)) | (np.isnan(got) & np.isnan(exp))))[0]
            head = idx[:6]
            print("tensor %d: %d of %d elements differ; first at %s\n  input:    %s\n  got:      %s\n  expected: %s" % (
                k, idx.size, got.size, head.tolist(), hexes(x, head), hexes(got, head), hexes(exp, head)))
            names = [name for name, m in ev.cast_wrong_models(x, wire).items() if ev.same_cast(got, m)]
            print("  the device output equals the wrong model(s): %s" % (names if names else "none of them"))
        assert np.isnan(got[np.isnan(x)]).all()
    return ok


def cast_patterns_present(parts):
    allbits = np.concatenate([bits(p) for p in parts])
    return all(v in allbits for v in (0x7f800001, 0x7fffffff, 0xff80ffff))


@pytest.mark.parametrize("wire", sorted(WIRES))
def test_cast_staged_tiles(gpu, monkeypatch, wire):
    """One 16-byte-aligned tensor of three whole 8 KiB wire tiles below the fusion threshold: the
    LDS-staged tile path of the pack and unpack kernels sees the whole set."""
    import torch
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(64 << 20))
    x = ev.cast_set(WIRES[wire])
    n = -(-x.size // 4096) * 4096
    x = np.resize(x, n)
    t = torch.from_numpy(x.copy()).cuda()
    assert t.data_ptr() % 16 == 0 and cast_patterns_present([x])
    outs = gpu.fused_allreduce_cast([t], wire)
    torch.cuda.synchronize()
    assert check_cast(outs, [x], WIRES[wire])
    assert np.array_equal(bits(t.cpu().numpy()), bits(x))  # the input unchanged


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("wire", sorted(WIRES))
def test_cast_small_views(gpu, monkeypatch, wire, aligned):
    """The set cut into many views of odd sizes, 4-byte aligned only (every element through the
    per-element path) or each starting on 16 bytes (quads, and the ragged ends per element)."""
    import torch
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", str(64 << 20))
    x = ev.cast_set(WIRES[wire])
    rng = ev.rng_for(4, aligned)
    sizes = []
    while sum(sizes) < x.size:
        sizes.append(min(int(round(2 ** rng.uniform(0, 9))) | 1, x.size - sum(sizes)))
    base = torch.zeros(x.size + 4 * len(sizes) + 8, dtype=torch.float32, device="cuda")
    views, parts, off, pos = [], [], 0 if aligned else 1, 0
    for k in sizes:
        views.append(base[off:off + k])
        parts.append(x[pos:pos + k])
        views[-1].copy_(torch.from_numpy(parts[-1].copy()))
        pos += k
        off += k + 1
        if aligned:
            off = (off + 3) // 4 * 4
    assert cast_patterns_present(parts)
    assert all(v.data_ptr() % 16 == 0 for v in views) if aligned else views[0].data_ptr() % 16 == 4
    outs = gpu.fused_allreduce_cast(views, wire)
    torch.cuda.synchronize()
    assert check_cast(outs, parts, WIRES[wire])


@pytest.mark.parametrize("wire", sorted(WIRES))
def test_cast_range(gpu, monkeypatch, wire):
    """One tensor above a threshold of 4096 bytes (the range cast through the scratch buffer): aligned
    (whole tiles staged, then quads, then single elements) and offset by one element (per element)."""
    import torch
    monkeypatch.setenv("TIPS_FUSION_THRESHOLD", "4096")
    x = ev.cast_set(WIRES[wire])
    x = x[:x.size - (x.size % 4 == 0)]  # a remainder after the quads
    base = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
    for view in (base[:x.size], base[1:]):
        view.copy_(torch.from_numpy(x.copy()))
        assert cast_patterns_present([x])
        outs = gpu.fused_allreduce_cast([view], wire)
        torch.cuda.synchronize()
        assert check_cast(outs, [x], WIRES[wire])
        del outs


# ---------------------------------------------------------------------------
# the schedules

@pytest.mark.parametrize("kind", ["ring", "direct", "oneshot"])
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_schedules(gpu, oracle, dtype, kind):
    """Three virtual ranks' plans on the fold's edge set: the ring against the oracle's ring (a
    storage-type add per step; test_edge_values_cpu.py holds it against the closed form in numpy),
    direct and one-shot against the fp32-accumulating fold."""
    ins = list(ev.tuple_set(dtype)[:3])
    if kind == "ring":
        exp = oracle.ring(ins, code=dtype)[0]
    else:
        exp = oracle.fold(ins, code=dtype, wide_acc=True)
        assert same_bits(exp, ev.fold_ref(ins, dtype), dtype)
    models = None if kind == "ring" else (lambda: ev.wrong_models(ins, dtype))  # (the models are the fold's)
    for r, got in enumerate(simulate(kind, ins, dtype)):
        assert same(got, exp, dtype, ins, models, "%s, rank %d" % (kind, r))
