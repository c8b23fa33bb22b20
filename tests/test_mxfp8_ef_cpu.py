"""MXFP8 error feedback without a GPU: the restatement's own properties
(tests/mxfp8_ef_util.py), the point of the feature - the error of the mean output falls with the
number of steps where the plain wire's stays - the state-size formula and the Python surface."""
import numpy as np
import pytest

import mxfp8_ef_util as ef
import mxfp8_util as mx


# ---------------------------------------------------------------- the restatement's own properties

def test_zero_state_gives_the_plain_wire():
    """With an all-zero residual the wire is mxfp8_util.quantize's on inputs without -0; an input -0
    becomes +0 (-0 + +0 = +0) and encodes as 0x00, not 0x80 - nothing else changes."""
    rng = np.random.default_rng(1)
    n = 4099
    elems = mx.round_up(n, 64)
    x = mx.spread_blocks(n, rng)
    x[x == 0] = np.float32(1.0)
    flat = mx.flat_of([x], [0], elems)
    mask = ef.mask_of([n], [0], elems)
    wire, r = ef.quantize_ef(flat, mask, np.zeros(mx.scales_offset(elems), np.float32))
    assert np.array_equal(wire, mx.quantize(flat))
    assert np.isfinite(r).all() and not r[~mask].any()
    x[5::7] = np.float32(-0.0)
    flat = mx.flat_of([x], [0], elems)
    plain = mx.quantize(flat)
    wire, _ = ef.quantize_ef(flat, mask, np.zeros(mx.scales_offset(elems), np.float32))
    neg_zero = np.zeros(plain.size, bool)
    neg_zero[:n][5::7] = True
    assert (plain[neg_zero] == 0x80).all() and (wire[neg_zero] == 0x00).all()
    assert np.array_equal(wire[~neg_zero], plain[~neg_zero])


def test_a_poisoned_block_resets_its_residual_and_no_other():
    rng = np.random.default_rng(2)
    nb = 9
    x = rng.standard_normal((nb, 32)).astype(np.float32)
    r = (rng.standard_normal((nb, 32)) / 64).astype(np.float32)
    mask = np.ones((nb, 32), bool)
    _, sb0, r0 = ef.quantize_blocks_ef(x, r, mask)
    assert (sb0 != 255).all() and r0.any(axis=1).all()
    for k, bad in [(1, np.nan), (4, np.inf), (7, -np.inf)]:
        x[k, 3 * k] = bad
    x[5, 0], r[5, 0] = np.float32(3.0e38), np.float32(3.0e38)  # x + r overflows
    codes, sb, rn = ef.quantize_blocks_ef(x, r, mask)
    hit = np.isin(np.arange(nb), [1, 4, 5, 7])
    assert (sb[hit] == 255).all() and (codes[hit] == 0x7F).all() and (sb[~hit] != 255).all()
    assert (rn[hit].view(np.uint32) == 0).all()  # +0, every element
    assert np.array_equal(rn[~hit].view(np.uint32), r0[~hit].view(np.uint32))
    # positions without a tensor element: their residual is neither read nor written, and they count as +0
    mask[2, 20:] = False
    r[2, 20:] = np.float32(777.0)
    x[2, 20:] = np.float32(1.0e30)
    codes, sb, rn = ef.quantize_blocks_ef(x, r, mask)
    c2 = (x[2] + r[2]).astype(np.float32)
    c2[20:] = 0
    want_codes, want_sb = mx.quantize_blocks(c2[None, :])
    assert (rn[2, 20:] == 777.0).all() and np.array_equal(codes[2], want_codes[0]) and sb[2] == want_sb[0]
    assert (codes[2, 20:] == 0).all()
    # the fold: a poisoned source block resets the owner residual of that block alone
    elems = nb * 32
    wires = [mx.quantize(rng.standard_normal(elems).astype(np.float32)) for _ in range(3)]
    wires[1][mx.scales_offset(elems) + 6] = 255
    wires[1][6 * 32:7 * 32] = 0x7F
    o = (rng.standard_normal(5 * 32) / 16).astype(np.float32)
    out, on = ef.fold_ef(np.zeros_like(wires[0]), wires, elems, 3, 5, o)
    sbs = out[mx.scales_offset(elems) + 3:][:5]
    assert list(sbs == 255) == [False, False, False, True, False]
    on = on.reshape(5, 32)
    assert (on[3].view(np.uint32) == 0).all() and on[[0, 1, 2, 4]].any(axis=1).all()


def test_residuals_stay_finite_over_random_steps():
    """Finite states stay finite whatever arrives: huge, tiny, NaN and Inf inputs over 40 steps at p = 1 and 3."""
    rng = np.random.default_rng(3)
    n = 700
    elems = mx.round_up(n, 64)
    mask = ef.mask_of([n], [0], elems)
    for p in (1, 3):
        states = [np.zeros(ef.ef_elems(elems, p), np.float32) for _ in range(p)]
        for step in range(40):
            flats = []
            for r in range(p):
                x = mx.spread_blocks(n, rng, -140, 127)
                if step % 5 == 1:
                    x[rng.integers(n, size=3)] = [np.nan, np.inf, -np.inf]
                flats.append(mx.flat_of([x], [0], elems))
            out, states = ef.collective_ef(flats, states, 1.0, mask)
            assert all(np.isfinite(s).all() for s in states), (p, step)
            assert np.isnan(out).any() == (step % 5 == 1)  # the step is lost, the next one is not


# ---------------------------------------------------------------- the point of the feature

T = 64
NB = 24


def persistent_inputs(p, seed):
    """NB blocks per rank. Every block has one outlier of magnitude 1 (its position and sign differ per
    rank) and 31 persistent components, the same on every rank: (k + 0.45) / 32 with k in 8 ... 15 -
    values in [0.25, 0.5) that sit 0.45 of a grid step above an e4m3 grid point under the outlier's
    scale (step 1 / 32), so the plain quantiser drops 0.45 / 32 of each of them on every rank and step."""
    rng = np.random.default_rng(seed)
    comp = ((rng.integers(8, 16, size=(NB, 32)) + 0.45) / 32).astype(np.float32)
    flats = []
    for _ in range(p):
        x = comp.copy()
        pos = rng.integers(32, size=NB)
        x[np.arange(NB), pos] = rng.choice(np.array([-1.0, 1.0], np.float32), size=NB)
        flats.append(x.reshape(-1))
    return flats


def ef_bound(flats, steps):
    """The bound on |mean over `steps` outputs - true sum| per block, from the definition alone.

    Sender r, step t: c_t = x + r_{t-1} + e_t, r_t = c_t - y_t + d_t with |e_t| <= 2^-24 |c_t| and
    |d_t| <= 2^-24 |r_t| (one f32 add, one f32 subtract). Summing over t = 1 ... T telescopes:
    SUM y_t + r_T = T x + r_0 + SUM (e_t + d_t), r_0 = 0. A quantisation errs by at most amax(c) / 16
    of its block (rules 2-3: the largest scaled magnitude lies in (224, 448], the grid step there is
    at most 32 and 16 below 256), so |r_t| <= amax(c_t) / 16 and, by induction,
    amax(c_t) <= amax(x) + amax(c_{t-1}) / 16 <= A_r = amax(x) * 16 / 15 (times 1 + 2^-20 for the add
    roundings). Owner: acc_t = SUM_r y_t^r + h_t, |h_t| <= (p - 1) 2^-24 S with S = SUM_r A_r * 17 / 16
    (a y is at most its block's amax rounded up by one sixteenth); c_t = acc_t + o_{t-1} + e'_t,
    o_t = c_t - out_t + d'_t, amax(c_t) <= C = S * 16 / 15 (same induction), |o_t| <= C / 16. So
      SUM_t out_t = T SUM_r x_r - SUM_r r_T^r - o_T + SUM_t (h_t + e'_t + d'_t + SUM_r (e_t^r + d_t^r))
      |mean - SUM_r x_r| <= (SUM_r A_r / 16 + C / 16) / T + 2^-24 (2 SUM_r A_r + (p - 1) S + 2 C).
    p = 1 has no owner: (A / 16) / T + 2^-24 * 2 A."""
    p = len(flats)
    amax = [np.abs(f.astype(np.float64)).reshape(-1, 32).max(axis=1) for f in flats]
    A = np.sum(amax, axis=0) * (16.0 / 15.0) * (1 + 2.0 ** -20)
    if p == 1:
        return A / 16 / steps + 2.0 ** -24 * 2 * A
    S = A * 17.0 / 16.0
    C = S * (16.0 / 15.0) * (1 + 2.0 ** -20)
    return (A / 16 + C / 16) / steps + 2.0 ** -24 * (2 * A + (p - 1) * S + 2 * C)


@pytest.mark.parametrize("p", [1, 2, 8])
def test_error_of_the_mean_falls_with_the_steps(p):
    """T = 64 steps of the same input: the mean output's error against the f64 sum is within the
    telescoping bound at every T, which falls as 1 / T; the plain wire gives the same output every
    step, so its error stays what it is - and on these inputs that is above the feedback bound."""
    flats = persistent_inputs(p, 10 + p)
    elems = flats[0].size
    exact = np.sum([f.astype(np.float64) for f in flats], axis=0)
    states = [np.zeros(ef.ef_elems(elems, p), np.float32) for _ in range(p)]
    total = np.zeros(elems, np.float64)
    worst = {}
    for t in range(1, T + 1):
        out, states = ef.collective_ef(flats, states)
        total += out.astype(np.float64)
        if t in (1, 4, 16, 64):
            err = np.abs(total / t - exact).reshape(-1, 32).max(axis=1)
            bound = ef_bound(flats, t)
            worst[t] = float(np.max(err / bound))
            assert (err <= bound).all(), (t, worst[t])
    b1, b64 = ef_bound(flats, 1), ef_bound(flats, T)
    assert (b64 < b1 / 60).all()  # the 2^-24 terms are all that does not fall
    plain = mx.collective(flats).astype(np.float64)
    assert np.array_equal(mx.collective(flats).astype(np.float64), plain)  # the same rounding every step
    plain_err = np.abs(plain - exact).reshape(-1, 32).max(axis=1)
    print("p = %d: worst error / bound per T %s; plain error / feedback bound at T = 64: %.1f ... %.1f"
          % (p, worst, float(np.min(plain_err / b64)), float(np.max(plain_err / b64))))
    assert (plain_err > b64).all()  # constant in T: above the feedback bound on every block
    err64 = np.abs(total / T - exact).reshape(-1, 32).max(axis=1)
    assert (err64 < plain_err).all()


def test_sum_of_outputs_telescopes_at_one_rank():
    """SUM_t y_t + r_T = T x (+ r_0 = 0) up to the adds' roundings, element by element."""
    flats = persistent_inputs(1, 20)
    state = [np.zeros(ef.ef_elems(flats[0].size, 1), np.float32)]
    total = np.zeros(flats[0].size, np.float64)
    for _ in range(T):
        out, state = ef.collective_ef(flats, state)
        total += out.astype(np.float64)
    lhs = total + state[0][:flats[0].size].astype(np.float64)
    assert np.max(np.abs(lhs - T * flats[0].astype(np.float64))) <= T * 2.0 ** -24 * 2 * (16.0 / 15.0) * 1.01


# ---------------------------------------------------------------- the state's size

@pytest.mark.parametrize("elems", [0, 32, 100, 128, 224, 256, 8192, 70016, (1 << 26) + 64])
@pytest.mark.parametrize("p", [1, 2, 3, 8, 16])
def test_ef_bytes_formula(elems, p):
    """4 * (round_up(E, 256) + 32 * per), per = chunk 0's blocks (0 on one rank); B < 8: chunk 0 holds every block."""
    import tips_amd
    from tips_amd import _lib
    nb = -(-elems // 32)
    per = 0 if p == 1 else min(nb, mx.round_up(-(-nb // p), 8))
    want = 4 * (mx.round_up(elems, 256) + 32 * per)
    assert _lib.lib().tips_mxfp8_ef_bytes(elems, p) == want == ef.ef_bytes(elems, p)
    assert tips_amd.mxfp8_ef_bytes(elems, p) == want
    if p > 1 and nb < 8:
        assert per == nb and all(ef.chunk_of(nb, p, q) == (nb, nb) for q in range(1, p))


def test_ef_refusals_without_a_device():
    from tips_amd import _lib
    L = _lib.lib()
    one, _k = _lib.i64_array([64])
    some, _k4 = _lib.ptr_array([4096])
    assert L.tips_mxfp8_ef_bytes(-1, 1) == -1
    for bad in (0, 17, -2):
        assert L.tips_mxfp8_ef_bytes(64, bad) == -1 and b"nranks" in L.tips_last_error()
    assert L.tips_mxfp8_quantize_ef(None, None, 0, None, None, None) == 0      # nothing to do
    assert L.tips_mxfp8_quantize_ef(some, one, 1, None, None, None) == -1      # null wire
    assert L.tips_mxfp8_fold_ef(None, some, 0, 64, 0, 1, None, None) == -1
    assert L.tips_mxfp8_fold_ef(None, some, 1, 64, 1, 2, None, None) == -1     # 2 blocks in all
    assert L.tips_mxfp8_fold_ef(None, some, 1, 64, 2, 0, None, None) == 0      # an empty range at the end
    assert L.tips_allreduce_mxfp8_ef(None, None, -1, 1.0, None, 0, None) == -1
    assert L.tips_allreduce_mxfp8_ef(None, None, 10, float("inf"), None, 0, None) == -1
    assert L.tips_allreduce_mxfp8_ef(None, None, 0, 1.0, None, 0, None) == -2  # not initialised
    assert L.tips_fused_allreduce_mxfp8_ef_flat(some, one, 1, None, 1.0, None, 0, None) == -1  # null flat


# ---------------------------------------------------------------- the Python surface

def test_error_feedback_is_a_stateful_object():
    import tips_amd
    from tips_amd import Compression
    a, b = Compression.fp8.error_feedback(), Compression.fp8.error_feedback()
    assert isinstance(a, tips_amd.MXFP8ErrorFeedback) and isinstance(a, tips_amd.Compressor) and a is not b
    assert Compression.fp8 is tips_amd.MXFP8Compressor  # the marker keeps its bits
    x = np.arange(5, dtype=np.float32)
    c, ctx = a.compress(x)
    assert c is x and ctx is None and a.decompress(c, ctx) is x
    assert a.state_dict() == {}


def test_state_dict_round_trip():
    import torch
    from tips_amd import Compression
    a = Compression.fp8.error_feedback()
    sig_list = ("list", "cuda:0", (300, 129, 4099), 2)
    sig_tensor = ("tensor", "embedding.weight", 70001, "cuda:0")
    state = {sig_list: torch.arange(7, dtype=torch.float32), sig_tensor: torch.full((3,), 0.5)}
    a.load_state_dict(state)
    got = a.state_dict()
    assert set(got) == {sig_list, sig_tensor}
    assert all(torch.equal(got[k], state[k]) and got[k] is not state[k] for k in state)
    got[sig_list][0] = 99.0  # a copy: the object's state is its own
    assert a.state_dict()[sig_list][0] == 0.0
    b = Compression.fp8.error_feedback()
    b.load_state_dict(a.state_dict())
    assert all(torch.equal(b.state_dict()[k], state[k]) for k in state)
    b.reset()
    assert b.state_dict() == {} and len(a.state_dict()) == 2
    with pytest.raises(ValueError):
        a.load_state_dict({"not a signature": torch.zeros(4)})
    with pytest.raises(ValueError):
        a.load_state_dict({sig_list: torch.zeros(4, dtype=torch.float64)})
    assert len(a.state_dict()) == 2  # a refused load changes nothing


def test_value_errors_of_the_surface():
    """Before any collective: nothing is initialised by these calls."""
    import tips_amd
    from tips_amd import Compression
    e = Compression.fp8.error_feedback()
    x = np.ones(4, np.float32)
    with pytest.raises(ValueError, match="name"):
        tips_amd.allreduce(x, compression=e)
    with pytest.raises(ValueError, match="fused=False"):
        tips_amd.allreduce_grads([x], compression=e, fused=False)
    for op in ("Max", "Min", "Adasum"):
        with pytest.raises(ValueError, match="Compression.fp8"):
            tips_amd.allreduce(x, compression=e, op=op, name="t")
        with pytest.raises(ValueError, match="Compression.fp8"):
            tips_amd.allreduce_grads([x], compression=e, op=op)
