"""numpy restatement of the MXFP8 wire (include/tips_hip.h, "MXFP8 wire"): quantise,
dequantise, fold and the collective over flat f32 layouts. The encoder is integer and bit operations
only; the two f32 multiplies and the fold's f32 adds are numpy float32 operations (IEEE, one rounding
each, subnormals kept). No dependency on the library: a list's offsets are an argument."""
import numpy as np

BLOCK = 32
QNAN = 0x7FC00000
INF = 0x7F800000
MAX448 = 0x43E00000  # 448.0f


def round_up(x, a):
    return -(-x // a) * a


def scales_offset(elems):
    return round_up(elems, 256)


def wire_bytes(elems):
    return round_up(elems, 256) + round_up(-(-elems // BLOCK), 256)


def encode_e4m3(v):
    """f32 values with |v| <= 448 -> e4m3fn codes (uint8), round to nearest even, sign kept."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    a = b & 0x7FFFFFFF
    assert a.size == 0 or a.max() <= MAX448
    r = a - 0x3C000000  # normal codes: exponent rebias 127 -> 7, then 20 fraction bits go
    normal = (r + 0x7FFFF + ((r >> 20) & 1)) >> 20
    ex = a >> 23
    mant = np.where(ex > 0, (a & 0x7FFFFF) | 0x800000, a & 0x7FFFFF)
    sh = np.clip(141 - np.maximum(ex, 1), 1, 40)  # |v| = mant * 2^(ex - 150); codes below 8 count 2^-9
    q = mant >> sh
    rem = mant & ((np.int64(1) << sh) - 1)
    half = np.int64(1) << (sh - 1)
    sub = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    code = np.where(a >= 0x3C800000, normal, sub)
    return (code | ((b >> 24) & 0x80)).astype(np.uint8)


def decode_e4m3(code):
    """e4m3fn codes -> f32 (0x7F / 0xFF: the quiet NaN)."""
    c = np.asarray(code, dtype=np.uint8).astype(np.uint32)
    m = c & 0x7F
    normal = (m << 20) + 0x3C000000
    sub = (m.astype(np.float32) * np.float32(2.0 ** -9)).view(np.uint32)
    bits = np.where(m >= 8, normal, sub) | ((c & 0x80) << 24)
    return np.where(m == 0x7F, np.uint32(QNAN), bits).astype(np.uint32).view(np.float32)


def scale_value(sb):
    """2^(sb - 127) as f32 for scale bytes 0 ... 254 (0: the subnormal 2^-127), NaN for 255."""
    sb = np.asarray(sb).astype(np.uint32)
    bits = np.where(sb == 255, np.uint32(QNAN), np.where(sb == 0, np.uint32(0x00400000), sb << 23))
    return bits.astype(np.uint32).view(np.float32)


def scale_bytes(amax_bits):
    """The scale byte of blocks whose largest |x| has these (finite) f32 bits."""
    am = np.asarray(amax_bits).astype(np.int64)
    s = np.maximum(am >> 23, 1) - 127 - 8 + ((am & 0x7FFFFF) > 0x600000)
    s = np.clip(s, -127, 119)
    return np.where(am == 0, 0, s + 127).astype(np.uint8)


def quantize_blocks(x):
    """x: f32 [nblocks, 32] -> (codes uint8 [nblocks, 32], scale bytes uint8 [nblocks])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = x.view(np.uint32)
    a = bits & 0x7FFFFFFF
    am = a.max(axis=1) if x.shape[0] else np.zeros(0, np.uint32)
    poisoned = am >= INF
    sb = scale_bytes(np.where(poisoned, 0, am))
    mul = ((254 - sb.astype(np.uint32)) << 23).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        v = (np.where(poisoned[:, None], np.float32(0), x) * mul[:, None]).astype(np.float32)
    vb = v.view(np.uint32)
    clamped = (np.minimum(vb & 0x7FFFFFFF, MAX448) | (vb & 0x80000000)).astype(np.uint32).view(np.float32)
    codes = encode_e4m3(clamped).reshape(x.shape)
    codes[poisoned] = 0x7F
    sb = sb.copy()
    sb[poisoned] = 0xFF
    return codes, sb


def flat_of(tensors, offsets, elems):
    """The flat f32 layout of a list: tensor i at element offsets[i], +0 everywhere else."""
    flat = np.zeros(elems, np.float32)
    for t, o in zip(tensors, offsets):
        t = np.asarray(t, np.float32).reshape(-1)
        flat[o:o + t.size] = t
    return flat


def quantize(flat):
    """flat f32 [E] -> the wire buffer (uint8 [wire_bytes(E)]), every byte defined."""
    elems = flat.size
    so = scales_offset(elems)
    x = np.zeros(so, np.float32)
    x[:elems] = flat
    codes, sb = quantize_blocks(x.reshape(-1, BLOCK))
    wire = np.zeros(wire_bytes(elems), np.uint8)
    wire[:so] = codes.reshape(-1)
    wire[so:so + sb.size] = sb
    return wire


def dequantize_blocks(codes, sb):
    with np.errstate(all="ignore"):
        y = (decode_e4m3(codes) * scale_value(sb)[:, None]).astype(np.float32)
    return y


def canonical(y):
    y = np.ascontiguousarray(y, dtype=np.float32).copy()
    y.view(np.uint32)[np.isnan(y)] = QNAN
    return y


def dequantize(wire, elems, factor=1.0):
    """wire -> flat f32 [E]: decode * 2^(scale - 127), then * f32(factor) when factor != 1."""
    so = scales_offset(elems)
    nb = -(-elems // BLOCK)
    codes = np.zeros(nb * BLOCK, np.uint8)
    codes[:min(so, nb * BLOCK)] = wire[:min(so, nb * BLOCK)]
    y = dequantize_blocks(codes.reshape(-1, BLOCK), wire[so:so + nb]).reshape(-1)[:elems]
    if float(factor) != 1.0:
        with np.errstate(all="ignore"):
            y = (y * np.float32(factor)).astype(np.float32)
    return canonical(y)


def fold_acc(wires, elems, begin, count):
    """((y0 + y1) + y2) + ... over blocks [begin, begin + count) of the wires, f32 [count, 32]."""
    so = scales_offset(elems)
    acc = None
    for w in wires:
        y = dequantize_blocks(w[begin * BLOCK:(begin + count) * BLOCK].reshape(-1, BLOCK), w[so + begin:so + begin + count])
        with np.errstate(all="ignore"):
            acc = y if acc is None else (acc + y).astype(np.float32)
    return acc


def fold(dst, wires, elems, begin, count):
    """dst (a wire buffer, copied) with blocks [begin, begin + count) = quantise(fold of the wires)."""
    out = dst.copy()
    if count:
        so = scales_offset(elems)
        codes, sb = quantize_blocks(fold_acc(wires, elems, begin, count))
        out[begin * BLOCK:(begin + count) * BLOCK] = codes.reshape(-1)
        out[so + begin:so + begin + count] = sb
    return out


def collective(flats, factor=1.0):
    """dequantise(quantise(fold over ranks in rank order of quantise(x_r)), factor), flat f32 [E]."""
    elems = flats[0].size
    wires = [quantize(f) for f in flats]
    if len(wires) == 1:
        return dequantize(wires[0], elems, factor)
    nb = scales_offset(elems) // BLOCK
    return dequantize(fold(wires[0], wires, elems, 0, nb), elems, factor)


def edge_values():
    """Every non-negative e4m3fn grid value, every midpoint between neighbours and each midpoint
    +- 1 f32 ulp, and their negatives (f32, all |v| <= 448)."""
    grid = decode_e4m3(np.arange(0x7F, dtype=np.uint8)).astype(np.float64)
    mid = ((grid[:-1] + grid[1:]) / 2).astype(np.float32)  # (exact in f32)
    assert np.array_equal(mid.astype(np.float64), (grid[:-1] + grid[1:]) / 2)
    pos = np.concatenate([grid.astype(np.float32), mid, np.nextafter(mid, np.float32(np.inf)),
                          np.nextafter(mid, np.float32(-np.inf))]).astype(np.float32)
    return np.concatenate([pos, -pos])


def spread_blocks(n, rng, lo=-140, hi=127):
    """n normal values whose per-block magnitudes are spread over 2^lo ... 2^hi (finite f32)."""
    x = rng.standard_normal(n)
    e = rng.integers(lo, hi - 2, size=-(-n // BLOCK), endpoint=True)
    with np.errstate(all="ignore"):
        v = (x * np.exp2(np.repeat(e, BLOCK)[:n].astype(np.float64))).astype(np.float32)
    v[~np.isfinite(v)] = np.float32(3.0e38)
    return v
