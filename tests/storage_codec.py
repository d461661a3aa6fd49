"""The three half-range storages of include/marconet_hip.h — plain f16 (MNET_F16), split half (MNET_F16X2) and fp16+8 (MNET_F16M, activations and the
conv-weight layout) — WRITTEN OUT from the header text as data, plus the tables the byte tests run: no device use, no call into marconet_amd/mxfmt.py or
marconet_amd/packing.py (those are among the things under test).  tests/test_storage_codec.py proves on a CPU that every page is what it claims to be and
that the host packers write these bytes; tests/test_storage_codec_gpu.py feeds the tables to every device writer and reader and compares BYTES.

Arithmetic.  numpy integers and fp64 only.  Every quantity below is exact in fp64: an fp32 value, a half, v - hi (Sterbenz-like: |v - hi| <= ulp(hi) / 2),
a power-of-two scaling, the sum of two halves.  The one inexact sum — the fp16+8 decode hi + lo8 * 2^(E - 138) of a block no conforming writer emits
(E = 254 under hi = 2^-24 spans 130 bits) — goes through `_sum_to_f32`, which rounds ONCE (fp64 sum rounded to odd, then to fp32).  Roundings are
`_rne`: round to nearest even onto the grid of a binary format given by its precision and its smallest normal exponent.

The rule (header, MNET_F16M).  Per (pixel, 32-channel block):  hi = f16(v);  m = max |hi|;
    E = 0                                        when m == 0
    E = max(floor(log2 m) + 120, 105)            otherwise            (s = 2^(E - 127);  the floor 105 = 127 - 15 - 7: blocks of fp16 subnormals)
    lo8 = e4m3((v - hi) * 2^(138 - E))           when E > 0           (= (v - hi) * 2^11 / s, round to nearest even, the sign kept when it rounds to zero)
    lo8 = e4m3((v - hi) * 0)                     when E == 0          (0x00, or 0x80 under a negative residual: a zero byte may carry a sign)
    decode: v' = fl32(hi + lo8 * 2^(E - 138)) for E >= 12, fl32(hi + lo8 * 0) for E < 12 — one rounding.
The scaled residual never leaves e4m3's range on finite input: it is at most 2^7 in a block of normal halves and 2^8 under the floor (`lo_reach`).
Conv weights: the same with ONE exponent per output channel, E_w = clamp(floor(log2 m) + 120, 11, 254) over the row (no floor at 105: a row with
0 < m < 2^-15 is outside the format — `weight_rows_defined` — 256 W of a layer never is), hi8 = e4m3(hi * 2^(127 - E_w)), the trailing byte E_w - 11."""
import numpy as np

F16_MAX = 65504.0
PERM = np.array(list(range(0, 8)) + list(range(16, 24)) + list(range(8, 16)) + list(range(24, 32)))      # storage order of the 32 lo bytes
INV_PERM = np.argsort(PERM)
E_FLOOR = 105
PAGE = 256                    # values per page: 8 blocks of 32 channels


# ================================================================================================================ number formats
def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def bits32(x):
    return f32(x).view(np.uint32)


def from_bits32(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def _floor_log2(a):
    """floor(log2 a) for finite a > 0 (frexp: exact); 0 where a == 0"""
    _, e = np.frexp(a)
    return np.where(a > 0, e - 1, 0).astype(np.int64)


def _rne(x, p, emin):
    """x (fp64) rounded to nearest even onto the format with p stored mantissa bits and smallest normal exponent emin (subnormals below it); no overflow
    handling — the caller compares with the format's maximum.  Signed zeros, inf and NaN pass through."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(x)
        ex = np.maximum(_floor_log2(np.where(fin, np.abs(x), 0.0)), emin)
        q = np.ldexp(1.0, (ex - p).astype(np.int32))
        return np.where(fin, np.rint(np.where(fin, x, 0.0) / q) * q, x)


def f16_round(v):
    """fp32 / fp64 values -> the half each rounds to, as fp64 (+-inf from 65520 on)"""
    r = _rne(v, 10, -14)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(r) > F16_MAX, np.copysign(np.inf, r), r)


def f16_bits(v):
    """the bits of f16_round(v) (uint16); the cast below is exact — the value is a half already"""
    with np.errstate(over="ignore"):
        return f16_round(v).astype(np.float16).view(np.uint16)


def f16_value(b):
    return np.ascontiguousarray(b, dtype=np.uint16).view(np.float16).astype(np.float64)


def _e4m3_table():
    t = np.zeros(256, dtype=np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        v = m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)
        if (c & 0x7f) == 0x7f:
            v = np.nan
        t[c] = -v if c & 0x80 else v
    return t


E4M3_VALUE = _e4m3_table()        # OCP e4m3 (fn): no infinities, 0x7f / 0xff NaN, largest finite 448 = 0x7e
E4M3_MAX = 448.0


def e4m3_bits(x):
    """fp64 -> e4m3 byte, round to nearest even, the sign kept on a zero; beyond 448 after rounding (or NaN): 0x7f | sign, what the device conversions give"""
    r = _rne(x, 3, -6)
    a = np.abs(r)
    with np.errstate(invalid="ignore"):
        bad = ~(a <= E4M3_MAX)
    a = np.where(bad, 0.0, a)
    e = _floor_log2(a)
    normal = a >= 2.0 ** -6
    code = np.where(normal, ((e + 7) << 3) + (np.ldexp(a, (3 - e).astype(np.int32)).astype(np.int64) - 8), np.ldexp(a, 9).astype(np.int64))
    code = np.where(bad, 0x7f, code)
    return (code | (np.signbit(r).astype(np.int64) << 7)).astype(np.uint8)


def _sum_to_f32(a, b):
    """fl32(a + b) with ONE rounding (a, b fp64): the fp64 sum is rounded to odd when it is inexact (two-sum error term), which makes the second rounding
    to fp32's 24 bits the rounding of the exact sum"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = a + b
        bb = s - a
        err = (a - (s - bb)) + (b - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0)
        i = s.view(np.int64).copy()
        away = (err > 0) == (s > 0)                       # the exact sum lies further from zero than s
        i = np.where(fix & ((i & 1) == 0), np.where(away, i + 1, i - 1), i)
        return i.view(np.float64).astype(np.float32)


# ================================================================================================================ the storages
def _blocks(v):
    v = f32(v)
    assert v.shape[-1] % 32 == 0
    return v.reshape(v.shape[:-1] + (v.shape[-1] // 32, 32))


def encode_f16(v):
    """fp32 [...] -> uint8 [..., 2 per element]"""
    b = f16_bits(f32(v))
    return b.view(np.uint8).reshape(b.shape[:-1] + (b.shape[-1] * 2,))


def decode_f16(raw):
    """uint8 -> fp32 bits"""
    return bits32(f16_value(np.ascontiguousarray(raw).view(np.uint16)).astype(np.float32))


def encode_split(v):
    """split half: per 32-channel block 64 bytes of hi = f16(v), then 64 bytes of lo = f16(v - hi).  fp32 [..., C] -> uint8 [..., 4 C]"""
    vb = _blocks(v).astype(np.float64)
    hi = f16_round(vb)
    with np.errstate(invalid="ignore"):
        lo = vb - hi
    out = np.stack((f16_bits(hi), f16_bits(lo)), axis=-2)                    # [..., C/32, 2, 32] halves
    return np.ascontiguousarray(out).view(np.uint8).reshape(vb.shape[:-2] + (vb.shape[-2] * 128,))


def decode_split(raw):
    """uint8 [..., 4 C] -> fp32 bits [..., C]: fl32(hi + lo), one rounding (the sum of two halves is exact in fp64)"""
    raw = np.ascontiguousarray(raw)
    h = f16_value(raw.view(np.uint16)).reshape(raw.shape[:-1] + (raw.shape[-1] // 128, 2, 32))
    with np.errstate(invalid="ignore"):
        s = (h[..., 0, :] + h[..., 1, :]).astype(np.float32)
    return bits32(s.reshape(raw.shape[:-1] + (raw.shape[-1] // 4,)))


def block_exponent(hi):
    """hi [..., 32] (values of halves, finite) -> E [..., 1]"""
    m = np.abs(hi).max(axis=-1, keepdims=True)
    assert np.isfinite(m).all(), "the scale byte of a block that holds an inf / NaN is not defined"
    return np.where(m > 0, np.maximum(_floor_log2(m) + 120, E_FLOOR), 0)


def _lo_scaled(lo, E, first):
    """(v - hi) * 2^(138 - E) where E >= first, (v - hi) * 0 below (signed zero)"""
    return np.where(E >= first, lo * np.ldexp(1.0, (138 - np.maximum(E, first)).astype(np.int32)), lo * 0.0)


def encode_hm(v):
    """fp16+8 activations, finite blocks only.  fp32 [..., C] -> uint8 [..., 4 C]: bytes 0-63 hi | 64-95 lo8 in PERM order | 96 E | 97-127 zero"""
    vb = _blocks(v).astype(np.float64)
    hi = f16_round(vb)
    E = block_exponent(hi)
    lo8 = e4m3_bits(_lo_scaled(vb - hi, E, 1))
    out = np.zeros(vb.shape[:-1] + (128,), dtype=np.uint8)
    out[..., 0:64] = f16_bits(hi).view(np.uint8).reshape(vb.shape[:-1] + (64,))
    out[..., 64:96] = lo8[..., PERM]
    out[..., 96] = E[..., 0].astype(np.uint8)
    return out.reshape(vb.shape[:-2] + (vb.shape[-2] * 128,))


def decode_hm(raw):
    """uint8 [..., 4 C] -> fp32 bits [..., C]: fl32(hi + lo8 * 2^(E - 138)), one rounding; the lo scale is 0 for E < 12 (hm_lo_scale)"""
    raw = np.ascontiguousarray(raw)
    b = raw.reshape(raw.shape[:-1] + (raw.shape[-1] // 128, 128))
    hi = f16_value(np.ascontiguousarray(b[..., 0:64]).view(np.uint16))
    lo = E4M3_VALUE[b[..., 64:96]][..., INV_PERM]
    E = b[..., 96:97].astype(np.int64)
    sl = np.where(E >= 12, np.ldexp(1.0, (np.maximum(E, 12) - 138).astype(np.int32)), 0.0)
    with np.errstate(invalid="ignore"):
        out = _sum_to_f32(hi, lo * sl)
    return bits32(out.reshape(raw.shape[:-1] + (raw.shape[-1] // 4,)))


DECODE = {"f16": decode_f16, "split": decode_split, "mx": decode_hm}
ENCODE = {"f16": encode_f16, "split": encode_split, "mx": encode_hm}


def lo_reach(v):
    """largest |scaled residual| an fp16+8 encoding of v asks e4m3 for (<= 256 on every finite page: never saturated, never NaN)"""
    vb = _blocks(v).astype(np.float64)
    hi = f16_round(vb)
    return float(np.abs(_lo_scaled(vb - hi, block_exponent(hi), 1)).max())


# ---------------------------------------------------------------------------------------------------------------- conv weights
def mx_weight_rows(cout_pad, kh, kw, cin_pad):
    """rows of the [rows, kh, kw, cin_pad] tensor of 4-byte elements that holds cout_pad packed rows and, right behind them, one byte per output channel"""
    row_bytes = kh * kw * cin_pad * 4
    return cout_pad + -(-cout_pad // row_bytes)


def stored_weight_values(w_oihw, storage, scale=1.0, sigma=None, cout_pad=None, cin_pad=None):
    """the fp32 value mnet_pack_weights rounds into the storage, in its own fp32 steps: fl32(w / sigma) when there is a fold, times fl32(scale) (times 256
    in the blocked storages: a power of two, folded into the factor); zero padding; laid out [cout_pad, kh, kw, cin_pad]"""
    w = f32(w_oihw)
    o, i, kh, kw = w.shape
    if sigma is not None:
        w = w / np.float32(sigma)
    factor = np.float32(scale) * np.float32(256.0 if storage in ("split", "mx") else 1.0)
    w = w * factor
    out = np.zeros((cout_pad or o, kh, kw, cin_pad or i), dtype=np.float32)
    out[:o, :, :, :i] = w.transpose(0, 2, 3, 1)
    return out


def weight_row_exponent(hi_rows):
    """hi [O, K] -> E_w [O]"""
    m = np.abs(hi_rows).max(axis=1)
    return np.where(m > 0, np.clip(_floor_log2(m) + 120, 11, 254), 11)


def weight_rows_defined(v):
    """every output channel's max |f16(v)| is 0 or >= 2^-15 (below, the scaled residual can leave e4m3's range: there is no floor on weight rows)"""
    m = np.abs(f16_round(f32(v).reshape(v.shape[0], -1).astype(np.float64))).max(axis=1)
    return bool(((m == 0) | (m >= 2.0 ** -15)).all())


def encode_weight_hm(v):
    """fp16+8 conv weights.  v fp32 [O, KH, KW, I] = the values to store (`stored_weight_values`) -> uint8 [mx_weight_rows * KH * KW * I * 4]"""
    O, KH, KW, I = v.shape
    assert I % 32 == 0 and weight_rows_defined(v)
    vb = f32(v).reshape(O, KH * KW * I // 32, 32).astype(np.float64)
    hi = f16_round(vb)
    assert np.isfinite(hi).all()
    E = weight_row_exponent(hi.reshape(O, -1)).reshape(O, 1, 1)
    hi8 = e4m3_bits(hi * np.ldexp(1.0, (127 - E).astype(np.int32)))
    lo8 = e4m3_bits(_lo_scaled(vb - hi, E, 12))
    rows = np.zeros(vb.shape[:-1] + (128,), dtype=np.uint8)
    rows[..., 0:64] = f16_bits(hi).view(np.uint8).reshape(vb.shape[:-1] + (64,))
    p0, p1 = PERM[:16], PERM[16:]
    rows[..., 64:80], rows[..., 80:96] = lo8[..., p0], hi8[..., p0]
    rows[..., 96:112], rows[..., 112:128] = lo8[..., p1], hi8[..., p1]
    out = np.zeros(mx_weight_rows(O, KH, KW, I) * KH * KW * I * 4, dtype=np.uint8)
    out[: rows.size] = rows.reshape(-1)
    out[rows.size: rows.size + O] = (E.reshape(-1) - 11).astype(np.uint8)
    return out


def encode_weight(v, storage):
    """[O, KH, KW, I] stored values -> the packed tensor's bytes, flat"""
    if storage == "mx":
        return encode_weight_hm(v)
    if storage == "f32":
        return f32(v).view(np.uint8).reshape(-1)
    return ENCODE[storage](f32(v)).reshape(-1)


# ================================================================================================================ the writer table
def _p2(k):
    return float(np.ldexp(1.0, k))


def _below(x):
    """the next fp32 towards zero"""
    return float(np.nextafter(np.float32(x), np.float32(0.0)))


def _rng(seed):
    return np.random.default_rng(seed)


def _fill(rng, mag, n=32):
    """n fp32 values of full mantissas, |v| < 0.9 mag"""
    return (rng.uniform(-0.9, 0.9, n) * mag).astype(np.float32)


def _hi(v):
    return f16_round(f32(v).astype(np.float64))


def _page(blocks):
    assert len(blocks) == 8
    return f32(np.concatenate([f32(b).reshape(32) for b in blocks]))


POW2_K = (-24, -15, -14, -8, 0, 15)
ROUND_UP_K = (-15, -14, -8, 0, 15, -3, 1, 10)        # 2^k: the half the largest fp32 below it rounds up to
SUBNORMAL_MAX = (_p2(-24), 3 * _p2(-24), _p2(-22), 5 * _p2(-21), _p2(-18), 1023 * _p2(-24), _p2(-16), 1.5 * _p2(-15))
UNDERFLOW_D = tuple(range(10, 31))


def _tie_value(k, t, neg_h, neg_t, mant):
    """an fp32 value of a block with max |hi| = 2^k (k >= -6) whose scaled residual is exactly +-t (t a midpoint of two e4m3 codes, t < 128):
    v = h + t * 2^(k - 18), h a half of exponent j chosen so that the residual stays inside h's rounding interval and v fits fp32's 24 bits"""
    g = max(int(np.floor(np.log2(t))), -7)               # e4m3 binade of t (-7: the subnormal range, codes 0 .. 7)
    j = min(k, k + g - 5)
    h = np.ldexp(1.0 + (mant % 1024) / 1024.0, j) * (-1.0 if neg_h else 1.0)
    v = h + (-t if neg_t else t) * np.ldexp(1.0, k - 18)
    assert float(np.float32(v)) == v, "tie value not an fp32"
    return v


def _e4m3_ties():
    """(t, lower code) for every pair of adjacent positive codes 0x00 .. 0x7e"""
    return [((E4M3_VALUE[c] + E4M3_VALUE[c + 1]) / 2, c) for c in range(0, 0x7e)]


def _tie_pages():
    """ties below 128 in blocks of maximum 1.0 (E = 120), both signs of the residual under both signs of hi; ties 136 .. 248 — reachable only under the floor —
    in blocks of maximum 2^-16 (E = 105).  [256, 448] is out of every writer's reach (`lo_reach`)."""
    ties = [(t, c) for t, c in _e4m3_ties() if t < 128]
    elems = []
    for n, (t, c) in enumerate(ties):
        for neg_t in (False, True):
            elems.append(_tie_value(0, t, (n + neg_t) % 3 == 0, neg_t, 37 * n + 5))
    blocks = []
    for i in range(0, len(elems), 31):
        part = elems[i:i + 31]
        blocks.append([1.0 if (i // 31) % 2 == 0 else -1.0] + part + [0.0] * (31 - len(part)))
    high = []
    for n, (t, c) in enumerate((t, c) for t, c in _e4m3_ties() if 128 < t < 256):
        for neg_t in (False, True):
            h = (3 + 5 * n) * _p2(-24) * (-1.0 if n % 2 else 1.0)
            high.append(h + (-t if neg_t else t) * _p2(-33))
    assert len(high) <= 31
    blocks.append([_p2(-16)] + high + [0.0] * (31 - len(high)))
    while len(blocks) % 8:
        blocks.append([0.0] * 32)
    return [_page(blocks[i:i + 8]) for i in range(0, len(blocks), 8)]


def _half_tie_page():
    """values exactly halfway between two adjacent halves: even and odd lower neighbour, both signs, subnormal / normal / top binades"""
    rng = _rng(11)
    blocks = []
    for b, j in enumerate((-24, -20, -14, -9, -1, 0, 7, 15)):          # exponent of the lower half's unit: the half is n * 2^(j - 10) (j = -24: subnormal grid)
        unit = _p2(-24) if j <= -15 else _p2(j - 10)
        base = 0 if j <= -15 else 1024
        ns = rng.integers(0, 1023, 32) + base
        ns[0], ns[1], ns[2], ns[3] = base, base + 1, base + 1022, base + 1021      # even, odd, even (rounds up into 2^(j+1) or stays), odd
        if j == 15:
            ns = np.minimum(ns, 2045)                                   # (2046.5 * 32 = 65488 is the last tie below 65504; 65520 is on the overflow page)
        sign = np.where(np.arange(32) % 2 == 0, 1.0, -1.0) if b % 2 else np.ones(32)
        blocks.append((ns + 0.5) * unit * sign)
    return _page(blocks)


def _finite_pages():
    rng = _rng(3)
    pages = []

    def add(name, cls, v):
        pages.append({"name": name, "cls": cls, "v": f32(v)})

    # block maximum exactly 2^k: blocks 0-5 one k each, 6 / 7 a negative maximum
    blocks = []
    for k, sgn in [(k, 1.0) for k in POW2_K] + [(-24, -1.0), (0, -1.0)]:
        b = _fill(rng, _p2(k))
        b[int(rng.integers(0, 32))] = sgn * _p2(k)
        blocks.append(b)
    add("max_pow2", "max_pow2", _page(blocks))
    # the largest fp32 below 2^k is the block's maximum and rounds UP to 2^k in half: the scale has to come from hi
    blocks = []
    for n, k in enumerate(ROUND_UP_K):
        b = _fill(rng, _p2(k - 1))
        b[(5 * n + 2) % 32] = _below(_p2(k)) * (-1.0 if n % 3 == 2 else 1.0)
        blocks.append(b)
    add("max_rounds_up", "max_rounds_up", _page(blocks))
    # 65504 and the largest fp32 that still rounds to it
    top = _below(65520.0)
    blocks = []
    for n, m in enumerate((65504.0, top, -65504.0, -top, 65504.0, top, _below(65504.0), -top)):
        b = _fill(rng, 65504.0 if n < 4 else 100.0)
        b[(7 * n + 1) % 32] = m
        blocks.append(b)
    add("half_max", "half_max", _page(blocks))
    for n, p in enumerate(_tie_pages()):
        add("e4m3_ties_%d" % n, "e4m3_ties", p)
    add("half_ties", "half_ties", _half_tie_page())
    # elements 2^-10 ... 2^-30 below their block's maximum, residuals that underflow e4m3 (both signs: signed zero bytes)
    blocks = []
    for b in range(8):
        mx = (1.0, -1.0, 1.5, 640.0, _p2(-8) * 1.25, 65504.0, 3.0, -0.0078125)[b]
        blk = np.zeros(32)
        blk[0] = mx
        for i in range(1, 32):
            d = UNDERFLOW_D[(i - 1 + 10 * (b % 3)) % len(UNDERFLOW_D)]
            # (1 + 2^-11 + 2^-13): above the half tie -> hi rounds up, a negative residual; (1 + 2^-12): a positive one
            frac = (1 + _p2(-11) + _p2(-13)) if (i + b) % 2 else (1 + _p2(-12))
            blk[i] = abs(mx) * _p2(-d) * frac * (-1.0 if i % 3 == 0 else 1.0)
        blocks.append(blk)
    add("lo_underflow", "lo_underflow", _page(blocks))
    # blocks of fp16 subnormals down to max |hi| = 2^-24: the floor of the exponent at 105
    blocks = []
    for n, m in enumerate(SUBNORMAL_MAX):
        b = _fill(rng, m)
        b[(3 * n) % 32] = m * (-1.0 if n % 2 else 1.0)
        b[(3 * n + 1) % 32] = (3 if n else 1) * _p2(-25)       # a half tie on the subnormal grid: 3 * 2^-25 -> 2^-23, 2^-25 -> 0 (residuals -+2^-25: the largest)
        blocks.append(b)
    add("subnormal_blocks", "subnormal_blocks", _page(blocks))
    # every hi is +-0 while v != 0
    tiny = [1e-9, -_p2(-26), _p2(-25), -_p2(-25), 1e-40, -1e-42, _p2(-100), -_p2(-126), _below(_p2(-25)), -_below(_p2(-25)), _p2(-149), -_p2(-149)]
    blocks = [np.array([1e-9, -_p2(-26), _p2(-25)] + [0.0] * 29)]                     # the block of the finding
    for b in range(1, 8):
        blk = np.array([tiny[(i + b) % len(tiny)] * (1.0 if (i * b) % 5 else -1.0) for i in range(32)])
        if b % 2:
            blk[b::4] = 0.0
        if b == 7:
            blk = -np.abs(blk)                                                         # every residual negative
        blocks.append(blk)
    add("zero_hi", "zero_hi", _page(blocks))
    add("zeros", "zeros", np.zeros(PAGE))
    # -0.0: alone, among +0, among values
    blocks = [np.full(32, -0.0), np.where(np.arange(32) % 2 == 0, -0.0, 0.0), np.where(np.arange(32) % 3 == 0, -0.0, 1.0)]
    b3 = _fill(rng, 4.0)
    b3[::5] = -0.0
    blocks += [b3, np.where(np.arange(32) < 8, -0.0, 0.0), np.where(np.arange(32) == 31, -0.0, 0.0), np.where(np.arange(32) % 2 == 0, -0.0, -_p2(-26)),
               np.where(np.arange(32) % 2 == 0, -0.0, _p2(-20))]
    add("neg_zero", "neg_zero", _page(blocks))
    # one non-zero element per block, in each of the four 8-channel chunks
    blocks = []
    for b, (pos, val) in enumerate([(3, 1.0009765), (12, -317.123), (21, 6.1e-5), (30, -2.5e-7), (0, 65000.0), (15, 2.9e-8), (16, -1.0), (31, 0.33333334)]):
        blk = np.zeros(32)
        blk[pos] = np.float32(val)
        blocks.append(blk)
    add("one_nonzero", "one_nonzero", _page(blocks))
    # fp32 subnormals: alone, and below a normal maximum
    sub = [from_bits32(np.uint32(x)).item() for x in (1, 2, 0x7fffff, 0x400000, 0x80000001, 0x807fffff, 12345, 0x80300000)]
    blocks = []
    for b in range(8):
        blk = np.array([sub[(i + b) % 8] for i in range(32)], dtype=np.float64)
        if b >= 4:
            blk[(b * 5) % 32] = (1.0, -_p2(-14), _p2(-24), 300.0)[b - 4]
        blocks.append(blk)
    add("f32_subnormal", "f32_subnormal", _page(blocks))
    # ordinary data, decades of magnitude across a block: what the other tests use
    add("gaussian", "gaussian", (rng.standard_normal(PAGE) * np.logspace(-4, 3, PAGE)[rng.permutation(PAGE)]).astype(np.float32))
    return pages


def _nonfinite_pages():
    """block 0 (and block 5) of a page holds the non-finite elements next to finite neighbours; the other blocks are finite"""
    rng = _rng(5)
    pages = []
    for name, bad in (("inf", (np.inf, -np.inf)), ("nan", (np.nan, -np.nan)), ("overflow", (65520.0, -1e6, 3.0e38, -65520.0))):
        v = (rng.standard_normal(PAGE) * 3).astype(np.float32)
        mask = np.zeros(PAGE, dtype=bool)
        for n, x in enumerate(bad):
            for pos in ((1 + 9 * n) % 32, 5 * 32 + (20 + 3 * n) % 32):
                v[pos] = x
                mask[pos] = True
        pages.append({"name": name, "cls": "nonfinite", "v": v, "bad": mask})
    return pages


_CACHE = {}


def writer_pages():
    if "w" not in _CACHE:
        _CACHE["w"] = _finite_pages()
    return _CACHE["w"]


def nonfinite_pages():
    if "n" not in _CACHE:
        _CACHE["n"] = _nonfinite_pages()
    return _CACHE["n"]


def writer_table():
    """fp32 [pages, 256]: the finite pages"""
    return f32(np.stack([p["v"] for p in writer_pages()]))


# ---------------------------------------------------------------------------------------------------------------- class predicates
def tie_census(v):
    """the e4m3 ties among the scaled residuals of page v: a set of (binade of t, sign of the residual, lower code odd)"""
    vb = _blocks(v).astype(np.float64)
    hi = f16_round(vb)
    sc = _lo_scaled(vb - hi, block_exponent(hi), 1).reshape(-1)
    found = set()
    mids = {t: c for t, c in _e4m3_ties()}
    for x in sc:
        c = mids.get(abs(float(x)))
        if c is not None:
            found.add((c >> 3, bool(x < 0), bool(c & 1)))
    return found


def half_tie_count(v):
    """elements of v that lie exactly halfway between two adjacent halves"""
    x = f32(v).astype(np.float64).reshape(-1)
    h = f16_round(x).astype(np.float16)
    other = np.nextafter(h, np.where(x > h.astype(np.float64), np.inf, -np.inf).astype(np.float16))
    return int(((x != h.astype(np.float64)) & (x == (h.astype(np.float64) + other.astype(np.float64)) / 2)).sum())


def _underflow_ok(v):
    """every element but the block's first lies in the binades 2^-10 ... 2^-30 below it, and zero lo bytes of both signs occur"""
    a = np.abs(_blocks(v).astype(np.float64))
    ratio = a[:, 1:] / a[:, :1]
    lo = encode_hm(v).reshape(8, 128)[:, 64:96]
    return bool(((ratio < _p2(-9)) & (ratio >= _p2(-30))).all()) and bool((lo == 0x00).sum() >= 16) and bool((lo == 0x80).sum() >= 16)


def _bm(v):
    vb = _blocks(v).astype(np.float64)
    return np.abs(vb).max(-1), np.abs(f16_round(vb)).max(-1)


def _is_sub32(x):
    a = np.abs(f32(x))
    return (a > 0) & (a < np.float32(2.0 ** -126))


PREDICATES = {
    "max_pow2": lambda v: all(_bm(v)[1][b] == _p2(k) for b, k in enumerate(POW2_K + (-24, 0))),
    "max_rounds_up": lambda v: all(_bm(v)[1][b] == _p2(k) and _floor_log2(_bm(v)[0])[b] == k - 1 for b, k in enumerate(ROUND_UP_K)),
    "half_max": lambda v: bool((_bm(v)[1] == F16_MAX).all()) and bool((_bm(v)[0] > F16_MAX).sum() == 4) and bool((_bm(v)[0] == np.float64(_below(65520.0))).sum() == 4),
    "e4m3_ties": lambda v: len(tie_census(v)) > 0,
    "half_ties": lambda v: half_tie_count(v) == PAGE,
    "lo_underflow": _underflow_ok,
    "subnormal_blocks": lambda v: bool(((_bm(v)[1] > 0) & (_bm(v)[1] < _p2(-14))).all()) and _bm(v)[1].min() == _p2(-24)
    and bool((encode_hm(v).reshape(8, 128)[:, 96] == E_FLOOR).all()),
    "zero_hi": lambda v: bool((f16_round(f32(v).astype(np.float64)) == 0).all()) and bool((_bm(v)[0] > 0).all()),
    "zeros": lambda v: bool((bits32(v) == 0).all()),
    "neg_zero": lambda v: bool(((bits32(v) == 0x80000000).reshape(8, 32).sum(1) > 0).all()),
    "one_nonzero": lambda v: bool(((f32(v) != 0).reshape(8, 32).sum(1) == 1).all()) and {int(np.nonzero(b)[0][0]) // 8 for b in f32(v).reshape(8, 32)} == {0, 1, 2, 3},
    "f32_subnormal": lambda v: bool((_is_sub32(v).reshape(8, 32).sum(1) >= 31).all()),
    "gaussian": lambda v: bool(np.isfinite(v).all()) and float(np.abs(v).max()) < F16_MAX,
    "nonfinite": lambda v: True,
}


def nonfinite_mask(v):
    """elements whose half is inf / NaN (|v| >= 65520 included)"""
    return ~np.isfinite(f16_round(f32(v).astype(np.float64)))


# ================================================================================================================ the reader table
READER_E = (105, 106, 120, 127, 135, 142, 254)
READER_HI_BITS = (0x0000, 0x8000, 0x0001, 0x8001, 0x3c00, 0x3801, 0x7bff)       # +-0, +-2^-24, 1, 0.5 + ulp, 65504
LO_CODES = np.array([c for c in range(256) if (c & 0x7f) != 0x7f], dtype=np.uint8)   # the 254 non-NaN bytes


def _raw_block(hi_bits, lo_bytes, E):
    """32 hi bit patterns (channel order), 32 lo bytes (channel order), E -> the 128 bytes of one fp16+8 block"""
    b = np.zeros(128, dtype=np.uint8)
    b[0:64] = np.asarray(hi_bits, dtype=np.uint16).view(np.uint8)
    b[64:96] = np.asarray(lo_bytes, dtype=np.uint8)[PERM]
    b[96] = E
    return b


def reader_table_hm():
    """uint8 [blocks, 128], blocks a multiple of 8: for every E of READER_E, 254 blocks in which channel j of block i holds lo byte LO_CODES[(i + 7 j) % 254]
    (every byte in every position) over hi = READER_HI_BITS[(i + j) % 7] (every hi over every position); then E = 0 blocks with zero (0x00 / 0x80) lo bytes"""
    if "rh" in _CACHE:
        return _CACHE["rh"]
    j = np.arange(32)
    blocks = []
    for E in READER_E:
        for i in range(254):
            blocks.append(_raw_block(np.array(READER_HI_BITS, dtype=np.uint16)[(i + j) % 7], LO_CODES[(i + 7 * j) % 254], E))
    for i in range(7):
        blocks.append(_raw_block(np.array(READER_HI_BITS[:2], dtype=np.uint16)[(i + j) % 2], np.zeros(32), 0))                      # all-zero block, +-0 halves
        blocks.append(_raw_block(np.array(READER_HI_BITS[:2], dtype=np.uint16)[(i * j) % 2], np.where((j + i) % 3 == 0, 0x80, 0), 0))   # zero-hi block, signed zero bytes
    while len(blocks) % 8:
        blocks.append(np.zeros(128, dtype=np.uint8))
    _CACHE["rh"] = np.stack(blocks)
    return _CACHE["rh"]


def reader_table_hm_special():
    """property-only blocks: {"lo_nan": lo bytes 0x7f / 0xff among finite ones, "hi_nonfinite": hi = inf / NaN among finite ones}; uint8 [8, 128] each, with the
    mask of the elements that hold the special value"""
    j = np.arange(32)
    out = {}
    blocks, masks = [], []
    for b in range(8):
        lo = LO_CODES[(11 * b + 5 * j) % 254].copy()
        m = (j % 8) == b
        lo[m] = 0x7f if b % 2 == 0 else 0xff
        blocks.append(_raw_block(np.array(READER_HI_BITS, dtype=np.uint16)[(b + j) % 7], lo, (120, 127, 105, 135)[b % 4]))
        masks.append(m)
    out["lo_nan"] = (np.stack(blocks), np.stack(masks))
    blocks, masks = [], []
    for b in range(8):
        hi = np.array(READER_HI_BITS, dtype=np.uint16)[(b + j) % 7].copy()
        m = (j % 8) == (7 - b)
        hi[m] = (0x7c00, 0xfc00, 0x7e00, 0xfe01)[b % 4]
        blocks.append(_raw_block(hi, LO_CODES[(3 * b + 7 * j) % 254], (120, 127, 105, 135)[b % 4]))
        masks.append(m)
    out["hi_nonfinite"] = (np.stack(blocks), np.stack(masks))
    return out


SPLIT_LO_BITS = (0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0400, 0x1000, 0x9000, 0x2bff, 0xabff)   # +-0, subnormals, small normals


def reader_table_split():
    """uint8 [blocks, 128], blocks a multiple of 8: every hi of READER_HI_BITS over every lo of SPLIT_LO_BITS, rotated through the 32 positions"""
    if "rs" in _CACHE:
        return _CACHE["rs"]
    j = np.arange(32)
    blocks = []
    for i in range(77 + 3):
        hi = np.array(READER_HI_BITS, dtype=np.uint16)[(i + j) % 7]
        lo = np.array(SPLIT_LO_BITS, dtype=np.uint16)[(i // 7 + j + i) % 11]
        blocks.append(np.concatenate([hi, lo]).view(np.uint8))
    _CACHE["rs"] = np.stack(blocks)
    return _CACHE["rs"]


# ================================================================================================================ weight cases
# name -> (cout, cin, kh, kw, cout_pad, cin_pad): fp16+8 cases of the issue
MX_WEIGHT_SHAPES = {
    "k_lt_256_chunks": (6, 64, 3, 3, 32, 64),            # K / 8 = 72 chunks: one trip of the chunk loop; cout < cout_pad (zero rows, scale byte 0)
    "k_gt_256_chunks": (5, 512, 3, 3, 32, 512),          # K / 8 = 576: three trips
    "cin_inside_block": (8, 40, 3, 3, 32, 64),           # cin < cin_pad inside a block
    "one_by_one": (33, 96, 1, 1, 64, 96),                # 1x1; cout_pad two blocks
}
BIG_PLAIN_SHAPE = (2056, 2048, 1, 1)                     # > 16384 * 256 packed elements: the second grid-stride trip of pack_weights_kernel
SN_K = (40, 256, 360, 4608)
SN_SHAPES = {40: (7, 40, 1, 1, 32, 64), 256: (9, 256, 1, 1, 32, 256), 360: (5, 40, 3, 3, 32, 64), 4608: (4, 512, 3, 3, 32, 512)}


WEIGHT_PAGE_CLASSES = ("max_pow2", "e4m3_ties", "half_ties", "lo_underflow", "gaussian", "max_rounds_up", "one_nonzero", "neg_zero", "zeros", "half_max")


def weight_tensor(shape, seed):
    """fp32 OIHW weights whose rows are writer-table pages (repeated to the row length) times a power of two: 256 W = page * 2^shift exactly, shift <= 0
    bringing the row's maximum to 2^9 at most (and to 2^-10 at least) — ties stay ties.  Row 0 is the max_pow2 page: its maximum is 2^9 exactly once stored."""
    cout, cin, kh, kw = shape[:4]
    pages = [p["v"] for p in writer_pages() if p["cls"] in WEIGHT_PAGE_CLASSES]
    k = cin * kh * kw
    w = np.zeros((cout, k), dtype=np.float32)
    for o in range(cout):
        row = np.resize(np.roll(pages[0 if o == 0 else (o + seed) % len(pages)].astype(np.float64), 7 * o), k)
        m = np.abs(row).max()
        shift = min(0, 9 - int(np.ceil(np.log2(m)))) if m > 0 else 0
        if 0 < m < _p2(-10):                       # (a short row that caught only a page's small blocks: up into the range of weights)
            shift = -10 - int(np.floor(np.log2(m)))
        w[o] = row * _p2(shift - 8)
    return w.reshape(cout, cin, kh, kw)


def double_rounding_weight(scale, k, m=1023):
    """an fp32 w whose exact product with fl32(scale) lies less than half an fp32 ulp off the half tie T = 2^k (1 + (2 m + 1) / 2048), on the side of the ODD
    neighbour: fl32(w * scale) = T, which rounds to the even half, while ONE rounding of the exact product gives the odd one.  m = 1023: the even half is
    2^(k + 1), the odd one lies in the binade below — a packer that fuses the product into the conversion stores another half and, fp16+8, takes the row's
    scale from another binade.  None when no neighbour of T / scale lands in the interval."""
    f = float(np.float32(scale))
    T = _p2(k) * (1 + (2 * m + 1) / 2048.0)
    lo, hi = (T - _p2(k - 24), T) if m % 2 else (T, T + _p2(k - 24))
    w = np.float32(T / f)
    for _ in range(8):
        w = np.nextafter(w, np.float32(0))
    for _ in range(17):
        p = float(w) * f                                # 24 x 24 bits: exact in fp64
        if lo < p < hi:
            even, odd = _p2(k) * (1 + (m + (m % 2)) / 1024.0), _p2(k) * (1 + (m + 1 - (m % 2)) / 1024.0)
            assert np.float32(w) * np.float32(scale) == np.float32(T) and f16_round(np.float64(np.float32(T))) == even and f16_round(p) == odd
            return float(w)
        w = np.nextafter(w, np.float32(np.inf))
    return None


DR_SCALE = next(sc for sc in (0.3, 0.7, 0.45, 0.6, 0.35, 0.55, 0.9, 0.15, 0.8, 0.65) if double_rounding_weight(sc, 0) is not None)
DR_SHAPE = (6, 32, 1, 1, 32, 32)


def double_rounding_case():
    """weights [6, 32, 1, 1] for pack_weights(scale = DR_SCALE): the maximum of rows 0-3 is a double-rounding element below a power of two (either sign; stored
    near 2^-3, 2^2, 2^-8, 2^4 before the blocked storages' 256); row 4 holds -0.0 and tiny negative weights (a -0 product must stay -0); row 5 carries
    double-rounding elements at other ties of its binade"""
    rng = _rng(9)
    w = (rng.uniform(-0.4, 0.4, (6, 32)) * _p2(-12)).astype(np.float32)
    for o, k in enumerate((-4, 1, -9, 3)):
        x = double_rounding_weight(DR_SCALE, k)
        w[o] = (rng.uniform(-0.4, 0.4, 32) * x).astype(np.float32)
        w[o, 5 + 7 * o] = x * (-1.0 if o % 2 else 1.0)
    w[4, ::2] = -0.0
    w[4, 1::4] = -_p2(-140)
    others = [x for x in (double_rounding_weight(DR_SCALE, -2, m) for m in range(0, 1023, 7)) if x is not None]
    w[5] = np.resize(np.array(others, dtype=np.float32), 32) * np.where(np.arange(32) % 3 == 0, -1.0, 1.0)
    return w.reshape(6, 32, 1, 1), len(others)


def sn_case(K, seed=0):
    """(w, u, v, sigma fp64, margin): sigma = sum_o u[o] * sum_k w[o][k] v[k] in fp64; margin = distance of sigma from the nearest fp32 rounding boundary,
    relative to sigma (the fold takes fl32 of the fp64 sum: at >= 2^-30 any fp64 summation order gives the same fp32)"""
    shape = SN_SHAPES[K]
    cout, cin, kh, kw = shape[:4]
    for attempt in range(64):
        rng = _rng(1000 * K + seed + attempt)
        w = (rng.standard_normal((cout, cin, kh, kw)) * 0.05).astype(np.float32)
        u = rng.standard_normal(cout).astype(np.float32)
        v = rng.standard_normal(cin * kh * kw).astype(np.float32)
        u /= np.float32(np.linalg.norm(u))
        v /= np.float32(np.linalg.norm(v))
        sigma = float(np.dot(u.astype(np.float64), w.reshape(cout, -1).astype(np.float64) @ v.astype(np.float64)))
        s32 = np.float32(sigma)
        lo, hi = float(np.nextafter(s32, np.float32(-np.inf))), float(np.nextafter(s32, np.float32(np.inf)))
        margin = min(abs(sigma - (lo + float(s32)) / 2), abs(sigma - (hi + float(s32)) / 2)) / abs(sigma)
        if margin >= 2.0 ** -30 and abs(sigma) > 1e-3:
            return w, u, v, sigma, margin
    raise AssertionError("no well-separated sigma found")
