"""The operand-range contract of mnet_conv2d_nhwc (include/marconet_hip.h, "operand range") as data: a scene whose (pixel, 32-channel block) scales
span the format — fp16-subnormal blocks at the floor E = 105, E = 0 blocks, blocks 2^6 apart inside a pixel, weight rows 2^10 apart — the fp64 reference of
every kernel family written from the header's words, and a bound that judges EVERY OUTPUT ALONE.  Host only (numpy fp64, the spec codec of
tests/storage_codec.py, the host weight packer): tests/test_conv_range_table.py proves the scene, the references and the teeth of the bound on a CPU,
tests/test_conv_range_gpu.py launches every kernel build on it.

The bound.   |got - ref|(o) <= gamma * A_o + f_o + r_o
  A_o    sum of the absolute values of the terms of output o's reference sum (every product of every MFMA that feeds it)
  gamma  the relative error of an fp32 accumulation of those terms in SOME order: measured on the reference alone (`measure_gamma`: two fp32
         summation orders on the CPU against fp64, the largest |fp32 - fp64| / A_o over all live outputs, times 8 for the spread between orders),
         pinned in GAMMA, never above the derivable ceiling K * 2^-24 (K rounded adds of at most A_o each, half an ulp = 2^-24 relative apiece)
  f_o    the family's absolute floor.  None for f32, plain f16 and the fp16+8 LDS-DMA / strip / one-wave kernels (their operands enter the MFMAs as
         stored).  Split half and the register-staged fp16+8 kernel multiply f16 `lo` halves, which stop at the f16-subnormal step: one step, 2^-24,
         per element — 2^-24 * sum |W_hi| over the taps that hold a live activation, plus the mirror term 2^-24 * sum |X_hi| over live weights (both in
         the kernel's 256 W units, i.e. / 256).  It covers how a decode of a lo byte (fp16+8, register-staged) lands on that grid.
  r_o    one step of the output storage at the reference value, from the format: f16 ulp; split half: f16 ulp of the lo half; fp16+8: one e4m3 step of
         the scaled residual under the block's scale (the largest scale the block can take within the bound), 2^-24 for a block whose halves are all
         zero; 0 for f32 and for an fp32 output.  Steps are taken at |value| + (gamma A_o + f_o): what the stored neighbour of the reference can need.
  A_o == 0 (no non-zero product in the window): the output must be exactly 0.

Units: the blocked storages hold 256 W; every term below is in those units and `unit` = 1/256 brings the sum back."""
import sys

import numpy as np

from tests import storage_codec as S

BANDS = ("sub", "small", "unit", "large", "mixed", "zero")
BAND_W = 8                                   # columns per band: a 3x3 window lies wholly inside a band at columns 1 .. 6 of it
WCLASSES = ("normal", "x16", "x2m6", "zero", "single")       # by output channel, repeating
WSCALE = {"normal": 1.0, "x16": 16.0, "x2m6": 2.0 ** -6, "zero": 0.0, "single": 1.0}
ZERO_COLS = 3                                # the first columns of the zero band hold pixels whose every block is zero
IN_POW = -19                                 # in_scale = 2^-19: the unit band (binades -2 .. 1) lands in the f16-subnormal band

# name -> tests/conv_contract.py::SHAPES format: (n, h, w, c0, c1 of the two-source launches, cout, k, stride, pad, valid widths, big)
SHAPES = {
    "a": (2, 8, 48, 64, 64, 72, 1, (1, 1), 0, (), False),
    "b": (2, 8, 48, 64, 64, 72, 3, (1, 1), 1, (), False),
    "c64": (1, 128, 512, 64, 0, 64, 3, (1, 1), 1, (), True),
    "c256": (1, 128, 512, 64, 0, 256, 3, (1, 1), 1, (), True),
    "d": (2, 8, 64, 32, 0, 128, 3, (1, 1), 1, (), False),
    "a1": (1, 8, 48, 64, 64, 72, 1, (1, 1), 0, (), False),                 # a coherent image of shape a alone: 384 pixels, what the fp32 skinny kernel takes (<= 512)
}
BAND_OFFSET = {"d": 5}                      # 64 columns hold eight bands: start at the zero band, so that it comes twice (one block per pixel: half the zero blocks)
BLOCKED = ("split", "mx")
FAMILIES = ("f32", "f16", "split", "mx_dma", "mx_reg")


def cout_of(storage, sname):
    """the blocked storages carry whole 32-channel blocks: cout 72 becomes 96 there (the smallest legal map that keeps the cout tail of the tiles)"""
    c = SHAPES[sname][5]
    return -(-c // 32) * 32 if storage in BLOCKED else c


def top_binade(K):
    """largest top binade of the large band: |y| <= K * 2^-6 * 2^4 * 2^(k + 1) < 2^15 for every output (|W| < 2^-6 in a normal row, x 2^4 in the widest)"""
    k = 0
    while K * 2.0 ** -2 * 2.0 ** (k + 2) < 2.0 ** 15:          # binade k + 1 still fits
        k += 1
    return k


def band_ranges(K):
    kl = top_binade(K)
    return {"sub": (-24, -16), "small": (-14, -8), "unit": (-2, 1), "large": (kl - 3, kl), "mixed_lo": (-9, -6), "mixed_hi": (0, 3)}


def column_band(x, offset=0):
    return (x // BAND_W + offset) % len(BANDS)


def _ulp16(a):
    """the f16 step at |a| (fp64 array); 2^-24 in the subnormal range and at 0"""
    return np.ldexp(1.0, (np.maximum(S._floor_log2(np.abs(a)), -14) - 10).astype(np.int32))


def _coherent(rng, mag):
    """f16 value of mag plus a positive residual of 0.2 .. 0.45 of its ulp"""
    h = S.f16_round(mag)
    return h + rng.uniform(0.2, 0.45, mag.shape) * _ulp16(h)


def activations(h, w, C, K, seed, offset=0):
    """fp32 [2, h, w, C]: image 0 coherent (all positive), image 1 the same magnitudes under random signs; the class of a pixel's blocks follows its column"""
    rng = np.random.default_rng(seed)
    B = C // 32
    rg = band_ranges(K)
    kmap = np.zeros((h, w, B), dtype=np.int64)
    zero = np.zeros((h, w, B), dtype=bool)
    for y in range(h):
        for x in range(w):
            band = BANDS[column_band(x, offset)]
            for b in range(B):
                name = band
                if band == "mixed":
                    name = "mixed_lo" if (x + y + b) % 2 == 0 else "mixed_hi"
                if band == "zero":
                    name = "unit"
                    zero[y, x, b] = x % BAND_W < ZERO_COLS or (x + y + b) % 2 == 0
                lo, hi = rg[name]
                taken = {int(kmap[y, x - 1, b]) if x else None, int(kmap[y - 1, x, b]) if y else None, int(kmap[y, x, b - 1]) if b else None}
                free = [k for k in range(lo, hi + 1) if k not in taken] or list(range(lo, hi + 1))
                kmap[y, x, b] = free[int(rng.integers(len(free)))]
    u = rng.uniform(0.5, 1.99, (h, w, B, 32))
    top = rng.integers(0, 32, (h, w, B))
    np.put_along_axis(u, top[..., None], rng.uniform(1.0, 1.99, (h, w, B, 1)), axis=-1)
    v = _coherent(rng, np.ldexp(u, kmap[..., None].astype(np.int32)))
    signed_zero = np.where(np.arange(32) % 2 == 0, 0.0, -0.0)
    v = np.where(zero[..., None], signed_zero, v).reshape(h, w, C)
    sign = np.where(rng.integers(0, 2, v.shape) == 0, 1.0, -1.0)
    out = np.stack([v, v * sign]).astype(np.float32)
    assert (S.f16_round(out.astype(np.float64))[0] == S.f16_round(v)).all()          # the fp32 cast keeps every half
    return out


def weights(cout, cin, k, seed):
    """fp32 OIHW.  256 W = an f16 value plus a positive residual (0.2 .. 0.45 ulp) in [1, 4), times the row's power of two; the first half of the rows all
    positive, the second under random signs"""
    rng = np.random.default_rng(seed)
    K = k * k * cin
    v = _coherent(rng, 2.0 * rng.uniform(0.5, 1.99, (cout, K))).astype(np.float32).astype(np.float64)
    sign = np.where(rng.integers(0, 2, v.shape) == 0, 1.0, -1.0)
    sign[: cout // 2] = 1.0
    v = v * sign
    for o in range(cout):
        cls = WCLASSES[o % len(WCLASSES)]
        v[o] *= WSCALE[cls]
        if cls == "single":
            keep = v[o, (11 * o + 3) % K]
            v[o] = 0.0
            v[o, (11 * o + 3) % K] = keep
    w = (v / 256.0).astype(np.float32).reshape(cout, k, k, cin)
    assert (w.astype(np.float64) * 256.0 == v.reshape(w.shape)).all()
    return np.ascontiguousarray(w.transpose(0, 3, 1, 2))


_SCENES = {}


def scene(sname, two, storage="f32"):
    """{"x0", "x1" (None without a second source), "w" OIHW fp32} of a shape; x1 is drawn one band further along than x0 at every column"""
    cout = cout_of(storage, sname)
    key = (sname, two, cout)
    if key in _SCENES:
        return _SCENES[key]
    n, h, w, c0, c1, _, k, stride, pad, vws, big = SHAPES[sname]
    cin = c0 + (c1 if two else 0)
    K = k * k * cin
    seed = 7000 + 31 * list(SHAPES).index("c64" if big else sname) + (5 if two else 0)
    if big:                                  # the small scene tiled over the map; the top three rows coherent, the bottom three under random signs
        base = activations(8, 48, c0, K, seed)
        x0 = np.tile(base[0], (h // 8, w // 48 + 1, 1))[:h, :w].copy()
        x0[h - 3:] = np.tile(base[1][:3], (1, w // 48 + 1, 1))[:, :w]
        x0, x1 = x0[None], None
    else:
        x0 = activations(h, w, c0, K, seed, offset=BAND_OFFSET.get(sname, 0))[:n]
        x1 = activations(h, w, c1, K, seed + 1, offset=BAND_OFFSET.get(sname, 0) + 1)[:n] if two else None
    _SCENES[key] = {"x0": np.ascontiguousarray(x0), "x1": x1, "w": weights(cout, cin, k, seed + 2)}
    return _SCENES[key]


# ================================================================================================================ stored operands
def act_bytes(v, storage):
    """fp32 [..., C] -> the bytes the kernel reads (host encoders of the spec; fp32 as it is)"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    return v.view(np.uint8).reshape(v.shape[:-1] + (-1,)) if storage == "f32" else S.ENCODE[storage](v)


def act_parts(raw, storage):
    """bytes [..., 4 C or 2 C] -> the fp64 values of what they hold, [..., C] each: {"x"} | {"hi", "lo"} | {"hi", "lo8" (value), "E" (the block's byte)}"""
    raw = np.ascontiguousarray(raw)
    if storage == "f32":
        return {"x": raw.view(np.float32).astype(np.float64)}
    if storage == "f16":
        return {"x": S.f16_value(raw.view(np.uint16))}
    b = raw.reshape(raw.shape[:-1] + (raw.shape[-1] // 128, 128))
    flat = lambda t: t.reshape(raw.shape[:-1] + (-1,))
    hi = S.f16_value(np.ascontiguousarray(b[..., 0:64]).view(np.uint16))
    if storage == "split":
        return {"hi": flat(hi), "lo": flat(S.f16_value(np.ascontiguousarray(b[..., 64:128]).view(np.uint16)))}
    E = b[..., 96:97].astype(np.int64)
    lo8 = S.E4M3_VALUE[b[..., 64:96]][..., S.INV_PERM] * np.where(E >= 12, np.ldexp(1.0, (np.maximum(E, 12) - 138).astype(np.int32)), 0.0)
    return {"hi": flat(hi), "lo8": flat(lo8), "E": flat(np.broadcast_to(E, hi.shape))}


def stored_value(raw, storage):
    """the exact value of stored elements (fp64; the sum of the parts is exact there)"""
    p = act_parts(raw, storage)
    return p["x"] if "x" in p else p["hi"] + (p["lo"] if "lo" in p else p["lo8"])


def weight_bytes(w_oihw, storage):
    """the packed tensor of the host packer (marconet_amd.packing.pack_conv_weight, CPU path), as a torch tensor"""
    import torch
    from marconet_amd import packing
    dt = {"f32": torch.float32, "f16": torch.float16, "split": packing.SPLIT_DTYPE, "mx": packing.MX_DTYPE}[storage]
    return packing.pack_conv_weight(torch.from_numpy(np.ascontiguousarray(w_oihw)), dt)


def weight_parts(packed, storage, cout, kh, kw, cin):
    """packed tensor -> fp64 [cout, K] matrices (K = kh kw cin, tap-major): {"w"} | {"hi", "lo"} of 256 W | {"hi", "lo8", "hi8" (values), "E" [cout]}"""
    import torch
    from marconet_amd import packing
    raw = packing.untag(packed).contiguous().view(-1).view(torch.uint8).numpy()
    K = kh * kw * cin
    if storage in ("f32", "f16"):
        return {"w": act_parts(raw, storage)["x"].reshape(cout, K)}
    if storage == "split":
        p = act_parts(raw.reshape(cout * kh * kw, cin * 4), "split")
        return {"hi": p["hi"].reshape(cout, K), "lo": p["lo"].reshape(cout, K)}
    rows = raw[: cout * K * 4].reshape(cout, kh * kw * cin // 32, 128)
    E = raw[cout * K * 4: cout * K * 4 + cout].astype(np.int64) + 11
    hi = S.f16_value(np.ascontiguousarray(rows[..., 0:64]).view(np.uint16))
    lo8, hi8 = np.zeros(hi.shape), np.zeros(hi.shape)
    p0, p1 = S.PERM[:16], S.PERM[16:]
    lo8[..., p0], hi8[..., p0] = S.E4M3_VALUE[rows[..., 64:80]], S.E4M3_VALUE[rows[..., 80:96]]
    lo8[..., p1], hi8[..., p1] = S.E4M3_VALUE[rows[..., 96:112]], S.E4M3_VALUE[rows[..., 112:128]]
    s = np.ldexp(1.0, (E - 127).astype(np.int32))[:, None, None]
    return {"hi": hi.reshape(cout, K), "lo8": (lo8 * s * 2.0 ** -11).reshape(cout, K), "hi8": (hi8 * s).reshape(cout, K), "E": E}


def x_hi8(hi, E):
    """what the LDS-DMA kernels derive in-kernel: e4m3(hi / s_x) * s_x, round to nearest even, s_x = 2^(E - 127); 0 in an E = 0 block"""
    sc = np.ldexp(1.0, (127 - np.maximum(E, 1)).astype(np.int32))
    return np.where(E > 0, S.E4M3_VALUE[S.e4m3_bits(hi * sc)] / sc, 0.0)


# ================================================================================================================ the reference of one launch
def patches(a, k, pad, rows=None, fill=0.0):
    """[n, h, w, C] -> [n, len(rows), wo, k k C] (tap-major, channel-minor: the order of a weight row), stride 1"""
    n, h, w, C = a.shape
    ho, wo = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    rows = list(range(ho)) if rows is None else rows
    ap = np.full((n, h + 2 * pad, w + 2 * pad, C), fill, dtype=a.dtype)
    ap[:, pad:pad + h, pad:pad + w] = a
    out = np.empty((n, len(rows), wo, k * k, C), dtype=a.dtype)
    for r in range(k):
        for s in range(k):
            out[:, :, :, r * k + s] = ap[:, [y + r for y in rows], s:s + wo]
    return out.reshape(n, len(rows), wo, k * k * C)


def ref_rows(sname):
    n, h, w, c0, c1, cout, k, stride, pad, vws, big = SHAPES[sname]
    ho = h + 2 * pad - k + 1
    return [0, 1, ho - 2, ho - 1] if big else list(range(ho))


def _split_of(v):
    hi = S.f16_round(v)
    return hi, S.f16_round(v - hi)


class Case:
    """one launch on the scene: storage, shape, second source ("none" | "concat" | "center"), kernel family, optionally in_scale = 2^IN_POW.
    Holds the stored bytes (`raw0`, `raw1`, `wpacked`) and the family's reference: `terms` = [(X [P, K], W [cout, K])] in the kernel's units."""

    def __init__(self, storage, sname, src2="none", family=None, in_scale=False):
        self.storage, self.sname, self.src2, self.in_scale = storage, sname, src2, in_scale
        self.family = family or {"mx": "mx_dma"}.get(storage, storage)
        n, h, w, c0, c1, _, k, stride, pad, vws, big = SHAPES[sname]
        two = src2 != "none"
        sc = scene(sname, two, storage)
        self.cout, self.k, self.pad, self.c0, self.cin = cout_of(storage, sname), k, pad, c0, c0 + (c1 if two else 0)
        self.K = k * k * self.cin
        self.rows = ref_rows(sname)
        self.raw0 = act_bytes(sc["x0"], storage)
        self.raw1 = act_bytes(sc["x1"], storage) if two else None
        self.wpacked = weight_bytes(sc["w"], storage)
        self.w_true = sc["w"]
        xp = [act_parts(r, storage) for r in ((self.raw0, self.raw1) if two else (self.raw0,))]
        self.xparts = {kk: np.concatenate([p[kk] for p in xp], axis=-1) for kk in xp[0]}
        self.wparts = weight_parts(self.wpacked, storage, self.cout, k, k, self.cin)
        if src2 == "center":                     # x1 enters at the centre tap only
            m = np.ones((k * k, self.cin))
            m[:, c0:] = 0.0
            m[(k // 2) * k + k // 2, c0:] = 1.0
            self.wparts = {kk: (v * m.reshape(1, -1) if v.ndim == 2 else v) for kk, v in self.wparts.items()}
        self.shape_out = (self.xparts[next(iter(self.xparts))].shape[0], len(self.rows), w + 2 * pad - k + 1, self.cout)
        self.unit = 1.0 / 256.0 if storage in BLOCKED else 1.0
        self._e32 = {}
        self._build_terms()
        if big:                                  # (the parts of a big map are only needed for its terms)
            self.xparts = None

    def P(self, a, fill=0.0):
        """[n, h, w, C] -> the windows of the reference rows, [P, K]"""
        a = patches(a, self.k, self.pad, self.rows, fill)
        return a.reshape(-1, a.shape[-1])

    def _build_terms(self):
        x, w, fam = self.xparts, self.wparts, self.family
        if self.in_scale:                        # X' = fl32(decoded X * 2^IN_POW), staged in the storage's own form (the split-half sequence for both blocked types)
            v = x["x"] if "x" in x else x["hi"] + (x["lo"] if "lo" in x else S.f16_round(x["lo8"]))
            v = (v.astype(np.float32) * np.float32(2.0 ** IN_POW)).astype(np.float64)
            x = {"x": v} if self.storage == "f32" else {"x": S.f16_round(v)} if self.storage == "f16" else dict(zip(("hi", "lo"), _split_of(v)))
            if fam.startswith("mx"):
                fam = "mx_reg"
        if fam in ("f32", "f16"):
            self.terms = [(self.P(x["x"]), w["w"])]
            self.x_hi = self.w_hi = None
        elif fam == "split" or fam == "mx_reg":
            xl = x["lo"] if "lo" in x else S.f16_round(x["lo8"])         # the register-staged fp16+8 kernel decodes lo bytes to halves
            wl = w["lo"] if "lo" in w else S.f16_round(w["lo8"])
            xh, xl = self.P(x["hi"]), self.P(xl)
            self.terms = [(xh, w["hi"]), (xl, w["hi"]), (xh, wl)]
            self.x_hi, self.w_hi, self.x_live, self.w_live = xh, w["hi"], (xh != 0) | (xl != 0), (w["hi"] != 0) | (wl != 0)
        else:                                    # fp16+8 LDS-DMA / strip / one-wave: hi*hi on the f16 MFMA + (w_hi8*x_lo8 + w_lo8*x_hi8) on the scaled fp8 MFMA
            self.terms = [(self.P(x["hi"]), w["hi"]), (self.P(x["lo8"]), w["hi8"]), (self.P(x_hi8(x["hi"], x["E"])), w["lo8"])]
            self.x_hi = self.w_hi = None
        self.fam = fam

    # ---- reference, A_o, bound
    def ref(self):
        if not hasattr(self, "_ref"):
            self._ref = sum(X @ W.T for X, W in self.terms) * self.unit
            self._A = sum(np.abs(X) @ np.abs(W).T for X, W in self.terms) * self.unit
        return self._ref

    def A(self):
        self.ref()
        return self._A

    def floor(self):
        if self.x_hi is None:
            return 0.0
        return 2.0 ** -24 * (self.x_live.astype(np.float64) @ np.abs(self.w_hi).T + np.abs(self.x_hi) @ self.w_live.astype(np.float64).T) * self.unit

    def gamma(self):
        return ceiling(self.K) if self.fam in CEILING_FAMILIES else GAMMA[(self.fam, self.K)]

    def out_step(self, pre, out_f32=False):
        ref = self.ref()
        if self.storage == "f32" or out_f32:
            return np.zeros_like(ref)
        a = np.abs(ref) + pre
        if self.storage == "f16":
            r = _ulp16(a)
        elif self.storage == "split":
            r = _ulp16(np.abs(ref - S.f16_round(ref)) + pre)
        else:
            blk = S.f16_round(a).reshape(a.shape[0], -1, 32)
            E = np.broadcast_to(S.block_exponent(blk), blk.shape).reshape(a.shape)
            t = (np.abs(ref - S.f16_round(ref)) + pre) * np.ldexp(1.0, (138 - np.maximum(E, 1)).astype(np.int32))
            step = np.ldexp(1.0, (np.maximum(S._floor_log2(t), -6) - 3).astype(np.int32))
            r = np.where(E > 0, step * np.ldexp(1.0, (np.maximum(E, 1) - 138).astype(np.int32)), 2.0 ** -24)
        return np.where(self.A() == 0, 0.0, r)

    def bound(self, out_f32=False, gamma=None):
        pre = (self.gamma() if gamma is None else gamma) * self.A() + self.floor()
        return pre + self.out_step(pre, out_f32)

    # ---- fp32 re-evaluations of the reference: one accumulator, two association orders
    def eval32(self, order):
        if order in self._e32:
            return self._e32[order]
        P, cout = self.ref().shape
        acc = np.zeros((P, cout), dtype=np.float32)
        T = [(X.astype(np.float32), W.astype(np.float32)) for X, W in self.terms]      # (exact: every part is an fp32 value)

        def chunk(X, W, k0, n, adjacent):
            """fp32 sum of n products by a binary tree (numpy's elementwise multiply and add: every step rounded once, no contraction)"""
            p = X[:, None, k0:k0 + n] * W[None, :, k0:k0 + n]
            while p.shape[-1] > 1:
                h = p.shape[-1] // 2
                p = p[..., 0::2] + p[..., 1::2] if adjacent else p[..., :h] + p[..., h:]
            return p[..., 0]

        if order == 0:                           # the shape of an MFMA k-loop: 16 products per step, the three products of a step next to each other, k ascending
            for k0 in range(0, self.K, 16):
                for X, W in T:
                    acc += chunk(X, W, k0, 16, True)
        else:                                    # one product after the other, steps of 8 with the other pairing, k descending
            for X, W in reversed(T):
                for k0 in reversed(range(0, self.K, 8)):
                    acc += chunk(X, W, k0, 8, False)
        self._e32[order] = acc.astype(np.float64) * self.unit
        return self._e32[order]

    # ---- classes of an output
    def out_bands(self):
        """band index of every output's column, or -1 where its window crosses a band edge; [P]"""
        n, rows, wo, _ = self.shape_out
        x = np.arange(wo)
        inside = np.ones(wo, dtype=bool) if self.k == 1 else (x % BAND_W >= 1) & (x % BAND_W <= BAND_W - 2)
        b = np.where(inside, column_band(x, BAND_OFFSET.get(self.sname, 0)), -1)
        return np.broadcast_to(b[None, None, :], (n, rows, wo)).reshape(-1)

    def out_images(self):
        """image of every output: 0 coherent, 1 random signs (the big maps: the top rows coherent, the bottom rows random); [P]"""
        n, rows, wo, _ = self.shape_out
        if SHAPES[self.sname][-1]:
            img = np.array([0, 0, 1, 1])[None, :, None]
        else:
            img = np.arange(n)[:, None, None]
        return np.broadcast_to(img, (n, rows, wo)).reshape(-1)

    def row_classes(self):
        return np.arange(self.cout) % len(WCLASSES)

    # ---- mutants: what a subtly wrong kernel would compute (fp64)
    def mutant(self, name):
        t = self.terms
        mm = lambda i, X=None, W=None: (t[i][0] if X is None else X) @ (t[i][1] if W is None else W).T
        sub = lambda X: np.where(np.abs(X) < 2.0 ** -14, 0.0, X)
        if self.fam == "mx_dma":
            x = self.xparts
            E = self.P(x["E"].astype(np.float64))
            if name == "drop_fp8":
                v = mm(0)
            elif name == "xlo8_x2":
                v = mm(0) + 2 * mm(1) + mm(2)
            elif name == "wlo8_x2":
                v = mm(0) + mm(1) + 2 * mm(2)
            elif name == "drop_xlo8":
                v = mm(0) + mm(2)
            elif name == "flush_hi8":
                v = mm(0) + mm(1) + mm(2, X=self.P(x_hi8(sub(x["hi"]), x["E"])))
            elif name == "flush_f16":
                v = mm(0, X=sub(t[0][0])) + mm(1) + mm(2)
            elif name in ("other_block_scale", "next_pixel_scale"):
                Eb = x["E"].reshape(x["E"].shape[:-1] + (-1, 32))
                if name == "other_block_scale":   # the scale byte of the pixel's next block (of the same source)
                    c0b = self.c0 // 32
                    E2 = np.concatenate([np.roll(Eb[..., :c0b, :], -1, axis=-2), np.roll(Eb[..., c0b:, :], -1, axis=-2)], axis=-2).reshape(x["E"].shape)
                else:
                    E2 = np.roll(x["E"], -1, axis=2)
                f = np.ldexp(1.0, (self.P(E2.astype(np.float64)) - E).astype(np.int32))
                v = mm(0) + mm(1, X=t[1][0] * f) + mm(2, X=t[2][0] * f)
            elif name == "next_row_wscale":
                Ew = self.wparts["E"]
                v = mm(0) + (mm(1) + mm(2)) * np.ldexp(1.0, (np.roll(Ew, -1) - Ew).astype(np.int32))[None, :]
            else:
                raise KeyError(name)
        else:
            if name == "drop_hi_lo":
                v = mm(0) + mm(1)
            elif name == "drop_lo_hi":
                v = mm(0) + mm(2)
            elif name == "flush_lo":
                v = mm(0) + mm(1, X=sub(t[1][0])) + mm(2, W=sub(t[2][1]))
            else:
                raise KeyError(name)
        return v * self.unit


_CASES = {}


def case(storage, sname, src2="none", family=None, in_scale=False):
    family = family or {"mx": "mx_dma"}.get(storage, storage)
    key = (storage, sname, src2, family, in_scale)
    if key not in _CASES:
        _CASES[key] = Case(storage, sname, src2, family, in_scale)
    return _CASES[key]


# mutant -> the classes in which it must show: activation bands, or weight-row classes
_NORMAL = ("small", "unit", "large", "mixed")
MX_MUTANTS = {
    "drop_fp8": _NORMAL, "xlo8_x2": _NORMAL, "wlo8_x2": _NORMAL, "drop_xlo8": _NORMAL,
    "flush_hi8": ("sub",), "flush_f16": ("sub",),
    "other_block_scale": _NORMAL, "next_pixel_scale": _NORMAL,
    "next_row_wscale": ("w:x16", "w:x2m6"),
}
SPLIT_MUTANTS = {"drop_hi_lo": _NORMAL, "drop_lo_hi": _NORMAL, "flush_lo": ("small",)}


def ceiling(K):
    return K * 2.0 ** -24


# ================================================================================================================ gamma
# the launches gamma is measured on, per family: every K of the GPU tier (shape, second source)
GAMMA_CASES = (("a", "none"), ("a", "concat"), ("d", "none"), ("b", "none"), ("b", "concat"), ("c64", "none"))
_STORAGE_OF = {"f32": "f32", "f16": "f16", "split": "split", "mx_dma": "mx", "mx_reg": "mx"}


def measure_gamma(families=FAMILIES, cases=GAMMA_CASES):
    """{(family, K): 8 * max over the outputs with A_o > 0, both orders and every measured launch of that K of |fp32 - fp64| / A_o}"""
    out = {}
    for fam in families:
        for sname, src2 in cases:
            if sname == "d" and not fam.startswith("mx"):
                continue
            c = case(_STORAGE_OF[fam], sname, src2, family=fam)
            live = c.A() > 0
            worst = max(float((np.abs(c.eval32(o) - c.ref())[live] / c.A()[live]).max()) for o in (0, 1))
            out[(fam, c.K)] = max(out.get((fam, c.K), 0.0), 8.0 * worst)
    return out


# python -m tests.conv_range        (prints this table; tests/test_conv_range_table.py recomputes it and compares)
# families whose kernels exceeded the measured gamma in the unit band on the MI355X and fall back to the ceiling K * 2^-24 (header, "operand range")
CEILING_FAMILIES = ()
GAMMA = {
    ("f16", 64): 1.5880392611291756e-06, ("f16", 128): 2.9151239940362626e-06, ("f16", 576): 3.9933067436178495e-06, ("f16", 1152): 5.489174802793728e-06,
    ("f32", 64): 1.984461780511724e-06, ("f32", 128): 2.932564443710739e-06, ("f32", 576): 4.142572164342294e-06, ("f32", 1152): 5.878190510743361e-06,
    ("mx_dma", 64): 2.1171152772179635e-06, ("mx_dma", 128): 2.941272026453679e-06, ("mx_dma", 288): 4.967407620972983e-06,
    ("mx_dma", 576): 5.889227320557222e-06, ("mx_dma", 1152): 6.935290024860511e-06,
    ("mx_reg", 64): 2.284967418173033e-06, ("mx_reg", 128): 2.989210501399099e-06, ("mx_reg", 288): 5.02959858093302e-06,
    ("mx_reg", 576): 6.705912138465976e-06, ("mx_reg", 1152): 7.227594434474934e-06,
    ("split", 64): 2.2377585423777345e-06, ("split", 128): 2.937819816383996e-06, ("split", 576): 6.220220869939643e-06, ("split", 1152): 7.805378802130299e-06,
}


if __name__ == "__main__":
    g = measure_gamma()
    print("GAMMA = {")
    for key in sorted(g):
        print("    %r: %r,        # %.3f of the ceiling K * 2^-24" % (key, g[key], g[key] / ceiling(key[1])))
    print("}")
    sys.exit(0)
