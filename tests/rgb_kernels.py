"""The two RGB output kernels of marconet_amd/csrc/aux_kernels.hip — mnet_torgb and mnet_conv3x3_rgb — as data: pure-Python mirrors of their host launch
arithmetic, fp64 references written out from the formulas of include/marconet_hip.h, the case tables of tests/test_rgb_kernels_gpu.py with the launch regime every
case is there for, and seeded inputs.  No device needed: the CPU tier (tests/test_rgb_kernels.py) checks that every case lands in the regime it names, that the
references agree with F.conv2d / F.interpolate, that tanh is kept out of saturation and that the references tell a wrong kernel from a right one; the GPU tier
asserts the regime again before it launches.

The launch formulas are COPIED from the sources (the line each one mirrors is named next to it); when one of those lines changes, change its mirror here and
re-derive the shapes below.  The references work on the STORED operands: x goes through the host packers of marconet_amd/packing.py / mxfmt.py and is decoded by
them, never by the device converter."""
import os
import re
import zlib

import numpy as np

F32, F16, SPLIT, MX = "fp32", "f16", "split", "mx"
STORAGES = (F32, F16, SPLIT, MX)
WG = 256
ACT_NONE, ACT_LRELU, ACT_TANH = 0, 2, 4            # include/marconet_hip.h: MNET_ACT_NONE, MNET_ACT_LRELU, MNET_ACT_TANH
BOUND = 2e-5                                        # |got - ref64| <= BOUND * (A + 1) per output element (the project's fp32-kernel bound, on the sum of magnitudes)
F16_EPS = 2.0 ** -11                                # one f16 rounding of conv3x3_rgb's f16 NHWC output: + F16_EPS * |ref|


def _cdiv(a, b):
    return (a + b - 1) // b


def _torgb_u():
    """the #define MNET_TORGB_U line of aux_kernels.hip (read, not copied)"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marconet_amd", "csrc", "aux_kernels.hip")
    with open(src) as f:
        return int(re.search(r"#define MNET_TORGB_U (\d+)", f.read()).group(1))


U = _torgb_u()
TORGB_TRIPS = 4               # mnet_torgb: `e && atoi(e) > 0 ? atoi(e) : 4` (MNET_TORGB_TRIPS unset)
TORGB_CAP = 1024              # mnet_torgb: `const int gx = (int)(wgs < 1024 ? wgs : 1024);`
TORGB_C = (64, 128, 256, 512)


# ================================================================================================================ launch mirrors
def torgb_launch(h, w, c):
    """-> (cpp, ppb, groups, gx, step, loop_trips) of mnet_torgb.
    cpp, ppb: torgb_kernel `const int cpp = C >> 3;` and `ppb = 256 / cpp` (lanes per pixel, pixel lanes per workgroup);
    groups: mnet_torgb `(((long long)h * w + (256 / (c / 8)) - 1) / (256 / (c / 8)) + MNET_TORGB_U - 1) / MNET_TORGB_U`;
    gx: `wgs = (groups + trips - 1) / trips` and the cap line, grid (gx, n); step: torgb_kernel `const int step = gridDim.x * ppb;`;
    loop_trips: the trips of workgroup 0's pixel lane 0 through `for (int pix0 = blockIdx.x * ppb + pl; pix0 < HW; pix0 += U * step)` — the most any lane makes"""
    cpp = c // 8
    ppb = WG // cpp
    hw = h * w
    groups = _cdiv(_cdiv(hw, ppb), U)
    gx = min(_cdiv(groups, TORGB_TRIPS), TORGB_CAP)
    step = gx * ppb
    return cpp, ppb, groups, gx, step, _cdiv(hw, U * step)


def torgb_walk(h, w, c):
    """the loop of torgb_kernel walked for every pixel lane: {(bx, pl): [live u of trip 0, of trip 1, ...]} — live u: the u < U with `pix0 + u * step < HW`
    (torgb_kernel: `if (pix >= HW) continue;`; the load of a dead u is clamped to pix0).  A lane that never enters the loop has []."""
    cpp, ppb, groups, gx, step, _ = torgb_launch(h, w, c)
    hw = h * w
    out = {}
    for bx in range(gx):
        for pl in range(ppb):
            out[bx, pl] = [sum(1 for u in range(U) if pix0 + u * step < hw) for pix0 in range(bx * ppb + pl, hw, U * step)]
    return out


def torgb_regime(h, w, c):
    """the predicates of a ToRGB launch over its arithmetic:
    idle_pixel_lanes  hw % ppb != 0: the last workgroup-row of pixels leaves pixel lanes without a pixel;
    ragged_u          some live pix0 has a dead u (pix0 + u * step >= hw): the clamped load and the `pix >= HW` exit of the tail lanes;
    capped            groups / 4 > 1024: the gx cap binds, so a lane makes more than four trips;
    trips             the set of trip counts over the pixel lanes that enter the loop;
    uneven_exit_in_wave  a wave holds pixel lanes (64 / cpp of them; one when C = 512) that leave the loop at different trips;
    uneven_u_in_wave     a wave holds pixel lanes with different numbers of live u in the same trip;
    covered           every pixel is written exactly once (a check of this mirror and of the launch arithmetic, not of the kernel)"""
    cpp, ppb, groups, gx, step, loop_trips = torgb_launch(h, w, c)
    hw = h * w
    walk = torgb_walk(h, w, c)
    per_wave = max(1, 64 // cpp)
    uneven_exit = uneven_u = False
    for bx in range(gx):
        for w0 in range(0, ppb, per_wave):
            lanes = [walk[bx, pl] for pl in range(w0, min(w0 + per_wave, ppb))]
            uneven_exit |= len({len(v) for v in lanes}) > 1
            for t in range(max(len(v) for v in lanes)):
                uneven_u |= len({v[t] for v in lanes if len(v) > t}) > 1
    seen = np.zeros(hw, dtype=np.int64)
    for bx in range(gx):
        for pl in range(ppb):
            for pix0 in range(bx * ppb + pl, hw, U * step):
                for u in range(U):
                    if pix0 + u * step < hw:
                        seen[pix0 + u * step] += 1
    return {"idle_pixel_lanes": hw % ppb != 0,
            "ragged_u": any(live < U for v in walk.values() for live in v),
            "capped": groups > TORGB_TRIPS * TORGB_CAP,
            "trips": {len(v) for v in walk.values() if v},
            "uneven_exit_in_wave": uneven_exit, "uneven_u_in_wave": uneven_u,
            "covered": bool((seen == 1).all())}


RGB_TH, RGB_TW = 8, 32        # conv3x3_rgb_kernel: `constexpr int TH = 8, TW = 32`


def rgb_launch(h, w):
    """-> (tiles_y, tiles_x, last_rows, last_cols) of mnet_conv3x3_rgb: `const int tiles = ((h + 7) / 8) * ((w + 31) / 32);`, grid (tiles, n);
    rows / columns of the last tile row / column that are inside the image (conv3x3_rgb_kernel: `if (oy >= H || ox >= W) return;`)"""
    ty, tx = _cdiv(h, RGB_TH), _cdiv(w, RGB_TW)
    return ty, tx, h - (ty - 1) * RGB_TH, w - (tx - 1) * RGB_TW


def rgb_instantiation(storage):
    """the conv3x3_rgb_kernel instantiation a storage resolves to (mnet_conv3x3_rgb's dispatch), and the trips of its `for (int half ...)` loop"""
    return {F16: ("<f16, 64>", 1), F32: ("<float, 64, false, hs>", 1), SPLIT: ("<float, 64, true, hs>", 2), MX: ("<float, 64, true, hm>", 2)}[storage]


# ================================================================================================================ fp64 references
def up2_axis(size, swap=False, shift=0):
    """bilinear x2, align_corners=False, along one axis of ``size`` source samples, from the definition: output i samples the source at (i + 0.5) / 2 - 0.5,
    clamped at 0; taps floor(src) and floor(src) + 1, the latter clamped at size - 1 -> (tap a, tap b, weight of a, weight of b): weights 0.25 / 0.75 inside,
    1 / 0 at the clamped first sample.  ``swap`` exchanges the two weights, ``shift`` moves tap b by that many samples (clamped): the perturbations of the CPU tier"""
    i = np.arange(2 * size)
    src = np.maximum((i + 0.5) / 2.0 - 0.5, 0.0)
    a = np.floor(src).astype(np.int64)
    fb = src - a
    b = np.clip(a + 1 + shift, 0, size - 1)
    fa = 1.0 - fb
    return (a, b, fb, fa) if swap else (a, b, fa, fb)


def up2(img, swap=False, shift=0):
    """img fp64 [n, h2, w2, k] -> [n, 2 h2, 2 w2, k]"""
    ya, yb, wya, wyb = up2_axis(img.shape[1], swap, 0)
    xa, xb, wxa, wxb = up2_axis(img.shape[2], swap, shift)
    rows = lambda r: img[:, r][:, :, xa] * wxa[None, None, :, None] + img[:, r][:, :, xb] * wxb[None, None, :, None]
    return rows(ya) * wya[None, :, None, None] + rows(yb) * wyb[None, :, None, None]


def torgb_ref(x, wgt, style, scale_b, bias, skip, swap=False, shift=0):
    """out = tanh(sb * sum_c w * (x * s) + bias + up2(skip)) in fp64.  x [n,h,w,c] (the stored values), wgt [3,c], style [n,c], scale_b [n] or None (1),
    bias [>=3], skip [n,h/2,w/2,4] or None -> (ref [n,h,w,3], pre-activation, A [n,h,w,3]) with A = |sb| * sum |w x s| + |bias| + sum_taps |weight * skip|"""
    x, wgt, style, bias = (np.asarray(v, dtype=np.float64) for v in (x, wgt, style, bias))
    n = x.shape[0]
    sb = np.ones(n) if scale_b is None else np.asarray(scale_b, dtype=np.float64).reshape(n)
    xs = x * style[:, None, None, :]
    pre = (xs @ wgt.T) * sb[:, None, None, None] + bias[:3]
    mag = (np.abs(xs) @ np.abs(wgt).T) * np.abs(sb)[:, None, None, None] + np.abs(bias[:3])
    if skip is not None:
        skip = np.asarray(skip, dtype=np.float64)
        pre = pre + up2(skip, swap, shift)[..., :3]
        mag = mag + up2(np.abs(skip))[..., :3]
    return np.tanh(pre), pre, mag


def conv_rgb_ref(x, wgt, bias, act, tap_shift=None):
    """act(sum w x + bias) in fp64 with explicit zero padding.  x [n,h,w,cin]; wgt [3,3,3,cin] (cout, ky, kx, cin); bias [3]; act ACT_NONE / ACT_TANH
    -> (ref [n,h,w,3], pre-activation, A = sum |w x| + |bias|).  ``tap_shift`` (ky, kx): that tap reads one pixel further right (a CPU-tier perturbation)"""
    x, wgt, bias = (np.asarray(v, dtype=np.float64) for v in (x, wgt, bias))
    n, h, w, cin = x.shape
    xp = np.zeros((n, h + 2, w + 3, cin))
    xp[:, 1:h + 1, 1:w + 1] = x
    pre = np.zeros((n, h, w, 3)) + bias[:3]
    mag = np.zeros((n, h, w, 3)) + np.abs(bias[:3])
    for ky in range(3):
        for kx in range(3):
            dx = kx + (1 if tap_shift == (ky, kx) else 0)
            win = xp[:, ky:ky + h, dx:dx + w]
            pre += win @ wgt[:, ky, kx].T
            mag += np.abs(win) @ np.abs(wgt[:, ky, kx]).T
    assert act in (ACT_NONE, ACT_TANH)
    return (np.tanh(pre) if act == ACT_TANH else pre), pre, mag


# ================================================================================================================ storage
def store(x32, storage):
    """fp32 numpy [..., C] -> (the host tensor in ``storage`` as the kernel gets it, the values it holds as fp64 numpy): the HOST packers only"""
    import torch
    from marconet_amd import packing
    t = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32))
    if storage == F32:
        return t, x32.astype(np.float64)
    s = packing.from_float(t, {F16: torch.float16, SPLIT: packing.SPLIT_DTYPE, MX: packing.MX_DTYPE}[storage])
    return s, packing.to_float(s).double().numpy()


def block_magnitudes(c):
    """per channel: the magnitude of its 32-channel block — 2^-6, 1, 2^5, repeating.  x is multiplied by it and the weights are divided by it, so every block
    contributes comparably and a misread block exponent or a swapped half moves the result"""
    return np.repeat(np.array([2.0 ** -6, 1.0, 2.0 ** 5])[np.arange(c // 32) % 3], 32)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


SCALE_B = np.array([1.3, -0.7, 0.9], dtype=np.float32)          # n = 3: one negative; mean square 1


def torgb_inputs(c, h, w, n=3):
    """seeded fp32 operands of a ToRGB case (x not yet stored).  Pre-activation: the modulated sum has variance c * g^2 * E[s^2] * E[sb^2] with
    E[s^2] = E[(|z| + 0.5)^2] = 2.048 and E[sb^2] = 1; g makes its standard deviation 0.4; bias 0.2 and a skip of 0.3 bring the whole to about 0.5.
    The skip's channel 3 holds values of the order 1e4: the kernel must neither add them in nor write them out"""
    r = _rng("torgb", c, h, w, n)
    mag = block_magnitudes(c)
    g = 0.4 / np.sqrt(2.048 * c)
    d = {"x": (r.standard_normal((n, h, w, c)) * mag).astype(np.float32),
         "wgt": (r.standard_normal((3, c)) * g / mag).astype(np.float32),
         "style": (np.abs(r.standard_normal((n, c))) + 0.5).astype(np.float32),
         "scale_b": SCALE_B[np.arange(n) % 3].copy(),
         "bias": np.concatenate([r.standard_normal(3) * 0.2, [0.0]]).astype(np.float32),
         "skip": None}
    if h % 2 == 0 and w % 2 == 0:
        skip = r.standard_normal((n, h // 2, w // 2, 4)) * 0.3
        skip[..., 3] = (np.abs(r.standard_normal((n, h // 2, w // 2))) + 1.0) * 1e4 * np.where(r.random((n, h // 2, w // 2)) < 0.5, -1.0, 1.0)
        d["skip"] = skip.astype(np.float32)
    return d


def conv_rgb_inputs(n, h, w, storage):
    """seeded operands of a conv3x3_rgb case: x fp32 (not yet stored), wgt [3,3,3,64] ROUNDED to what the kernel is given (f16 for an f16 x, fp32 otherwise) as
    fp32 numpy, bias.  576 products of variance g^2 give an interior pre-activation a standard deviation of 0.5 (less at the halo)"""
    r = _rng("conv3x3_rgb", n, h, w)
    mag = block_magnitudes(64)
    wgt = (r.standard_normal((3, 3, 3, 64)) * (0.5 / 24.0) / mag).astype(np.float32)
    if storage == F16:
        wgt = wgt.astype(np.float16).astype(np.float32)
    return {"x": (r.standard_normal((n, h, w, 64)) * mag).astype(np.float32), "wgt": wgt, "bias": (r.standard_normal(3) * 0.1).astype(np.float32)}


# ================================================================================================================ case tables
# Every case: (regime name, shape).  The shapes are the smallest that reach the regime; ppb = 2048 / C pixel lanes per workgroup.
def torgb_cases(c):
    ppb = 2048 // c
    return [("fewer pixels than pixel lanes", (2, 2)),            # C = 512: as many (4 = ppb); the strict case there is the 1 x 3 map below
            ("fewer pixels than pixel lanes, no skip", (1, 3)),
            ("odd map, no skip", (3, 5)),
            ("exactly one full trip of one workgroup", (2, 2 * ppb)),
            ("mixed tails", (6, 10)),
            ("two trips", (2, 3 * ppb)),
            ("three trips", (2, 5 * ppb)),
            ("one pixel into the second trip, no skip", (1, 4 * ppb + 1)),
            ("tails differ inside a wave, no skip", (1, ppb + 3)),
            ("four workgroups x four trips, no ragged u", (8, 8 * ppb)),
            ("five workgroups, four trips, ragged u", (10, 8 * ppb - 2))]


def _tl(p, c):
    return dict(zip(("cpp", "ppb", "groups", "gx", "step", "loop_trips"), torgb_launch(p[0], p[1], c)))


def _tr(p, c):
    return torgb_regime(p[0], p[1], c)


TORGB_REGIME = {
    "fewer pixels than pixel lanes": lambda p, c: (p[0] * p[1] <= _tl(p, c)["ppb"] and _tl(p, c)["gx"] == 1 and _tr(p, c)["trips"] == {1} and _tr(p, c)["ragged_u"]
                                                   and (_tr(p, c)["idle_pixel_lanes"] or c == 512) and p[0] % 2 == 0 and p[1] % 2 == 0),
    "fewer pixels than pixel lanes, no skip": lambda p, c: p[0] * p[1] < _tl(p, c)["ppb"] and _tr(p, c)["idle_pixel_lanes"] and _tr(p, c)["trips"] == {1},
    "odd map, no skip": lambda p, c: p[0] % 2 == 1 and p[1] % 2 == 1 and _tr(p, c)["ragged_u"],
    "exactly one full trip of one workgroup": lambda p, c: (p[0] * p[1] == U * _tl(p, c)["ppb"] and _tl(p, c)["gx"] == 1 and _tr(p, c)["trips"] == {1}
                                                            and not _tr(p, c)["ragged_u"] and not _tr(p, c)["idle_pixel_lanes"]),
    "mixed tails": lambda p, c: _tl(p, c)["gx"] == 1 and _tr(p, c)["ragged_u"] and p[0] % 2 == 0 and p[1] % 2 == 0,
    "two trips": lambda p, c: _tl(p, c)["gx"] == 1 and _tr(p, c)["trips"] == {2} and _tr(p, c)["ragged_u"],
    "three trips": lambda p, c: _tl(p, c)["gx"] == 1 and _tr(p, c)["trips"] == {3} and _tr(p, c)["ragged_u"],
    "one pixel into the second trip, no skip": lambda p, c: _tl(p, c)["gx"] == 1 and _tr(p, c)["trips"] == {1, 2} and (_tr(p, c)["uneven_exit_in_wave"] or c == 512),
    "tails differ inside a wave, no skip": lambda p, c: _tl(p, c)["gx"] == 1 and _tr(p, c)["trips"] == {1} and (_tr(p, c)["uneven_u_in_wave"] or c == 512),
    "four workgroups x four trips, no ragged u": lambda p, c: (_tl(p, c)["gx"] == 4 and _tr(p, c)["trips"] == {4} and not _tr(p, c)["ragged_u"]
                                                               and not _tr(p, c)["idle_pixel_lanes"]),
    "five workgroups, four trips, ragged u": lambda p, c: (_tl(p, c)["gx"] == 5 and _tr(p, c)["trips"] <= {3, 4} and 4 in _tr(p, c)["trips"] and _tr(p, c)["ragged_u"]
                                                           and (_tr(p, c)["idle_pixel_lanes"] or c == 512)),
}

# the gx cap: C = 512 (ppb = 4), 258 x 256 = 66 048 pixels = 16 512 workgroup-rows = 4 128 groups > 4 x 1024, so gx = 1024, step = 4 096 and the lanes of the first
# 512 pixels make a fifth trip, whose u = 1, 2, 3 are dead.  n = 1.  33.8 M elements: the host packer and the fp64 reference are what take the time (below a second
# per storage measured on the MI355X box, fp16+8 the slowest), so every storage runs it
TORGB_CAP_CASE = ("gx cap of 1024, fifth trip", 512, (258, 256))
TORGB_CAP_STORAGES = STORAGES


def torgb_cap_regime_ok():
    _, c, (h, w) = TORGB_CAP_CASE
    cpp, ppb, groups, gx, step, loop_trips = torgb_launch(h, w, c)
    first, last = _cdiv(h * w - 0, U * step), _cdiv(max(h * w - (gx * ppb - 1), 0), U * step)          # trips of the first and of the last pixel lane
    return groups > TORGB_TRIPS * TORGB_CAP and gx == TORGB_CAP and loop_trips == 5 and first == 5 and last == 4 and (h * w) % (U * step) < step


# the ToRGB chain as the generator runs it: three levels, each level's image the next level's skip
TORGB_CHAIN = ((512, (4, 6)), (512, (8, 12)), (256, (16, 24)))

CONV_RGB_CASES = [("all halo", (1, 1, 1)),
                  ("exactly one tile", (2, 8, 32)),
                  ("one short of a tile in each direction", (1, 7, 31)),
                  ("2x2 tiles with 1-pixel tails", (2, 9, 33)),
                  ("3x3 tiles, interior tile, ragged edges, batch offset", (3, 17, 70))]
CONV_RGB_ACTS = (ACT_NONE, ACT_TANH)
CONV_RGB_REQUESTS = ((True, True), (True, False), (False, True))          # (nhwc, nchw)

CONV_RGB_REGIME = {
    "all halo": lambda p: p[1:] == (1, 1) and rgb_launch(*p[1:]) == (1, 1, 1, 1),
    "exactly one tile": lambda p: rgb_launch(*p[1:]) == (1, 1, RGB_TH, RGB_TW) and p[0] > 1,
    "one short of a tile in each direction": lambda p: rgb_launch(*p[1:]) == (1, 1, RGB_TH - 1, RGB_TW - 1),
    "2x2 tiles with 1-pixel tails": lambda p: rgb_launch(*p[1:]) == (2, 2, 1, 1) and p[0] > 1,
    "3x3 tiles, interior tile, ragged edges, batch offset": lambda p: (rgb_launch(*p[1:])[:2] == (3, 3) and 0 < rgb_launch(*p[1:])[2] < RGB_TH
                                                                       and 1 < rgb_launch(*p[1:])[3] < RGB_TW and p[0] >= 3),
}
