"""The glyph-fusion kernels of marconet_amd/csrc/aux_kernels.hip (adain_crop_kernel, adain_stats / finalize / apply, glyph_scatter_kernel) as data:
fp64 references of the operations, a NumPy statement of the kernel's rounding points (CPU only), the error bound the GPU tier asserts, and the case
tables of tests/test_glyph_fusion_gpu.py.  No device needed: tests/test_glyph_fusion.py checks the references against oracle/marconet_oracle.py and
shows, case by case, that the bound leaves room for a correct kernel.

Layout: everything here is NCHW on the host (the oracle's layout); values are fp32 tensors that hold what the storage under test holds (`quantise`).

The bound (per element of the restyled-prior half; a = prior element, (pm, ps) / (fm, fs) = mean and sqrt(unbiased var + 1e-5) of the prior / feature
window of that channel, all in fp64):

    |got - ref| <= 4 * 2^-24 * ((|a| + |pm|) / ps * fs + |ref| + |fm|)                  fp32
                   + 2^-11 * |ref| + 2^-25                                              fp16: the one rounding of the output

The kernel evaluates (a - pm32) / ps32 * fs32 + fm32 in fp32 from fp64 sums: the subtraction's operands carry 2^-24 (|a| + |pm|) between them (pm is
rounded to fp32 first; a is exact), the quotient and the product one rounding each and those of ps32 / fs32, the sum one rounding of the result and
that of fm32.  A simulation of that arithmetic (randn, gw = 1, mean 100 / spread 0.01, mean 6e4 / spread 5) reached 2.2 of these units;
`mirror_adain_fp32` below reaches 2.6 on the cases of this file (tests/test_glyph_fusion.py prints the figure per case); 4 is that measurement with
headroom.  The blocked storages keep the project's tolerance (tests/test_kernels_gpu.py `_tol` x 2, relative to the glyph's largest value)."""
import functools

import numpy as np
import torch

F32, F16, SPLIT, MX = "fp32", "f16", "split", "mx"       # the storage names of tests/tail_regimes.py
ADAIN_EPS = 1e-5              # networks.py:522 of the reference (oracle.marconet_oracle.adain)
GN_EPS = 1e-6                 # norm1 of conv_*_fuse (oracle.marconet_oracle._gn_swish)
U32 = 2.0 ** -24              # unit roundoff of fp32
BOUND_UNITS = 4.0
BLOCKED_TOL = {SPLIT: 2e-6, MX: 2e-5}                     # tests/test_kernels_gpu.py `_tol`; used x 2 like test_adain_crop_and_scatter


def vec_n(storage):
    """channels per 16-byte chunk — aux_kernels.hip adain_launch: `const int N = chunk_n(dtype);`, common.h: `return dt == MNET_F32 ? 4 : 8;`"""
    return 4 if storage == F32 else 8


def storage_dtype(storage):
    from marconet_amd import packing
    return {F32: torch.float32, F16: torch.float16, SPLIT: packing.SPLIT_DTYPE, MX: packing.MX_DTYPE}[storage]


def encode(x_nchw, storage):
    """fp32 NCHW (host) -> the NHWC tensor in `storage` (host), through the HOST packers for the blocked storages"""
    from marconet_amd import packing
    return packing.from_float(x_nchw.permute(0, 2, 3, 1).contiguous(), storage_dtype(storage))


def decode(t_nhwc):
    """NHWC tensor of any storage (host) -> fp32 NCHW"""
    from marconet_amd import packing
    return packing.to_float(t_nhwc).permute(0, 3, 1, 2).contiguous()


def quantise(x_nchw, storage):
    """the fp32 values `storage` holds for x"""
    return x_nchw.float().clone() if storage == F32 else decode(encode(x_nchw, storage))


# ====================================================================================================================== references
def _crops(prior, feat, wd, g):
    img, x1, gw, y1 = wd
    return prior[g:g + 1, :, :, y1:y1 + gw].double(), feat[img:img + 1, :, :, x1:x1 + gw].double()


def _mean_std(v):
    """oracle.marconet_oracle.adain's `ms` in fp64: mean and sqrt(unbiased var + eps) over the window, per channel -> [1,C,1,1]"""
    f = v.reshape(v.shape[0], v.shape[1], -1)
    return f.mean(2)[:, :, None, None], (f.var(2) + ADAIN_EPS).sqrt()[:, :, None, None]


def ref_adain_fp64(prior, feat, windows):
    """per glyph the fp64 [2C, S, gw] output: adain(prior crop, feature crop) then cat with the feature crop.
    prior [G,C,S,S], feat [B,C,S,FW] (fp32, storage-rounded); windows: (img, x1, gw, y1) per glyph"""
    out = []
    for g, wd in enumerate(windows):
        cp, cl = _crops(prior, feat, wd, g)
        fm, fs = _mean_std(cl)
        pm, ps = _mean_std(cp)
        out.append(torch.cat(((cp - pm) / ps * fs + fm, cl), dim=1)[0])
    return out


def adain_bound(prior, feat, windows, storage):
    """per glyph the [C, S, gw] bound on |got - ref| of the restyled-prior half (module docstring); fp32 and f16 only"""
    assert storage in (F32, F16)
    out = []
    for g, wd in enumerate(windows):
        cp, cl = _crops(prior, feat, wd, g)
        fm, fs = _mean_std(cl)
        pm, ps = _mean_std(cp)
        ref = (cp - pm) / ps * fs + fm
        b = BOUND_UNITS * U32 * ((cp.abs() + pm.abs()) / ps * fs + ref.abs() + fm.abs())
        if storage == F16:
            b = b + 2.0 ** -11 * ref.abs() + 2.0 ** -25
        out.append(b[0])
    return out


def ref_gn_affine_fp64(ref, gamma, beta):
    """GroupNorm(2C/32 groups, eps 1e-6) of one glyph's fp64 [2C, S, gw] output as an affine: (scale [2C], shift [2C], |beta| + |mean * scale| [2C]).
    The statistics are over the window only (the kernel's output is zero beyond gw, and so is every later use of those columns).  The third value is
    the magnitude shift is assembled from: deviations of shift are measured against it, not against shift (which can cancel to nothing)"""
    c2 = ref.shape[0]
    v = ref.reshape(c2 // 32, -1)
    mean, rstd = v.mean(1), (v.var(1, unbiased=False) + GN_EPS).rsqrt()
    scale = gamma.double() * rstd.repeat_interleave(32)
    ms = mean.repeat_interleave(32) * scale
    return scale, beta.double() - ms, beta.double().abs() + ms.abs()


def gn_deviation(scale, shift, want):
    """(worst |scale - want| / |want|, worst |shift - want| / (|beta| + |mean * scale|)) of one glyph against ref_gn_affine_fp64's triple"""
    ws, wh, mag = want
    return (float(((scale.double() - ws).abs() / ws.abs()).max()), float(((shift.double() - wh).abs() / mag).max()))


def ref_scatter(feat, scale, shift, g_start, g_x1, g_w):
    """the reference's loop (oracle.marconet_oracle._prior_transform) in the dtype of `feat`: reads the unmodified feat, a later glyph of an image
    overwrites an earlier one, returns feat + res.  feat [B,C,S,FW], scale / shift [G,C,S,S] (columns gw..S unused)"""
    res = torch.zeros_like(feat)
    for b in range(feat.shape[0]):
        for g in range(int(g_start[b]), int(g_start[b + 1])):
            x1, gw = int(g_x1[g]), int(g_w[g])
            res[b, :, :, x1:x1 + gw] = feat[b, :, :, x1:x1 + gw] * scale[g, :, :, :gw] + shift[g, :, :, :gw]
    return feat + res


# ====================================================================================================================== the kernel's rounding points
def mirror_adain_fp32(prior, feat, windows, gamma, beta):
    """NumPy statement of adain_crop_kernel's arithmetic (CPU only; never an expected value on the GPU): fp64 one-pass sums and sums of
    squares of (value - the channel's value at the window's first pixel), the statistics (pm, ps, fm, fs) rounded to fp32 with ps = sqrtf((float)var + 1e-5f), the apply expression in fp32 one operation at a time, the
    GroupNorm sums in closed form from those statistics, mean / rstd rounded to fp32, scale = gamma * rstd and shift = beta - mean * scale in fp32.
    -> per glyph (fp32 [C, S, gw] restyled prior, fp32 scale [2C], fp32 shift [2C])"""
    f32 = np.float32
    ga32, be32 = gamma.numpy().astype(f32), beta.numpy().astype(f32)
    out = []
    for g, (img, x1, gw, y1) in enumerate(windows):
        a = prior[g, :, :, y1:y1 + gw].numpy().astype(f32)
        b = feat[img, :, :, x1:x1 + gw].numpy().astype(f32)
        C, S = a.shape[0], a.shape[1]
        cnt = float(S * gw)
        ka, kb = a[:, :1, :1].astype(np.float64), b[:, :1, :1].astype(np.float64)          # the pivots: the window's first pixel
        a64, b64 = a.astype(np.float64) - ka, b.astype(np.float64) - kb
        a0, a1, b0, b1 = a64.sum((1, 2)), (a64 * a64).sum((1, 2)), b64.sum((1, 2)), (b64 * b64).sum((1, 2))
        pd, fd = a0 / cnt, b0 / cnt
        pm, fm = ka[:, 0, 0] + pd, kb[:, 0, 0] + fd
        pdev, fdev = np.maximum(a1 - cnt * pd * pd, 0.0), np.maximum(b1 - cnt * fd * fd, 0.0)
        pv, fv = pdev / (cnt - 1.0), fdev / (cnt - 1.0)
        pm32, fm32 = pm.astype(f32), fm.astype(f32)
        ps32, fs32 = np.sqrt(pv.astype(f32) + f32(1e-5)), np.sqrt(fv.astype(f32) + f32(1e-5))
        assert ps32.dtype == f32 and fs32.dtype == f32
        e = lambda v: v[:, None, None]
        o = (a - e(pm32)) / e(ps32) * e(fs32) + e(fm32)
        assert o.dtype == f32
        r = fs32.astype(np.float64) / ps32.astype(np.float64)
        s1 = np.concatenate([cnt * fm, cnt * fm]).reshape(-1, 32).sum(1)
        s2 = np.concatenate([r * r * pdev + cnt * fm * fm, fdev + cnt * fm * fm]).reshape(-1, 32).sum(1)
        mean = s1 / (cnt * 32.0)
        var = np.maximum(s2 / (cnt * 32.0) - mean * mean, 0.0)
        mean32 = np.repeat(mean.astype(f32), 32)
        rstd32 = np.repeat((1.0 / np.sqrt(var + float(f32(GN_EPS)))).astype(f32), 32)
        sc = ga32 * rstd32
        sh = be32 - mean32 * sc
        assert sc.dtype == f32 and sh.dtype == f32
        out.append((torch.from_numpy(o), torch.from_numpy(sc), torch.from_numpy(sh)))
    return out


def store_output(o, storage):
    """what `storage` holds for one glyph's fp32 [2C, S, gw] output (the kernel's single rounding of the output)"""
    return o if storage == F32 else quantise(o[None], storage)[0]


# ====================================================================================================================== AdaIN cases
# tag -> (S, C, FW, storages).  plane = 256 / (C / N) pixel lanes; fold trips = ceil(C / 256); LDS of the fused kernel:
# 256 * N * 32 + 16 C + 32 C + 8 (2C / 32) bytes
ADAIN_CASES = {
    "w32": (32, 512, 96, (F32, F16, SPLIT, MX)),     # the workload's 32-px level: two fold trips, 88 KiB of LDS for the 8-wide storages
    "w64": (64, 256, 160, (F32, F16)),                # the workload's 64-px level, 4 pixel lanes in fp32
    "p1": (8, 1024, 24, (F32,)),                      # plane == 1, four fold trips, fp32 LDS above 64 KiB
    "p64": (16, 32, 48, (F16, MX)),                   # plane == 64, one GroupNorm group per half
    "min": (8, 64, 8, (F32, F16)),                    # FW == S, one image
}
DISPATCH_CASE = (8, 32, 24, 256)                      # S, C, FW, G: the glyph count at which split=None changes form (ops.ADAIN_SPLIT_BELOW)
PLAIN, CONST, OFFSET = "plain", "const", "offset"


def regimes(storage):
    return (PLAIN, CONST, OFFSET) if storage in (F32, F16) else (PLAIN, CONST)


def adain_plane(C, storage):
    return 256 // (C // vec_n(storage))


def adain_fold_trips(C):
    return (C + 255) // 256


def adain_lds_bytes(C, storage):
    return 256 * vec_n(storage) * 4 * 8 + 4 * C * 4 + 4 * C * 8 + (2 * C // 32) * 2 * 4


def rule_y1(S, gw):
    """glyphs.window: y1 = half - trunc(gw / 2)"""
    return S // 2 - int(gw / 2)


def adain_windows(S, FW):
    """(img, x1, gw, y1) per glyph — the window edges of the issue; every window lies inside its maps (asserted).  All but entry 6 are what
    glyphs.GlyphTables makes of `adain_centres` (tests/test_glyph_fusion.py)"""
    half, last = S // 2, (0 if FW == S else 1)
    odd = half + 3
    wins = [
        (0, 0, S, rule_y1(S, S)),                               # full width at x1 = 0
        (last, FW - S, S, rule_y1(S, S)),                       # full width, flush right
        (last, FW - half, half, rule_y1(S, half)),              # the narrowest the default rule produces, flush right
        (0, 0, odd, rule_y1(S, odd)),                           # odd width at the left edge
        (0, FW - 1, 1, rule_y1(S, 1)),                          # gw = 1 (bucketing with centre_w), the last column of the map
        (last, FW - 2, 2, rule_y1(S, 2)),                       # gw = 2 (the same)
        (0, min(3, FW - half - 1), half + 1, S - (half + 1)),   # an inner window whose y1 = S - gw is NOT the rule's value
        (last, 0, S - 1, rule_y1(S, S - 1)),                    # two glyphs, one window, different priors
        (last, 0, S - 1, rule_y1(S, S - 1)),
    ]
    assert wins[6][3] != rule_y1(S, wins[6][2])
    for img, x1, gw, y1 in wins:
        assert 0 <= img <= last and 1 <= gw <= S and 0 <= x1 and x1 + gw <= FW and 0 <= y1 and y1 + gw <= S, (img, x1, gw, y1)
    return wins


def adain_centres(S, FW):
    """per entry of adain_windows (image, window centre in columns, needs centre_w): the centre GlyphTables turns into that window — None for the
    hand-set entry 6.  centre_w: the centre lies beyond the map, which only mixed-width bucketing (centres at the 512-padded run's width) produces"""
    half, last = S // 2, (0 if FW == S else 1)
    return [(0, half, False), (last, FW - half, False), (last, FW, False), (0, 3, False), (0, FW - 1 + half, True), (last, FW - 2 + half, True),
            None, (last, half - 1, False), (last, half - 1, False)]


def planted(C):
    """the channels that carry the special data: 0, 31, 32, C-1 and, for C >= 512, 256 and 300 (second fold trip, across a GroupNorm group's edge)"""
    idx = [0, 31, 32, C - 1] + ([256, 300] if C >= 512 else [])
    out = []
    for i in idx:
        if i < C and i not in out:
            out.append(i)
    return out


def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=2)
def adain_inputs(tag, regime, storage):
    """-> (prior [G,C,S,S], feat [B,C,S,FW], windows, gamma [2C], beta [2C]): fp32 host tensors holding what `storage` holds.  Treat as read-only.
    The special channels alternate over `planted`: entries 0, 2, 4 change the PRIOR channel, entries 1, 3, 5 the FEATURE channel"""
    S, C, FW, storages = ADAIN_CASES[tag]
    assert storage in storages and regime in regimes(storage)
    wins = adain_windows(S, FW)
    G, B = len(wins), 1 + max(w[0] for w in wins)
    prior = _rnd((G, C, S, S), 26) * 1.5 + 0.2
    feat = _rnd((B, C, S, FW), 25)
    idx = planted(C)
    if regime == CONST:           # variance 0: eps decides ps / fs
        prior[:, idx[0::2]] = 1.3
        feat[:, idx[1::2]] = -0.7
    elif regime == OFFSET:        # a mean far larger than the spread
        spread = 0.01 if storage == F32 else 0.5
        prior[:, idx[0::2]] = 100.0 + spread * _rnd((G, len(idx[0::2]), S, S), 31)
        feat[:, idx[1::2]] = 100.0 + spread * _rnd((B, len(idx[1::2]), S, FW), 32)
    gamma, beta = _rnd((2 * C,), 29).abs() + 0.5, _rnd((2 * C,), 30) * 0.3
    return quantise(prior, storage), quantise(feat, storage), wins, gamma, beta


# GroupNorm affine tolerances: 4 x the worst deviation (gn_deviation: scale, shift) of mirror_adain_fp32 from ref_gn_affine_fp64 over the glyphs and
# storages of the (case, regime) — measured on the CPU by tests/test_glyph_fusion.py::test_gn_tolerances_are_four_times_the_mirror, which fails when a
# literal here is not that figure (rounded up to two digits).  Never derived from the kernel's output.
GN_MIRROR_WORST = {        # (case, regime): (scale, shift) — the mirror's worst deviation, rounded up to two digits
    ("w32", PLAIN): (1.3e-7, 1.8e-7), ("w32", CONST): (1.3e-7, 1.8e-7), ("w32", OFFSET): (1.3e-7, 1.8e-7),
    ("w64", PLAIN): (1.2e-7, 1.5e-7), ("w64", CONST): (1.3e-7, 1.8e-7), ("w64", OFFSET): (1.2e-7, 1.6e-7),
    ("p1", PLAIN): (1.2e-7, 1.7e-7), ("p1", CONST): (1.2e-7, 1.7e-7), ("p1", OFFSET): (1.2e-7, 1.7e-7),
    ("p64", PLAIN): (1.2e-7, 1.3e-7), ("p64", CONST): (1.1e-7, 1.2e-7), ("p64", OFFSET): (8.4e-8, 1.2e-7),
    ("min", PLAIN): (1.1e-7, 1.2e-7), ("min", CONST): (1.1e-7, 1.3e-7), ("min", OFFSET): (8.7e-8, 1.7e-7),
}
GN_TOL = {k: (4.0 * v[0], 4.0 * v[1]) for k, v in GN_MIRROR_WORST.items()}      # 3.4e-7 ... 7.2e-7: three orders under the 2e-4 / 2e-3 of the older test


def gn_tol(tag, regime):
    return GN_TOL[(tag, regime)]


# ====================================================================================================================== scatter cases
# tag -> (S, C, FW, counts per image, [(x1, gw)] per glyph in order, storages)
SCATTER_CASES = {
    # the middle image has no glyphs; nested: glyph 0 wide, glyph 1 inside it (0 owns both flanks); x = 0 and the last column; gw = 1
    "empty_middle": (8, 64, 40, (2, 0, 3), [(2, 8), (4, 3), (0, 5), (39, 1), (32, 8)], (F32, F16, SPLIT, MX)),
    "empty_first": (8, 32, 24, (0, 2, 1), [(0, 8), (8, 8), (16, 8)], (F32, F16)),             # + adjacent windows: x1 + gw == next x1
    "empty_last": (8, 32, 24, (1, 2, 0), [(16, 8), (3, 1), (4, 6)], (F32, F16)),
    # triple overlap: columns 6..8 are covered by all three, the last one wins; then adjacent; S = 12: a full run of 8 rows and a short one of 4
    "triple_s12": (12, 64, 40, (3, 2), [(0, 12), (4, 9), (6, 3), (10, 10), (20, 12)], (F32, F16, SPLIT, MX)),
    # FW * C / N = 36 * 4 = 144: one partly idle workgroup; with C = 96 it is 432 = 256 + 176: a last partial workgroup after a full one
    "partial_wg": (8, 32, 36, (2, 1), [(0, 5), (30, 6), (17, 4)], (F16,)),
    "partial_wg2": (12, 96, 36, (2, 2), [(1, 12), (7, 2), (24, 12), (35, 1)], (F32, F16, SPLIT, MX)),
    # the workload's run count (S = 32: four runs), a nested pair and a window ending at FW
    "s32": (32, 32, 72, (3, 1), [(0, 32), (10, 7), (40, 32), (56, 16)], (F32, F16, MX)),
}
SCATTER_RUN = 8               # aux_kernels.hip: #define MNET_SCATTER_RUN 8


def scatter_tables(tag):
    S, C, FW, counts, wins, _ = SCATTER_CASES[tag]
    assert sum(counts) == len(wins)
    g_start = [0]
    for c in counts:
        g_start.append(g_start[-1] + c)
    for x1, gw in wins:
        assert 0 <= x1 and 1 <= gw <= S and x1 + gw <= FW, (x1, gw)
    return g_start, [w[0] for w in wins], [w[1] for w in wins]


def scatter_owner(tag):
    """[B][FW] owner glyph of every column (-1: none) — the last glyph of the image whose window covers it"""
    S, C, FW, counts, wins, _ = SCATTER_CASES[tag]
    g_start, _, _ = scatter_tables(tag)
    own = -np.ones((len(counts), FW), np.int64)
    for b in range(len(counts)):
        for g in range(g_start[b], g_start[b + 1]):
            own[b, wins[g][0]:wins[g][0] + wins[g][1]] = g
    return own


@functools.lru_cache(maxsize=2)
def scatter_inputs(tag, storage):
    """-> (feat [B,C,S,FW], scale [G,C,S,S], shift [G,C,S,S]) fp32 host tensors holding what `storage` holds.  Read-only"""
    S, C, FW, counts, wins, storages = SCATTER_CASES[tag]
    assert storage in storages
    feat = _rnd((len(counts), C, S, FW), 41)
    scale, shift = _rnd((len(wins), C, S, S), 42), _rnd((len(wins), C, S, S), 43)
    return quantise(feat, storage), quantise(scale, storage), quantise(shift, storage)
