"""No device: the references, the case tables and the error bound of tests/test_glyph_fusion_gpu.py (all in tests/glyph_fusion.py).

- the fp64 references are the oracle's operations (oracle.marconet_oracle.adain + cat; the glyph loop of _prior_transform);
- the windows of every AdaIN case are what glyphs.GlyphTables produces (but for the one hand-set y1), and equal glyphs.window where the scalar rule applies;
- every case lands in the launch regime it is there for (pixel lanes, fold trips, LDS size, partial workgroups, short row runs);
- for every (case, data regime, storage) the GPU tier runs, a NumPy statement of the kernel's rounding points stays inside the bound the GPU tier
  asserts — the condition that keeps the bound honest: where the mirror exceeds it the CASE is changed, never the bound;
- the GroupNorm tolerances written beside the cases are four times what that mirror deviates from the fp64 affine."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import glyph_fusion as GF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMBOS = [(tag, regime, storage) for tag, (_, _, _, storages) in GF.ADAIN_CASES.items() for storage in storages for regime in GF.regimes(storage)]


def _src(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


# ====================================================================================================================== references
@pytest.mark.parametrize("tag", ["min", "p64"])
def test_ref_adain_is_the_oracles_adain_and_cat(tag):
    from oracle import marconet_oracle as O
    storage = GF.ADAIN_CASES[tag][3][0]
    prior, feat, wins, _, _ = GF.adain_inputs(tag, GF.PLAIN, storage)
    refs = GF.ref_adain_fp64(prior, feat, wins)
    for g, (img, x1, gw, y1) in enumerate(wins):
        cp, cl = prior[g:g + 1, :, :, y1:y1 + gw], feat[img:img + 1, :, :, x1:x1 + gw]
        want = torch.cat((O.adain(cp, cl), cl), dim=1)[0]                       # networks.py:429-431 of the reference, in fp32
        assert refs[g].dtype == torch.float64 and refs[g].shape == want.shape == (2 * prior.shape[1], prior.shape[2], gw)
        err = (refs[g] - want.double()).abs().max().item()
        assert err <= 2e-5 * refs[g].abs().max().item(), "glyph %d: %.3e" % (g, err)
        assert torch.equal(refs[g][prior.shape[1]:].float(), cl[0])             # the feature half is the crop itself


def test_ref_scatter_is_the_oracles_glyph_loop(monkeypatch):
    """oracle._prior_transform with its convolutions replaced by table look-ups (glyph k of the call order gets scale[k], shift[k]): what is left is the
    loop itself — windows from locs, reads from the unmodified map, later glyphs overwrite earlier ones, feat + res — and ref_scatter reproduces it"""
    from marconet_amd import glyphs
    from oracle import marconet_oracle as O
    S, C, FW, counts = 8, 4, 40, (3, 0, 2)
    half = S // 2
    locs = torch.tensor([[0.30, 0, 0.36, 0, 0.05, 0], [0.5, 0, 0.5, 0, 0.5, 0], [0.99, 0, 0.80, 0, 0.1, 0]])       # overlapping and clipped windows
    G = sum(counts)
    g = torch.Generator().manual_seed(3)
    feat = torch.randn((3, C, S, FW), generator=g, dtype=torch.float64)
    scale, shift = torch.randn((G, C, S, S), generator=g, dtype=torch.float64), torch.randn((G, C, S, S), generator=g, dtype=torch.float64)
    calls = {"scale": 0, "shift": 0}

    def two_conv(sd, key, x):
        kind = key.rsplit("_", 1)[1]
        k = calls[kind]
        calls[kind] += 1
        return {"scale": scale, "shift": shift}[kind][k:k + 1, :, :, :x.shape[-1]]

    monkeypatch.setattr(O, "_two_conv", two_conv)
    monkeypatch.setattr(O, "res_text_block", lambda sd, key, x: x)
    priors = [torch.randn((n, C, S, S), generator=g, dtype=torch.float64) for n in counts]
    want = O._prior_transform({}, feat, priors, locs, "64", half)
    assert calls == {"scale": G, "shift": G}
    tab = glyphs.GlyphTables(locs.numpy(), list(counts), FW, half, "cpu")
    assert tab.g_start.tolist() == [0, 3, 3, 5]
    k = 0
    for b, n in enumerate(counts):
        for c in range(n):
            assert (int(tab.g_x1[k]), int(tab.g_w[k]), int(tab.g_y1[k])) == glyphs.window(float(locs[b, 2 * c]), FW, half)
            k += 1
    x1, gw = tab.g_x1.tolist(), tab.g_w.tolist()
    assert x1[1] < x1[0] + gw[0] and x1[2] == 0 and x1[3] + gw[3] == FW and gw[3] < S                               # overlap, both edges, a clipped one
    got = GF.ref_scatter(feat, scale, shift, tab.g_start.tolist(), x1, gw)
    assert torch.equal(got, want)
    assert torch.equal(got[1], feat[1])                                                                            # the image without glyphs


# ====================================================================================================================== windows
@pytest.mark.parametrize("tag", list(GF.ADAIN_CASES))
def test_adain_windows_come_from_glyph_tables(tag):
    from marconet_amd import glyphs
    S, C, FW, _ = GF.ADAIN_CASES[tag]
    half = S // 2
    wins, centres = GF.adain_windows(S, FW), GF.adain_centres(S, FW)
    assert len(wins) == len(centres) == 9 and centres[6] is None
    for bucketed in (False, True):
        cw = 2 * FW if bucketed else FW
        pick = [i for i, c in enumerate(centres) if c is not None and c[2] == bucketed]
        nimg = 1 + max(w[0] for w in wins)
        per = [[i for i in pick if wins[i][0] == b] for b in range(nimg)]
        locs = np.zeros((nimg, 2 * max(len(p) for p in per)), np.float32)
        for b, p in enumerate(per):
            for k, i in enumerate(p):
                locs[b, 2 * k] = (centres[i][1] + 0.5) / cw
        tab = glyphs.GlyphTables(locs, [len(p) for p in per], FW, half, "cpu", centre_w=cw if bucketed else None)
        order = [i for p in per for i in p]
        assert tab.G == len(order)
        for k, i in enumerate(order):
            got = (int(tab.g_img[k]), int(tab.g_x1[k]), int(tab.g_w[k]), int(tab.g_y1[k]))
            assert got == wins[i], (tag, i, got, wins[i])
            if not bucketed:
                b = wins[i][0]
                assert glyphs.window(float(locs[b, 2 * per[b].index(i)]), FW, half) == (wins[i][1], wins[i][2], wins[i][3])
    widths = sorted(w[2] for w in wins)
    assert widths[:2] == [1, 2] and S in widths and half in widths and half + 3 in widths
    assert any(w[1] == 0 and w[2] == S for w in wins) and any(w[1] == FW - S and w[2] == S for w in wins)
    assert wins[7] == wins[8]


# ====================================================================================================================== launch regimes
def test_mirrored_constants_are_the_sources():
    hip = _src("marconet_amd", "csrc", "aux_kernels.hip")
    ops = _src("marconet_amd", "ops.py")
    assert re.search(r"#define MNET_SCATTER_RUN %d\b" % GF.SCATTER_RUN, hip)
    assert "ADAIN_SPLIT_BELOW = %d " % GF.DISPATCH_CASE[3] in ops and "G < ADAIN_SPLIT_BELOW" in ops
    launch = hip[hip.index("static int adain_launch"):hip.index('extern "C" int mnet_adain_crop_concat(')]
    assert "const int N = chunk_n(dtype);" in launch                                           # ... which is the one definition in common.h:
    assert "static inline int chunk_n(int dt) { return dt == MNET_F32 ? 4 : 8; }" in _src("marconet_amd", "csrc", "common.h")
    assert ("(size_t)256 * N * 4 * sizeof(double) + (size_t)4 * C * sizeof(float) + (size_t)4 * C * sizeof(double) +" in launch
            and "(size_t)(2 * C / 32) * 2 * sizeof(float);" in launch)                       # adain_lds_bytes
    assert "lds <= 160 * 1024" in launch


def test_adain_cases_land_in_their_regimes():
    lds = GF.adain_lds_bytes
    assert GF.adain_fold_trips(512) == 2 and lds(512, GF.F16) == lds(512, GF.MX) == 90368 > 65536 >= lds(512, GF.F32)      # w32: 88 KiB for the 8-wide
    assert GF.adain_plane(256, GF.F32) == 4 and GF.adain_plane(256, GF.F16) == 8                                           # w64
    assert GF.adain_plane(1024, GF.F32) == 1 and GF.adain_fold_trips(1024) == 4 and 65536 < lds(1024, GF.F32) <= 160 * 1024  # p1
    assert GF.adain_plane(32, GF.F16) == GF.adain_plane(32, GF.MX) == 64 and 2 * 32 // 32 == 2                              # p64: one group per half
    assert GF.ADAIN_CASES["min"][0] == GF.ADAIN_CASES["min"][2] and max(w[0] for w in GF.adain_windows(8, 8)) == 0         # min
    assert lds(2048, GF.F16) == 164864 > 160 * 1024                                                                         # the launch adain_launch refuses
    for tag, (S, C, FW, storages) in GF.ADAIN_CASES.items():
        for st in storages:
            n = GF.vec_n(st)
            assert C % n == 0 and 256 % (C // n) == 0 and C % 32 == 0 and FW >= S and lds(C, st) <= 160 * 1024
        if tag != "min":
            assert max(w[0] for w in GF.adain_windows(S, FW)) == 1
    assert GF.planted(512) == [0, 31, 32, 511, 256, 300] and GF.planted(32) == [0, 31] and GF.planted(64) == [0, 31, 32, 63]
    # second fold trip and both sides of a GroupNorm group's edge (31 | 32); 256 changes the prior, 300 the feature
    assert GF.planted(512)[0::2] == [0, 32, 256] and GF.planted(512)[1::2] == [31, 511, 300]


def test_scatter_cases_land_in_their_regimes():
    own = {tag: GF.scatter_owner(tag) for tag in GF.SCATTER_CASES}
    assert GF.scatter_tables("empty_middle")[0] == [0, 2, 2, 5]
    assert GF.scatter_tables("empty_first")[0][:2] == [0, 0] and GF.scatter_tables("empty_last")[0][-2:] == [3, 3]
    assert own["empty_middle"][0, 1:11].tolist() == [-1, 0, 0, 1, 1, 1, 0, 0, 0, -1]             # nested: the outer glyph owns both flanks
    assert own["empty_middle"][2, 0] == 2 and own["empty_middle"][2, 39] == 4                    # x = 0; gw = 1 is overwritten by the window ending at FW
    assert (own["empty_middle"][1] == -1).all()
    assert own["empty_first"][1].tolist() == [0] * 8 + [1] * 8 + [-1] * 8                        # adjacent: x1 + gw == next x1
    assert own["empty_last"][1, 2:11].tolist() == [-1, 1, 2, 2, 2, 2, 2, 2, -1]                  # gw = 1 next to its neighbour
    assert own["triple_s12"][0, :14].tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 2, 1, 1, 1, 1, -1]     # triple overlap at 6..8: the last one wins
    assert own["partial_wg2"][1, 35] == 3 and own["partial_wg2"][1, 34] == 2                      # gw = 1 on the last column, inside a wider window
    assert own["s32"][0, 9:18].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 0] and own["s32"][0, 71] == 2 and own["s32"][0, 39] == -1
    for tag, (S, C, FW, counts, wins, storages) in GF.SCATTER_CASES.items():
        for st in storages:
            assert C % GF.vec_n(st) == 0 and (st in (GF.F32, GF.F16) or C % 32 == 0)
    per = lambda tag, st: GF.SCATTER_CASES[tag][2] * (GF.SCATTER_CASES[tag][1] // GF.vec_n(st))
    assert per("partial_wg", GF.F16) == 144 and per("partial_wg2", GF.F16) == 432 and per("partial_wg2", GF.F32) == 864     # id >= FW * cpp in the last workgroup
    assert sorted({c[0] for c in GF.SCATTER_CASES.values()}) == [8, 12, 32] and 12 % GF.SCATTER_RUN == 4                      # S = 12: a short last run


# ====================================================================================================================== the bound leaves room
@functools.lru_cache(maxsize=None)
def _mirror_figures(tag, regime, storage):
    """-> (worst mirror error / asserted bound, worst GroupNorm scale deviation, worst shift deviation) over the glyphs of the combination"""
    prior, feat, wins, gamma, beta = GF.adain_inputs(tag, regime, storage)
    C = prior.shape[1]
    refs = GF.ref_adain_fp64(prior, feat, wins)
    mir = GF.mirror_adain_fp32(prior, feat, wins, gamma, beta)
    bounds = GF.adain_bound(prior, feat, wins, storage) if storage in (GF.F32, GF.F16) else None
    ratio = ds = dh = 0.0
    for g in range(len(wins)):
        stored = GF.store_output(torch.cat((mir[g][0], refs[g][C:].float()), 0), storage)
        err = (stored[:C].double() - refs[g][:C]).abs()
        if bounds is not None:
            ratio = max(ratio, float((err / bounds[g]).max()))
        else:
            ratio = max(ratio, float(err.max() / (GF.BLOCKED_TOL[storage] * 2.0 * refs[g].abs().max())))
        a, b = GF.gn_deviation(mir[g][1], mir[g][2], GF.ref_gn_affine_fp64(refs[g], gamma, beta))
        ds, dh = max(ds, a), max(dh, b)
    return ratio, ds, dh


@pytest.mark.parametrize("tag,regime,storage", COMBOS)
def test_mirror_of_the_kernel_stays_inside_the_bound(tag, regime, storage):
    ratio, ds, dh = _mirror_figures(tag, regime, storage)
    print("%s %s %s: mirror error / bound %.3f (fp32 part alone: %.2f units of %g)  GN scale %.3e shift %.3e"
          % (tag, regime, storage, ratio, ratio * GF.BOUND_UNITS, GF.BOUND_UNITS, ds, dh))
    assert ratio <= 1.0
    if storage == GF.F32:
        assert ratio <= 0.75       # a correct kernel keeps a quarter of the bound in hand (fma contraction and summation order move it by less)


@pytest.mark.parametrize("tag", list(GF.ADAIN_CASES))
def test_gn_tolerances_are_four_times_the_mirror(tag):
    storages = GF.ADAIN_CASES[tag][3]
    for regime in (GF.PLAIN, GF.CONST, GF.OFFSET):
        figs = [_mirror_figures(tag, regime, st) for st in storages if regime in GF.regimes(st)]
        worst = (max(f[1] for f in figs), max(f[2] for f in figs))
        lit, tol = GF.GN_MIRROR_WORST[(tag, regime)], GF.gn_tol(tag, regime)
        print("%s %s: mirror worst scale %.3e shift %.3e  literal %r  tolerance %.2e / %.2e" % (tag, regime, worst[0], worst[1], lit, tol[0], tol[1]))
        for k in range(2):
            assert worst[k] <= lit[k] <= 1.25 * worst[k], "the literal is the measured figure rounded up: re-measure"
            assert tol[k] == 4.0 * lit[k] and tol[k] < 1e-5             # three orders under the 2e-4 / 2e-3 of test_adain_crop_and_scatter


def test_a_biased_variance_shows_on_the_constant_feature_channel_only():
    """cnt instead of cnt - 1 in BOTH variances scales ps and fs alike: fs / ps, and with it every ordinary channel, moves by less than the bound.
    Where the feature channel is constant fs = sqrt(eps) stays and ps alone shrinks: the restyled prior moves by 1 / (2 cnt) of its spread — outside
    the per-element bound, inside the older tolerance relative to the glyph's largest value (tests/test_kernels_gpu.py: 2e-5 x 2 in fp32)"""
    prior, feat, wins, _, _ = GF.adain_inputs("min", GF.CONST, GF.F32)
    refs, bounds = GF.ref_adain_fp64(prior, feat, wins), GF.adain_bound(prior, feat, wins, GF.F32)
    C = prior.shape[1]
    img, x1, gw, y1 = wins[0]
    cp, cl = prior[0, :, :, y1:y1 + gw].double(), feat[img, :, :, x1:x1 + gw].double()
    st = lambda v: (v.mean((1, 2), keepdim=True), (v.var((1, 2), unbiased=False, keepdim=True) + GF.ADAIN_EPS).sqrt())
    (pm, ps), (fm, fs) = st(cp), st(cl)
    over = ((cp - pm) / ps * fs + fm - refs[0][:C]).abs() / bounds[0]
    const_feat = GF.planted(C)[1::2]
    plain = [c for c in range(C) if c not in GF.planted(C)]
    assert over[const_feat].max() > 10.0 and over[plain].max() < 1.0
    assert ((cp - pm) / ps * fs + fm - refs[0][:C]).abs().max() <= 2e-5 * 2 * refs[0].abs().max()
