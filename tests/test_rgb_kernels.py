"""No device: the spec of the two RGB output kernels (tests/rgb_kernels.py) checked against itself and against the sources.  Every case of
tests/test_rgb_kernels_gpu.py lands in the launch regime it names; the mirrored lines are still in aux_kernels.hip; the written-out fp64 references agree
with F.conv2d / F.interpolate; tanh stays out of saturation in every tanh case, so a wrong pre-activation cannot hide; and the references tell a subtly wrong
kernel from a right one by more than 100 x the GPU tier's bound."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import rgb_kernels as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def _body(src, start, end):
    a = src.index(start)
    return src[a:src.index(end, a)]


def test_mirrored_lines_are_the_sources():
    hip = _src("marconet_amd", "csrc", "aux_kernels.hip")
    assert re.search(r"#define MNET_TORGB_U %d\b" % R.U, hip) and R.U == 4
    host = _body(hip, 'extern "C" int mnet_torgb', "MNET_LAUNCH_CHECK")
    assert "(((long long)h * w + (256 / (c / 8)) - 1) / (256 / (c / 8)) + MNET_TORGB_U - 1) / MNET_TORGB_U" in host
    assert "e && atoi(e) > 0 ? atoi(e) : %d" % R.TORGB_TRIPS in host and "const long long wgs = (groups + trips - 1) / trips;" in host
    assert "const int gx = (int)(wgs < %d ? wgs : %d);" % (R.TORGB_CAP, R.TORGB_CAP) in host and "dim3(gx, n), dim3(256)" in host
    assert "c >= 64 && c <= 512 && (c & (c - 1)) == 0" in host and "!skip || (h % 2 == 0 && w % 2 == 0)" in host
    kern = _body(hip, "void __launch_bounds__(256) torgb_kernel", 'extern "C" int mnet_torgb')
    assert "const int cpp = C >> 3;" in kern and "ppb = 256 / cpp" in kern and "const int step = gridDim.x * ppb;" in kern
    assert "for (int pix0 = blockIdx.x * ppb + pl; pix0 < HW; pix0 += U * step)" in kern
    assert "ld8<T>(xb + (size_t)(pq < HW ? pq : pix0) * C, vv[u]);" in kern and "if (pix >= HW) continue;" in kern
    assert "const int mu = ch - (cpp > 16 ? cpp - 16 : 0);" in kern
    assert kern.count("tanhf(r0 - r0 + r0)") == 1                                      # the overflow rule as the kernel writes it
    rgb = _body(hip, "void __launch_bounds__(256) conv3x3_rgb_kernel", 'extern "C" int mnet_conv3x3_rgb')
    assert "constexpr int TH = %d, TW = %d, PW = TW + 2, PH = TH + 2;" % (R.RGB_TH, R.RGB_TW) in rgb
    assert "for (int half = 0; half < CIN / 32; ++half)" in rgb and "if (oy >= H || ox >= W) return;" in rgb and "if (oy_ >= H || ox_ >= W) return;" in rgb
    assert rgb.count("tanhf(r[0] - r[0] + r[0])") == 2 and rgb.count("r[0] = tanhf(r[0]);") == 1          # blocked and f16: the rule; fp32: plain tanhf
    host = _body(hip, 'extern "C" int mnet_conv3x3_rgb', "MNET_LAUNCH_CHECK")
    assert "const int tiles = ((h + 7) / 8) * ((w + 31) / 32);" in host and "dim3(tiles, n), dim3(256)" in host
    assert "conv3x3_rgb_kernel<float, 64, SPLIT, std::conditional_t<SPLIT, T, hs>>" in host and "(conv3x3_rgb_kernel<f16, 64>)" in host
    assert "cin == 64" in host and "act == MNET_ACT_NONE || act == MNET_ACT_TANH" in host
    hdr = _src("include", "marconet_hip.h")
    for name, value in (("NONE", R.ACT_NONE), ("LRELU", R.ACT_LRELU), ("TANH", R.ACT_TANH)):
        assert re.search(r"MNET_ACT_%s\s*=\s*%d\b" % (name, value), hdr)


def test_launch_mirrors_on_known_shapes():
    """the mirrors against launches worked out by hand from the sources"""
    assert R.torgb_launch(2, 2, 512) == (64, 4, 1, 1, 4, 1) and R.torgb_launch(2, 2, 64) == (8, 32, 1, 1, 32, 1)
    assert R.torgb_launch(6, 10, 256) == (32, 8, 2, 1, 8, 2) and R.torgb_launch(6, 10, 512) == (64, 4, 4, 1, 4, 4)
    assert R.torgb_launch(64, 64, 256) == (32, 8, 128, 32, 256, 4)                    # the 64-px level: 32 workgroups x 4 trips
    assert R.torgb_launch(10, 254, 64) == (8, 32, 20, 5, 160, 4) and R.torgb_launch(10, 30, 512) == (64, 4, 19, 5, 20, 4)
    assert R.torgb_launch(258, 256, 512) == (64, 4, 4128, 1024, 4096, 5) and R.torgb_launch(256, 256, 512) == (64, 4, 4096, 1024, 4096, 4)
    assert R.torgb_walk(6, 10, 256)[0, 3] == [4, 4] and R.torgb_walk(6, 10, 256)[0, 4] == [4, 3] and R.torgb_walk(2, 2, 64)[0, 4] == []
    assert R.rgb_launch(1, 1) == (1, 1, 1, 1) and R.rgb_launch(8, 32) == (1, 1, 8, 32) and R.rgb_launch(9, 33) == (2, 2, 1, 1)
    assert R.rgb_launch(17, 70) == (3, 3, 1, 6) and R.rgb_launch(128, 2048) == (16, 64, 8, 32)


@pytest.mark.parametrize("c", R.TORGB_C)
def test_every_torgb_case_lands_in_its_regime(c):
    cases = R.torgb_cases(c)
    assert {name for name, _ in cases} == set(R.TORGB_REGIME)
    for name, p in cases:
        reg = R.torgb_regime(p[0], p[1], c)
        assert reg["covered"], (name, p)
        assert R.TORGB_REGIME[name](p, c), (c, name, p, R.torgb_launch(p[0], p[1], c), reg)
        assert ("no skip" in name) == (p[0] % 2 == 1 or p[1] % 2 == 1), (name, p)
    regs = [R.torgb_regime(p[0], p[1], c) for _, p in cases]
    assert set().union(*(r["trips"] for r in regs)) == {1, 2, 3, 4}                     # trip counts 1 to 4; the fifth is the capped case
    assert any(r["ragged_u"] for r in regs) and any(not r["ragged_u"] for r in regs) and any(r["idle_pixel_lanes"] for r in regs)
    assert not any(r["capped"] for r in regs)
    if c < 512:                                                                         # C = 512: a wave is ONE pixel
        assert any(r["uneven_exit_in_wave"] for r in regs) and any(r["uneven_u_in_wave"] for r in regs)
        with_skip = [r for (name, _), r in zip(cases, regs) if "no skip" not in name]
        # ... and where the skip taps are read.  A skip needs hw % 4 == 0, so the live tails change at a multiple of 4 pixel lanes: inside a wave only at C = 64
        assert any(r["uneven_u_in_wave"] for r in with_skip) == (c == 64)


def test_the_capped_torgb_case_makes_a_fifth_trip():
    name, c, (h, w) = R.TORGB_CAP_CASE
    assert R.torgb_cap_regime_ok(), R.torgb_launch(h, w, c)
    assert R.torgb_launch(h, w, c)[3:] == (R.TORGB_CAP, R.TORGB_CAP * 4, 5) and h % 2 == 0 and w % 2 == 0
    assert set(R.TORGB_CAP_STORAGES) >= {R.F16, R.MX}
    for cc, (hh, ww) in R.TORGB_CHAIN:
        assert cc in R.TORGB_C and hh % 2 == 0 and ww % 2 == 0
    assert [p for _, p in R.TORGB_CHAIN] == [(4, 6), (8, 12), (16, 24)] and [cc for cc, _ in R.TORGB_CHAIN] == [512, 512, 256]


def test_every_conv_rgb_case_lands_in_its_regime():
    assert {name for name, _ in R.CONV_RGB_CASES} == set(R.CONV_RGB_REGIME)
    for name, p in R.CONV_RGB_CASES:
        assert R.CONV_RGB_REGIME[name](p), (name, p, R.rgb_launch(p[1], p[2]))
    assert set(R.CONV_RGB_ACTS) == {R.ACT_NONE, R.ACT_TANH} and set(R.CONV_RGB_REQUESTS) == {(True, True), (True, False), (False, True)}
    # every storage has an instantiation of its own or shares the template with a different staging type: four kernels, and the two blocked ones walk both halves
    assert len({R.rgb_instantiation(s)[0] for s in R.STORAGES}) == 4
    assert [R.rgb_instantiation(s)[1] for s in (R.SPLIT, R.MX)] == [2, 2]


def test_references_agree_with_torch_in_fp64():
    r = np.random.default_rng(5)
    for n, h2, w2 in ((2, 1, 1), (1, 1, 4), (2, 3, 1), (3, 5, 7), (1, 2, 2)):
        img = r.standard_normal((n, h2, w2, 4))
        want = F.interpolate(torch.from_numpy(img).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
        assert np.abs(R.up2(img) - want).max() <= 1e-12
    a, b, wa, wb = R.up2_axis(3)
    assert a.tolist() == [0, 0, 0, 1, 1, 2] and b.tolist() == [1, 1, 1, 2, 2, 2] and wa.tolist() == [1.0, 0.75, 0.25, 0.75, 0.25, 0.75] and (wa + wb == 1).all()
    for n, h, w in ((1, 1, 1), (2, 9, 33), (2, 4, 7)):
        x, wgt, bias = r.standard_normal((n, h, w, 64)), r.standard_normal((3, 3, 3, 64)), r.standard_normal(3)
        conv = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wgt).permute(0, 3, 1, 2), torch.from_numpy(bias), padding=1).permute(0, 2, 3, 1)
        for act, want in ((R.ACT_NONE, conv), (R.ACT_TANH, torch.tanh(conv))):
            ref, pre, mag = R.conv_rgb_ref(x, wgt, bias, act)
            assert np.abs(ref - want.numpy()).max() <= 1e-12 * max(1.0, np.abs(want.numpy()).max()) and (mag >= np.abs(pre)).all()
    n, h, w, c = 3, 4, 6, 64
    x, wgt, style, sb, bias = r.standard_normal((n, h, w, c)), r.standard_normal((3, c)) / 8, r.standard_normal((n, c)), r.standard_normal(n), r.standard_normal(4)
    skip = r.standard_normal((n, h // 2, w // 2, 4))
    tx = torch.from_numpy(x * style[:, None, None, :]).permute(0, 3, 1, 2)
    conv = F.conv2d(tx, torch.from_numpy(wgt).reshape(3, c, 1, 1)) * torch.from_numpy(sb).reshape(n, 1, 1, 1) + torch.from_numpy(bias[:3]).reshape(1, 3, 1, 1)
    up = F.interpolate(torch.from_numpy(skip[..., :3]).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
    for sk, want in ((None, torch.tanh(conv)), (skip, torch.tanh(conv + up))):
        ref, pre, mag = R.torgb_ref(x, wgt, style, sb, bias, sk)
        assert np.abs(ref - want.permute(0, 2, 3, 1).numpy()).max() <= 1e-12 and (mag >= np.abs(pre)).all()
    ref1, _, _ = R.torgb_ref(x, wgt, style, None, bias, None)
    assert np.abs(ref1 - R.torgb_ref(x, wgt, style, np.ones(n), bias, None)[0]).max() == 0.0


def _tanh_share(ref):
    return float((np.abs(ref) < 0.9).mean())


@pytest.mark.parametrize("storage", R.STORAGES)
def test_tanh_stays_out_of_saturation(storage):
    """a condition on the inputs, not a measurement of the kernels: in every tanh case at least 95 % of the reference outputs have |ref| < 0.9"""
    for c in R.TORGB_C:
        for name, (h, w) in R.torgb_cases(c):
            d = R.torgb_inputs(c, h, w)
            x64 = R.store(d["x"], storage)[1]
            for skip in ({None, "skip"} if d["skip"] is not None else {None}):
                for sb in (d["scale_b"], None):
                    ref, _, _ = R.torgb_ref(x64, d["wgt"], d["style"], sb, d["bias"], d["skip"] if skip else None)
                    assert _tanh_share(ref) >= 0.95, (c, name, storage, skip, sb is None, _tanh_share(ref))
    for name, (n, h, w) in R.CONV_RGB_CASES:
        d = R.conv_rgb_inputs(n, h, w, storage)
        ref, _, _ = R.conv_rgb_ref(R.store(d["x"], storage)[1], d["wgt"], d["bias"], R.ACT_TANH)
        assert _tanh_share(ref) >= 0.95, (name, storage, _tanh_share(ref))


def test_the_chain_and_the_capped_case_stay_out_of_saturation():
    skip = None
    for c, (h, w) in R.TORGB_CHAIN:
        d = R.torgb_inputs(c, h, w)
        skip4 = None if skip is None else np.concatenate([skip, np.zeros(skip.shape[:-1] + (1,))], axis=-1)
        ref, _, _ = R.torgb_ref(R.store(d["x"], R.MX)[1], d["wgt"], d["style"], d["scale_b"], d["bias"], skip4)
        assert _tanh_share(ref) >= 0.95, (c, h, w, _tanh_share(ref))
        skip = ref
    _, c, (h, w) = R.TORGB_CAP_CASE
    d = R.torgb_inputs(c, h, w, n=1)
    ref, _, _ = R.torgb_ref(R.store(d["x"], R.F16)[1], d["wgt"], d["style"], d["scale_b"], d["bias"], d["skip"])
    assert _tanh_share(ref) >= 0.95, _tanh_share(ref)


def test_the_storages_hold_what_the_inputs_ask_of_them():
    """the blocked storages get blocks of different magnitudes, and the stored values differ from storage to storage (so the reference must use the stored ones)"""
    mag = R.block_magnitudes(512)
    assert mag[::32].tolist()[:4] == [2.0 ** -6, 1.0, 32.0, 2.0 ** -6] and len(set(mag.tolist())) == 3 and set(R.block_magnitudes(64).tolist()) == {2.0 ** -6, 1.0}
    d = R.torgb_inputs(128, 6, 10)
    held = {s: R.store(d["x"], s)[1] for s in R.STORAGES}
    assert np.array_equal(held[R.F32], d["x"].astype(np.float64))
    err = {s: float(np.abs(held[s] - held[R.F32]).max() / np.abs(held[R.F32]).max()) for s in (R.F16, R.SPLIT, R.MX)}
    assert 0 < err[R.SPLIT] < err[R.MX] < err[R.F16] < 2.0 ** -10, err
    assert d["skip"] is not None and np.abs(d["skip"][..., 3]).min() >= 1e4 and len({tuple(r) for r in d["style"].tolist()}) == 3 and (d["scale_b"] < 0).sum() == 1


def test_the_references_discriminate():
    """each perturbation of a subtly wrong kernel moves the reference by more than 100 x the GPU tier's bound at some output element"""
    c, (h, w) = 256, (6, 10)
    d = R.torgb_inputs(c, h, w)
    x64 = R.store(d["x"], R.MX)[1]
    ref, _, mag = R.torgb_ref(x64, d["wgt"], d["style"], d["scale_b"], d["bias"], d["skip"])
    bound = R.BOUND * (mag + 1.0)
    swapped = d["wgt"].copy()
    swapped[:, [3, 4]] = swapped[:, [4, 3]]                                             # two channels' weights, in one 8-channel lane
    across = d["wgt"].copy()
    across[:, [5, 37]] = across[:, [37, 5]]                                             # ... and across two 32-channel blocks
    moved = {"weights of channels 3 and 4 swapped": R.torgb_ref(x64, swapped, d["style"], d["scale_b"], d["bias"], d["skip"])[0],
             "weights of channels 5 and 37 swapped": R.torgb_ref(x64, across, d["style"], d["scale_b"], d["bias"], d["skip"])[0],
             "a skip tap one pixel further": R.torgb_ref(x64, d["wgt"], d["style"], d["scale_b"], d["bias"], d["skip"], shift=1)[0],
             "0.25 / 0.75 swapped": R.torgb_ref(x64, d["wgt"], d["style"], d["scale_b"], d["bias"], d["skip"], swap=True)[0],
             "skip channel 3 added to channel 2": R.torgb_ref(x64, d["wgt"], d["style"], d["scale_b"], d["bias"], d["skip"][..., [0, 1, 3, 3]])[0],
             "scale_b ignored": R.torgb_ref(x64, d["wgt"], d["style"], None, d["bias"], d["skip"])[0]}
    for what, other in moved.items():
        assert float((np.abs(other - ref) / bound).max()) > 100.0, ("torgb", what, float((np.abs(other - ref) / bound).max()))
    n, hh, ww = 2, 9, 33
    for storage in (R.F16, R.SPLIT):
        e = R.conv_rgb_inputs(n, hh, ww, storage)
        x64 = R.store(e["x"], storage)[1]
        for act in R.CONV_RGB_ACTS:
            ref, _, mag = R.conv_rgb_ref(x64, e["wgt"], e["bias"], act)
            bound = R.BOUND * (mag + 1.0)
            swapped = e["wgt"].copy()
            swapped[..., [3, 4]] = swapped[..., [4, 3]]
            halves = e["wgt"].copy()
            halves[..., [5, 37]] = halves[..., [37, 5]]
            moved = {"weights of channels 3 and 4 swapped": R.conv_rgb_ref(x64, swapped, e["bias"], act)[0],
                     "weights of channels 5 and 37 swapped": R.conv_rgb_ref(x64, halves, e["bias"], act)[0],
                     "the centre tap one pixel further": R.conv_rgb_ref(x64, e["wgt"], e["bias"], act, tap_shift=(1, 1))[0],
                     "a corner tap one pixel further": R.conv_rgb_ref(x64, e["wgt"], e["bias"], act, tap_shift=(2, 2))[0]}
            for what, other in moved.items():
                assert float((np.abs(other - ref) / bound).max()) > 100.0, ("conv3x3_rgb", storage, act, what, float((np.abs(other - ref) / bound).max()))
