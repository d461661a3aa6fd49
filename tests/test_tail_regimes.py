"""No device: every case of tests/test_tail_kernels_gpu.py lands in the launch regime it names (tests/tail_regimes.py mirrors the host arithmetic of
aux_kernels.hip / ops.py), and the mirrored constants are still the ones the sources hold — so a change to a grid cap, a run length or the slice rule
fails here instead of quietly turning a multi-trip case into a single-trip one."""
import os
import re

import pytest

from tests import tail_regimes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def _body(src, start, end):
    a = src.index(start)
    return src[a:src.index(end, a)]


def test_mirrored_constants_are_the_sources():
    hip = _src("marconet_amd", "csrc", "aux_kernels.hip")
    ops = _src("marconet_amd", "ops.py")
    assert re.search(r"#define MNET_UPS_RUN %d\b" % R.UPS_RUN, hip)
    ups = _body(hip, 'extern "C" int mnet_upsample2x_convert_nhwc', "MNET_LAUNCH_CHECK")
    assert "(per + 255) / 256 < %d ? (per + 255) / 256 : %d" % (R.UPS_CAP, R.UPS_CAP) in ups
    assert "(h + MNET_UPS_RUN - 1) / MNET_UPS_RUN) * w * (c / N)" in ups
    assert "(NWG & 7u) == 0u" in hip and "id += gridDim.x * 256u" in hip
    assert "slices = max(1, min(%d, (h * w) // 512))" % R.GN_SLICE_CAP in ops
    assert "const int per = (HW + slices - 1) / slices;" in hip
    aff = _body(hip, "static void affine_act_launch", "MNET_LAUNCH_CHECK")
    assert "(c / N >= 128 ? 2 : 1)" in aff and "(per + 256 * ppt - 1) / (256 * ppt)" in aff
    flag = _body(hip, 'extern "C" int mnet_nonfinite_flag', "MNET_LAUNCH_CHECK")
    assert "(nv + 255) / 256 < %d ?" % R.FLAG_CAP in flag and ": %d);" % R.FLAG_CAP in flag
    conv = _body(hip, 'extern "C" int mnet_convert', "MNET_LAUNCH_CHECK")
    assert "(n8 + 255) / 256 < %d ? (n8 + 255) / 256 : %d" % (R.CONVERT_CAP, R.CONVERT_CAP) in conv
    sr = _body(hip, 'extern "C" int mnet_sr_postprocess', "MNET_LAUNCH_CHECK")
    assert "(npix + 255) / 256 < %d ? (npix + 255) / 256 : %d" % (R.SR_CAP, R.SR_CAP) in sr
    fba = _body(hip, 'extern "C" int mnet_fused_bias_act', "MNET_LAUNCH_CHECK")
    assert "(total + 255) / 256 < %d ? (total + 255) / 256 : %d" % (R.FBA_CAP, R.FBA_CAP) in fba


def test_launch_mirrors_on_known_shapes():
    """the mirrors against launches worked out by hand from the sources"""
    assert R.ups_launch(8, 9, 12, 64, R.MX) == (3 * 12 * 8, 2, 1, True)              # the first shape of test_round6_gpu.py: 16 workgroups
    assert R.ups_launch(3, 13, 5, 64, R.MX) == (4 * 5 * 8, 1, 1, False)
    assert R.ups_launch(1, 32, 512, 256, R.F32)[:3] == (8 * 512 * 64, 1024, 1)
    assert R.ups_launch(1, 128, 2048, 64, R.F16)[:3] == (32 * 2048 * 8, 2048, 1) and R.ups_launch(1, 132, 2048, 64, R.F16)[2] == 2
    assert [R.gn_slices(*hw) for hw in ((16, 40), (6, 10), (32, 32), (32, 64), (32, 512), (128, 512), (128, 2048))] == [1, 1, 2, 4, 32, 128, 128]
    assert R.gn_launch(32, 512, 1024, R.F32) == (32, 512, 512, 1) and R.gn_launch(1, 1025, 64, R.F16) == (2, 513, 512, 32)
    assert R.affine_ppt(512, R.F32) == 2 and R.affine_ppt(256, R.F32) == 1 and R.affine_ppt(1024, R.MX) == 2 and R.affine_ppt(512, R.F16) == 1
    assert R.affine_launch(45, 1024, R.MX) == (5760, 2, 12, 128)                      # "11 workgroups of 512 + a quarter" (test_round6_gpu.py)
    assert R.flag_launch(7, R.F16) == (0, 1, 0, 7) and R.flag_launch(4096 * 256 * 4, R.F32) == (4096 * 256, 4096, 1, 0)
    assert R.flag_launch(4096 * 256 * 4 + 5, R.F32) == (4096 * 256 + 1, 4096, 2, 1)
    assert R.convert_launch(8) == (1, 1, 1) and R.convert_launch(16384 * 256 * 8) == (16384 * 256, 16384, 1) and R.convert_launch(16384 * 256 * 8 + 8)[2] == 2
    assert R.sr_launch(65536 * 256) == (65536, 1) and R.sr_launch(65536 * 256 + 1) == (65536, 2)
    assert R.fba_launch(16384 * 256) == (16384, 1) and R.fba_launch(16384 * 256 + 1) == (16384, 2)


def test_the_shortest_last_slice_the_rule_allows():
    """HW = q * s + r with s = min(128, HW // 512) slices: per = q + 1 (r > 0) and the last slice holds q + r - s + 1 pixels — never empty, since
    q >= 512 > s; the shortest share of a full slice is q = 512, r = 1, s = 128: 386 of 513 pixels, at HW = 65537"""
    ratio, hw = R.gn_shortest_last_slice()
    assert hw == 65537 and ratio == 386 / 513
    assert R.gn_launch(1, 65537, 32, R.F16)[:3] == (128, 513, 386)
    for hw in range(512, 1 << 17, 37):
        s, per, last, _ = R.gn_launch(1, hw, 32, R.F16)
        assert 0 < last <= per and per * (s - 1) + last == hw


@pytest.mark.parametrize("dtype", R.STORAGES)
def test_every_case_lands_in_its_regime(dtype):
    if dtype in (R.F32, R.F16):
        sizes = R.flag_sizes(dtype)
        assert {name for name, _ in sizes} == set(R.FLAG_REGIME)
        for name, numel in sizes:
            assert R.FLAG_REGIME[name](numel, dtype), ("nonfinite_flag", name, numel, R.flag_launch(numel, dtype))
        assert {numel % R.vec_n(dtype) for _, numel in sizes} == {0, 1, R.vec_n(dtype) - 1}
    for name, p in R.GN_CASES + [R.GN_BATCH_CASE]:
        assert R.GN_REGIME[name](p, dtype), ("groupnorm_affine", name, p, R.gn_launch(p[1], p[2], p[3], dtype))
        assert p[4] is None or len(p[4]) == p[0]
    assert {name for name, _ in R.GN_CASES} == set(R.GN_REGIME)
    assert {p[3] for _, p in R.GN_CASES} == {32, 64, 256, 1024}
    ragged = [v for _, p in R.GN_CASES if p[4] for v in zip(p[4], [p[2]] * len(p[4]))]
    assert any(v == 1 for v, w in ragged) and any(v == w for v, w in ragged) and any(1 < v < w for v, w in ragged) and any(p[4] is None for _, p in R.GN_CASES)
    for name, p in R.UPS_CASES:
        assert R.UPS_REGIME[name](p, dtype), ("upsample2x", name, p, R.ups_launch(*p, dtype))
    assert R.UPS_REGIME[R.UPS_CAP_CASE[0]](R.UPS_CAP_CASE[1][dtype], dtype), ("upsample2x", R.UPS_CAP_CASE[1][dtype], R.ups_launch(*R.UPS_CAP_CASE[1][dtype], dtype))
    assert {name for name, _ in R.UPS_CASES} | {R.UPS_CAP_CASE[0]} == set(R.UPS_REGIME)
    for name, p in R.AFFINE_CASES[dtype]:
        assert R.AFFINE_REGIME[name](p, dtype), ("affine_act", name, p, R.affine_launch(p[1][0] * p[1][1], p[2], dtype))
    assert {name for name, _ in R.AFFINE_CASES[dtype]} == set(R.AFFINE_REGIME)


def test_flat_kernel_cases_pass_their_caps():
    assert R.convert_regime_ok(), R.convert_launch(R.CONVERT_COUNT)
    assert R.sr_regime_ok() and R.fba_regime_ok()
    assert {c for _, p in R.AFFINE_CASES[R.F32] for c in (p[2],)} >= {512, 1024}          # the fp32 two-chunk form at both widths that reach it
