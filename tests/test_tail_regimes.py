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


# ====================================================================================================================== upfold3x3
def test_upfold_mirrored_constants_are_the_sources():
    hip = _src("marconet_amd", "csrc", "upfold_kernels.hip")
    assert re.search(r"#define MNET_UPF_RUN %d\b" % R.UPF_RUN, hip) and R.UPF_RUN == 8
    upf = _body(hip, 'extern "C" int mnet_upfold3x3_nhwc', "MNET_LAUNCH_CHECK")
    assert "((h + MNET_UPF_RUN - 1) / MNET_UPF_RUN) * 2 * w * (c / N)" in upf
    assert "(per + 255) / 256 < %d ? (per + 255) / 256 : %d" % (R.UPF_CAP, R.UPF_CAP) in upf and "dim3(gx, n), dim3(256)" in upf
    assert "(long long)h * w * (c / N) * 4 < (1ll << 31) && (long long)w * 9 * c < (1ll << 29)" in upf
    assert "(NWG & 7u) == 0u" in hip and "id < items_per_image; id += gridDim.x * 256u" in hip
    assert "y0 = (int)(col / (unsigned)W2) * R, y1 = min(y0 + R, H)" in hip


def test_upfold_launch_mirror_on_known_shapes():
    """worked out by hand from the launcher"""
    assert R.upf_launch(2, 9, 6, 256, R.MX) == (2 * 12 * 32, 3, 1, False)             # two runs x 12 hi-res columns x 32 chunks: three workgroups per image
    assert R.upf_launch(2, 16, 16, 256, R.MX) == (2 * 32 * 32, 8, 1, True)            # the generator's 16 -> 32 level, two glyphs
    assert R.upf_launch(1, 32, 32, 256, R.MX) == (4 * 64 * 32, 32, 1, True)
    assert R.upf_launch(3, 5, 7, 64, R.F32) == (14 * 16, 1, 1, False)
    assert R.upf_launch(1, 8, 8192, 32, R.F16)[:3] == (16384 * 4, 256, 1)
    assert R.upf_launch(1, 2, 65536, 32, R.MX)[:3] == (2048 * 256, 2048, 1) and R.upf_launch(1, 2, 65537, 32, R.MX)[:3] == (2048 * 256 + 8, 2048, 2)
    assert [R.upf_runs(h) for h in (1, 7, 8, 9, 16, 17, 24)] == [(1, 1), (1, 7), (1, 8), (2, 1), (2, 8), (3, 1), (3, 8)]


@pytest.mark.parametrize("dtype", R.STORAGES)
def test_every_upfold_case_lands_in_its_regime(dtype):
    for name, p in R.UPF_CASES:
        assert R.UPF_REGIME[name](p, dtype), ("upfold3x3", name, p, R.upf_launch(*p, dtype), R.upf_runs(p[1]))
        assert R.upf_guards_ok(*p, dtype) and p[3] % 32 == 0
    name, shapes = R.UPF_CAP_CASE
    p = shapes[dtype]
    per, gx, trips, remap = R.upf_launch(*p, dtype)
    assert R.UPF_REGIME[name](p, dtype), ("upfold3x3", name, p, (per, gx, trips, remap))
    assert per == 524800 and 0 < per - gx * R.WG < gx * R.WG and remap            # a partial second trip, (gx * 1) % 8 == 0
    assert p[2] * 9 * p[3] < 1 << 29 and p[1] * p[2] * (p[3] // R.vec_n(dtype)) * 4 < 1 << 31
    assert {name for name, _ in R.UPF_CASES} | {R.UPF_CAP_CASE[0]} == set(R.UPF_REGIME)
    hs = [p[1] for nm, p in R.UPF_CASES if nm.startswith("H%8=")]
    assert sorted(h % 8 for h in hs) == list(range(8)) and {p[0] for nm, p in R.UPF_CASES if nm.startswith("H%8=")} == {3, 8}
    assert [p[1] for nm, p in R.UPF_CASES if nm == "three runs"] == [17, 24] and [p[1] for nm, p in R.UPF_CASES if nm == "one run, H<8"] == [1, 2, 3, 7]
    # the remap is on and off among the cases with several runs, and on in a case where the image alone has it off (the batch-invariance test)
    assert any(R.upf_launch(*p, dtype)[3] and not R.upf_launch(1, *p[1:], dtype)[3] for _, p in R.UPF_CASES)


HEADROOM = {}


@pytest.mark.parametrize("dtype", R.STORAGES)
def test_upfold_reference_headroom(dtype):
    """what the bound of tests/test_kernels_gpu._check leaves to the kernel: fold_ref's formula evaluated in fp32 on the stored values and rounded ONCE to
    the storage by the host packer lies within half the storage's bound (relative to max |ref|) of the fp64 fold_ref, on every small case with the
    seed and the input scale the GPU tier uses — a kernel that sums in fp32 and rounds once has the other half for its own order of sums"""
    import torch
    from marconet_amd import packing as P
    from tests.test_kernels_gpu import _tol, ALL_DTYPES
    from tests.test_upfold import fold_f32, fold_input, fold_ref
    tag = ALL_DTYPES[R.STORAGES.index(dtype)]
    sdt = {R.F32: torch.float32, R.F16: torch.float16, R.SPLIT: P.SPLIT_DTYPE, R.MX: P.MX_DTYPE}[dtype]
    worst = 0.0
    for name, p in dict((p, (nm, p)) for nm, p in R.UPF_CASES).values():
        zv = P.to_float(P.from_float(fold_input(p, 600, R.upf_z_scale(p)), sdt))                              # the values the storage holds, NHWC
        z = zv.permute(0, 3, 1, 2).contiguous()
        ref = fold_ref(z.double(), p[3])
        got = P.to_float(P.from_float(fold_f32(z, p[3]).permute(0, 2, 3, 1).contiguous(), sdt)).permute(0, 3, 1, 2).double()
        rel = (got - ref).abs().max().item() / ref.abs().max().item()
        worst = max(worst, rel / _tol(tag))
        assert rel <= 0.5 * _tol(tag), "%s %s %s: fp32 + one rounding is %.3e of max |ref|, bound %.1e" % (dtype, name, p, rel, _tol(tag))
    print("upfold headroom %s: fp32 evaluation + one storage rounding uses at most %.3f of the bound" % (dtype, worst))


def test_upfold_banded_reference_is_the_whole_map_reference():
    """the two-trip map is compared in column bands (tests/test_upfold.fold_ref_banded): bands of 1, 2, 3, 5 columns and one band, with a band that ends at the
    map's edge and one that is a single column, give fold_ref's fp64 values exactly"""
    import torch
    from tests.test_upfold import fold_ref, fold_ref_banded
    for h, w in ((2, 11), (3, 1), (1, 2), (5, 7)):
        z = torch.randn((2, 9 * 4, h, w), generator=torch.Generator().manual_seed(610 + w), dtype=torch.float64)
        whole = fold_ref(z, 4)
        for band in (1, 2, 3, 5, w, w + 3):
            assert torch.equal(fold_ref_banded(z, 4, band), whole), (h, w, band)


def test_upfold_refuses_maps_past_its_index_guards_without_a_device():
    """the launcher's two "image too large" guards (32-bit element offsets inside a low-res row of z; 32-bit item index per image) answer MNET_E_ARG before
    anything is enqueued — fake pointers, as tests/test_upfold.py::test_upfold_refuses_bad_arguments_without_a_device"""
    import ctypes
    from marconet_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 127) // 128 * 128
    z, y = ctypes.c_void_p(a), ctypes.c_void_p(a + 2048)
    f = lib.mnet_upfold3x3_nhwc
    for dt, n_ch in ((0, 4), (1, 8), (2, 8), (3, 8)):                       # MNET_F32, MNET_F16, MNET_F16X2, MNET_F16M
        w_row = (1 << 29) // (9 * 32) + 1                                   # the first width with w * 9 * c >= 2^29 at c = 32
        assert (w_row - 1) * 9 * 32 < 1 << 29 <= w_row * 9 * 32 and 1 * w_row * (32 // n_ch) * 4 < 1 << 31
        assert f(z, y, dt, 1, 1, w_row, 32, None, None, 0, None, None) == -1
        assert b"image too large" in lib.mnet_last_error()
        h_big = (1 << 31) // (65536 * (32 // n_ch) * 4)                     # h * w * (c / N) * 4 == 2^31 exactly at w = 65536: the first refused height
        assert h_big * 65536 * (32 // n_ch) * 4 == 1 << 31 and 65536 * 9 * 32 < 1 << 29
        assert f(z, y, dt, 1, h_big, 65536, 32, None, None, 0, None, None) == -1
        assert b"image too large" in lib.mnet_last_error()
