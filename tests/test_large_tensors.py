"""not-gpu: where in memory an element lies — the table of tests/large_tensors.py crosses the wrap points it claims, every size guard of the launchers
refuses exactly from its stated value, and the planner's LDS-DMA / register-staged boundary sits at the address-range limits the header states.
Everything here is answered before any HIP call (placeholder addresses, as tests/test_abi.py and tests/test_upfold_f32z.py do): a refused value answers
MNET_E_ARG with the guard's message; the last accepted value is shown to be past the guard by the message of a LATER check, never by launching."""
import ctypes
import os
import re

import pytest

from tests import large_tensors as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 20                  # a 128-byte aligned placeholder address: checked for presence and alignment, never dereferenced


def _lib():
    from marconet_amd import _lib
    return _lib, _lib.load()


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def test_image_size_divides_no_wrap_point():
    assert L.E == 3 << 20 and all(h * w * c == L.E and (h * w) % 32 == 0 and w % 16 == 0 and (h * w) % 512 == 0 for h, w, c in L.SHAPES.values())
    for s in (2, 4):
        for name, off in L.wrap_points(s).items():
            assert off % L.E != 0 and off % (L.SMALL[0] * L.SMALL[1] * L.SMALL[2]) != 0, (s, name)
    assert L.wrap_points(4) == {"W1": 1 << 29, "W2": 1 << 30, "W3": 1 << 31} and L.wrap_points(2) == {"W1": 1 << 30, "W2": 1 << 31, "W3": 1 << 31}
    # the images the issue names: 170, 341, 682 at s = 4; 341, 682 at s = 2; two whole images beyond W3
    assert {k: v[0] for k, v in L.wrap_images(L.N, L.E, 4).items()} == {"W1": 170, "W2": 341, "W3": 682}
    assert {k: v[0] for k, v in L.wrap_images(L.N, L.E, 2).items()} == {"W1": 341, "W2": 682, "W3": 682}
    assert (L.N - 2) * L.E > 1 << 31 and (L.N - 3) * L.E < 1 << 31
    assert abs(L.N * L.E * 4 / L.GIB - 8.03) < 0.01 and abs(L.N * L.E * 2 / L.GIB - 4.01) < 0.01


def test_every_row_crosses_what_it_claims_strictly_inside_an_image():
    rows = L.rows()
    assert len(rows) == len(L.CONV) + len(L.STREAM)
    for name, tensors in rows.items():
        ns = {n for n, e, s in tensors.values()}
        assert len(ns) == 1, name                                              # one batch: the slots of the tensors are the same images
        for tname, (n, e, s) in tensors.items():
            for wname, (img, inside) in L.wrap_images(n, e, s).items():
                assert 0 < inside < e and 0 < img < n - 1, (name, tname, wname)     # strictly inside an image that has both neighbours
        assert max(len(L.crossed(n, e, s)) for n, e, s in tensors.values()) >= 2, name     # at least one tensor beyond 2^32 bytes / 2^31 elements
    for name in L.CONV:
        t, claims = L.conv_tensors(name), L.conv_claims(name)
        assert set(t) == set(claims), name
        for tname, (n, e, s) in t.items():
            got = L.crossed(n, e, s)
            want = claims[tname]
            if s == 2:                                                         # W2 and W3 are one offset at s = 2 (2^31 elements = 2^32 bytes)
                assert got == ("W1", "W2", "W3") and want == ("W2", "W3"), (name, tname)
            else:
                assert got == want, (name, tname, got)
    # the rows whose input is smaller than the output say so
    assert L.crossed(*L.conv_tensors("mx-shuffle2")["x0"]) == ("W1",)
    assert L.crossed(*L.STREAM["upsample2x-mx"]["src"]) == ("W1",) and L.crossed(*L.STREAM["upsample2x-f16"]["src"]) == ()
    # many small images: a 512-pixel tile touches four images and the per-tile base n_first * img0 passes 2^32 bytes in the 4-byte storages
    h, w, c = L.SMALL
    assert 512 // (h * w) + 2 == 4 and (L.N_SMALL - 4) * h * w * c * 4 > 1 << 32 and L.N_SMALL * h * w * c > 1 << 31


def test_probe_slots_are_what_the_definition_gives():
    assert sorted(L.tensor_slots(L.N, L.E, 4)) == [0, 169, 170, 171, 340, 341, 342, 681, 682, 683, 684]
    assert sorted(L.tensor_slots(L.N, L.E, 2)) == [0, 340, 341, 342, 681, 682, 683, 684]
    for name, tensors in L.rows().items():
        slots = L.probe_slots(tensors)
        n = next(iter(tensors.values()))[0]
        want = {0, n - 1}
        for _, e, s in tensors.values():
            for off in L.wrap_points(s).values():
                if off < n * e:
                    want |= {off // e - 1, off // e, off // e + 1}
        assert slots == sorted(want) and slots[0] == 0 and slots[-1] == n - 1 and len(slots) <= 32, name
    # a quarter-size input adds its own wrap image: W1 of the shuffle row's x lies in image 682
    assert 682 in L.tensor_slots(*L.conv_tensors("mx-shuffle2")["x0"])
    two = L.probe_slots(L.conv_tensors("mx-dma16-256-two"))
    assert {340, 341, 342, 681, 682, 683} <= set(two)                          # x0 / x1 (E / 2 per image): W1 in image 341, W2 in image 682


def test_a_32_bit_address_product_goes_wrong_inside_a_probed_slot():
    """the reading of the table behind the GPU tier: whichever 32-bit form a hand-written product takes — a signed or an unsigned byte offset, a signed
    element offset, of an element or of an image's base — on whichever tensor of whichever row, the first image it gets wrong is a probe slot, so
    assertion (a) sees it (and (b) the filler slots behind it).  Two mutations spelled out: the fp16+8 epilogue's store offset (size_t)pix * cout * 4 as
    (int) on the cout-64 LDS-DMA row, and upsample2x's destination base (size_t)n * 4 * H * W * C as (int)"""
    for name, tensors in L.rows().items():
        slots = set(L.probe_slots(tensors))
        for tname, (n, e, s) in tensors.items():
            for product in ("int bytes", "unsigned bytes", "int elements"):
                for base in (False, True):
                    img = L.first_wrapped_image(n, e, s, product, base)
                    assert img is None or img in slots, (name, tname, product, base, img)
    # (int)pix * cout * 4 with cout = 64: negative from pixel 2^23 on, which lies in image 170 (of 96 x 512 pixels) — the image of W1 of y
    n, e, s = L.conv_tensors("mx-dma13-64")["y"]
    assert (1 << 31) // (64 * 4) == 1 << 23 and (1 << 23) // (96 * 512) == 170 == L.first_wrapped_image(n, e, s, "int bytes")
    assert {169, 170, 171} <= set(L.probe_slots(L.conv_tensors("mx-dma13-64")))
    # (int)n * 4 * H * W * C: images 683 and 684 get a negative base — the neighbour of W3's image and the last image, both probed
    n, e, s = L.STREAM["upsample2x-mx"]["dst"]
    assert L.first_wrapped_image(n, e, s, "int elements", True) == 683 and 683 * e >= 1 << 31 > 682 * e
    assert {683, 684} <= set(L.probe_slots(L.STREAM["upsample2x-mx"]))


def test_no_row_needs_more_than_32_gib():
    worst = max(L.rows().items(), key=lambda kv: L.need_bytes(kv[1]))
    assert L.need_bytes(worst[1]) <= L.LIMIT, worst[0]
    conv = max(L.need_bytes(t) for name, t in L.rows().items() if name.startswith("conv/"))
    assert abs(conv / L.GIB - 24.08) < 0.1                                     # x + y + residual of a 4-byte conv row
    assert worst[0].startswith("stream/glyph_scatter_affine") and L.need_bytes(worst[1]) / L.GIB < 28.1      # four tensors; the fold's z + y: 26.1 GiB


# ---- guards at their boundaries -------------------------------------------------------------------------------------------------------------
def _desc(dtype, n, h, w, c0, cout, k=1, stride=1, pad=0):
    from marconet_amd import _lib
    d = _lib.ConvDesc()
    d.dtype = dtype
    d.x0 = d.wgt = d.y = A
    d.n, d.h, d.w = n, h, w
    d.ho, d.wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    d.c0, d.cout, d.kh, d.kw = c0, cout, k, k
    d.stride_h = d.stride_w = stride
    d.pad_h = d.pad_w = pad
    return d


@pytest.mark.parametrize("which", ["output", "input"])
def test_conv_too_many_pixels(which):
    """n * ho * wo == 2^31 (a padded 1x1: the output is the larger map) and n * h * w == 2^31 (stride 2: the input is) are refused by the planner and by
    the launch entry alike; one image fewer is planned (the register-staged kernel: 64-bit offsets, no further limit) and a pinned LDS-DMA request then
    fails a LATER check"""
    _l, lib = _lib()
    geo = dict(h=254, w=254, pad=1) if which == "output" else dict(h=256, w=256, stride=2)
    d = _desc(0, 32768, c0=8, cout=4, **geo)
    assert (d.n * d.ho * d.wo == 1 << 31 and d.n * d.h * d.w < 1 << 31) if which == "output" else (d.n * d.h * d.w == 1 << 31 and d.n * d.ho * d.wo < 1 << 31)
    assert lib.mnet_conv2d_plan(ctypes.byref(d), 0) == -1 and b"conv: too many pixels" in lib.mnet_last_error()
    assert lib.mnet_conv2d_nhwc_ex(ctypes.byref(d), 0, None) == -1 and b"conv: too many pixels" in lib.mnet_last_error()
    d = _desc(0, 32767, c0=8, cout=4, **geo)
    assert lib.mnet_conv2d_plan(ctypes.byref(d), 0) == _l.ALGO_REG_STAGED
    assert lib.mnet_conv2d_plan(ctypes.byref(d), _l.ALGO_DMA_CFG0) == -1 and b"too many pixels" not in lib.mnet_last_error() and b"LDS-DMA" in lib.mnet_last_error()


def _streaming_guards():
    """name -> (function, arguments as a function of the guarded value, the guard's message, the later check's (return code, message))"""
    P = A + 4                                                                   # 4-byte aligned only
    return {
        "nchw_to_nhwc": ("mnet_nchw_to_nhwc", lambda n: (A, A, 7, n, 8, 1, 1, 8, None), b"nchw_to_nhwc: grid too large", (-1, b"bad dtype")),
        "nhwc_to_nchw": ("mnet_nhwc_to_nchw", lambda n: (A, 7, A, n, 8, 1, 1, 8, None), b"nhwc_to_nchw: grid too large", (-1, b"bad dtype")),
        "upsample2x": ("mnet_upsample2x_convert_nhwc", lambda n: (A, 7, A, 7, n, 1, 1, 8, None, None), b"upsample2x: bad args", (-1, b"bad dtype")),
        "groupnorm_affine": ("mnet_groupnorm_affine", lambda n: (A, 7, n, 1, 1, 32, None, A, A, 1e-6, A, 1, A, A, None), b"groupnorm: bad geometry", (-1, b"bad dtype")),
        "groupnorm_affine_from_partial": ("mnet_groupnorm_affine_from_partial", lambda n: (P, n, 1, 32, 32, None, A, A, 1e-6, A, A, None),
                                          b"groupnorm_from_partial: bad geometry", (-2, b"8-byte aligned")),
        "groupnorm_affine_from_partial_ring": ("mnet_groupnorm_affine_from_partial_ring", lambda n: (P, A, n, 1, 128, 32, A, A, 1e-6, A, A, None),
                                               b"groupnorm_from_partial_ring: bad geometry", (-2, b"8-byte aligned")),
        "affine_act": ("mnet_affine_act_nhwc", lambda n: (A, A, 7, n, 1, 32, A, None, 0, None), b"affine_act: bad args", (-1, b"bad dtype")),
        "torgb": ("mnet_torgb", lambda n: (A, 7, n, 1, 1, 64, A, A, None, A, None, A, None), b"torgb: bad args", (-1, b"bad dtype")),
        "conv3x3_rgb": ("mnet_conv3x3_rgb", lambda n: (A, 7, n, 1, 1, 64, A, A, 0, A, None, None), b"conv3x3_rgb: bad args", (-1, b"bad dtype")),
        "polyphase_ring_fix": ("mnet_polyphase_ring_fix", lambda n: (A, A, A, A, A, 3, n, 8, 1 << 28, 32, A, None), b"polyphase_ring_fix: bad geometry",
                               (-1, b"map too large")),
        "demod": ("mnet_demod", lambda n: (A, A, A, n, 16388, 64, None), b"demod: bad args", (-1, b"too large")),
        "scatter": ("mnet_glyph_scatter_affine", lambda n: (A, A, A, A, 1, n, 65536 * 8, 32, 32, A, A, A, None), b"scatter: too many images", (-1, b"S too large")),
        "adain_split": ("mnet_adain_crop_concat_split", lambda n: (A, A, A, 7, n, 32, 32, 32, A, A, A, A, None, None, 0.0, None, None, A, A, 1, None),
                        b"adain_split: bad geometry", (-1, b"bad dtype")),
    }


@pytest.mark.parametrize("name", sorted(_streaming_guards()))
def test_grid_limit_at_65536(name):
    """n (B for the scatter, G for adain_split) is a grid dimension: 65536 is refused with the launcher's own message, 65535 passes that check"""
    _l, lib = _lib()
    fn, args, msg, (later_rc, later_msg) = _streaming_guards()[name]
    f = getattr(lib, fn)
    assert f(*args(65536)) == -1 and msg in lib.mnet_last_error(), lib.mnet_last_error()
    assert f(*args(65535)) == later_rc and later_msg in lib.mnet_last_error() and msg not in lib.mnet_last_error(), lib.mnet_last_error()


@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
def test_upsample2x_image_too_large(dtype):
    """h * w * (c / N) * 4 == 2^31 (N channels per 16-byte chunk: 4 in fp32, 8 in the three others) is refused; one row fewer is past the guard (a later
    check, the alignment of src, answers)"""
    _l, lib = _lib()
    c, per = 32, 32 // (4 if dtype == 0 else 8)
    w = 1 << 14
    h = (1 << 29) // (w * per)
    assert h * w * per * 4 == 1 << 31
    f = lib.mnet_upsample2x_convert_nhwc
    assert f(A, dtype, A, dtype, 1, h, w, c, None, None) == -1 and b"upsample2x: image too large" in lib.mnet_last_error()
    assert f(A + 4, dtype, A, dtype, 1, h - 1, w, c, None, None) == -2 and b"upsample2x" in lib.mnet_last_error() and b"too large" not in lib.mnet_last_error()
    if dtype >= 2:                                                             # into f16: the same limit (the chunk count is the source's)
        assert f(A, dtype, A, 1, 1, h, w, c, None, None) == -1 and b"upsample2x: image too large" in lib.mnet_last_error()


@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
def test_affine_act_image_too_large(dtype):
    """hw * (c / N) == 2^31 is refused, one pixel fewer is past the guard (the alignment check answers)"""
    _l, lib = _lib()
    c, per = 32, 32 // (4 if dtype == 0 else 8)
    hw = (1 << 31) // per
    f = lib.mnet_affine_act_nhwc
    assert f(A, A, dtype, 1, hw, c, A, None, 0, None) == -1 and b"affine_act: image too large" in lib.mnet_last_error()
    assert f(A + 4, A, dtype, 1, hw - 1, c, A, None, 0, None) == -2 and b"affine_act" in lib.mnet_last_error() and b"too large" not in lib.mnet_last_error()


# ---- the planner at the address-range limits --------------------------------------------------------------------------------------------------
_LIMITS = [("mx", 3, 64, (2047, 2048), (2048, 2048), 13), ("mx", 3, 96, (1365, 2048), (1366, 2048), 13), ("f16", 1, 64, (2047, 2048), (2048, 2048), 5)]


def _formula(h, w, phys):
    return 2 * h * w < 1 << 23, 2 * h * w * phys * 2 < (1 << 31) - 1


@pytest.mark.parametrize("storage,dtype,c0,ok,bad,pin", _LIMITS, ids=["%s-c%d" % (r[0], r[2]) for r in _LIMITS])
def test_planner_at_the_activation_address_limits(storage, dtype, c0, ok, bad, pin):
    _l, lib = _lib()
    phys = c0 * (1 if storage == "f16" else 2)
    binds = {("mx", 64): (False, False), ("mx", 96): (True, False), ("f16", 64): (False, True)}[(storage, c0)]      # (24-bit holds, 31-bit holds) past the limit
    assert _formula(*ok, phys) == (True, True) and _formula(*bad, phys) == binds and L.dma_limit_ok(*ok, phys) and not L.dma_limit_ok(*bad, phys)
    plan = lambda hw, algo, n=2: lib.mnet_conv2d_plan(ctypes.byref(_desc(dtype, n, hw[0], hw[1], c0, 64, k=3, pad=1)), algo)
    strips = [_l.ALGO_STRIP_CFG0 + i for i in range(3)]
    for n in (1, 2, 3):                                                        # the batch does not enter
        k = plan(ok, _l.ALGO_AUTO, n)
        assert k >= _l.ALGO_DMA_CFG0 and k != _l.ALGO_REG_STAGED, k
        assert plan(ok, _l.ALGO_DMA_CFG0 + pin, n) == _l.ALGO_DMA_CFG0 + pin
        assert plan(bad, _l.ALGO_AUTO, n) == _l.ALGO_REG_STAGED
        assert plan(bad, _l.ALGO_DMA_CFG16, n) == -1 and b"not eligible" in lib.mnet_last_error()          # a pinned LDS-DMA id (16 has a build for both storages)
        assert plan(bad, _l.ALGO_DMA_CFG0 + pin, n) == -1 and b"LDS-DMA" in lib.mnet_last_error()
        assert plan(bad, _l.ALGO_LDS_DMA, n) == -1
        for s in strips:
            assert plan(bad, s, n) == -1, s
    if c0 == 64:                                                               # whole-row tiles of a 2048-wide map: the eligible side takes the 64x512 strip tile
        assert plan(ok, _l.ALGO_AUTO) == _l.ALGO_STRIP_CFG0 + 1 == plan(ok, _l.ALGO_STRIP_CFG0 + 1)
    # the maps of section 4 of the GPU tier: the largest h * w the formula accepts that is no multiple of 512, and one row past it
    row = L.LARGEST[(storage, c0)]
    assert row["phys"] == phys and L.dma_limit_ok(*row["ok"], phys) and not L.dma_limit_ok(*row["past"], phys) and (row["ok"][0] * row["ok"][1]) % 512 != 0
    hw = row["ok"][0] * row["ok"][1]
    assert not L.dma_limit_ok(1, hw + 1, phys)                                 # h * w is the largest the formula accepts at all
    assert _l.ALGO_DMA_CFG0 <= plan(row["ok"], _l.ALGO_AUTO) < _l.ALGO_STRIP_CFG0 and plan(row["past"], _l.ALGO_AUTO) == _l.ALGO_REG_STAGED


def test_planner_at_the_weight_address_limits():
    """256 * K * 2 < 2^30 and cout * K * 2 < 2^31 - 1, K = kh * kw * cin in halves (f16: 32 taps, two sources so that the activation bounds stay far away)"""
    _l, lib = _lib()

    def plan(c0, c1, cout, algo):
        d = _desc(1, 1, 32, 64, c0, cout)
        d.kh, d.kw, d.pad_h, d.pad_w = 4, 8, 0, 0
        d.ho, d.wo = 32 - 4 + 1, 64 - 8 + 1
        d.x1, d.c1 = A, c1
        return lib.mnet_conv2d_plan(ctypes.byref(d), algo)

    pin = _l.ALGO_DMA_CFG0 + 3
    # 256 * K * 2 == 2^30 at K = 2^21
    assert 256 * 32 * (32768 + 32768) * 2 == 1 << 30
    assert plan(32768, 32768, 64, _l.ALGO_AUTO) == _l.ALGO_REG_STAGED
    assert plan(32768, 32768, 64, pin) == -1 and b"LDS-DMA" in lib.mnet_last_error()
    assert plan(32768, 32768 - 64, 64, _l.ALGO_AUTO) >= _l.ALGO_DMA_CFG0 and plan(32768, 32768 - 64, 64, pin) == pin
    # cout * K * 2 >= 2^31 - 1 at cout = 1024, K = 2^20; cout = 1016 is inside
    assert 1024 * 32 * 32768 * 2 == 1 << 31 and 1016 * 32 * 32768 * 2 < (1 << 31) - 1
    assert plan(16384, 16384, 1024, _l.ALGO_AUTO) == _l.ALGO_REG_STAGED
    assert plan(16384, 16384, 1024, _l.ALGO_DMA_CFG0 + 1) == -1 and b"LDS-DMA" in lib.mnet_last_error()
    assert plan(16384, 16384, 1016, _l.ALGO_AUTO) >= _l.ALGO_DMA_CFG0 and plan(16384, 16384, 1016, _l.ALGO_DMA_CFG0 + 1) == _l.ALGO_DMA_CFG0 + 1


def test_header_states_the_address_range_limits():
    src = open(os.path.join(ROOT, "include", "marconet_hip.h")).read()
    m = re.search(r"Address range of the LDS-DMA and strip kernels(.*?)MNET_CONV_ALGO_DMA_CFG0 \+ id pins", src, flags=re.S)
    assert m, "the eligibility list says nothing about the address range"
    text = " ".join(m.group(1).split())
    for phrase in ("I = 512 / (h * w) + 2", "I * h * w < 2^23", "I * h * w * P * 2 < 2^31 - 1", "cout * K * 2 < 2^31 - 1", "256 * K * 2 < 2^30",
                   "twice that for MNET_F16X2 / MNET_F16M", "n * h * w < 2^31", "n * ho * wo < 2^31", "MNET_CONV_ALGO_REG_STAGED"):
        assert phrase in text, phrase
    assert re.search(r"#define MNET_ABI_VERSION 4\b", src)
