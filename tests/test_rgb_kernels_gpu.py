"""-m gpu: mnet_torgb and mnet_conv3x3_rgb — the kernels that write the pixels the user sees — against the fp64 references of tests/rgb_kernels.py, on every
storage, in every launch regime of its case tables (the regime is asserted before each launch), into output buffers between guard bands of 0xFF bytes.

Values: |got - ref64| <= 2e-5 * (A + 1) per output element, A the sum of the magnitudes of the terms of that element's pre-activation (tanh is 1-Lipschitz, so the
bound of the pre-activation carries through; the + 1 covers tanhf itself); conv3x3_rgb's f16 NHWC output adds 2^-11 * |ref| for its one f16 rounding.  Bytes: the
padding channels, the two outputs of conv3x3_rgb against each other, the three output requests, scale_b = NULL against ones, image i of a batch against its own
launch.  The overflow rule of include/marconet_hip.h: a pre-activation that is not finite is stored as NaN (fp32 conv3x3_rgb: +-1), and nothing else changes.
Refused launches leave the output untouched.

rgb_kernels.json in the report directory holds error / bound of every case.  Largest margins measured on an MI355X (error / bound; 1 would be the bound):
    torgb, the case table      fp32 0.0023    f16 0.0026    split 0.0030    mx 0.0024
    torgb, the capped case     fp32 0.0013    f16 0.0013    split 0.0013    mx 0.0014      (258 x 256 x 512, n = 1: 0.53 s, 0.48 s, 0.66 s, 0.85 s per test, nearly
                                                                                            all of it the host's packing and fp64 reference)
    torgb chain (worst level)  fp32 0.0009    f16 0.0007    split 0.0012    mx 0.0007
    conv3x3_rgb                fp32 0.0088    f16 0.7252    split 0.0114    mx 0.0084
The f16 figure of conv3x3_rgb is the rounding of the f16 output itself: where 2^-11 |ref| is the larger part of the bound, an error of half an f16 ulp comes
close to it (|ref| = 1, A = 10: 4.9e-4 of 7.1e-4).  The bound is the project's, not tightened towards these figures.  No defect was found in either kernel."""
import json
import os

import numpy as np
import pytest
import torch

from tests import rgb_kernels as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096                  # guard elements before and after every output buffer (a multiple of 128 bytes in fp32 and f16)
REPORT = {"torgb": {}, "torgb_chain": {}, "conv3x3_rgb": {}}


def _ops():
    from marconet_amd import ops
    return ops


def _lib():
    from marconet_amd import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _write_report(report_dir):
    yield
    out = {k: {s: dict(v, largest=max(v.values())) for s, v in d.items() if v} for k, d in REPORT.items()}
    with open(os.path.join(report_dir, "rgb_kernels.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_x(x32, storage):
    """fp32 numpy [n,h,w,c] -> (device tensor in ``storage`` through the HOST packer, the stored values in fp64)"""
    t, x64 = R.store(x32, storage)
    t = t.to(DEV)
    assert t.data_ptr() % 128 == 0
    return t, x64


def _guarded(shape, dtype):
    """-> (the whole buffer, the view of ``shape`` in its middle): every byte 0xFF (NaN in f16 and fp32)"""
    numel = int(np.prod(shape))
    buf = torch.empty(numel + 2 * GUARD, dtype=dtype, device=DEV)
    buf.view(torch.uint8).fill_(0xFF)
    view = buf[GUARD:GUARD + numel].view(shape)
    assert view.data_ptr() % 128 == 0
    return buf, view


def _all_ff(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def _guards_intact(buf):
    return _all_ff(buf[:GUARD]) and _all_ff(buf[-GUARD:])


def _bits(t):
    """host int view of a device fp32 / f16 tensor, for byte comparisons (NaN payloads and signed zeros included)"""
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _torgb(x, c, wgt, style, scale_b, bias, skip, shape=None):
    """one mnet_torgb launch into a guarded buffer -> fp32 [n,h,w,4] on the device; the guards are checked"""
    ops, lib = _ops(), _lib()
    n, h, w = shape if shape is not None else x.shape[:3]
    buf, out = _guarded((n, h, w, 4), torch.float32)
    lib.check(lib.load().mnet_torgb(ops._p(x), ops._dt(x), n, h, w, c, ops._p(wgt), ops._p(style), ops._p(scale_b), ops._p(bias), ops._p(skip), ops._p(out), ops._stream()),
              "mnet_torgb")
    torch.cuda.synchronize()
    assert _guards_intact(buf), "torgb wrote outside its output"
    return out


def _conv_rgb(x, wgt, bias, act, nhwc=True, nchw=True, cin=64):
    """one mnet_conv3x3_rgb launch into guarded buffers -> (y_nhwc or None, y_nchw or None)"""
    ops, lib = _ops(), _lib()
    n, h, w = x.shape[:3]
    odt = torch.float16 if x.dtype == torch.float16 else torch.float32
    b1, y1 = _guarded((n, h, w, 8), odt) if nhwc else (None, None)
    b2, y2 = _guarded((n, 3, h, w), torch.float32) if nchw else (None, None)
    lib.check(lib.load().mnet_conv3x3_rgb(ops._p(x), ops._dt(x), n, h, w, cin, ops._p(wgt), ops._p(bias), act, ops._p(y1), ops._p(y2), ops._stream()), "mnet_conv3x3_rgb")
    torch.cuda.synchronize()
    assert all(_guards_intact(b) for b in (b1, b2) if b is not None), "conv3x3_rgb wrote outside an output"
    return y1, y2


def _margin(got, ref, bound, what):
    """got, ref, bound numpy of one shape -> max error / bound; printed, then asserted <= 1"""
    assert np.isfinite(got).all(), "%s: %d non-finite outputs" % (what, int((~np.isfinite(got)).sum()))
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    m = float(ratio.max())
    if m > 1.0:
        i = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError("%s: error %.3e > bound %.3e at %s (got %.9g, ref %.9g); %d of %d elements beyond the bound"
                             % (what, abs(float(got[i]) - ref[i]), bound[i], i, got[i], ref[i], int((ratio > 1).sum()), ratio.size))
    return m


def _log(kernel, storage, case, m):
    REPORT[kernel].setdefault(storage, {})[case] = round(m, 6)


# ====================================================================================================================== ToRGB: values and bytes
def _torgb_case(c, h, w, storage, n=3):
    d = R.torgb_inputs(c, h, w, n)
    x, x64 = _dev_x(d["x"], storage)
    dev = {k: _dev(d[k]) for k in ("wgt", "style", "scale_b", "bias", "skip")}
    return d, x, x64, dev


@pytest.mark.parametrize("storage", R.STORAGES)
@pytest.mark.parametrize("c", R.TORGB_C)
def test_torgb_values_and_bytes(c, storage):
    """every geometry of the table x (no skip, a skip whose channel 3 is large) x (scale_b given, NULL), n = 3 with distinct style rows and one negative scale_b"""
    ones = torch.ones(3, dtype=torch.float32, device=DEV)
    for name, (h, w) in R.torgb_cases(c):
        assert R.TORGB_REGIME[name]((h, w), c), (name, h, w, c)
        d, x, x64, dev = _torgb_case(c, h, w, storage)
        assert (d["skip"] is None) == ("no skip" in name)
        for skip_name in ((None, "skip") if d["skip"] is not None else (None,)):
            skip, skip_dev = (d["skip"], dev["skip"]) if skip_name else (None, None)
            for sb, sb_dev in ((d["scale_b"], dev["scale_b"]), (None, None)):
                what = "torgb c=%d %dx%d %s %s skip=%s scale_b=%s" % (c, h, w, name, storage, skip_name, sb is not None)
                ref, _, mag = R.torgb_ref(x64, d["wgt"], d["style"], sb, d["bias"], skip)
                out = _torgb(x, c, dev["wgt"], dev["style"], sb_dev, dev["bias"], skip_dev)
                got = out.cpu().numpy()
                m = _margin(got[..., :3], ref, R.BOUND * (mag + 1.0), what)
                print("%-110s margin %.4f" % (what, m))
                _log("torgb", storage, "%d %dx%d skip=%s scale_b=%s" % (c, h, w, skip_name, sb is not None), m)
                assert (_bits(out[..., 3]) == 0).all(), "%s: out[..., 3] is not +0 everywhere" % what
                if sb is None:                                           # NULL is ones, byte for byte
                    assert np.array_equal(_bits(out), _bits(_torgb(x, c, dev["wgt"], dev["style"], ones, dev["bias"], skip_dev))), what
                else:                                                   # image i of the batch == its own launch
                    for i in range(3):
                        alone = _torgb(x[i:i + 1].contiguous(), c, dev["wgt"], dev["style"][i:i + 1].contiguous(), sb_dev[i:i + 1].contiguous(), dev["bias"],
                                       None if skip_dev is None else skip_dev[i:i + 1].contiguous())
                        assert np.array_equal(_bits(alone[0]), _bits(out[i])), "%s: image %d alone differs from image %d of the batch" % (what, i, i)


@pytest.mark.parametrize("storage", R.TORGB_CAP_STORAGES)
def test_torgb_capped_grid_fifth_trip(storage):
    name, c, (h, w) = R.TORGB_CAP_CASE
    assert R.torgb_cap_regime_ok() and R.torgb_launch(h, w, c)[3:] == (R.TORGB_CAP, 4 * R.TORGB_CAP, 5)
    d, x, x64, dev = _torgb_case(c, h, w, storage, n=1)
    ref, _, mag = R.torgb_ref(x64, d["wgt"], d["style"], d["scale_b"], d["bias"], d["skip"])
    out = _torgb(x, c, dev["wgt"], dev["style"], dev["scale_b"], dev["bias"], dev["skip"])
    m = _margin(out.cpu().numpy()[..., :3], ref, R.BOUND * (mag + 1.0), "torgb %s %s" % (name, storage))
    print("torgb %s %s margin %.4f" % (name, storage, m))
    _log("torgb", storage, "capped %d %dx%d" % (c, h, w), m)
    assert (_bits(out[..., 3]) == 0).all()


@pytest.mark.parametrize("storage", R.STORAGES)
def test_torgb_chain_of_three_levels(storage):
    """4 -> 8 -> 16 px as the generator chains them: each level's image is the next level's skip.  Reference: the composed fp64 formula; a level's bound is its own
    plus the largest bound of the level below (the bilinear is a convex combination of the image below, and tanh is 1-Lipschitz)"""
    skip_dev, skip_ref, below = None, None, 0.0
    for level, (c, (h, w)) in enumerate(R.TORGB_CHAIN):
        d, x, x64, dev = _torgb_case(c, h, w, storage)
        skip4 = None if skip_ref is None else np.concatenate([skip_ref, np.zeros(skip_ref.shape[:-1] + (1,))], axis=-1)
        ref, _, mag = R.torgb_ref(x64, d["wgt"], d["style"], d["scale_b"], d["bias"], skip4)
        bound = R.BOUND * (mag + 1.0) + below
        out = _torgb(x, c, dev["wgt"], dev["style"], dev["scale_b"], dev["bias"], skip_dev)
        m = _margin(out.cpu().numpy()[..., :3], ref, bound, "torgb chain level %d %s" % (level, storage))
        print("torgb chain level %d c=%d %dx%d %s margin %.4f" % (level, c, h, w, storage, m))
        _log("torgb_chain", storage, "level %d c=%d %dx%d" % (level, c, h, w), m)
        assert (_bits(out[..., 3]) == 0).all()
        skip_dev, skip_ref, below = out, ref, float(bound.max())


# ====================================================================================================================== conv3x3_rgb: values and bytes
@pytest.mark.parametrize("storage", R.STORAGES)
def test_conv_rgb_values_and_bytes(storage):
    """every shape x act in {NONE, TANH} x the three output requests"""
    for name, (n, h, w) in R.CONV_RGB_CASES:
        assert R.CONV_RGB_REGIME[name]((n, h, w)), (name, n, h, w)
        d = R.conv_rgb_inputs(n, h, w, storage)
        x, x64 = _dev_x(d["x"], storage)
        wgt = _dev(d["wgt"].astype(np.float16) if storage == R.F16 else d["wgt"])
        bias = _dev(d["bias"])
        for act in R.CONV_RGB_ACTS:
            what = "conv3x3_rgb %s %s act %d %s" % ((n, h, w), name, act, storage)
            ref, _, mag = R.conv_rgb_ref(x64, d["wgt"], d["bias"], act)
            bound = R.BOUND * (mag + 1.0) + (R.F16_EPS * np.abs(ref) if storage == R.F16 else 0.0)
            y1, y2 = _conv_rgb(x, wgt, bias, act, True, True)
            assert y1.dtype == (torch.float16 if storage == R.F16 else torch.float32)
            g1 = y1.float().cpu().numpy()
            m = _margin(g1[..., :3], ref, bound, what)
            print("%-100s margin %.4f" % (what, m))
            _log("conv3x3_rgb", storage, "%dx%dx%d act %d" % (n, h, w, act), m)
            assert (_bits(y1[..., 3:]) == 0).all(), "%s: y_nhwc[..., 3:8] is not zero" % what
            # y_nchw holds exactly the values of y_nhwc (in f16: the f16-rounded ones, widened)
            assert np.array_equal(_bits(y2), _bits(y1[..., :3].float().permute(0, 3, 1, 2))), "%s: y_nchw differs from y_nhwc" % what
            only1, none2 = _conv_rgb(x, wgt, bias, act, True, False)
            none1, only2 = _conv_rgb(x, wgt, bias, act, False, True)
            assert none1 is None and none2 is None
            assert np.array_equal(_bits(only1), _bits(y1)), "%s: the NHWC-only request differs" % what
            assert np.array_equal(_bits(only2), _bits(y2)), "%s: the NCHW-only request differs" % what
        if n > 1:                                                       # image i of the batch == its own launch
            y1, y2 = _conv_rgb(x, wgt, bias, R.ACT_TANH, True, True)
            for i in range(n):
                a1, a2 = _conv_rgb(x[i:i + 1].contiguous(), wgt, bias, R.ACT_TANH, True, True)
                assert np.array_equal(_bits(a1[0]), _bits(y1[i])) and np.array_equal(_bits(a2[0]), _bits(y2[i])), "%s: image %d alone differs" % (name, i)


# ====================================================================================================================== the overflow rule
def _same_except(got, base, mask, what):
    """byte-identical to ``base`` wherever ``mask`` is False"""
    diff = (_bits(got) != _bits(base)) & ~mask
    assert not diff.any(), "%s: %d elements outside the planted region changed" % (what, int(diff.sum()))


@pytest.mark.parametrize("storage", (R.F16, R.F32))
def test_torgb_nonfinite_x_element_is_nan_at_its_pixel_only(storage):
    """one inf and, separately, one NaN element of x at an interior pixel and at the last pixel (whose u are ragged): that pixel's RGB is NaN, its channel 3 is 0,
    every other pixel keeps its bytes"""
    c, (h, w) = 128, dict(R.torgb_cases(128))["five workgroups, four trips, ragged u"]
    assert R.torgb_regime(h, w, c)["ragged_u"]
    d = R.torgb_inputs(c, h, w)
    dev = {k: _dev(d[k]) for k in ("wgt", "style", "scale_b", "bias", "skip")}
    base = _torgb(_dev_x(d["x"], storage)[0], c, dev["wgt"], dev["style"], dev["scale_b"], dev["bias"], dev["skip"])
    assert torch.isfinite(base).all()
    for value in (np.inf, -np.inf, np.nan):
        for img, y, xx, ch in ((1, h // 2, w // 2 + 1, 77), (2, h - 1, w - 1, c - 1), (0, 0, 0, 0)):
            x32 = d["x"].copy()
            x32[img, y, xx, ch] = value
            out = _torgb(_dev_x(x32, storage)[0], c, dev["wgt"], dev["style"], dev["scale_b"], dev["bias"], dev["skip"])
            what = "torgb %s x[%d,%d,%d,%d] = %s" % (storage, img, y, xx, ch, value)
            assert torch.isnan(out[img, y, xx, :3]).all(), "%s: the pixel's RGB is %s" % (what, out[img, y, xx].tolist())
            assert (_bits(out[..., 3]) == 0).all(), what
            mask = np.zeros((3, h, w, 4), dtype=bool)
            mask[img, y, xx, :3] = True
            _same_except(out, base, mask, what)


@pytest.mark.parametrize("storage", R.STORAGES)
def test_torgb_overflowing_style_row_is_nan_on_its_image_only(storage):
    """a style row of 3e38 on image 1 of 3 over positive x (>= 2) and positive weights: every product overflows, image 1's RGB is all NaN — not tanh's 1 —
    and images 0 and 2 keep their bytes"""
    c, (h, w) = 256, (6, 10)
    r = np.random.default_rng(77)
    x, _ = _dev_x((np.abs(r.standard_normal((3, h, w, c))) + 2.0).astype(np.float32), storage)
    wgt = _dev(((np.abs(r.standard_normal((3, c))) + 0.5) / c).astype(np.float32))
    style = (np.abs(r.standard_normal((3, c))) + 0.5).astype(np.float32)
    bias, sb = _dev(np.array([0.1, -0.2, 0.3, 0.0], dtype=np.float32)), _dev(R.SCALE_B)
    skip = _dev(R.torgb_inputs(c, h, w)["skip"])
    base = _torgb(x, c, wgt, _dev(style), sb, bias, skip)
    assert torch.isfinite(base).all()
    style[1] = 3e38
    out = _torgb(x, c, wgt, _dev(style), sb, bias, skip)
    assert torch.isnan(out[1, ..., :3]).all(), "torgb %s: %d of image 1's RGB values are not NaN" % (storage, int((~torch.isnan(out[1, ..., :3])).sum()))
    assert (_bits(out[..., 3]) == 0).all()
    assert np.array_equal(_bits(out[0]), _bits(base[0])) and np.array_equal(_bits(out[2]), _bits(base[2]))


def test_conv_rgb_f16_inf_element_is_nan_in_its_neighbourhood_only():
    """one inf element of x (at a corner where four tiles meet, and at the image's last pixel): NaN in exactly the in-image 3 x 3 neighbourhood, in both outputs"""
    n, h, w = 3, 17, 70
    d = R.conv_rgb_inputs(n, h, w, R.F16)
    wgt, bias = _dev(d["wgt"].astype(np.float16)), _dev(d["bias"])
    assert (d["wgt"] != 0).all()
    b1, b2 = _conv_rgb(_dev_x(d["x"], R.F16)[0], wgt, bias, R.ACT_TANH)
    assert torch.isfinite(b1).all() and torch.isfinite(b2).all()
    for img, y, xx, ch in ((1, 8, 32, 5), (2, h - 1, w - 1, 63), (0, 0, 31, 40)):
        x32 = d["x"].copy()
        x32[img, y, xx, ch] = np.inf
        y1, y2 = _conv_rgb(_dev_x(x32, R.F16)[0], wgt, bias, R.ACT_TANH)
        hood = np.zeros((n, h, w), dtype=bool)
        hood[img, max(y - 1, 0):y + 2, max(xx - 1, 0):xx + 2] = True
        what = "conv3x3_rgb f16 x[%d,%d,%d,%d] = inf" % (img, y, xx, ch)
        m1 = np.zeros((n, h, w, 8), dtype=bool)
        m1[..., :3] = hood[..., None]
        m2 = np.broadcast_to(hood[:, None], (n, 3, h, w))
        assert np.array_equal(torch.isnan(y1).cpu().numpy(), m1), "%s: NaN at %d NHWC elements, expected %d" % (what, int(torch.isnan(y1).sum()), int(m1.sum()))
        assert np.array_equal(torch.isnan(y2).cpu().numpy(), m2), "%s: NaN at %d NCHW elements, expected %d" % (what, int(torch.isnan(y2).sum()), int(m2.sum()))
        _same_except(y1, b1, m1, what)
        _same_except(y2, b2, m2, what)


@pytest.mark.parametrize("storage", (R.SPLIT, R.MX, R.F32))
def test_conv_rgb_overflowing_weights_of_one_channel(storage):
    """fp32 weights of 3e38 on output channel 1 only, x positive (>= 2): the pre-activation of channel 1 is +inf everywhere.  Split-half and fp16+8 input: channel 1 is
    NaN everywhere, in both outputs.  fp32 input: exactly +1 — the documented difference.  Channels 0 and 2 keep their bytes"""
    n, h, w = 2, 9, 33
    d = R.conv_rgb_inputs(n, h, w, storage)
    r = np.random.default_rng(78)
    x, _ = _dev_x((np.abs(r.standard_normal((n, h, w, 64))) + 2.0).astype(np.float32), storage)
    wgt = (d["wgt"] * R.block_magnitudes(64) * 0.2).astype(np.float32)
    bias = _dev(d["bias"])
    b1, b2 = _conv_rgb(x, _dev(wgt), bias, R.ACT_TANH)
    assert torch.isfinite(b1).all() and torch.isfinite(b2).all()
    wgt[1] = 3e38
    y1, y2 = _conv_rgb(x, _dev(wgt), bias, R.ACT_TANH)
    if storage == R.F32:
        assert (_bits(y1[..., 1]) == np.float32(1.0).view(np.int32)).all() and (_bits(y2[:, 1]) == np.float32(1.0).view(np.int32)).all()
    else:
        assert torch.isnan(y1[..., 1]).all() and torch.isnan(y2[:, 1]).all(), "conv3x3_rgb %s: an infinite pre-activation was not stored as NaN" % storage
    for o in (0, 2):
        assert np.array_equal(_bits(y1[..., o]), _bits(b1[..., o])) and np.array_equal(_bits(y2[:, o]), _bits(b2[:, o]))
    assert (_bits(y1[..., 3:]) == 0).all()


# ====================================================================================================================== refusals with real buffers
def _refused(call, outs):
    from marconet_amd._lib import MarconetHipError
    with pytest.raises(MarconetHipError):
        call()
    torch.cuda.synchronize()
    assert all(_all_ff(o) for o in outs), "a refused launch wrote to its output"


def test_refused_launches_leave_the_output_untouched():
    ops, lib = _ops(), _lib()
    L = lib.load()

    def torgb(h, w, c, with_skip):
        x = torch.zeros((1, h, w, c), dtype=torch.float16, device=DEV)
        wgt, style, bias = torch.zeros((3, c), device=DEV), torch.ones((1, c), device=DEV), torch.zeros(4, device=DEV)
        skip = torch.zeros((1, max(h // 2, 1), max(w // 2, 1), 4), device=DEV) if with_skip else None
        buf, out = _guarded((1, h, w, 4), torch.float32)
        _refused(lambda: lib.check(L.mnet_torgb(ops._p(x), ops._dt(x), 1, h, w, c, ops._p(wgt), ops._p(style), None, ops._p(bias), ops._p(skip), ops._p(out),
                                                ops._stream()), "mnet_torgb"), [buf])

    torgb(5, 6, 128, True)            # a skip and odd h
    torgb(6, 5, 128, True)            # a skip and odd w
    torgb(4, 4, 96, False)            # no power of two
    torgb(4, 4, 1024, False)          # beyond 512

    def conv(cin, act):
        x = torch.zeros((1, 8, 32, cin), dtype=torch.float32, device=DEV)
        wgt, bias = torch.zeros((3, 3, 3, cin), device=DEV), torch.zeros(3, device=DEV)
        b1, y1 = _guarded((1, 8, 32, 8), torch.float32)
        b2, y2 = _guarded((1, 3, 8, 32), torch.float32)
        _refused(lambda: lib.check(L.mnet_conv3x3_rgb(ops._p(x), ops._dt(x), 1, 8, 32, cin, ops._p(wgt), ops._p(bias), act, ops._p(y1), ops._p(y2), ops._stream()),
                                   "mnet_conv3x3_rgb"), [b1, b2])

    conv(32, R.ACT_TANH)
    conv(64, R.ACT_LRELU)
