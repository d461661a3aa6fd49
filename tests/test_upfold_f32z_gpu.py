"""-m gpu: the tap planes of the tap-conv + fold form in fp32 — the one-wave tile's fp32-output build (MNET_CONV_ALGO_FLAG_F32_OUT, conv_dma_w4_f32.hip), the fold
with z in fp32 and y in fp16+8 (mnet_upfold3x3_f32z_nhwc, upfold_kernel<float, hm>), and the generator with both.

Conv: exact.  The fp32 value is by construction the value the fp16+8 build encodes, so mxfmt.pack_act(fp32 output) equals the fp16+8 output byte for byte.
Fold: tests/tail_regimes.py's 20 cases and its two-trip case, against the fp64 fold of the fp32 planes under the fp16+8 bound of tests/test_upfold_gpu.py.
Generator: the priors against the oracle on the trained-like regime, table in test_generator_priors_with_fp32_planes_on_the_trained_like_regime."""
import functools

import numpy as np
import pytest
import torch

from oracle import marconet_oracle as O
from tests import storage_codec as SC
from tests import tail_regimes as R
from tests import test_upfold_gpu as U
from tests.test_kernels_gpu import MX, _check, _tol
from tests.test_upfold import epilogue_ref, fold_input, fold_ref, fold_ref_banded

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 512


def _ops():
    from marconet_amd import ops
    return ops


def _P():
    from marconet_amd import packing
    return packing


def _guarded(shape, dtype):
    """a tensor of 4-byte elements between GUARD bytes of 0xA5 on each side → (whole byte buffer, tensor)"""
    nbytes = int(np.prod(shape)) * 4
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, _P().tag(buf[GUARD:GUARD + nbytes].view(dtype).reshape(shape))


def _guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all().item()) and bool((buf[-GUARD:] == 0xA5).all().item())


def _untouched(buf):
    return bool((buf == 0xA5).all().item())


# ================================================================================================================== the conv, exact
# (n, h, w, cin, cout): 1x1 with one k-slab and with three; cout 288 = a second channel tile with 32 live channels, 576 = a third with 64; 32 pixels = one partial
# tile, 288 = a full and a partial one; 33 maps of 32x32 with cout 288 = 264 tiles: a second trip of the persistent grid
CONV_CASES = [(1, 4, 8, 32, 288), (1, 4, 8, 96, 576), (1, 9, 32, 32, 576), (1, 9, 32, 96, 288), (33, 32, 32, 32, 288)]
CONV_IDS = ["%dx%dx%dx%dx%d" % c for c in CONV_CASES]
SPECIAL_PAGES = ("zero_hi", "neg_zero", "subnormal_blocks", "zeros", "gaussian")


def _conv_operands(case, seed):
    """x [n,h,w,cin] fp32 whose 32-channel blocks cycle through storage_codec's pages (blocks whose every hi is +-0, signed zeros, fp16-subnormal blocks, ...) and
    Gaussian blocks; weights [cout,cin,1,1]: output channels 0-31 copy input block 0 (so the OUTPUT holds fp16-subnormal and all-zero blocks too), channels 32-63
    its negation, channels 64-95 the copy times 2^-8 (the fp16-subnormal inputs become output blocks whose every hi is +-0 while v != 0), the rest Gaussian"""
    n, h, w, cin, cout = case
    g = torch.Generator().manual_seed(seed)
    pages = {p["name"]: p["v"] for p in SC.writer_pages()}
    special = torch.from_numpy(np.concatenate([pages[k].reshape(8, 32) for k in SPECIAL_PAGES]).astype(np.float32))      # [40, 32]
    npix, nb = n * h * w, cin // 32
    x = torch.randn((npix, nb, 32), generator=g)
    take = torch.arange(npix * nb).reshape(npix, nb)
    sel = (take % 3) != 2                                                  # two blocks in three from the pages, one Gaussian
    x[sel] = special[(take[sel] * 7) % special.shape[0]]
    wgt = torch.randn((cout, cin, 1, 1), generator=g) * (cin ** -0.5)
    wgt[:96] = 0.0
    wgt[torch.arange(32), torch.arange(32)] = 1.0
    wgt[32 + torch.arange(32), torch.arange(32)] = -1.0
    wgt[64 + torch.arange(32), torch.arange(32)] = 2.0 ** -8
    return x.reshape(n, h, w, cin), wgt


@pytest.mark.parametrize("case", CONV_CASES, ids=CONV_IDS)
def test_fp32_output_is_the_value_the_fp16_8_build_encodes(case):
    from marconet_amd import _lib, mxfmt
    ops, P = _ops(), _P()
    n, h, w, cin, cout = case
    x, wgt = _conv_operands(case, 700 + cin + cout)
    xd = P.from_float(x, P.MX_DTYPE).to(DEV)
    wd = P.pack_conv_weight(wgt.to(DEV), P.MX_DTYPE)
    one_wave = _lib.ALGO_DMA_CFG16
    assert ops.conv_plan(xd, cout, 1, 1, algo=one_wave) == one_wave and ops.conv_plan(xd, cout, 1, 1, algo=one_wave | _lib.ALGO_FLAG_F32_OUT) == one_wave
    buf32, y32 = _guarded((n, h, w, cout), torch.float32)
    bufm, ym = _guarded((n, h, w, cout), P.MX_DTYPE)
    assert ops.conv2d(xd, wd, cout, 1, 1, out=y32, algo=one_wave, out_f32=True) is y32
    ops.conv2d(xd, wd, cout, 1, 1, out=ym, algo=one_wave)
    torch.cuda.synchronize()
    assert _guards_intact(buf32) and _guards_intact(bufm), "guard bytes around y were written"
    v = y32.cpu()
    assert bool(torch.isfinite(v).all())
    want = mxfmt.pack_act(v).reshape(-1)
    got = P.untag(ym).contiguous().cpu().view(torch.uint8).reshape(-1)
    bad = (want != got).nonzero().reshape(-1)
    assert bad.numel() == 0, "%d bytes differ, first at byte %d (pixel %d, byte %d of its row)" % (bad.numel(), int(bad[0]), int(bad[0]) // (cout * 4), int(bad[0]) % (cout * 4))
    # the case is what it is there for: the OUTPUT has fp16-subnormal blocks (channels 0-31), blocks whose every hi is +-0 while v != 0 (channels 64-95) and all-zero blocks
    hmax = lambda b: b.half().float().abs().amax(-1)
    b0, b2 = v[..., :32].reshape(-1, 32), v[..., 64:96].reshape(-1, 32)
    assert bool(((hmax(b0) > 0) & (hmax(b0) < 2.0 ** -14)).any()) and bool(((hmax(b2) == 0) & (b2.abs().amax(-1) > 0)).any()) and bool((b0.abs().amax(-1) == 0).any())
    # AUTO names the same build whatever the launch size
    buf_auto, y_auto = _guarded((n, h, w, cout), torch.float32)
    ops.conv2d(xd, wd, cout, 1, 1, out=y_auto, out_f32=True)
    torch.cuda.synchronize()
    assert torch.equal(y_auto.cpu().view(torch.int32), v.view(torch.int32)) and _guards_intact(buf_auto)


def test_fp32_output_refusals_enqueue_nothing():
    """any epilogue term, another storage, a launch the planner gives to another tile: MarconetHipError before any HIP call, y keeps its bytes"""
    from marconet_amd import _lib
    ops, P = _ops(), _P()
    case = (2, 8, 8, 64, 288)
    n, h, w, cin, cout = case
    x, wgt = _conv_operands(case, 720)
    xd = P.from_float(x, P.MX_DTYPE).to(DEV)
    wd = P.pack_conv_weight(wgt.to(DEV), P.MX_DTYPE)
    buf, y = _guarded((n, h, w, cout), torch.float32)
    vec_c, vec_nc = torch.ones(cout, device=DEV), torch.ones((n, cout), device=DEV)
    res = P.new_tensor((n, h, w, cout), P.MX_DTYPE, DEV, zero=True)
    refused = [dict(bias=vec_c), dict(out_scale=vec_nc), dict(post_scale=vec_nc), dict(residual=res), dict(gn_partial=ops.gn_partial_buffer(n, h, w, cout, DEV)),
               dict(valid_w=torch.full((n,), w, dtype=torch.int32, device=DEV)), dict(act=ops.ACT_LRELU), dict(act=ops.ACT_LRELU_SQRT2), dict(act=ops.ACT_RELU),
               dict(algo=_lib.ALGO_DMA_CFG0 + 15), dict(algo=_lib.ALGO_DMA_CFG0 + 10), dict(algo=_lib.ALGO_REG_STAGED), dict(shuffle2=True)]
    for kw in refused:
        with pytest.raises((_lib.MarconetHipError, RuntimeError)):
            ops.conv2d(xd, wd, cout, 1, 1, out=y, out_f32=True, **kw)
    # a map whose 32-pixel fragments straddle images: the one-wave tile hands it to the 8-wave tile, which has no such build
    x6 = P.new_tensor((2, 6, 6, cin), P.MX_DTYPE, DEV, zero=True)
    with pytest.raises(_lib.MarconetHipError, match="one-wave"):
        ops.conv2d(x6, wd, cout, 1, 1, out=y.reshape(-1)[:2 * 36 * cout].view(2, 6, 6, cout), out_f32=True)
    # other storages
    for dt in (P.SPLIT_DTYPE, torch.float16, torch.float32):
        xo = P.new_tensor((n, h, w, cin), dt, DEV, zero=True)
        wo = P.pack_conv_weight(wgt.to(DEV), dt)
        with pytest.raises(_lib.MarconetHipError, match="MNET_F16M"):
            ops.conv2d(xo, wo, cout, 1, 1, out=y, out_f32=True)
    # the wrapper wants an fp32 out
    with pytest.raises(RuntimeError):
        ops.conv2d(xd, wd, cout, 1, 1, out=P.new_tensor((n, h, w, cout), P.MX_DTYPE, DEV), out_f32=True)
    torch.cuda.synchronize()
    assert _untouched(buf)


# ================================================================================================================== the fold
UPF_IDS = U.UPF_IDS


def _z_guarded(z32, p):
    """fp32 z [n,h,w,9c] → the same values on the device between 0xFF bytes (NaN) of at least one low-res row + two pixels on each side, 128-byte aligned"""
    n, h, w, c = p
    guard = -(-((w + 2) * 9 * c * 4) // 128) * 128
    buf = torch.full((z32.numel() + 2 * (guard // 4),), float("nan"), dtype=torch.float32, device=DEV)
    buf.view(torch.uint8).fill_(0xFF)
    view = buf[guard // 4:guard // 4 + z32.numel()]
    view.copy_(z32.reshape(-1))
    z = view.view(n, h, w, 9 * c)
    assert z.data_ptr() % 128 == 0
    return buf, z


@functools.lru_cache(maxsize=4)
def _operands(p):
    """→ (fp32 z on the host, fp64 sums [n,c,2h,2w] of its values, the three vectors): computed once per case"""
    z = fold_input(p, 600, R.upf_z_scale(p))
    return z, fold_ref(U._nchw(z).double().contiguous(), p[3]), U._vectors(p[0], p[3], 601)


def _compare(name, got, ref, ybuf, guard):
    assert not bool(torch.isnan(got).any()), "%s: NaN in y — the kernel read a guard byte around z or a vector" % name
    ratio = (got.double() - ref).abs().max().item() / (_tol(MX) * max(ref.abs().max().item(), 1e-6))
    print("upfold f32z %s: error / bound %.3f" % (name, ratio))
    _check(name, got, ref, MX, extra=1.0)
    assert U._y_guards_intact(ybuf, guard), "%s: guard bytes around y were written" % name


def _run_small(regime, p, mixes, act):
    ops = _ops()
    z32, sums, vec = _operands(tuple(p))
    zbuf, z = _z_guarded(z32, p)
    for absent in mixes:
        v = dict(zip(U.ALL3, vec))
        for k in absent:
            v[k] = None
        ybuf, guard, y = U._y_guarded(p, R.MX)
        r = ops.upfold3x3(z, p[3], act=act, out=y, **{k: U._vec_guarded(None if t is None else t.to(DEV)) for k, t in v.items()})
        torch.cuda.synchronize()
        assert r is y
        ref = epilogue_ref(sums, v["out_scale"], v["bias"], act, v["post_scale"])
        _compare("%s %s act %d without %s" % (regime, p, act, "+".join(absent) or "nothing"), U._nchw(U._host(y)), ref, ybuf, guard)


@pytest.mark.parametrize("case", R.UPF_CASES, ids=UPF_IDS)
def test_fold_of_fp32_planes_matches_fp64_in_every_launch_regime(case):
    """upfold_kernel<float, hm>: the regimes of upfold_kernel<hm> (same thread map, same grid: the fp16+8 launch arithmetic)"""
    regime, p = case
    assert R.UPF_REGIME[regime](p, R.MX), (regime, R.upf_launch(*p, R.MX), R.upf_runs(p[1]))
    _run_small(regime, p, U.MIXES_REMAP if regime.startswith("several workgroups") else U.MIXES, _ops().ACT_LRELU_SQRT2)


@pytest.mark.parametrize("act", [0, 2, 3])
def test_fold_of_fp32_planes_activation_arms(act):
    regime, p = R.UPF_CASES[10]                                                 # three runs, remap off
    assert R.UPF_REGIME[regime](p, R.MX)
    _run_small(regime, p, [()], act)


def test_fold_of_fp32_planes_second_grid_stride_trip():
    """tests/test_upfold_gpu.py::test_fold_second_grid_stride_trip with z as fp32 (151 MB); the source is the one that test draws"""
    ops = _ops()
    regime, shapes = R.UPF_CAP_CASE
    p = shapes[R.MX]
    assert R.UPF_REGIME[regime](p, R.MX), R.upf_launch(*p, R.MX)
    n, h, w, c = p
    src = U._cap_source(p)
    sums = fold_ref_banded(U._nchw(src).double().contiguous(), c, 8200)
    zbuf, z = _z_guarded(src, p)
    vec = U._vectors(n, c, 621)
    for absent in U.MIXES:
        v = dict(zip(U.ALL3, vec))
        for k in absent:
            v[k] = None
        ybuf, guard, y = U._y_guarded(p, R.MX)
        ops.upfold3x3(z, c, act=ops.ACT_LRELU_SQRT2, out=y, **{k: U._vec_guarded(None if t is None else t.to(DEV)) for k, t in v.items()})
        torch.cuda.synchronize()
        got = ops.convert(y, torch.float32).float().cpu()
        ref = epilogue_ref(sums, v["out_scale"], v["bias"], 3, v["post_scale"])
        first2 = R.UPF_CAP * R.WG // (c // R.vec_n(R.MX))                      # the second trip's items: hi-res columns first2 ... of both rows of the run
        e2 = (U._nchw(got).double() - ref)[:, :, :, first2:].abs().max().item()
        assert first2 < 2 * w and e2 <= _tol(MX) * ref.abs().max().item(), "second trip (hi-res columns %d ...): %.3e" % (first2, e2)
        _compare("%s %s without %s" % (regime, p, "+".join(absent) or "nothing"), U._nchw(got), ref, ybuf, guard)
        del got, ref, y, ybuf


@pytest.mark.parametrize("case", U.BATCH_CASES, ids=["remap_on_in_the_batch_only", "three_runs"])
def test_one_glyph_alone_gives_its_batch_bytes_with_fp32_planes(case):
    ops, P = _ops(), _P()
    regime, p = case
    n, h, w, c = p
    assert R.UPF_REGIME[regime](p, R.MX) and not R.upf_launch(1, h, w, c, R.MX)[3]
    z32, _, (os_, bs, ps) = _operands(tuple(p))
    zd = z32.to(DEV)
    raw = lambda t: P.untag(t).contiguous().cpu().view(torch.uint8)
    kw = dict(bias=bs.to(DEV), act=ops.ACT_LRELU_SQRT2, out_dtype=P.MX_DTYPE)
    yb = ops.upfold3x3(zd, c, out_scale=os_.to(DEV), post_scale=ps.to(DEV), **kw)
    assert yb.dtype == P.MX_DTYPE
    for i in (0, 1, n - 1):
        y1 = ops.upfold3x3(zd[i:i + 1].contiguous(), c, out_scale=os_[i:i + 1].contiguous().to(DEV), post_scale=ps[i:i + 1].contiguous().to(DEV), **kw)
        torch.cuda.synchronize()
        assert torch.equal(raw(yb[i:i + 1]), raw(y1)), "image %d of %s" % (i, p)


def test_fold_of_fp32_planes_refusals_enqueue_nothing():
    from marconet_amd import _lib
    ops, P = _ops(), _P()
    n, h, w, c = 2, 4, 4, 32
    zd = fold_input((n, h, w, c), 640).to(DEV)
    ybuf, guard, y = U._y_guarded((n, h, w, c), R.MX)
    odd = torch.zeros(c + 4, device=DEV)[1:1 + c]
    for kw in (dict(act=ops.ACT_TANH), dict(act=ops.ACT_RELU), dict(bias=odd)):
        with pytest.raises(_lib.MarconetHipError):
            ops.upfold3x3(zd, c, out=y, **kw)
    with pytest.raises(RuntimeError):
        ops.upfold3x3(zd, c + 32, out=y)
    for dt in (P.SPLIT_DTYPE, torch.float16):                                   # fp32 planes fold into fp16+8 only
        with pytest.raises(RuntimeError):
            ops.upfold3x3(zd, c, out_dtype=dt)
    with pytest.raises(RuntimeError):                                           # ... and only fp32 planes do
        ops.upfold3x3(zd.half(), c, out=y)
    torch.cuda.synchronize()
    assert bool((ybuf == 0xA5).all().item())
    # without out / out_dtype an fp32 z keeps the same-storage entry point: fp32 y
    assert ops.upfold3x3(zd, c).dtype == torch.float32


# ================================================================================================================== the generator
@pytest.fixture(scope="module")
def trained_like(harness_weights):
    from marconet_amd import checkpoints
    sde, sdg, sds, _ = harness_weights["trained_like"]
    _, gan, _ = checkpoints.build_networks(sde, sdg, sds, DEV)
    return gan.TextGenerator, sdg


def prior_errors(tg, sdg, seed, monkeypatch):
    """forward_nhwc(need_image=False, precision="fp16x2") on make_styles(seed, 6) / make_labels(seed + 1, 6) with the tap planes in fp32 ("f32") and under the knob
    networks._UPFOLD_HM_Z ("hm") → {form: (fp32-output conv launches, prior64 error, prior32 error)}, (max |prior64|, max |prior32|) of the oracle"""
    from marconet_amd import networks, ops, synthetic
    styles, labels = synthetic.make_styles(seed, 6), synthetic.make_labels(seed + 1, 6)
    ref = O.tspgan_forward(sdg, styles, labels)
    sd, ld = styles.to(DEV).float().contiguous(), labels.to(DEV).long().contiguous()
    out = {}
    for form, knob in (("f32", False), ("hm", True)):
        calls = {"f32": 0, "fold": 0}
        conv, fold = ops.conv2d, ops.upfold3x3

        def conv_counted(*a, **k):
            calls["f32"] += 1 if k.get("out_f32") else 0
            return conv(*a, **k)

        def fold_counted(z, *a, **k):
            calls["fold"] += 1
            assert (z.dtype == torch.float32) == (not knob)
            return fold(z, *a, **k)

        with monkeypatch.context() as m:
            m.setattr(ops, "conv2d", conv_counted)
            m.setattr(ops, "upfold3x3", fold_counted)
            m.setattr(networks, "_UPFOLD_HM_Z", knob)
            with torch.no_grad(), ops.on_device(sd):
                img, p64, p32 = tg.forward_nhwc(sd, ld, need_image=False, precision="fp16x2")
                p64, p32 = ops.nhwc_to_nchw(p64), ops.nhwc_to_nchw(p32)
            torch.cuda.synchronize()
        assert img is None and calls["fold"] == 2
        out[form] = (calls["f32"], (p64.cpu() - ref[1]).abs().max().item(), (p32.cpu() - ref[2]).abs().max().item())
    return out, (float(ref[1].abs().max()), float(ref[2].abs().max()))


def test_generator_priors_with_fp32_planes_on_the_trained_like_regime(trained_like, monkeypatch):
    """forward_nhwc in the fp16x2 mode's own arithmetic with the tap planes in fp32 (as shipped) and in fp16+8 (MNET_UPFOLD_HM_Z=1), both priors against the oracle.

    Max-abs errors against the oracle, trained-like weights, 6 glyphs, styles / labels seeds s / s + 1 (the "fp16+8" columns are the parent's form: the "fold"
    columns of tests/test_regimes_gpu.py::test_generator_fp16x2_arithmetic_on_the_trained_like_regime):
        seed   prior64 fp32 planes  fp16+8 planes    prior32 fp32 planes  fp16+8 planes      max |prior64|  max |prior32|
        91     2.208e-4             2.208e-4         2.098e-4             2.190e-4           7.06           6.06
        92     2.191e-4             2.470e-4         2.126e-4             2.187e-4           6.64           7.45
        93     2.708e-4             2.736e-4         2.541e-4             2.763e-4           6.96           7.97
    (measured on an MI355X.)  The fp16+8 columns reproduce the parent's table digit for digit: the knob runs the parent's kernels.  With fp32 planes every error is
    equal or lower — one rounding of Z less.
    Bar: 1e-3 x max(1, max |p|), the north star's, for both forms.  The test runs seed 91."""
    tg, sdg = trained_like
    errs, (m64, m32) = prior_errors(tg, sdg, 91, monkeypatch)
    for form in ("f32", "hm"):
        print("trained_like gan fp16x2 tap planes %-3s fp32-output launches %d  prior64 %.3e (|p| max %.2f)  prior32 %.3e (|p| max %.2f)"
              % ((form,) + errs[form][:2] + (m64, errs[form][2], m32)))
    assert errs["f32"][0] == 2 and errs["hm"][0] == 0                             # 16→32 and 32→64 write fp32 planes; the knob keeps fp16+8
    for form in ("f32", "hm"):
        assert errs[form][1] <= 1e-3 * max(1.0, m64), (form, errs[form])
        assert errs[form][2] <= 1e-3 * max(1.0, m32), (form, errs[form])
