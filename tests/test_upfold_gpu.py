"""mnet_upfold3x3_nhwc and the tap-conv + fold form of the generator's up-convs (fp16+8 storage) on the device, against the fp64 statement of
tests/test_upfold.py.

End-to-end bound (check b): the new form's max-abs error against fp64 lrelu√2(d·conv3x3(bilinear_x2(x_stored·s)) + b)·post is compared with the two-launch
form's error on the same stored inputs, e_new <= K_END_TO_END · e_two.  Ratios e_new / e_two measured on an MI355X, seeds 77 / 78 / 79 of every case (both
errors are a few 1e-5 on outputs of magnitude 2: the ratio of two maxima over a few hundred values is noisy on the small maps):
    case 1  (2,1,1,64,32)      0.982  1.704  1.088
    case 2  (1,1,5,64,32)      0.743  1.493  1.965
    case 3  (3,5,7,64,64)      0.932  0.870  1.126
    case 4  (2,4,4,64,32)      1.330  1.024  1.481
    case 5  (2,9,6,64,256)     0.899  0.869  1.299
    case 6  (2,16,16,512,256)  1.108  1.025  1.349
    heavy-tailed (case 6's shape, synthetic "trained"-regime weights, log-uniform style scales over three decades)  1.192  1.123  0.963
K_END_TO_END = the largest of them, 1.965, + 0.25 for the unmeasured seeds.  The test runs seed 77."""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import tail_regimes as R
from tests.test_kernels_gpu import MX, SPLIT, _check, _tol
from tests.test_upfold import epilogue_ref, fold_input, fold_ref, fold_ref_banded

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = int(re.search(r"#define MNET_UPF_RUN (\d+)", open(os.path.join(ROOT, "marconet_amd", "csrc", "upfold_kernels.hip")).read()).group(1))
# (N, h, w, Cin, C)
CASES = [(2, 1, 1, 64, 32),                 # clamp and zero padding meet on every side
         (1, 1, 5, 64, 32),                 # the same on a one-row map
         (3, 5, 7, 64, 64),                 # odd, non-square, two channel blocks
         (2, 4, 4, 64, 32),                 # small square map
         (2, RUN + 1, 6, 64, 256),          # a run boundary (the second run is one row), 2 x 12 x 32 = 768 items: three workgroups per image
         (2, 16, 16, 512, 256)]             # a level's channel counts: the planner accepts
IDS = ["%dx%dx%dx%dx%d" % c for c in CASES]
K_END_TO_END = 1.965 + 0.25                 # see the module docstring


def _ops():
    from marconet_amd import ops
    return ops


def _P():
    from marconet_amd import packing
    return packing


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _store(x_nhwc):
    """fp32 NHWC (cpu) → (fp16+8 tensor on the device, the fp32 values it holds)"""
    s = _P().from_float(x_nhwc.contiguous(), _P().MX_DTYPE)
    return s.to(DEV), _P().to_float(s)


def _host(t):
    return _P().to_float(t.cpu())


def _nchw(v):
    return v.permute(0, 3, 1, 2)


def _vectors(n, c, seed):
    """out_scale [n,c], bias [c], post_scale [n,c]"""
    return _rnd((n, c), seed).abs() + 0.5, _rnd((c,), seed + 1, 0.3), _rnd((n, c), seed + 2).abs() + 0.25


# ------------------------------------------------------------------------------------------------------------------ (a) the fold alone, (c) guards
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fold_alone_matches_fp64(case):
    """a random stored Z through the kernel with all of out_scale / bias / post_scale and with each one absent, against the fp64 fold of the same
    stored values: the bound tests/test_tail_kernels_gpu.py gives affine_act in this storage (one storage rounding on top of fp32 sums).  y sits
    between 0xA5 guard bytes, which stay intact."""
    ops, P = _ops(), _P()
    n, h, w, _, c = case
    zd, zv = _store(_rnd((n, h, w, 9 * c), 500 + h * w, 1.5))
    sums = fold_ref(_nchw(zv).double().contiguous(), c)
    os_, bs, ps = _vectors(n, c, 510)
    nbytes, guard = n * 4 * h * w * c * 4, 512
    for drop in (None, "out_scale", "bias", "post_scale"):
        v = dict(out_scale=os_, bias=bs, post_scale=ps)
        if drop:
            v[drop] = None
        buf = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
        y = P.tag(buf[guard:guard + nbytes].view(P.MX_DTYPE).reshape(n, 2 * h, 2 * w, c))
        r = ops.upfold3x3(zd, c, act=ops.ACT_LRELU_SQRT2, out=y, **{k: None if t is None else t.to(DEV) for k, t in v.items()})
        torch.cuda.synchronize()
        assert r is y
        ref = epilogue_ref(sums, v["out_scale"], v["bias"], 3, v["post_scale"])
        _check("upfold %s without %s" % (case, drop), _nchw(_host(y)), ref, MX)
        b = buf.cpu()
        assert bool((b[:guard] == 0xA5).all()) and bool((b[guard + nbytes:] == 0xA5).all()), "guard bytes around y were written"


@pytest.mark.parametrize("act", [0, 2, 3])
def test_fold_activation_arms(act):
    ops = _ops()
    n, h, w, _, c = CASES[2]
    zd, zv = _store(_rnd((n, h, w, 9 * c), 520, 1.5))
    os_, bs, ps = _vectors(n, c, 521)
    y = ops.upfold3x3(zd, c, out_scale=os_.to(DEV), bias=bs.to(DEV), act=act, post_scale=ps.to(DEV))
    torch.cuda.synchronize()
    _check("upfold act %d" % act, _nchw(_host(y)), epilogue_ref(fold_ref(_nchw(zv).double().contiguous(), c), os_, bs, act, ps), MX)


# ------------------------------------------------------------------------------------------------------------------ (b) end to end
def _layer(case, seed, heavy=False):
    """stored x, style rows s (largest magnitude of a row in [0.5, 1), like mnet_style_rows'), weights, demodulation d, bias, the next layer's style"""
    from marconet_amd import synthetic
    n, h, w, cin, c = case
    xd, xv = _store(_rnd((n, h, w, cin), seed, 1.0))
    if heavy:
        wgt = synthetic._t(synthetic._heavy(seed, "upfold.w", (c, cin, 3, 3))) * (cin * 9) ** -0.5
        s = synthetic._t(synthetic._loguniform(seed, "upfold.s", (n, cin), 10.0 ** -1.5, 10.0 ** 1.5))
        post = synthetic._t(synthetic._loguniform(seed, "upfold.p", (n, c), 10.0 ** -1.5, 10.0 ** 1.5))
    else:
        wgt = _rnd((c, cin, 3, 3), seed + 1, (cin * 9) ** -0.5)
        s = 1.0 + 0.1 * _rnd((n, cin), seed + 2)
        post = 1.0 + 0.1 * _rnd((n, c), seed + 3)
    s = s / torch.exp2(torch.floor(torch.log2(s.abs().amax(dim=1, keepdim=True))) + 1.0)
    post = post / torch.exp2(torch.floor(torch.log2(post.abs().amax(dim=1, keepdim=True))) + 1.0)
    d = torch.rsqrt((wgt.double() ** 2).sum(dim=(2, 3)).t().unsqueeze(0).mul(s.double().unsqueeze(2) ** 2).sum(dim=1) + 1e-8).float()      # [n, c]
    return xd, xv, s, wgt, d, _rnd((c,), seed + 4, 0.1), post


def end_to_end_errors(case, seed=77, heavy=False):
    """→ (e_new, e_two, scale): max-abs errors of tap conv + fold and of up-sample + conv against fp64 on the same stored inputs, and max |ref|"""
    ops, P = _ops(), _P()
    n, h, w, cin, c = case
    xd, xv, s, wgt, d, b, post = _layer(case, seed, heavy)
    xs = _nchw(xv).double() * s.double()[:, :, None, None]
    ref = epilogue_ref(F.conv2d(F.interpolate(xs, scale_factor=2, mode="bilinear", align_corners=False), wgt.double(), padding=1), d, b, 3, post)
    sd, dd, bd, pd = s.to(DEV), d.to(DEV), b.to(DEV), post.to(DEV)
    w_tap = P.pack_tapconv_weight(wgt.to(DEV), P.MX_DTYPE)
    w_full = P.pack_conv_weight(wgt.to(DEV), P.MX_DTYPE)
    z = ops.conv2d(ops.affine_act(xd, sd), w_tap, 9 * c, 1, 1)
    y_new = ops.upfold3x3(z, c, out_scale=dd, bias=bd, act=ops.ACT_LRELU_SQRT2, post_scale=pd)
    y_two = ops.conv2d(ops.upsample2x(xd, scale=sd), w_full, c, 3, 3, (1, 1), (1, 1), out_scale=dd, bias=bd, act=ops.ACT_LRELU_SQRT2, post_scale=pd)
    torch.cuda.synchronize()
    e_new = (_nchw(_host(y_new)).double() - ref).abs().max().item()
    e_two = (_nchw(_host(y_two)).double() - ref).abs().max().item()
    return e_new, e_two, ref.abs().max().item()


E2E = [pytest.param(c, False, id=i) for c, i in zip(CASES, IDS)] + [pytest.param(CASES[5], True, id="heavy_tailed")]


@pytest.mark.parametrize("case,heavy", E2E)
def test_end_to_end_error_against_the_two_launch_form(case, heavy):
    e_new, e_two, scale = end_to_end_errors(case, heavy=heavy)
    print("upfold end to end %s heavy=%s: e_new %.3e  e_two %.3e  ratio %.3f  (ref max %.3e)" % (case, heavy, e_new, e_two, e_new / e_two, scale))
    assert e_two > 0.0
    assert e_new <= K_END_TO_END * e_two


# ------------------------------------------------------------------------------------------------------------------ (d) batch invariance
@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=[IDS[2], IDS[4]])
def test_one_glyph_alone_gives_its_batch_bytes(case):
    ops, P = _ops(), _P()
    _, h, w, _, c = case
    zd, _ = _store(_rnd((3, h, w, 9 * c), 530, 1.5))
    os_, bs, ps = _vectors(3, c, 531)
    yb = ops.upfold3x3(zd, c, out_scale=os_.to(DEV), bias=bs.to(DEV), act=ops.ACT_LRELU_SQRT2, post_scale=ps.to(DEV))
    y1 = ops.upfold3x3(zd[1:2].contiguous(), c, out_scale=os_[1:2].contiguous().to(DEV), bias=bs.to(DEV), act=ops.ACT_LRELU_SQRT2,
                       post_scale=ps[1:2].contiguous().to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(P.untag(yb[1:2]).contiguous().cpu().view(torch.uint8), P.untag(y1).cpu().view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ (g) every storage, every launch regime
# The cases of tests/tail_regimes.py (UPF_CASES / UPF_CAP_CASE): each names the launch regime it is there for and asserts it before it launches.  z lies inside a
# larger buffer whose other bytes are 0xFF — NaN in every storage — at least one low-res row and two pixels on each side, so a clamped index that leaves the
# buffer puts a NaN into y; out_scale / bias / post_scale lie between NaN floats; y between 0xA5 bytes, which must stay.  Reference: fold_ref + epilogue_ref in fp64
# of the stored values, through _check with the storage's own bound (test_tail_regimes.py::test_upfold_reference_headroom shows that half of it is free).
DT = {R.F32: torch.float32, R.F16: torch.float16, R.SPLIT: SPLIT, R.MX: MX}
ALL3 = ("out_scale", "bias", "post_scale")
MIXES_REMAP = [(), ("out_scale",), ("bias",), ("post_scale",), ALL3]          # the vectors that are ABSENT
MIXES = [(), ALL3]
ACCEPTED = dict((s, 0) for s in R.STORAGES)                                    # launches the entry point accepted, per storage
WORST = dict((s, 0.0) for s in R.STORAGES)                                     # worst error / bound, per storage


def _sdt(dtype):
    return {R.F32: torch.float32, R.F16: torch.float16, R.SPLIT: _P().SPLIT_DTYPE, R.MX: _P().MX_DTYPE}[dtype]


def _esize(dtype):
    return 2 if dtype == R.F16 else 4


def _between(raw, guard, fill):
    """a copy of the byte tensor ``raw`` (device or host) between ``guard`` bytes of ``fill`` on each side → (whole buffer, the view of the copy), on the device"""
    assert guard % 128 == 0
    buf = torch.full((raw.numel() + 2 * guard,), fill, dtype=torch.uint8, device=DEV)
    buf[guard:guard + raw.numel()].copy_(raw)
    return buf, buf[guard:guard + raw.numel()]


def _z_guarded(stored, p, dtype):
    """a stored z [n,h,w,9c] (host or device) → the same bytes on the device between 0xFF guards of at least one low-res row + two pixels, 128-byte aligned"""
    n, h, w, c = p
    guard = -(-((w + 2) * 9 * c * _esize(dtype)) // 128) * 128
    buf, view = _between(_P().untag(stored).contiguous().view(torch.uint8).reshape(-1), guard, 0xFF)
    z = _P().tag(view.view(_sdt(dtype)).reshape(n, h, w, 9 * c))
    assert z.data_ptr() % 128 == 0 and z.data_ptr() == buf.data_ptr() + guard
    return buf, z


def _vec_guarded(t):
    """an fp32 vector between 64 NaN floats on each side"""
    if t is None:
        return None
    buf = torch.full((t.numel() + 128,), float("nan"), dtype=torch.float32, device=DEV)
    buf[64:64 + t.numel()].copy_(t.reshape(-1))
    return buf[64:64 + t.numel()].view(t.shape)


def _y_guarded(p, dtype):
    n, h, w, c = p
    nbytes, guard = n * 4 * h * w * c * _esize(dtype), 512
    buf = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, guard, _P().tag(buf[guard:guard + nbytes].view(_sdt(dtype)).reshape(n, 2 * h, 2 * w, c))


def _y_guards_intact(buf, guard):
    return bool((buf[:guard] == 0xA5).all().item()) and bool((buf[-guard:] == 0xA5).all().item())


@functools.lru_cache(maxsize=4)
def _small_operands(p, dtype):
    """→ (stored z on the host, fp64 sums [n,c,2h,2w] of the values it holds, the three vectors): one pass through the HOST packer; computed once per (case, storage)"""
    s = _P().from_float(fold_input(p, 600, R.upf_z_scale(p)), _sdt(dtype))
    sums = fold_ref(_nchw(_P().to_float(s)).double().contiguous(), p[3])
    return s, sums, _vectors(p[0], p[3], 601)


def _compare(name, dtype, got, ref, ybuf, guard):
    """got / ref NCHW: no NaN (a read outside z), the storage's bound, the guards of y"""
    assert not bool(torch.isnan(got).any()), "%s: NaN in y — the kernel read a guard byte around z or a vector" % name
    ratio = (got.double() - ref).abs().max().item() / (_tol(DT[dtype]) * max(ref.abs().max().item(), 1e-6))
    ACCEPTED[dtype] += 1
    WORST[dtype] = max(WORST[dtype], ratio)
    print("upfold %-5s accepted launches %3d   this error / bound %.3f   worst so far %.3f" % (dtype, ACCEPTED[dtype], ratio, WORST[dtype]))
    _check(name, got, ref, DT[dtype], extra=1.0)
    assert _y_guards_intact(ybuf, guard), "%s: guard bytes around y were written" % name


def _run_small(regime, p, dtype, mixes, act):
    ops = _ops()
    s, sums, vec = _small_operands(tuple(p), dtype)
    zbuf, z = _z_guarded(s, p, dtype)
    for absent in mixes:
        v = dict(zip(ALL3, vec))
        for k in absent:
            v[k] = None
        ybuf, guard, y = _y_guarded(p, dtype)
        r = ops.upfold3x3(z, p[3], act=act, out=y, **{k: _vec_guarded(None if t is None else t.to(DEV)) for k, t in v.items()})
        torch.cuda.synchronize()
        assert r is y
        ref = epilogue_ref(sums, v["out_scale"], v["bias"], act, v["post_scale"])
        _compare("upfold %s %s %s act %d without %s" % (regime, p, dtype, act, "+".join(absent) or "nothing"), dtype, _nchw(_host(y)), ref, ybuf, guard)
    assert bool((zbuf[:z.data_ptr() - zbuf.data_ptr()] == 0xFF).all().item())


UPF_IDS = ["%s-%dx%dx%dx%d" % ((nm.replace(" ", "_").replace(",", ""),) + p) for nm, p in R.UPF_CASES]


@pytest.mark.parametrize("dtype", R.STORAGES)
@pytest.mark.parametrize("case", R.UPF_CASES, ids=UPF_IDS)
def test_fold_launch_regimes_match_fp64(case, dtype):
    """upfold_kernel<T> of every storage with several workgroups per image: the XCD-aware order on and off (all three vectors, each one absent, none), H % RUN =
    0 ... 7 with two runs, three runs, one run (H < RUN, H = RUN: both edges in one full run), W = 1 (every column clamps on both sides) and W = 2"""
    regime, p = case
    assert R.UPF_REGIME[regime](p, dtype), (regime, R.upf_launch(*p, dtype), R.upf_runs(p[1]))
    _run_small(regime, p, dtype, MIXES_REMAP if regime.startswith("several workgroups") else MIXES, _ops().ACT_LRELU_SQRT2)


@pytest.mark.parametrize("dtype", R.STORAGES)
@pytest.mark.parametrize("act", [0, 2, 3])
def test_fold_activation_arms_on_every_storage(act, dtype):
    regime, p = R.UPF_CASES[10]                                                 # three runs, remap off
    assert R.UPF_REGIME[regime](p, dtype)
    _run_small(regime, p, dtype, [()], act)


@functools.lru_cache(maxsize=2)
def _cap_source(p):
    return fold_input(p, 620)


@pytest.mark.parametrize("dtype", R.STORAGES)
def test_fold_second_grid_stride_trip(dtype):
    """more than 2048 x 256 (chunk, hi-res column, run) items in one image: the capped grid makes a second, partial trip, with the XCD remap of the workgroup index
    (2048 % 8 == 0).  z (151 MB in the 4-byte storages) is encoded and decoded by mnet_convert on the device (its codec has tests of its own:
    test_tail_kernels_gpu.py::test_convert_second_grid_stride_trip); the fp64 reference is evaluated in column bands (tests/test_tail_regimes.py checks it equal to the whole-map one)"""
    ops, P = _ops(), _P()
    regime, shapes = R.UPF_CAP_CASE
    p = shapes[dtype]
    assert R.UPF_REGIME[regime](p, dtype), R.upf_launch(*p, dtype)
    n, h, w, c = p
    src = _cap_source(p).to(DEV)
    zd = src if dtype == R.F32 else ops.convert(src, _sdt(dtype))
    zv = (zd if dtype == R.F32 else ops.convert(zd, torch.float32)).cpu()
    zbuf, z = _z_guarded(zd, p, dtype)
    del src, zd
    sums = fold_ref_banded(_nchw(zv).double().contiguous(), c, 8200)
    del zv
    vec = _vectors(n, c, 621)
    for absent in MIXES:
        v = dict(zip(ALL3, vec))
        for k in absent:
            v[k] = None
        ybuf, guard, y = _y_guarded(p, dtype)
        ops.upfold3x3(z, c, act=ops.ACT_LRELU_SQRT2, out=y, **{k: _vec_guarded(None if t is None else t.to(DEV)) for k, t in v.items()})
        torch.cuda.synchronize()
        got = (y if dtype == R.F32 else ops.convert(y, torch.float32)).float().cpu()
        ref = epilogue_ref(sums, v["out_scale"], v["bias"], 3, v["post_scale"])
        # the second trip's items are the last of the image: hi-res columns first2 ... of both rows of the (only) run
        first2 = R.UPF_CAP * R.WG // (c // R.vec_n(dtype))
        e2 = (_nchw(got).double() - ref)[:, :, :, first2:].abs().max().item()
        assert first2 < 2 * w and e2 <= _tol(DT[dtype]) * ref.abs().max().item(), "second trip (hi-res columns %d ...): %.3e" % (first2, e2)
        _compare("upfold %s %s %s without %s" % (regime, p, dtype, "+".join(absent) or "nothing"), dtype, _nchw(got), ref, ybuf, guard)
        del got, ref, y, ybuf


BATCH_CASES = [R.UPF_CASES[3], R.UPF_CASES[10]]        # (8, 9, 24, 64): the batch has the remap on, one image alone has it off; (3, 17, 24, 64): off in both, three runs


@pytest.mark.parametrize("dtype", R.STORAGES)
@pytest.mark.parametrize("case", BATCH_CASES, ids=["remap_on_in_the_batch_only", "three_runs"])
def test_one_glyph_alone_gives_its_batch_bytes_on_every_storage(case, dtype):
    ops, P = _ops(), _P()
    regime, p = case
    n, h, w, c = p
    assert R.UPF_REGIME[regime](p, dtype) and not R.upf_launch(1, h, w, c, dtype)[3]
    assert R.upf_launch(*p, dtype)[3] == (case is BATCH_CASES[0])
    s, _, (os_, bs, ps) = _small_operands(tuple(p), dtype)
    zd = s.to(DEV)
    raw = lambda t: P.untag(t).contiguous().cpu().view(torch.uint8)
    yb = ops.upfold3x3(zd, c, out_scale=os_.to(DEV), bias=bs.to(DEV), act=ops.ACT_LRELU_SQRT2, post_scale=ps.to(DEV))
    for i in (0, 1, n - 1):
        y1 = ops.upfold3x3(zd[i:i + 1].contiguous(), c, out_scale=os_[i:i + 1].contiguous().to(DEV), bias=bs.to(DEV), act=ops.ACT_LRELU_SQRT2,
                           post_scale=ps[i:i + 1].contiguous().to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(raw(yb[i:i + 1]), raw(y1)), "image %d of %s in %s" % (i, p, dtype)


# ------------------------------------------------------------------------------------------------------------------ (e) refused launches
def test_refused_launches_enqueue_nothing():
    from marconet_amd import _lib
    ops, P = _ops(), _P()
    n, h, w, _, c = CASES[3]
    zd, _ = _store(_rnd((n, h, w, 9 * c), 540))
    y = P.new_tensor((n, 2 * h, 2 * w, c), P.MX_DTYPE, DEV, zero=True)
    before = P.untag(y).cpu().clone()
    odd = torch.zeros(c + 4, device=DEV)[1:1 + c]                           # a 4-byte-offset view: contiguous, not 16-byte aligned
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4
    for kw in (dict(act=ops.ACT_TANH), dict(act=ops.ACT_RELU), dict(bias=odd)):
        with pytest.raises(_lib.MarconetHipError):
            ops.upfold3x3(zd, c, out=y, **kw)
    with pytest.raises(RuntimeError):
        ops.upfold3x3(zd, c + 32, out=y)
    torch.cuda.synchronize()
    assert torch.equal(P.untag(y).cpu(), before)
    # the plan: fp16+8 storage and the table's levels only, whatever the batch
    x = P.new_tensor((2, 16, 16, 512), P.MX_DTYPE, DEV, zero=True)
    assert ops.upfold_plan(x, 256) >= 0 and ops.upfold_plan(x, 512) >= 0
    assert ops.upfold_plan(P.new_tensor((1, 16, 16, 512), P.MX_DTYPE, DEV, zero=True), 256) == ops.upfold_plan(x, 256)
    assert ops.upfold_plan(P.new_tensor((2, 8, 8, 512), P.MX_DTYPE, DEV, zero=True), 512) < 0          # 8→16 keeps up-sample + conv
    assert ops.upfold_plan(x, 128) < 0 and ops.upfold_plan(x, 256, levels={}) < 0
    assert ops.upfold_plan(P.new_tensor((2, 16, 16, 512), P.SPLIT_DTYPE, DEV, zero=True), 256) < 0
    assert ops.upfold_plan(torch.zeros((2, 16, 16, 512), dtype=torch.float16, device=DEV), 256) < 0


# ------------------------------------------------------------------------------------------------------------------ (e, f) the layer
@pytest.fixture(scope="module")
def generator(ckpts):
    from marconet_amd import synthetic
    from marconet_amd.networks import TSPGAN
    gan = TSPGAN()
    gan.load_state_dict(ckpts[1], strict=True)
    gan = gan.eval().to(DEV)
    return gan.TextGenerator, synthetic.make_styles(111, 2).to(DEV).float().contiguous(), synthetic.make_labels(112, 2).to(DEV).long().contiguous()


def _run(tg, styles, labels, precision, monkeypatch, no_upfold=False, levels=None):
    """forward_nhwc up to the 64-px level → (bytes of prior64, bytes of prior32, number of fold launches, number of up-sample launches)"""
    from marconet_amd import networks
    ops, P = _ops(), _P()
    calls = {"fold": 0, "ups": 0}
    fold, ups = ops.upfold3x3, ops.upsample2x
    monkeypatch.setattr(ops, "upfold3x3", lambda *a, **k: (calls.__setitem__("fold", calls["fold"] + 1), fold(*a, **k))[1])
    monkeypatch.setattr(ops, "upsample2x", lambda *a, **k: (calls.__setitem__("ups", calls["ups"] + 1), ups(*a, **k))[1])
    monkeypatch.setattr(networks, "_NO_UPFOLD", no_upfold)
    if levels is not None:
        monkeypatch.setattr(ops, "UPFOLD_LEVELS", levels)
    with torch.no_grad(), ops.on_device(styles):
        _, p64, p32 = tg.forward_nhwc(styles, labels, need_image=False, precision=precision)
    torch.cuda.synchronize()
    raw = lambda t: P.untag(t).contiguous().cpu().view(torch.uint8).clone()
    return raw(p64), raw(p32), calls["fold"], calls["ups"]


def test_generator_takes_the_fold_in_fp16x2_only(generator, monkeypatch):
    tg, styles, labels = generator
    with monkeypatch.context() as m:
        new = _run(tg, styles, labels, "fp16x2", m)
    assert new[2:] == (2, 2), new[2:]                      # 16→32 and 32→64 fold, 4→8 and 8→16 up-sample
    with monkeypatch.context() as m:
        knob = _run(tg, styles, labels, "fp16x2", m, no_upfold=True)
    assert knob[2:] == (0, 4)
    with monkeypatch.context() as m:
        refused = _run(tg, styles, labels, "fp16x2", m, levels={})      # a refused plan: the layer falls back to the two-launch form, same bytes
    assert refused[2:] == (0, 4) and torch.equal(refused[0], knob[0]) and torch.equal(refused[1], knob[1])
    assert not torch.equal(new[0], knob[0])                 # (the new form rounds at other places: other bytes, inside the parity bars)
    for mode in ("fp16x3", "fp16", "fp32"):
        with monkeypatch.context() as m:
            assert _run(tg, styles, labels, mode, m)[2:] == (0, 4), mode
