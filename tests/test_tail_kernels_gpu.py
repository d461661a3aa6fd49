"""-m gpu: the streaming ("tail") kernels of csrc/aux_kernels.hip in their multi-workgroup launch regimes — grid caps and the second trip of the
grid-stride loops, GroupNorm slice folds (2 ... 128 slices, short last slice), the XCD-aware workgroup order and the zig-zag row runs of the up-sample,
the two-chunks-per-thread GroupNorm apply, and the finiteness flag (no op-level test before this one).

Every case names the launch regime it is there for and asserts, through the mirrors of the host arithmetic in tests/tail_regimes.py, that its shape
really lands there (tests/test_tail_regimes.py makes the same assertion without a device).

References: the same operation in fp64 on the CPU on the values the storage holds — split-half and fp16+8 tensors are encoded and decoded by the HOST
packers (packing.from_float / to_float), the device mnet_convert appears only in the test that is about it.  Tolerances: `_tol` of test_kernels_gpu.py
with the `extra` factor of the small-shape test of the same op; GroupNorm scale / shift directly: the 2e-6 of test_mx_gpu.py.  Flag, convert,
SR post-processing and fused_bias_act are compared exactly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import tail_regimes as R
from tests.test_kernels_gpu import ALL_DTYPES, MX, SPLIT, _check, _nchw, _nhwc, _q, _tol  # noqa: F401  (the op-level helpers, shared not copied)

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {R.F32: torch.float32, R.F16: torch.float16, R.SPLIT: SPLIT, R.MX: MX}
assert [DT[s] for s in R.STORAGES] == ALL_DTYPES


def _ops():
    from marconet_amd import ops
    return ops


def _P():
    from marconet_amd import packing
    return packing


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _sdt(dtype):
    """storage name -> torch dtype / tag"""
    return {R.F32: torch.float32, R.F16: torch.float16, R.SPLIT: _P().SPLIT_DTYPE, R.MX: _P().MX_DTYPE}[dtype]


def _store(x_nhwc, dtype):
    """fp32 NHWC (cpu) -> (the tensor in storage `dtype` on the device, the fp32 NHWC values it holds): one pass through the host packer"""
    s = _P().from_float(x_nhwc.contiguous(), _sdt(dtype))
    return s.to(DEV), _P().to_float(s)


def _host(t):
    """device tensor of any storage -> fp32 on the host, decoded by the host packer"""
    return _P().to_float(t.cpu())


def _bytes(t):
    return t.cpu().contiguous().view(torch.uint8)


# ====================================================================================================================== nonfinite_flag
def _bits(dtype):
    """(numpy unsigned type, torch signed view type, +inf, -inf, NaN with the lowest mantissa bit only, negative quiet NaN)"""
    if dtype == R.F16:
        return np.uint16, torch.int16, (0x7c00, 0xfc00, 0x7c01, 0xfe00)
    return np.uint32, torch.int32, (0x7f800000, 0xff800000, 0x7f800001, 0xffc00000)


def _finite_patterns(dtype):
    """bit patterns of FINITE values a wrong mask would misread: the largest finite value and its negative (exponent 0b11110, mantissa all ones),
    subnormals, +-0, every exponent with exactly one bit clear under an all-ones mantissa (NaN-like but for one bit), and for fp32 words whose 16-bit
    halves look like f16 infinities.  f16: every finite pattern there is (63 488), + one repeat so that the period is odd and every pattern falls on
    both halves of a 32-bit word; fp32: the hand-picked ones + seeded random finite words, odd period too"""
    if dtype == R.F16:
        b = np.arange(65536, dtype=np.uint32)
        b = b[(b & 0x7c00) != 0x7c00].astype(np.uint16)
        assert b.size == 63488 and 0x7bff in b and 0xfbff in b and 0x0001 in b and 0x8000 in b
        return np.concatenate([b, np.array([0x3c00], np.uint16)])
    hand = [0x7f7fffff, 0xff7fffff, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00000000, 0x80000000, 0x00800000, 0x7f000000,
            0x3f807c00, 0x7c003f80, 0x7c007c00, 0xfc00fc00, 0x7c00fc00, 0x7bff7c00, 0x00007c00, 0x7c000000, 0x477fe000, 0xc77fe000]
    hand += [(0x7fffffff & ~(1 << bit)) | sign for bit in range(23, 31) for sign in (0, 0x80000000)]
    rs = np.random.RandomState(5)
    r = rs.randint(0, 1 << 32, size=4096 + 1 - len(hand) % 2, dtype=np.uint64).astype(np.uint32)
    r = np.where((r & 0x7f800000) == 0x7f800000, r & ~np.uint32(0x00800000), r)
    b = np.concatenate([np.array(hand, np.uint32), r])
    assert b.size % 2 == 1 and ((b & 0x7f800000) != 0x7f800000).all()
    return b


def _finite_tensor(numel, dtype):
    """a device tensor of `numel` finite values that cycles through _finite_patterns"""
    _, view_t, _ = _bits(dtype)
    pat = _finite_patterns(dtype)
    b = np.resize(pat, numel)
    t = torch.from_numpy(b.view(np.int16 if dtype == R.F16 else np.int32).copy()).view(_sdt(dtype))
    assert torch.isfinite(t).all()
    return t.to(DEV)


def _signed(bits, np_t):
    return int(np.array([bits], np_t).view(np.int16 if np_t is np.uint16 else np.int32)[0])


@pytest.mark.parametrize("dtype", [R.F32, R.F16])
def test_nonfinite_flag_finite_values_a_wrong_mask_would_misread(dtype):
    """0 for tensors of finite values only: every finite f16 pattern on both halves of a word (the largest finite value 65504 = 0x7bff and its
    negative, subnormals, +-0, exponents one bit short of all ones under an all-ones mantissa), the same classes in fp32 plus words whose halves
    look like f16 infinities; in the vector loop and in the scalar tail (whose fp32 test once compared against 3.0e38 and flagged the finite values
    above it, torch.finfo(float32).max among them)"""
    ops = _ops()
    n = R.vec_n(dtype)
    period = _finite_patterns(dtype).size
    x0 = _finite_tensor(period, dtype).cpu().double()
    assert x0.max().item() == torch.finfo(_sdt(dtype)).max and x0.min().item() == -torch.finfo(_sdt(dtype)).max
    for numel in (2 * period, 2 * period + 1, 2 * period + n - 1):
        x = _finite_tensor(numel, dtype)
        assert R.flag_launch(numel, dtype)[1] > 1
        assert ops.nonfinite_flag(x).item() == 0, "finite tensor of %d %s flagged" % (numel, dtype)
    # ... and each pattern alone in the scalar tail (numel < N: thread 0 of block 0 reads it as a float)
    pat = _finite_patterns(dtype)
    pick = pat[:64] if dtype == R.F32 else pat[np.r_[0:64, 0x3ff - 8:0x400 + 8, 0x7bff - 64:0x7bff + 1, 63488 - 64:63488]]
    np_t, view_t, _ = _bits(dtype)
    x = _finite_tensor(n - 1, dtype)
    flag = torch.empty((1,), dtype=torch.int32, device=DEV)
    got = []
    for b in pick:
        x.view(view_t)[n - 2] = _signed(int(b), np_t)
        got.append(ops.nonfinite_flag(x, out=flag).clone())
    assert torch.stack(got).sum().item() == 0


def _flag_params():
    return [pytest.param(dt, name, numel, id="%s-%s-%d" % (dt, name.replace(" ", "_"), numel)) for dt in (R.F32, R.F16) for name, numel in R.flag_sizes(dt)]


@pytest.mark.parametrize("dtype,regime,numel", _flag_params())
def test_nonfinite_flag_finds_one_special_value_anywhere(dtype, regime, numel):
    """exactly one +inf / -inf / NaN (lowest mantissa bit only; negative quiet) planted at every lane of the first 16-byte vector, of the last full
    vector, of a vector only the second grid-stride trip reaches, and at every position of the scalar tail: 1 each time, 0 before and after"""
    ops = _ops()
    assert R.FLAG_REGIME[regime](numel, dtype)
    n = R.vec_n(dtype)
    nv, grid, trips, tail = R.flag_launch(numel, dtype)
    np_t, view_t, specials = _bits(dtype)
    x = _finite_tensor(numel, dtype)
    xi = x.view(view_t)
    pos = set(range(min(n, nv * n))) | set(range(max(0, (nv - 1) * n), nv * n)) | set(range(nv * n, numel))
    if trips == 2:
        second = grid * R.WG + 5                       # a vector index no thread reaches on its first trip
        assert grid * R.WG <= second < nv
        pos |= set(range(second * n, second * n + n)) | set(range(grid * R.WG * n, grid * R.WG * n + n))
    assert len(pos) >= min(numel, n) and max(pos) == numel - 1
    flag = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    assert ops.nonfinite_flag(x, out=flag).item() == 0
    got, want = [], 0
    for p in sorted(pos):
        keep = xi[p].clone()
        for s in specials:
            xi[p] = _signed(s, np_t)
            got.append(ops.nonfinite_flag(x, out=flag).clone())       # (stream order: the clone reads the flag before the next launch's memset)
            want += 1
        xi[p] = keep
    got = torch.stack(got).reshape(-1).cpu()
    miss = [(sorted(pos)[i // len(specials)], hex(specials[i % len(specials)])) for i in (got != 1).nonzero().reshape(-1).tolist()]
    assert not miss, "%s numel=%d: not flagged (position, bits): %s" % (dtype, numel, miss[:12])
    assert got.numel() == want and ops.nonfinite_flag(x, out=flag).item() == 0


@pytest.mark.parametrize("dtype", [R.F32, R.F16])
def test_nonfinite_flag_zeroes_the_flag_on_the_stream_first(dtype):
    """the flag of the LAST call: bad then good into the same element gives 0 (the hipMemsetAsync is ordered before the kernel and after the previous
    one), good then bad gives 1; only the one element is written"""
    ops = _ops()
    n = R.vec_n(dtype)
    np_t, view_t, specials = _bits(dtype)
    good = _finite_tensor(300 * n + 3, dtype)
    bad = good.clone()
    bad.view(view_t)[137 * n + 1] = _signed(specials[2], np_t)
    out = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    ops.nonfinite_flag(bad, out=out[1:2])
    ops.nonfinite_flag(good, out=out[1:2])
    ops.nonfinite_flag(good, out=out[2:3])
    ops.nonfinite_flag(bad, out=out[2:3])
    torch.cuda.synchronize()
    assert out.tolist() == [7, 0, 1, 7]
    ops.nonfinite_flag(bad, out=out[1:2])
    ops.nonfinite_flag(bad, out=out[1:2])
    assert out.tolist() == [7, 1, 1, 7]


def test_nonfinite_flag_refuses_blocked_storages_and_other_flags():
    """argument checks that return before anything is enqueued: the flag keeps the value it had"""
    ops = _ops()
    from marconet_amd._lib import MarconetHipError
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    for dtype in (SPLIT, MX):
        x = _nhwc(_rnd((1, 32, 2, 2), 1), dtype)
        with pytest.raises(MarconetHipError, match="MNET_F32 or MNET_F16"):
            ops.nonfinite_flag(x, out=flag)
    good = _finite_tensor(64, R.F32)
    fflag = torch.full((1,), 7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(TypeError):
        ops.nonfinite_flag(good, out=fflag)
    lflag = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    with pytest.raises(TypeError):
        ops.nonfinite_flag(good, out=lflag)
    two = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError):
        ops.nonfinite_flag(good, out=two)
    torch.cuda.synchronize()
    assert flag.item() == 7 and fflag.item() == 7.0 and lflag.item() == 7 and two.tolist() == [7, 7]


# ====================================================================================================================== groupnorm_affine
def _gn_input(p, seed):
    """a map whose mean is several times its spread (SS/cnt - mean^2 cancels ~40-fold), different per image and group"""
    n, h, w, c, _ = p
    return _rnd((n, c, h, w), seed, 0.5) + 3.0 + 0.4 * _rnd((n, c // 32, 1, 1), seed + 1).repeat_interleave(32, dim=1)


def _gn_reference(xv, i, v, gamma, beta):
    """fp64 statistics of image i over columns < v: mean, biased variance, eps 1e-6 -> (scale [c], shift [c])"""
    c = xv.shape[1]
    g = xv[i, :, :, :v].double().reshape(c // 32, -1)
    mean, var = g.mean(1), g.var(1, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + 1e-6)).repeat_interleave(32)
    sc = gamma.double() * rstd
    return sc, beta.double() - mean.repeat_interleave(32) * sc


@pytest.mark.parametrize("dtype", R.STORAGES)
@pytest.mark.parametrize("case", R.GN_CASES, ids=["%s-%dx%dx%d-%s" % (nm.replace(" ", "_"), p[1], p[2], p[3], "ragged" if p[4] else "full") for nm, p in R.GN_CASES])
def test_groupnorm_affine_folds_every_slice(case, dtype):
    """gn_partial_kernel<T> + gn_finalize_kernel with 2 ... 128 slices (the cap), H*W not divisible by the slice count (a short last slice — the
    shortest the slice rule allows: 386 of 513 pixels), ragged valid widths that cut across slice borders, c = 32 ... 1024 (fp32, c = 1024: one
    pixel lane per workgroup): against fp64 statistics, as the normalised map (the bound of test_kernels_gpu.py::test_groupnorm_affine) and as
    scale / shift directly (2e-6 relative, test_mx_gpu.py; the shift, whose magnitude is |mean| * scale ~ 8 here, relative to max(1, |shift|))"""
    ops = _ops()
    regime, p = case
    assert R.GN_REGIME[regime](p, dtype), (regime, R.gn_launch(p[1], p[2], p[3], dtype))
    n, h, w, c, vw = p
    xd, xv = _store(_gn_input(p, 400).permute(0, 2, 3, 1), dtype)
    xv = xv.permute(0, 3, 1, 2)                                        # NCHW view of the stored values
    gamma, beta = 1 + 0.1 * _rnd((c,), 402), 0.1 * _rnd((c,), 403)
    vwd = None if vw is None else torch.tensor(vw, dtype=torch.int32, device=DEV)
    sc, sh = ops.groupnorm_affine(xd, gamma.to(DEV), beta.to(DEV), 1e-6, vwd)
    torch.cuda.synchronize()
    sc, sh = sc.cpu(), sh.cpu()
    assert sc.shape == (n, c) and sh.shape == (n, c) and sc.dtype == torch.float32
    for i in range(n):
        v = w if vw is None else vw[i]
        xi = xv[i:i + 1, :, :, :v].double()
        ref = F.group_norm(xi, c // 32, gamma.double(), beta.double(), 1e-6)
        got = xi * sc[i].double()[None, :, None, None] + sh[i].double()[None, :, None, None]
        _check("groupnorm %s %s img=%d vw=%d %s" % (regime, p[1:4], i, v, dtype), got, ref, torch.float32, extra=2.0)
        rsc, rsh = _gn_reference(xv, i, v, gamma, beta)
        esc, esh = (sc[i].double() - rsc).abs().max().item(), (sh[i].double() - rsh).abs().max().item()
        print("    scale err %.3e (max %.3e)  shift err %.3e (max %.3e)" % (esc, rsc.abs().max().item(), esh, rsh.abs().max().item()))
        assert esc <= 2e-6 * rsc.abs().max().item(), "scale, image %d: %.3e" % (i, esc)
        assert esh <= 2e-6 * max(1.0, rsh.abs().max().item()), "shift, image %d: %.3e" % (i, esh)


@pytest.mark.parametrize("dtype", R.STORAGES)
@pytest.mark.parametrize("case", [R.GN_BATCH_CASE, R.GN_CASES[4]], ids=["4_slices", "32_slices"])
def test_groupnorm_affine_does_not_depend_on_the_batch(case, dtype):
    """ops.groupnorm_affine: "the fp64 fold order never depends on the batch" — an image's scale / shift alone and inside a batch of 3: the same bits"""
    ops = _ops()
    regime, p = case
    assert R.GN_REGIME[regime](p, dtype) and p[0] == 3
    n, h, w, c, vw = p
    xd, _ = _store(_gn_input(p, 410).permute(0, 2, 3, 1), dtype)
    gamma, beta = (1 + 0.1 * _rnd((c,), 412)).to(DEV), (0.1 * _rnd((c,), 413)).to(DEV)
    vwd = torch.tensor(vw, dtype=torch.int32, device=DEV)
    sc, sh = ops.groupnorm_affine(xd, gamma, beta, 1e-6, vwd)
    for i in range(n):
        s1, h1 = ops.groupnorm_affine(xd[i:i + 1].contiguous(), gamma, beta, 1e-6, vwd[i:i + 1].contiguous())
        assert torch.equal(s1[0], sc[i]) and torch.equal(h1[0], sh[i]), "image %d" % i
    sn, hn = ops.groupnorm_affine(xd, gamma, beta, 1e-6, None)           # (no valid_w == valid_w = w)
    sw, hw_ = ops.groupnorm_affine(xd, gamma, beta, 1e-6, torch.full((n,), w, dtype=torch.int32, device=DEV))
    assert torch.equal(sn, sw) and torch.equal(hn, hw_)


# ====================================================================================================================== upsample2x
UPS_FORMS = [(R.F32, None), (R.F16, None), (R.SPLIT, None), (R.MX, None), (R.SPLIT, R.F16), (R.MX, R.F16)]      # (source storage, output storage if it differs)


def _ups_check(name, p, src, dst, seed):
    """bilinear x2 (align_corners=False) of the stored values in fp64, with and without the per-(n, c) scale"""
    ops = _ops()
    n, h, w, c = p
    xd, xv = _store(_rnd((n, h, w, c), seed, 1.5), src)
    ref = F.interpolate(xv.permute(0, 3, 1, 2).double(), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    sc = _rnd((n, c), seed + 1).abs() + 0.5
    out_t = DT[dst or src]
    for scale in (None, sc):
        y = ops.upsample2x(xd, scale=None if scale is None else scale.to(DEV), out_dtype=None if dst is None else torch.float16)
        torch.cuda.synchronize()
        assert tuple(y.shape) == (n, 2 * h, 2 * w, c) and y.dtype == _sdt(dst or src)
        r = ref if scale is None else ref * scale.double()[:, None, None, :]
        _check("upsample2x %s %s %s->%s scale=%s" % (name, p, src, dst or src, scale is not None), _host(y), r, out_t)


@pytest.mark.parametrize("form", UPS_FORMS, ids=["%s_to_%s" % (s, d or s) for s, d in UPS_FORMS])
@pytest.mark.parametrize("case", R.UPS_CASES, ids=["%s-%dx%dx%dx%d" % ((nm.replace(" ", "_"),) + p) for nm, p in R.UPS_CASES])
def test_upsample2x_row_runs_and_workgroup_order(case, form):
    """every upsample2x_kernel<T, TD> with several workgroups per image: the XCD-aware order on (workgroups % 8 == 0) and off, H % 4 = 0 ... 3 with
    an even and an odd number of row runs (the last run walks up / down into the bottom border, short or full), H < 4, W = 1"""
    regime, p = case
    src, dst = form
    assert R.UPS_REGIME[regime](p, src), (regime, R.ups_launch(*p, src))
    _ups_check(regime, p, src, dst, 420)


@pytest.mark.parametrize("dtype", R.STORAGES)
def test_upsample2x_second_grid_stride_trip(dtype):
    """more than 2048 x 256 (chunk, column, run) items per image: the capped grid makes a second, partial trip (with the XCD remap of the
    workgroup index: 2048 % 8 == 0)"""
    regime, shapes = R.UPS_CAP_CASE
    p = shapes[dtype]
    assert R.UPS_REGIME[regime](p, dtype), R.ups_launch(*p, dtype)
    _ups_check(regime, p, dtype, None, 430)


# ====================================================================================================================== affine_act
def _affine_params():
    return [pytest.param(dt, nm, p, id="%s-%s-%dx%dx%d" % (dt, nm.replace(" ", "_"), p[1][0], p[1][1], p[2])) for dt in R.STORAGES for nm, p in R.AFFINE_CASES[dt]]


@pytest.mark.parametrize("dtype,regime,p", _affine_params())
def test_affine_act_two_chunks_and_one_trip(dtype, regime, p):
    """affine_act_kernel<T, 2> for every storage (fp32: c = 512 and 1024) with a last workgroup whose second chunks all lie beyond the image, and one
    where both chunks of half its threads do; affine_act_kernel<T, 1> on a map of more workgroups per image than the grid cap it used to have.
    Swish on / off, no shift, in place: against fp64"""
    ops = _ops()
    assert R.AFFINE_REGIME[regime](p, dtype), (regime, R.affine_launch(p[1][0] * p[1][1], p[2], dtype))
    n, (h, w), c = p
    xd, xv = _store(_rnd((n, h, w, c), 440, 2.0) + 0.3, dtype)
    sc, sh = _rnd((n, c), 441) + 1.0, _rnd((n, c), 442, 0.3)
    scd, shd = sc.to(DEV), sh.to(DEV)
    t = xv.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
    name = "affine_act %s %s %s " % (regime, p, dtype)
    orig = _bytes(xd)
    _check(name + "swish", _host(ops.affine_act(xd, scd, shd, swish=True)), t * torch.sigmoid(t), DT[dtype])
    _check(name + "affine", _host(ops.affine_act(xd, scd, shd)), t, DT[dtype])
    _check(name + "scale only", _host(ops.affine_act(xd, scd)), xv.double() * sc.double()[:, None, None, :], DT[dtype])
    t0 = xv.double() * sc.double()[:, None, None, :]
    _check(name + "scale only swish", _host(ops.affine_act(xd, scd, swish=True)), t0 * torch.sigmoid(t0), DT[dtype])
    assert torch.equal(_bytes(xd), orig)                                                       # the input was not touched
    y = ops.affine_act(xd, scd, shd, swish=True, out=xd)                                       # in place
    assert y is xd
    _check(name + "in place", _host(xd), t * torch.sigmoid(t), DT[dtype])


# ====================================================================================================================== flat kernels past their grid caps
def _convert_source():
    """fp32 [rows, 64]: five decades of magnitude across the channels, a few all-zero 32-channel blocks and rows"""
    rows = R.CONVERT_COUNT // 64
    x = _rnd((rows, 64), 450) * torch.logspace(-3, 2, 64)
    x[::1001, :32] = 0.0
    x[rows // 2 - 1] = 0.0
    return x


@pytest.fixture(scope="module")
def convert_source():
    return _convert_source()


@pytest.mark.parametrize("pair", R.CONVERT_PAIRS, ids=["%s_to_%s" % p for p in R.CONVERT_PAIRS])
def test_convert_second_grid_stride_trip(pair, convert_source):
    """mnet_convert over more than 16384 x 256 chunks (a second, partial trip) for the conversions the pipeline makes: the whole result equals the host
    packer's, byte for byte, and the concatenation of two single-trip device conversions of the two halves"""
    ops, P = _ops(), _P()
    assert R.convert_regime_ok(), R.convert_launch(R.CONVERT_COUNT)
    src, dst = pair
    x = convert_source
    s_host = P.from_float(x, _sdt(src))                                   # the source in its storage, by the host packer
    vals = P.to_float(s_host)                                             # ... and the values it holds
    want = P.from_float(vals, _sdt(dst))
    sd = s_host.to(DEV)
    got = ops.convert(sd, _sdt(dst))
    torch.cuda.synchronize()
    assert got.dtype == _sdt(dst) and tuple(got.shape) == tuple(x.shape)
    gb, wb = _bytes(got), _bytes(want)
    if not torch.equal(gb, wb):
        bad = (gb != wb).reshape(x.shape[0], -1).any(1).nonzero().reshape(-1)
        raise AssertionError("convert %s -> %s: %d of %d rows differ from the host packer, first %s, last %s (the second trip starts at row %d)"
                             % (src, dst, bad.numel(), x.shape[0], bad[:4].tolist(), bad[-4:].tolist(), R.CONVERT_CAP * R.WG * 8 // 64))
    half = x.shape[0] // 2
    a, b = ops.convert(sd[:half].contiguous(), _sdt(dst)), ops.convert(sd[half:].contiguous(), _sdt(dst))
    assert torch.equal(torch.cat([_bytes(a), _bytes(b)]), gb)


def _sr_ties():
    """fp32 inputs s whose (s * 0.5 + 0.5) * 255 is exactly k + 0.5 in fp32, k = 128 ... 254 where one exists: v = fl((k + .5) / 255) or a neighbour
    with fl(v * 255) == k + .5; s = 2 v - 1 is exact for v in [.5, 1] and s * .5 + .5 gives v back"""
    out, ks = [], []
    for k in range(128, 255):
        v0 = np.float32((k + 0.5) / 255.0)
        for v in (v0, np.nextafter(v0, np.float32(0)), np.nextafter(v0, np.float32(2))):
            s = np.float32(2.0) * v - np.float32(1.0)
            if np.float32(v * np.float32(255.0)) == np.float32(k + 0.5) and np.float32(s * np.float32(0.5) + np.float32(0.5)) == v:
                out.append(s)
                ks.append(k)
                break
    return np.array(out, np.float32), ks


def test_sr_postprocess_second_grid_stride_trip():
    """mnet_sr_postprocess over more than 65536 x 256 pixels at c_ld = 3 (f16 input; uint8 and float outputs) against the numpy sequence of
    test_kernels_gpu.py::test_sr_postprocess_matches_script, exactly.  Rounding ties: from an f16 input the product (s/2 + .5) * 255 is exact in fp32
    and only s = 0 (and the subnormals that round to it in the + .5) reaches a tie, 127.5 -> 128; an fp32 input reaches ties k + .5 with k even and
    odd, where round-half-even and round-half-up differ"""
    ops = _ops()
    assert R.sr_regime_ok()
    g = torch.Generator().manual_seed(460)
    y = ((torch.rand(R.SR_SHAPE, generator=g) - 0.5) * 3.0).to(torch.float16)                 # beyond [-1, 1] to exercise the clip
    flat = y.view(-1)
    npix = flat.numel() // 3
    for pix in (0, 255, 256, R.SR_CAP * R.WG - 1, R.SR_CAP * R.WG, R.SR_CAP * R.WG + 4097, npix - 1):      # both trips, their border, the last pixel
        flat[pix * 3:pix * 3 + 3] = torch.tensor([0.0, -0.0, 2.0 ** -24], dtype=torch.float16)
    want = np.clip((y.float() * 0.5 + 0.5).flip(3).numpy(), 0, 1) * 255.0
    assert want.dtype == np.float32 and (want.reshape(-1, 3)[R.SR_CAP * R.WG] == 127.5).all()
    yd = y.to(DEV)
    got_u = ops.sr_postprocess(yd, u8=True).cpu().numpy()
    assert got_u.shape == R.SR_SHAPE and np.array_equal(got_u, np.rint(want).astype(np.uint8))
    assert (got_u.reshape(-1, 3)[[0, R.SR_CAP * R.WG, npix - 1]] == 128).all()
    del got_u
    got_f = ops.sr_postprocess(yd, u8=False).cpu().numpy()
    assert np.array_equal(got_f, want.astype(np.float32))
    # fp32: ties at even and odd k
    s, ks = _sr_ties()
    assert sum(k % 2 == 0 for k in ks) >= 8 and sum(k % 2 == 1 for k in ks) >= 8
    t = torch.from_numpy(np.resize(s, (1, 1, s.size, 3)).copy())
    w32 = np.clip((t * 0.5 + 0.5).flip(3).numpy(), 0, 1) * 255.0
    assert (w32 - np.floor(w32) == 0.5).all()
    g32 = ops.sr_postprocess(t.to(DEV), u8=True).cpu().numpy()
    assert np.array_equal(g32, np.rint(w32).astype(np.uint8)) and (g32 % 2 == 0).all()
    assert np.array_equal(ops.sr_postprocess(t.to(DEV), u8=False).cpu().numpy(), w32.astype(np.float32))


def test_fused_bias_act_second_grid_stride_trip():
    """mnet_fused_bias_act over more than 16384 x 256 elements with an odd `inner` (the bias index (i / inner) % C in 64-bit arithmetic on the second
    trip): the fp32 sequence x + b, leaky 0.2, * sqrt 2 holds no fused multiply-add — equal to numpy's, bit for bit"""
    ops = _ops()
    assert R.fba_regime_ok()
    x, b = _rnd(R.FBA_SHAPE, 470), _rnd((R.FBA_SHAPE[1],), 471)
    y = ops.fused_bias_act(x.to(DEV), b.to(DEV)).cpu()
    v = x.numpy() + b.numpy()[None, :, None, None]
    v = np.where(v > 0, v, v * np.float32(0.2)) * np.float32(2 ** 0.5)
    assert v.dtype == np.float32
    _check("fused_bias_act 2 trips", y, F.leaky_relu(x.double() + b.double().view(1, -1, 1, 1), 0.2) * 2 ** 0.5, torch.float32)
    assert np.array_equal(y.numpy(), v)
