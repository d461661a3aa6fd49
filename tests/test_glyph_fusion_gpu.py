"""-m gpu: the AdaIN + crop + concat kernels (fused, and the three-launch form) and the ordered glyph scatter of csrc/aux_kernels.hip, through
marconet_amd.ops only, at the workload's channel counts, at the pixel-lane extremes the argument check admits and at the window edges — against fp64
references of the same operations (tests/glyph_fusion.py; tests/test_glyph_fusion.py checks those, the case tables and the bound without a device).

AdaIN, per (case, data regime, storage): one fixture launches the three call forms once and keeps every tensor alive (the caching allocator could
otherwise hand a later call a block that already holds the right answer); the tests then assert
  1. value: per element against fp64 under the bound of tests/glyph_fusion.py (fp32 / f16); the blocked storages under `_tol` x 2 of the largest value;
  2. tail: columns gw..S decode to exactly 0 in all 2C channels;
  3. feature half: channels C..2C inside the window are the feature window's storage, byte for byte;
  4. forms: adain_crop_concat == adain_crop_concat_gn(split=False) byte for byte; split=True agrees to the older test's ulp bounds;
  5. independence: a glyph launched alone, and the glyph list reversed, give the same bytes (out) and bits (scale, shift) per glyph;
  6. the GroupNorm affine against fp64 under four times the deviation of the CPU mirror (literals in tests/glyph_fusion.py).
Scatter: fp32 / f16 bit for bit against the same fp32 operations on the CPU and one rounding to the storage; the blocked storages byte for byte through
the host packer; columns no glyph owns are a byte copy of the input."""
import os
import types

import pytest
import torch

from tests import glyph_fusion as GF
from tests.test_kernels_gpu import MX, SPLIT, _tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {GF.SPLIT: _tol(SPLIT), GF.MX: _tol(MX)}
assert TOL == GF.BLOCKED_TOL
SPLIT_ULP = {GF.F16: 1e-3, GF.MX: 1e-4, GF.F32: 2e-7, GF.SPLIT: 2e-7}       # test_adain_crop_and_scatter's bound between the two forms
WORST = {}                   # storage -> worst error / bound seen so far (printed by the value test)


def _ops():
    from marconet_amd import ops
    return ops


def _raw(t):
    """the bytes of a tensor of any storage, [..., C * element size]"""
    from marconet_amd import packing
    return packing.untag(t).contiguous().view(torch.uint8)


def _host(t):
    """NHWC device tensor of any storage -> fp32 NCHW on the host (host decoder)"""
    return GF.decode(t.cpu())


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _tables(wins):
    return tuple(_i32([w[k] for w in wins]) for k in (0, 1, 3, 2))          # g_img, g_x1, g_y1, g_w


COMBOS = [(tag, regime, storage) for tag, (_, _, _, storages) in GF.ADAIN_CASES.items() for storage in storages for regime in GF.regimes(storage)]


@pytest.fixture(scope="module", params=COMBOS, ids=["-".join(c) for c in COMBOS])
def run(request):
    tag, regime, storage = request.param
    ops = _ops()
    prior, feat, wins, gamma, beta = GF.adain_inputs(tag, regime, storage)
    r = types.SimpleNamespace(tag=tag, regime=regime, storage=storage, prior=prior, feat=feat, wins=wins, gamma=gamma, beta=beta,
                              S=prior.shape[2], C=prior.shape[1], FW=feat.shape[3], G=len(wins))
    r.refs = GF.ref_adain_fp64(prior, feat, wins)
    r.d_prior, r.d_feat = GF.encode(prior, storage).to(DEV), GF.encode(feat, storage).to(DEV)
    r.d_gamma, r.d_beta = gamma.to(DEV), beta.to(DEV)
    r.tab = _tables(wins)
    r.plain = ops.adain_crop_concat(r.d_prior, r.d_feat, *r.tab)
    r.fused = ops.adain_crop_concat_gn(r.d_prior, r.d_feat, *r.tab, r.d_gamma, r.d_beta, GF.GN_EPS, split=False)
    r.split = ops.adain_crop_concat_gn(r.d_prior, r.d_feat, *r.tab, r.d_gamma, r.d_beta, GF.GN_EPS, split=True)
    torch.cuda.synchronize()
    r.host = {"fused": _host(r.fused[0]), "split": _host(r.split[0])}
    r.keep = []
    yield r
    del r


def test_value_against_fp64_per_element(run):
    r = run
    bounds = GF.adain_bound(r.prior, r.feat, r.wins, r.storage) if r.storage in (GF.F32, GF.F16) else None
    for form in ("fused", "split"):
        worst = 0.0
        for g, (img, x1, gw, y1) in enumerate(r.wins):
            got = r.host[form][g, :, :, :gw].double()
            if bounds is not None:
                ratio = ((got[:r.C] - r.refs[g][:r.C]).abs() / bounds[g])
            else:
                ratio = (got - r.refs[g]).abs() / (TOL[r.storage] * 2.0 * r.refs[g].abs().max())
            k = int(ratio.argmax())
            worst = max(worst, float(ratio.reshape(-1)[k]))
            assert float(ratio.reshape(-1)[k]) <= 1.0, "%s glyph %d %r: error / bound %.3f at channel %d" % (
                form, g, r.wins[g], float(ratio.reshape(-1)[k]), k // (r.S * gw))
        WORST[r.storage] = max(WORST.get(r.storage, 0.0), worst)
        print("adain %s %s %s %s: worst error / bound %.3f   (worst so far per storage: %s)"
              % (r.tag, r.regime, r.storage, form, worst, ", ".join("%s %.3f" % kv for kv in sorted(WORST.items()))))


def test_tail_columns_are_zero(run):
    r = run
    plain = _host(r.plain)
    for name, t in (("plain", plain), ("fused", r.host["fused"]), ("split", r.host["split"])):
        assert t.shape == (r.G, 2 * r.C, r.S, r.S)
        for g, (img, x1, gw, y1) in enumerate(r.wins):
            assert (t[g, :, :, gw:] == 0).all(), "%s glyph %d: columns %d..%d" % (name, g, gw, r.S)


def test_feature_half_is_a_raw_copy(run):
    r = run
    fraw = _raw(r.d_feat)                                   # [B, S, FW, C * es]
    half = fraw.shape[-1]
    for name, out in (("plain", r.plain), ("fused", r.fused[0]), ("split", r.split[0])):
        oraw = _raw(out)                                    # [G, S, S, 2C * es]
        assert oraw.shape[-1] == 2 * half
        for g, (img, x1, gw, y1) in enumerate(r.wins):
            assert torch.equal(oraw[g, :, :gw, half:], fraw[img, :, x1:x1 + gw, :]), "%s glyph %d" % (name, g)


def test_call_forms_agree(run):
    r = run
    assert torch.equal(_raw(r.plain), _raw(r.fused[0]))                      # one kernel, with and without the GroupNorm output
    ulp = SPLIT_ULP[r.storage]
    ratio = (r.host["split"] - r.host["fused"]).abs() / (ulp + ulp * r.host["fused"].abs())       # allclose(rtol=ulp, atol=ulp), with the figure
    k = int(ratio.argmax())
    g, c = k // (2 * r.C * r.S * r.S), (k // (r.S * r.S)) % (2 * r.C)
    print("adain %s %s %s: split vs fused, worst |d| / (ulp + ulp |fused|) = %.3f at glyph %d %r channel %d"
          % (r.tag, r.regime, r.storage, float(ratio.reshape(-1)[k]), g, r.wins[g], c))
    assert torch.allclose(r.host["split"], r.host["fused"], rtol=ulp, atol=ulp)
    assert torch.allclose(r.split[1], r.fused[1], rtol=1e-6, atol=1e-7) and torch.allclose(r.split[2], r.fused[2], rtol=1e-6, atol=1e-6)
    print("adain %s %s %s: split == fused bit for bit: %s" % (r.tag, r.regime, r.storage, bool(
        torch.equal(_raw(r.split[0]), _raw(r.fused[0])) and torch.equal(r.split[1], r.fused[1]) and torch.equal(r.split[2], r.fused[2]))))


@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
def test_a_glyph_does_not_depend_on_its_neighbours(run, split):
    r = run
    ops = _ops()
    batch = r.split if split else r.fused
    for g in range(r.G):                                                     # each glyph alone
        tab = tuple(t[g:g + 1].contiguous() for t in r.tab)
        one = ops.adain_crop_concat_gn(r.d_prior[g:g + 1], r.d_feat, *tab, r.d_gamma, r.d_beta, GF.GN_EPS, split=split)
        r.keep.append((tab, one))
        assert torch.equal(_raw(one[0])[0], _raw(batch[0])[g]), "glyph %d alone: out" % g
        assert torch.equal(one[1][0], batch[1][g]) and torch.equal(one[2][0], batch[2][g]), "glyph %d alone: GroupNorm affine" % g
    rev = torch.arange(r.G - 1, -1, -1, device=DEV)                          # the glyph list reversed
    tab = tuple(t.flip(0).contiguous() for t in r.tab)
    back = ops.adain_crop_concat_gn(ops.take_rows(r.d_prior, rev), r.d_feat, *tab, r.d_gamma, r.d_beta, GF.GN_EPS, split=split)
    r.keep.append((tab, back))
    assert torch.equal(_raw(back[0]).flip(0), _raw(batch[0]))
    assert torch.equal(back[1].flip(0), batch[1]) and torch.equal(back[2].flip(0), batch[2])


def test_groupnorm_affine_against_fp64(run):
    r = run
    tol = GF.gn_tol(r.tag, r.regime)
    for form, (_, sc, sh) in (("fused", r.fused), ("split", r.split)):
        sc, sh = sc.cpu(), sh.cpu()
        worst = [0.0, 0.0]
        for g in range(r.G):
            dev = GF.gn_deviation(sc[g], sh[g], GF.ref_gn_affine_fp64(r.refs[g], r.gamma, r.beta))
            worst = [max(worst[0], dev[0]), max(worst[1], dev[1])]
            assert dev[0] <= tol[0] and dev[1] <= tol[1], "%s glyph %d %r: scale %.3e (tol %.2e) shift %.3e (tol %.2e)" % (
                form, g, r.wins[g], dev[0], tol[0], dev[1], tol[1])
        print("adain %s %s %s %s: GroupNorm scale %.3e / %.2e  shift %.3e / %.2e" % (r.tag, r.regime, r.storage, form, worst[0], tol[0], worst[1], tol[1]))


@pytest.mark.parametrize("storage", [GF.F32, GF.F16])
def test_split_none_changes_form_at_the_glyph_count(storage, monkeypatch):
    """split=None: the three-launch form below ops.ADAIN_SPLIT_BELOW glyphs, the fused kernel from there on — the entry point that runs is counted, and
    the results are those of the explicit call, bit for bit"""
    from marconet_amd import _lib
    ops = _ops()
    if os.environ.get("MNET_ADAIN_SPLIT", "") in ("0", "1"):
        pytest.skip("MNET_ADAIN_SPLIT pins the form")
    S, C, FW, G = GF.DISPATCH_CASE
    assert G == ops.ADAIN_SPLIT_BELOW
    base = GF.adain_windows(S, FW)
    wins = [base[g % len(base)] for g in range(G)]
    gen = torch.Generator().manual_seed(51)
    prior = GF.quantise(torch.randn((G, C, S, S), generator=gen) * 1.5 + 0.2, storage)
    feat = GF.quantise(torch.randn((2, C, S, FW), generator=gen), storage)
    gamma, beta = (torch.randn((2 * C,), generator=gen).abs() + 0.5).to(DEV), (torch.randn((2 * C,), generator=gen) * 0.3).to(DEV)
    d_prior, d_feat = GF.encode(prior, storage).to(DEV), GF.encode(feat, storage).to(DEV)
    lib = _lib.load()
    calls = []
    for name in ("mnet_adain_crop_concat_split", "mnet_adain_crop_concat_gn"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _n=name: (calls.append(_n), _fn(*a))[1])
    keep = []
    for n, want_split in ((G - 1, True), (G, False)):
        tab = _tables(wins[:n])
        res = {}
        for key, split in (("none", None), ("true", True), ("false", False)):
            del calls[:]
            res[key] = ops.adain_crop_concat_gn(d_prior[:n], d_feat, *tab, gamma, beta, GF.GN_EPS, split=split)
            assert calls == ["mnet_adain_crop_concat_split" if (want_split if split is None else split) else "mnet_adain_crop_concat_gn"], (n, key)
        torch.cuda.synchronize()
        keep.append((tab, res))
        same = res["true" if want_split else "false"]
        assert torch.equal(_raw(res["none"][0]), _raw(same[0])) and torch.equal(res["none"][1], same[1]) and torch.equal(res["none"][2], same[2])
        refs = GF.ref_adain_fp64(prior[:n], feat, wins[:n])                  # ... and both forms are right at this glyph count
        bounds = GF.adain_bound(prior[:n], feat, wins[:n], storage)
        for key in ("true", "false"):
            got = _host(res[key][0])
            for g in (0, 1, n - 2, n - 1):
                gw = wins[g][2]
                assert ((got[g, :C, :, :gw].double() - refs[g][:C]).abs() <= bounds[g]).all(), (n, key, g)
                assert (got[g, :, :, gw:] == 0).all()


# ====================================================================================================================== scatter
SCATTER = [(tag, storage) for tag, case in GF.SCATTER_CASES.items() for storage in case[5]]


@pytest.mark.parametrize("tag,storage", SCATTER, ids=["-".join(c) for c in SCATTER])
def test_scatter_bit_exact(tag, storage):
    ops = _ops()
    S, C, FW, counts, wins, _ = GF.SCATTER_CASES[tag]
    g_start, g_x1, g_w = GF.scatter_tables(tag)
    feat, scale, shift = GF.scatter_inputs(tag, storage)
    want = GF.ref_scatter(feat, scale, shift, g_start, g_x1, g_w)            # fp32: fl(fl(f * sc) + sh), then fl(f + .), from the values the storage holds
    assert want.dtype == torch.float32
    d_feat = GF.encode(feat, storage).to(DEV)
    d_in = d_feat.clone()
    out = ops.glyph_scatter_affine(d_feat, GF.encode(scale, storage).to(DEV), GF.encode(shift, storage).to(DEV), _i32(g_start), _i32(g_x1), _i32(g_w))
    torch.cuda.synchronize()
    assert torch.equal(_raw(d_feat), _raw(d_in))                             # the input is read, never written
    oraw, fraw = _raw(out).cpu(), _raw(d_feat).cpu()                         # [B, S, FW, C * es]
    own = GF.scatter_owner(tag)
    for b in range(len(counts)):
        free = torch.from_numpy(own[b] < 0)
        assert torch.equal(oraw[b][:, free], fraw[b][:, free]), "image %d: a column no glyph owns is a copy of the input" % b
        if counts[b] == 0:
            assert torch.equal(oraw[b], fraw[b]), "image %d has no glyphs" % b
    if storage == GF.F32:
        assert torch.equal(_host(out), want)
    elif storage == GF.F16:
        assert torch.equal(out.cpu().permute(0, 3, 1, 2), want.half())       # one rounding to the storage
    else:
        enc = _raw(GF.encode(want, storage))
        diff = (enc != oraw).any(-1)
        got = _host(out)
        print("scatter %s %s: bytes differ from the host packer's at %d of %d pixels; max |decoded - fp32 result| %.3e"
              % (tag, storage, int(diff.sum()), diff.numel(), float((got - want).abs().max())))
        assert torch.equal(oraw, enc)
