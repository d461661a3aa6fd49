"""CPU tier of the operand-range contract (tests/conv_range.py): the scene holds every class it claims, every family's reference is the header's sum, the
bound leaves the reference's own fp32 evaluation an 8-fold margin, and every mutant of the k-loop breaks it by 4x or more in the classes it targets."""
import numpy as np
import pytest

from tests import conv_range as R
from tests import storage_codec as S

SMALL = [("a", "none"), ("a", "concat"), ("b", "none"), ("b", "concat"), ("d", "none"), ("a1", "none")]


@pytest.mark.parametrize("sname,src2", SMALL)
def test_scene_census(sname, src2):
    sc = R.scene(sname, src2 != "none", "mx")
    K = R.SHAPES[sname][6] ** 2 * (R.SHAPES[sname][3] + (R.SHAPES[sname][4] if src2 != "none" else 0))
    rg = R.band_ranges(K)
    o0 = R.BAND_OFFSET.get(sname, 0)
    for src, off in (("x0", o0), ("x1", o0 + 1)):
        x = sc[src]
        if x is None:
            continue
        n, h, w, C = x.shape
        B = C // 32
        p = R.act_parts(R.act_bytes(x, "mx"), "mx")
        E = p["E"].reshape(n, h, w, B, 32)[..., 0]
        hi = p["hi"].reshape(n, h, w, B, 32)
        m = np.abs(hi).max(-1)
        band = np.array([R.column_band(c, off) for c in range(w)])
        for img in range(n):
            cnt = {}
            for bi, name in enumerate(R.BANDS):
                e, mm = E[img][:, band == bi], m[img][:, band == bi]
                if name == "sub":
                    ok = (e == 105) & (mm >= 2.0 ** -24) & (mm < 2.0 ** -15)
                elif name == "small":
                    ok = (mm >= 2.0 ** -14) & (mm < 2.0 ** -7)
                elif name == "unit":
                    ok = (mm >= 2.0 ** rg["unit"][0]) & (mm < 2.0 ** (rg["unit"][1] + 1))
                elif name == "large":
                    ok = (mm >= 2.0 ** rg["large"][0]) & (mm < 2.0 ** (rg["large"][1] + 1))
                elif name == "mixed":
                    ok = np.ones_like(e, dtype=bool)
                    if B > 1:
                        assert (np.abs(e[..., 0] - e[..., 1]) >= 6).all(), "mixed band: blocks of a pixel less than 2^6 apart"
                    else:
                        assert (np.abs(np.diff(e[..., 0], axis=1)) >= 6).all()
                else:
                    ok = np.ones_like(e, dtype=bool)
                    cols = np.nonzero(band == bi)[0]
                    allz = (cols % R.BAND_W) < R.ZERO_COLS
                    assert (e[:, allz] == 0).all()
                    cnt["zero_pixel"] = int(allz.sum()) * h * B
                    beside = e[:, ~allz]
                    if B > 1:
                        assert ((beside == 0).sum(-1) == 1).all(), "zero band: one zero block beside a live one"
                    cnt["zero_block"] = int((beside == 0).sum())
                    zb = hi[img][:, band == bi][e == 0]
                    assert (zb == 0).all() and np.signbit(zb).any(axis=-1).all() and (~np.signbit(zb)).any(axis=-1).all(), "E = 0 blocks hold +0 and -0 halves"
                assert ok.all(), "%s band of %s holds blocks outside its class" % (name, src)
                cnt.setdefault(name, int(ok.sum()))
            assert all(v >= 32 for v in cnt.values()), cnt
            vals = set(np.unique(E[img]).tolist())
            assert {0, 105} <= vals and len(vals - {0, 105}) >= 12, sorted(vals)
            adj = (E[img][:, 1:] != E[img][:, :-1])
            assert adj.mean() >= 0.5
    # image 0 is coherent: positive, each element above its half by 0.2 .. 0.45 of the half's step (up to the fp32 cast)
    v = sc["x0"][0].astype(np.float64)
    h16 = S.f16_round(v)
    res = (v - h16) / R._ulp16(h16)
    live = v != 0
    assert (v >= 0).all() and (res[live] > 0.19).all() and (res[live] < 0.46).all()
    if sc["x0"].shape[0] > 1:
        assert (np.abs(sc["x0"][1]) == np.abs(sc["x0"][0])).all() and (sc["x0"][1] < 0).any()
    assert S.weight_rows_defined(S.stored_weight_values(sc["w"], "mx"))
    for fam in R.FAMILIES:
        c = R.case(R._STORAGE_OF[fam], sname, src2, family=fam)
        assert float(np.abs(c.ref()).max()) < 2.0 ** 15
        assert int((c.A() == 0).sum()) >= 32, "no exact-zero outputs"


def test_big_scene_is_the_small_one_tiled():
    sc = R.scene("c64", False, "mx")
    x = sc["x0"]
    assert x.shape == (1, 128, 512, 64)
    assert (x[0, :3] >= 0).all() and (x[0, 125:] < 0).any()
    E = R.act_parts(R.act_bytes(np.concatenate([x[0, :3], x[0, 125:]]), "mx"), "mx")["E"]
    assert {0, 105} <= set(np.unique(E).tolist())
    for fam in ("f16", "split", "mx_dma"):
        for sname in ("c64", "c256"):
            assert float(np.abs(R.case(R._STORAGE_OF[fam], sname, family=fam).ref()).max()) < 2.0 ** 15


def test_the_parsed_operands_are_the_spec_s_bytes():
    """the parts the references multiply are read back from the bytes the kernels get: the host packer's weight bytes are the spec's, and the parts of
    an activation sum to the spec decoder's value"""
    import torch
    from marconet_amd import packing
    for storage in ("f16", "split", "mx"):
        c = R.case(storage, "b", "concat")
        got = packing.untag(c.wpacked).contiguous().view(-1).view(torch.uint8).numpy()
        want = S.encode_weight(S.stored_weight_values(c.w_true, storage), storage)
        assert np.array_equal(got[: want.size], want), storage
        dec = S.DECODE[storage](c.raw0).view(np.float32).astype(np.float64)
        assert np.array_equal(R.stored_value(c.raw0, storage).astype(np.float32).astype(np.float64), dec)


# the format's own error of each family against the fp64 convolution of the STORED activations and the TRUE weights: (relative to sum |W||X|,
# absolute per live tap in units of |W|), term by term from the header:
#   f16      W is stored as f16(W): 2^-11 |W|
#   split    256 W - hi - lo <= half a step of lo (2^-11 |lo| <= 2^-22 |256 W|, or 2^-25 under a lo of 2^-15 .. 2^-14 with 256 W >= 2^-6: 2^-19) and the
#            dropped lo*lo product (2^-11 * 2^-11)
#   fp16+8   LDS-DMA: x_hi8 = e4m3(hi / s) carries 2^-4 relative (3 mantissa bits) under w_lo <= 2^-11 |W|: 2^-15; w_hi8 likewise under x_lo8 <= 2^-11 |X|:
#            2^-15; the weights' lo8 byte itself, 2^-4 of a lo of 2^-11: 2^-15 — 1.5 * 2^-14 — plus lo*lo, 2^-22.  In an fp16-subnormal block x_lo is not
#            2^-11 of x but up to 2^-25 absolute: 2^-4 * 2^-25 |W| and lo*lo 2^-11 * 2^-25 |W| per tap
#            register-staged: the weights' lo8 byte (2^-15), lo*lo (2^-22), a lo byte decoded to a half that underflows: 2^-25 per activation, and the same
#            on a weight row 2^-6 down (lo of 2^-16 against 256 W >= 2^-6: 2^-19)
FORMAT_ERROR = {"f32": (2.0 ** -50, 0.0), "f16": (2.0 ** -11, 0.0), "split": (2.0 ** -19 + 2.0 ** -22, 0.0),
                "mx_dma": (1.5 * 2.0 ** -14 + 2.0 ** -22, 2.0 ** -29 + 2.0 ** -36), "mx_reg": (2.0 ** -15 + 2.0 ** -19 + 2.0 ** -22, 2.0 ** -25)}


_REF_CASES = [(f, s, t) for f in R.FAMILIES for s, t in SMALL + [("c64", "none")] if s != "d" or f.startswith("mx")]       # (the polyphase shape: fp16+8 only)


@pytest.mark.parametrize("fam,sname,src2", _REF_CASES)
def test_reference_is_the_convolution_up_to_the_format_s_error(fam, sname, src2):
    storage = R._STORAGE_OF[fam]
    c = R.case(storage, sname, src2, family=fam)
    xs = [R.stored_value(r, storage) for r in ((c.raw0, c.raw1) if c.raw1 is not None else (c.raw0,))]
    X = c.P(np.concatenate(xs, axis=-1))
    W = np.ascontiguousarray(c.w_true.transpose(0, 2, 3, 1)).reshape(c.cout, -1).astype(np.float64)
    exact = X @ W.T
    rel, ab = FORMAT_ERROR[fam]
    bound = rel * (np.abs(X) @ np.abs(W).T) + ab * ((X != 0).astype(np.float64) @ np.abs(W).T)
    err = np.abs(c.ref() - exact)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s %s %s: reference vs fp64 convolution, worst err / format bound %.3f; err / sum|W||X| %.3e" % (
        fam, sname, src2, worst, float((err / np.maximum(np.abs(X) @ np.abs(W).T, 1e-300)).max())))
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_margin_of_the_reference_alone_and_the_pinned_gamma(fam):
    got = R.measure_gamma(families=(fam,))
    assert got == {k: v for k, v in R.GAMMA.items() if k[0] == fam}, got
    for (f, K), g in got.items():
        assert g <= R.ceiling(K), (f, K, g / R.ceiling(K))
    for sname, src2 in R.GAMMA_CASES:
        if sname == "d" and not fam.startswith("mx"):
            continue
        c = R.case(R._STORAGE_OF[fam], sname, src2, family=fam)
        b = c.bound(gamma=R.GAMMA[(c.fam, c.K)])
        for order in (0, 1):
            err = np.abs(c.eval32(order) - c.ref())
            assert (err * 8.0 <= b * (1 + 2.0 ** -40)).all(), (fam, sname, src2, order, float((err / np.maximum(b, 1e-300)).max()))
            assert (c.eval32(order)[c.A() == 0] == 0).all()


def _class_masks(c, classes):
    """class name -> boolean [P, cout] of the outputs of the coherent image that belong to it"""
    P, cout = c.ref().shape
    img0 = (c.out_images() == 0)[:, None]
    bands, rows = c.out_bands()[:, None], c.row_classes()[None, :]
    out = {}
    for name in classes:
        if name.startswith("w:"):
            out[name] = img0 & (bands >= 0) & (rows == R.WCLASSES.index(name[2:]))
        else:
            out[name] = img0 & (bands == R.BANDS.index(name)) & np.ones((1, cout), dtype=bool)
    return out


_TEETH = [("mx_dma", m) for m in R.MX_MUTANTS] + [("split", m) for m in R.SPLIT_MUTANTS] + [("mx_reg", m) for m in R.SPLIT_MUTANTS]


@pytest.mark.parametrize("sname", ["a", "b"])
@pytest.mark.parametrize("fam,mutant", _TEETH)
def test_every_mutant_breaks_the_bound_fourfold_in_the_classes_it_targets(fam, mutant, sname):
    c = R.case(R._STORAGE_OF[fam], sname, "none", family=fam)
    targets = (R.MX_MUTANTS if fam == "mx_dma" else R.SPLIT_MUTANTS)[mutant]
    ratio = np.abs(c.mutant(mutant) - c.ref()) / np.maximum(c.bound(gamma=R.GAMMA[(c.fam, c.K)]), 1e-300)
    worst = {name: float(ratio[m].max()) for name, m in _class_masks(c, targets).items()}
    print("%s %s %s: worst error / bound per class %s" % (fam, mutant, sname, worst))
    assert all(v >= 4.0 for v in worst.values()), worst
    # against the ceiling K * 2^-24 (printed for every family; asserted for those that fell back to it: conv_range.CEILING_FAMILIES)
    ratio = np.abs(c.mutant(mutant) - c.ref()) / np.maximum(c.bound(gamma=R.ceiling(c.K)), 1e-300)
    worst_c = {name: float(ratio[m].max()) for name, m in _class_masks(c, targets).items()}
    print("   against the ceiling: %s" % worst_c)
    assert fam not in R.CEILING_FAMILIES or all(v >= 4.0 for v in worst_c.values()), worst_c
