"""CPU tier of the conv geometry contract (tests/conv_geometry.py): the table is what it says it is, the variants are a deterministic all-pairs
cover, the explicit-padding fp64 reference equals both torch's padded convolution and a literal evaluation of the header formula, the reference's own
arithmetic leaves the per-type bounds their headroom, and mnet_conv2d_plan answers every (storage, request, row, variant) as include/marconet_hip.h
says — which also fixes, from the header's rules alone, the launches the GPU tier (test_conv_geometry_gpu.py) must run."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests import conv_contract as C
from tests import conv_geometry as G

STORAGES = ("f32", "f16", "split", "mx")
_DTYPE = {"f32": 0, "f16": 1, "split": 2, "mx": 3}
_ADDR = 1 << 20          # any 128-byte aligned address: the planner checks presence and alignment of a buffer, never what is behind it
_BARE = G.to_row(dict(epi="bare", valid_w="none", src2="none", extra="none"))


def _small():
    return [r for r in G.ROWS if not G.flag(r, "big")]


def test_rows_are_what_the_table_says():
    """conv_prepare's ho/wo rule gives the stated output size, the '*' rows have ho*wo % 32 == 0 (and only they), both pixel-decode kinds occur"""
    pow2 = lambda v: v & (v - 1) == 0
    kinds = set()
    for rname, geo in G.ROWS.items():
        n, h, w, kh, kw, (sh, sw), (ph, pw) = geo[:7]
        ho, wo = G.out_size(geo)
        assert h + 2 * ph >= kh and w + 2 * pw >= kw and ho > 0 and wo > 0, rname
        assert (ho, wo) == G.OUT[rname], rname
        assert ((ho * wo) % 32 == 0) == G.flag(rname, "m32"), rname
        assert G.flag(rname, "same") == ((ho, wo) == (h, w) and (sh, sw) == (1, 1) and kh % 2 == 1 and kw % 2 == 1 and (ph, pw) == (kh // 2, kw // 2)), rname
        assert G.flag(rname, "big") == (n * ho * wo >= 65536), rname
        assert G.flag(rname, "big") or n == 4
        kinds.add(pow2(ho * wo) and pow2(wo))
        assert len(G.valid_widths(geo)) == n and min(G.valid_widths(geo)) == (0 if n == 4 else 300)
    assert kinds == {True, False}
    # the geometries the issue names as never run: stride on w only, stride 3, a remainder in (h + 2p - k) % stride, a 32-tap filter
    geos = list(G.ROWS.values())
    assert any(g[5] == (1, 2) for g in geos) and any(g[5] == (3, 3) for g in geos)
    assert any((g[1] + 2 * g[6][0] - g[3]) % g[5][0] for g in geos) and any(g[3] * g[4] == 32 for g in geos)


@pytest.mark.parametrize("storage", STORAGES)
def test_variants_cover_every_pair_and_are_deterministic(storage):
    for req in C.requests(storage):
        for rname in _small():
            lv = G.g_levels(storage, req, rname)
            seed = 7 + list(G.ROWS).index(rname)
            gs = C.all_pairs(lv, seed, G.G_NAMES)
            covered = set()
            for g in gs:
                assert set(g) == set(G.G_NAMES) and all(g[f] in lv[f] for f in G.G_NAMES)
                covered |= C.row_pairs(g, G.G_NAMES)
            for a, b in itertools.combinations(G.G_NAMES, 2):
                for la in lv[a]:
                    for lb in lv[b]:
                        assert ((a, la), (b, lb)) in covered, (storage, req, rname, a, la, b, lb)
            assert gs == C.all_pairs(lv, seed, G.G_NAMES)
            big = sorted((len(v) for v in lv.values()), reverse=True)
            assert len(gs) <= 2 * big[0] * big[1]                    # a greedy cover stays near the lower bound
        assert G.launches(storage, req) == G.launches(storage, req)
    # 'center' only where the header allows it; 'gn' only on fp16+8 'same' rows; transforms on the register-staged request only
    for req in C.requests(storage):
        for rname, ch, vname, row in G.launches(storage, req):
            assert row["src2"] != "center" or (G.flag(rname, "same") and storage != "f32")
            assert row["gn"] == "off" or (G.flag(rname, "same") and storage == "mx")
            assert row["xform"] == "none" or req == "reg"


@pytest.mark.parametrize("rname", list(G.ROWS))
def test_explicit_padding_reference_equals_torch_padding(rname):
    """fp64, decoded f32 operands: the reference built from the definition against F.conv2d(..., padding=(ph, pw)) (on the big maps: on the top,
    middle and bottom slabs of input rows that hold the reference rows' windows)"""
    geo = G.ROWS[rname]
    n, h, w, kh, kw, (sh, sw), (ph, pw) = geo[:7]
    chans = (8, 16, 12) if not G.flag(rname, "big") else (64, 64, 64 if rname == "big1x3" else 256)
    op = G.operands("f32", rname, chans)
    for vwl in ("none", "ragged"):
        row = dict(_BARE, src2="concat", valid_w=vwl)
        got = op.conv(row, "dec")
        x = op.xprime(row).clone()
        if vwl == "ragged":
            for i, v in enumerate(op.vws):
                x[i, :, :, v:] = 0
        wt = op.weights(row, "dec").double()
        if not op.big:
            ref = F.conv2d(x.double(), wt, stride=(sh, sw), padding=(ph, pw))
            assert ref.shape == got.shape and float((ref - got).abs().max()) <= 1e-13 * float(ref.abs().max())
            continue
        ho = op.ho
        top = F.conv2d(x[:, :, :2 * sh + kh].double(), wt, stride=(sh, sw), padding=(ph, pw))[:, :, :2]
        lo_in = (ho // 2 - 1) * sh - ph                                  # first input row of the middle reference rows: no padding row involved
        mid = F.conv2d(x[:, :, lo_in:lo_in + sh + kh].double(), wt, stride=(sh, sw), padding=(0, pw))[:, :, :2]
        first = (ho - 2) * sh - ph
        bot = F.conv2d(F.pad(x[:, :, first:].double(), (0, 0, 0, ph)), wt, stride=(sh, sw), padding=(0, pw))[:, :, :2]    # (the slab's bottom rows padded by hand)
        ref = torch.cat([top, mid, bot], dim=2)[..., :op.wo]
        assert ref.shape == got.shape and float((ref - got).abs().max()) <= 1e-13 * float(ref.abs().max())


@pytest.mark.parametrize("rname", ["1x1pad", "3x3beyond", "3x3s22a"])
def test_reference_equals_the_header_formula_written_out(rname):
    """three tiny rows (windows with no tap, a map smaller than its filter, pad_h != pad_w with a stride remainder): the reference against four
    literal loops over the header formula, ragged valid_w (a 0 included) and the loaded epilogue — the reference is pinned to the header, not to torch"""
    for storage, chans in (("f32", (8, 16, 12)), ("mx", (32, 32, 32))):
        op = G.operands(storage, rname, chans)
        for g in (dict(epi="loaded", valid_w="ragged", src2="concat", extra="none"), dict(epi="bare", valid_w="none", src2="none", extra="none"),
                  dict(epi="loaded", valid_w="ragged", src2="none", extra="swish")):
            row = G.to_row(g)
            ref, lit = op.reference(row, "dec"), G.four_loops(op, row)
            assert float((ref - lit).abs().max()) <= 1e-12 * max(float(lit.abs().max()), 1.0), (rname, storage, g)
            # outputs without a live tap hold the epilogue of an exact zero
            dead = ~G.live_mask(op.geo, op.vws if g["valid_w"] == "ragged" else None)
            zero = op.epilogue(row, torch.zeros_like(ref))
            sel = dead[:, None].expand_as(ref)
            assert torch.equal(ref[sel], zero[sel])
            if rname != "3x3s22a":
                assert bool(dead.any())


def test_center_variant_is_the_sum_of_two_convolutions():
    """MNET_CONV_ALGO_FLAG_X1_CENTER as the header writes it: conv_khxkw(x0; W[..., :c0]) + conv_1x1(x1; W[:, kh/2, kw/2, c0:])"""
    for rname in ("1x3", "3x1", "5x5", "h1"):
        op = G.operands("f16", rname, (64, 64, 96))
        n, h, w, kh, kw, (sh, sw), (ph, pw) = op.geo[:7]
        row = G.to_row(dict(epi="bare", valid_w="ragged", src2="center", extra="none"))
        x = op.x.clone().double()
        for i, v in enumerate(op.vws):
            x[i, :, :, v:] = 0
        wt = op.wt.double()
        ref = F.conv2d(x[:, :64], wt[:, :64], padding=(ph, pw)) + F.conv2d(x[:, 64:], wt[:, 64:, kh // 2:kh // 2 + 1, kw // 2:kw // 2 + 1])
        got = op.conv(row, "dec")
        assert float((ref - got).abs().max()) <= 1e-13 * float(ref.abs().max())


@pytest.mark.parametrize("rname", list(G.ROWS))
def test_reference_arithmetic_leaves_the_bounds_their_headroom(rname):
    """the bounds the GPU tier applies (_tolerances of the epilogue contract, unchanged) against what plain fp32 / f16 / fp16+8 arithmetic of the
    same operands gives on the CPU, relative to the output scale like the GPU tier: fp32 F.conv2d of the stored operands within a quarter of the f32
    bound (2e-5), with f16 output rounding within a quarter of the f16 bound (5e-3), the fp16+8 three-product emulation within half of the 'true'
    bound (4e-5).  Measured on the 1x1 ... 8x4 rows (K = 64 ... 4096) and the 8-channel variant: <= 5.1e-7, <= 3.9e-4, <= 1.1e-5.  A kernel that
    drops one tap moves a pixel by about 4e-2 of the output maximum on the 32-tap rows, more on the others."""
    from tests.test_conv_epilogue_contract_gpu import _tolerances
    big = G.flag(rname, "big")
    row = dict(_BARE, src2="concat", valid_w="ragged")
    chan_sets = [(64, 64, 64)] if big else [(64, 64, 96), (8, 16, 12)]
    tol32, tol16 = _tolerances("f32", C.ALGO_REG, row)[0][1], _tolerances("f16", C.ALGO_REG, row)[0][1]
    tolmx = dict(_tolerances("mx", C.dma(6), row))["true"]
    assert (tol32, tol16, tolmx) == (2e-5, 5e-3, 4e-5)
    for chans in chan_sets:
        op = G.operands("f32", rname, chans)
        ref = op.conv(row, "dec")
        scale = float(ref.abs().max())
        assert float((op.conv(row, "f32") - ref).abs().max()) <= 0.25 * tol32 * scale, (rname, chans)
        op = G.operands("f16", rname, chans)
        ref = op.conv(row, "dec")
        scale = float(ref.abs().max())
        assert float((op.conv(row, "f32").half().double() - ref).abs().max()) <= 0.25 * tol16 * scale, (rname, chans)
    if not big:
        op = G.operands("mx", rname, (64, 64, 96))
        ref = op.conv(row, "true")
        assert float((op.conv(row, "emu") - ref).abs().max()) <= 0.5 * tolmx * float(ref.abs().max()), rname


def _desc(storage, rname, chans, row):
    from marconet_amd import _lib
    n, h, w, kh, kw, (sh, sw), (ph, pw) = G.ROWS[rname][:7]
    c0, c1, cout = chans
    d = _lib.ConvDesc()
    d.dtype = _DTYPE[storage]
    d.x0, d.c0 = _ADDR, c0
    d.x1, d.c1 = (None, 0) if row["src2"] == "none" else (_ADDR, c1)
    d.n, d.h, d.w = n, h, w
    d.wgt, d.y = _ADDR, _ADDR
    d.cout, d.kh, d.kw = cout, kh, kw
    d.stride_h, d.stride_w, d.pad_h, d.pad_w = sh, sw, ph, pw
    d.ho, d.wo = G.out_size(G.ROWS[rname])
    xf = row["xform"] != "none"
    d.in_scale, d.in_shift, d.in_swish = (_ADDR if xf else None), (_ADDR if xf else None), int(row["xform"] == "swish")
    d.valid_w = _ADDR if row["valid_w"] != "none" else None
    d.out_scale = _ADDR if row["out_scale"] != "none" else None
    d.bias = _ADDR if row["bias"] != "none" else None
    d.residual = _ADDR if row["residual"] != "none" else None
    d.res_mod, d.act = 0, row["act"]
    d.post_scale = None
    d.gn_partial = _ADDR if row["gn"] == "on" else None
    return d


@pytest.mark.parametrize("storage", STORAGES)
def test_planner_equals_the_expectation_table(storage):
    """mnet_conv2d_plan for every (request, row, channels, variant) against what the header's rules give (G.expected): LDS-DMA eligible iff the
    channel rules hold and kh*kw <= 32 and kh, kw <= 8; strip only 3x3 / stride 1 / pad 1 on >= 65536 pixels; skinny only fp32 1x1 / stride 1 / pad 0;
    gn_partial only 'same'-size stride-1 fp16+8; the folded skip on odd 'same' filters; fp16+8 id 16 -> 15 when ho*wo % 32 != 0, id 9 -> 8 with
    GroupNorm sums.  The counts below are the launches the GPU tier must run: fixed here from the rules, not from what happens to run there."""
    from marconet_amd import _lib
    lib = _lib.load()
    bad, ran = [], {}
    for req, (algo, family) in sorted(C.requests(storage).items()):
        ran[req] = set()
        for rname, ch, vname, row in G.launches(storage, req):
            a = algo | (C.FLAG_X1_CENTER if row["src2"] == "center" else 0)
            k = int(lib.mnet_conv2d_plan(ctypes.byref(_desc(storage, rname, ch, row)), a))
            exp = G.expected(storage, req, rname, ch, row)
            msg = G.plan_mismatch(storage, exp, k, rname)
            if msg:
                bad.append("%s %s %s %s %s: %s" % (storage, req, rname, ch, vname, msg))
            if exp[0] != "refused":
                ran[req].add(rname)
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:40]))
    small = set(_small())
    eligible = small - {"6x6", "8x8s8"}
    for req, rows in ran.items():
        if req in ("reg", "auto"):
            assert rows == set(G.ROWS)                               # every row runs, the big maps included
        elif req == "skinny":
            assert rows == {"1x1"}
        elif req.startswith("strip"):
            assert rows == set()                                     # no row of the table is 3x3 / stride 1 / pad 1 on a big map
        else:                                                        # a pinned LDS-DMA id: every eligible row (and the big maps for the big-tile ids)
            assert rows & small == eligible, (req, sorted(eligible - rows))
            assert (rows - small == {"big1x3", "big3x3s2"}) == C.uses_shape(req, "big64")
    # fp16+8 id 16 runs itself on every '*' row and hands pad40 to id 15
    if storage == "mx":
        for rname, ch, vname, row in G.launches("mx", "dma16"):
            exp = G.expected("mx", "dma16", rname, ch, row)
            if exp[0] == "dma":
                assert exp[1] == (16 if G.flag(rname, "m32") else 15), rname
