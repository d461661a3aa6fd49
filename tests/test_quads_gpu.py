"""-m gpu: the quadrilateral page path on the device (mnet_quad_crop_u8, mnet_quad_paste_u8, quads.compose_page_quads,
MarconetPipeline.restore_page_quads) against the pure-host definition quads.warp_crop_host / warp_paste_host / compose_quads_host — byte for byte:
every comparison is np.array_equal.  The host references are computed once per module."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from marconet_amd import _lib, lq_io, ops, pages, quads
from tests.golden import cases_png
from tests.long_lines_cases import golden_line

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE_H, PAGE_W, GUARD = 70, 150, 4096
GENERAL = [(20.25, 8.5), (120.0, 14.75), (118.5, 40.0), (17.0, 30.5)]
BEYOND = [(120.0, 50.0), (165.0, 45.0), (170.0, 80.0), (125.0, 85.0)]          # reaches beyond the page's right edge and its bottom


def _orientations(x1, y1, x2, y2):
    tl, tr, br, bl = (x1, y1), (x2, y1), (x2, y2), (x1, y2)
    return {0: [tl, tr, br, bl], 1: [tr, br, bl, tl], 2: [br, bl, tl, tr], -1: [bl, tl, tr, br]}


def _crop_case(name, q, c0=0, w=None):
    cw, ch = quads.crop_size(q)
    return dict(name=name, M=quads.quad_map(q, cw, ch), w=cw - c0 if w is None else w, h=ch, c0=c0)


# ------------------------------------------------------------------------------------------------------------------------ the gather in
CROPS = [_crop_case("right angle, k = %d" % k, q) for k, q in _orientations(13, 7, 60, 29).items()] + [
    _crop_case("the general quadrilateral: 101 x 24, over tile column 63|64 and tile row 15|16", GENERAL),
    _crop_case("beyond two page edges", BEYOND),
    _crop_case("a window with c0 > 0", GENERAL, c0=37, w=40),
    _crop_case("wider than 64 and higher than 16 at a right angle", _orientations(2, 1, 149, 69)[1]),
    _crop_case("1 x 1", quads.box_quad([149, 69, 150, 70])),
]


@pytest.fixture(scope="module")
def crop_data():
    """a random page on the host and on the device + the host crop of every case, computed once"""
    page = np.random.default_rng(20241020).integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    want = [quads.warp_crop_host(page, c["M"], c["w"], c["h"], c["c0"]) for c in CROPS]
    assert (CROPS[4]["w"], CROPS[4]["h"]) == (101, 24) and (CROPS[7]["w"], CROPS[7]["h"]) == (68, 147) and (CROPS[8]["w"], CROPS[8]["h"]) == (1, 1)
    assert np.array_equal(want[0], page[7:29, 13:60]) and np.array_equal(want[1], np.rot90(page[7:29, 13:60], 1))
    assert np.array_equal(want[6], quads.warp_crop_host(page, CROPS[4]["M"], 101, 24)[:, 37:77])
    return dict(page=page, page_d=torch.from_numpy(page).to(DEV), want=want)


def _crop_table(sel):
    """the cases ``sel`` packed with a gap of 1, 2, 3 ... bytes before each, so that the offsets are odd and even and no multiple of a pixel"""
    tab = np.zeros((len(sel),), dtype=np.dtype(_lib.QuadCrop))
    off = 0
    for j, r in enumerate(sel):
        c = CROPS[r]
        off += j + 1
        tab[j] = (off, c["w"], c["h"], c["c0"], 0, c["M"])
        off += 3 * c["w"] * c["h"]
    return tab, off + 5


def _crop_launch(d, tab, size):
    buf = torch.full((size + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    dst = buf[GUARD:GUARD + size]
    ops.quad_crop_u8(d["page_d"], ops.table_to_device(tab, DEV), int(max(tab["w"].max(), 1)), int(max(tab["h"].max(), 1)), dst)
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + size], (host[:GUARD], host[GUARD + size:])


def _crop_check(d, sel, tab, size, got, guards, untouched=()):
    expect = np.full((size,), 0xCD, np.uint8)
    for j, r in enumerate(sel):
        if j in untouched:
            continue
        o, n = int(tab["offset"][j]), d["want"][r].size
        expect[o:o + n] = d["want"][r].reshape(-1)
        assert np.array_equal(got[o:o + n], expect[o:o + n]), CROPS[r]["name"]
    assert np.array_equal(got, expect)                                            # and the gaps between the crops are untouched
    assert all((g == 0xCD).all() for g in guards)


def test_crop_batch_equals_host(crop_data):
    sel = list(range(len(CROPS)))
    tab, size = _crop_table(sel)
    assert any(o % 2 for o in tab["offset"]) and any(o % 3 for o in tab["offset"])
    got, guards = _crop_launch(crop_data, tab, size)
    _crop_check(crop_data, sel, tab, size, got, guards)


def test_crop_is_batch_invariant(crop_data):
    for r in range(len(CROPS)):
        tab, size = _crop_table([r])
        got, guards = _crop_launch(crop_data, tab, size)
        _crop_check(crop_data, [r], tab, size, got, guards)


def _nan_coefficient(tab, size):
    tab["m"][1][7] = float("nan")


CROP_BAD = (
    ("negative offset", lambda tab, size: tab["offset"].__setitem__(1, -1)),
    ("the crop's end past dst_bytes", lambda tab, size: tab["offset"].__setitem__(1, size - 10)),
    ("an offset past dst_bytes", lambda tab, size: tab["offset"].__setitem__(1, size + 1)),
    ("an offset near 2^63", lambda tab, size: tab["offset"].__setitem__(1, 2 ** 63 - 2)),
    ("w = 0", lambda tab, size: tab["w"].__setitem__(1, 0)),
    ("negative h", lambda tab, size: tab["h"].__setitem__(1, -3)),
    ("negative c0", lambda tab, size: tab["c0"].__setitem__(1, -1)),
    ("a NaN coefficient", _nan_coefficient),
)


@pytest.mark.parametrize("name,edit", CROP_BAD, ids=[b[0] for b in CROP_BAD])
def test_unfollowable_crop_leaves_its_bytes_and_its_neighbours_stand(crop_data, name, edit):
    sel = [0, 5, 8]
    tab, size = _crop_table(sel)
    edit(tab, size)
    got, guards = _crop_launch(crop_data, tab, size)
    _crop_check(crop_data, sel, *_crop_table(sel), got, guards, untouched=(1,))


# ----------------------------------------------------------------------------------------------------------------------- the gather out
N_LINES, ROWS, LINE_W = 4, 16, 96
# (name, corners in the page, (rw, rh) of the upright foreground, line_index, src_w): disjoint quadrilaterals of the 150 x 70 page; k follows from rh at rows = 16
REGIONS = (
    ("a general quadrilateral, k = 1", [(10.25, 5.5), (80.0, 9.75), (78.5, 30.0), (8.0, 24.5)], (60, 16), 2, 37),
    ("read top to bottom, k = 2", _orientations(100, 5, 108, 45)[1], (40, 8), 0, 96),
    ("clipped by the page's corner", BEYOND, (45, 16), 3, 33),
    ("a slanted sliver, k = 8", [(5.0, 42.0), (60.0, 40.0), (61.0, 58.0), (6.0, 60.0)], (55, 2), 1, 90),
)
FEATHERS = (0, 3, 40)


def _record(q, rw, rh):
    xs, ys = [p[0] for p in q], [p[1] for p in q]
    bx0, by0 = max(0, math.floor(min(xs))), max(0, math.floor(min(ys)))
    bx1, by1 = min(PAGE_W, math.ceil(max(xs))), min(PAGE_H, math.ceil(max(ys)))
    return dict(out_quad=q, rw=rw, rh=rh, bbox=(bx0, by0, bx1 - bx0, by1 - by0))


@pytest.fixture(scope="module")
def paste_data():
    """random lines and a random page; the atlas ops.paste_u8 makes of the lines on the device, checked against pages.line_to_rect; per feather
    the host result of every region alone"""
    assert [pages.box_factor(r[2][1], ROWS) for r in REGIONS] == [1, 2, 1, 8]
    rng = np.random.default_rng(20241021)
    lines = rng.integers(0, 256, (N_LINES, ROWS, LINE_W, 3), dtype=np.uint8)
    page = rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    recs = [_record(q, rw, rh) for _, q, (rw, rh), _, _ in REGIONS]
    rects, y = [], 0
    for r in recs:
        rects.append((0, y, r["rw"], r["rh"]))
        y += r["rh"]
    fg_tab = pages.build_table(rects, [r[4] for r in REGIONS], 0, ROWS)
    fg_tab["line_index"] = [r[3] for r in REGIONS]
    atlas = torch.full((y, max(r["rw"] for r in recs), 3), 0, dtype=torch.uint8, device=DEV)
    ops.paste_u8(torch.from_numpy(lines).to(DEV), ops.table_to_device(fg_tab, DEV), atlas)
    atlas_h = atlas.cpu().numpy()
    fgs = [pages.line_to_rect(lines[li, :, :sw], rw, rh) for _, _, (rw, rh), li, sw in REGIONS]
    for (x0, y0, rw, rh), fg in zip(rects, fgs):
        assert np.array_equal(atlas_h[y0:y0 + rh, x0:x0 + rw], fg)
        assert (atlas_h[y0:y0 + rh, rw:] == 0).all()
    want, masks = {}, []
    for F in FEATHERS:
        want[F] = [quads.warp_paste_host(page.copy(), fg, quads.inverse_map(quads.quad_map(r["out_quad"], r["rw"], r["rh"])), r["rw"], r["rh"], F)
                   for r, fg in zip(recs, fgs)]
    masks = [(w != page).any(axis=2) for w in want[0]]                                          # (random bytes: a pasted pixel that keeps all three is rare, and harmless here)
    assert sum(m.astype(np.int64) for m in masks).max() == 1 and all(m.sum() > 50 for m in masks)
    assert masks[2][PAGE_H - 1, PAGE_W - 1]                                                     # the clipped region reaches the page's corner
    return dict(page=page, atlas=atlas, recs=recs, rects=rects, want=want)


def _paste_table(d, sel, F):
    return quads.paste_table([d["recs"][r] for r in sel], F, [d["rects"][r][:2] for r in sel])


def _paste_launch(d, tab):
    size = PAGE_H * PAGE_W * 3
    buf = torch.full((size + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    dst = buf[GUARD:GUARD + size].view(PAGE_H, PAGE_W, 3)
    dst.copy_(torch.from_numpy(d["page"]))
    got = ops.quad_paste_u8(d["atlas"], ops.table_to_device(tab, DEV), int(max(tab["bw"].max(), 1)), int(max(tab["bh"].max(), 1)), dst)
    assert got.data_ptr() == dst.data_ptr()
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + size].reshape(PAGE_H, PAGE_W, 3), (host[:GUARD], host[GUARD + size:])


def _paste_check(d, sel, F, got, guards, untouched=()):
    expect = d["page"].copy()
    for j, r in enumerate(sel):
        if j not in untouched:
            changed = (d["want"][F][r] != d["page"]).any(axis=2)
            expect[changed] = d["want"][F][r][changed]
        bx0, by0, bw, bh = d["recs"][r]["bbox"]
        assert np.array_equal(got[by0:by0 + bh, bx0:bx0 + bw], expect[by0:by0 + bh, bx0:bx0 + bw]), REGIONS[r][0]
    assert np.array_equal(got, expect)                                            # and outside the quadrilaterals the page is untouched
    assert all((g == 0xCD).all() for g in guards)


@pytest.mark.parametrize("feather", FEATHERS)
def test_paste_batch_equals_host_and_is_batch_invariant(paste_data, feather):
    sel = list(range(len(REGIONS)))
    got, guards = _paste_launch(paste_data, _paste_table(paste_data, sel, feather))
    _paste_check(paste_data, sel, feather, got, guards)
    for r in sel:                                                                 # each region launched alone gives the bytes it gives in the batch
        got, guards = _paste_launch(paste_data, _paste_table(paste_data, [r], feather))
        _paste_check(paste_data, [r], feather, got, guards)


def _set(field, value):
    def edit(tab):
        tab[field][1] = value
    return edit


def _nan_n(tab):
    tab["n"][1][4] = float("nan")


# region 1 of the launch (REGIONS[2], clipped by the corner: atlas rectangle (0, 24, 45, 16), bounding box (120, 45, 30, 25)) made unfollowable
PASTE_BAD = (
    ("negative ax0", _set("ax0", -1)),
    ("negative ay0", _set("ay0", -1)),
    ("the foreground beyond the atlas's right edge", _set("ax0", 16)),
    ("the foreground beyond the atlas's bottom", _set("ay0", 27)),
    ("ax0 + rw beyond 32 bits", _set("ax0", 2 ** 31 - 1)),
    ("rw of 0", _set("rw", 0)),
    ("negative rh", _set("rh", -16)),
    ("negative bx0", _set("bx0", -1)),
    ("negative by0", _set("by0", -1)),
    ("the bounding box beyond the page's right edge", _set("bx0", 121)),
    ("the bounding box beyond the page's bottom", _set("by0", 46)),
    ("by0 + bh beyond 32 bits", _set("by0", 2 ** 31 - 1)),
    ("bw of 0", _set("bw", 0)),
    ("negative bh", _set("bh", -25)),
    ("negative feather", _set("feather", -1)),
    ("feather beyond 1024", _set("feather", 1025)),
    ("a NaN coefficient", _nan_n),
)


@pytest.mark.parametrize("name,edit", PASTE_BAD, ids=[b[0] for b in PASTE_BAD])
def test_unfollowable_region_keeps_the_background_and_its_neighbours_stand(paste_data, name, edit):
    sel = [0, 2, 3]
    tab = _paste_table(paste_data, sel, 3)
    assert tuple(tab[1])[:8] == (0, 24, 45, 16, 120, 45, 30, 25) and paste_data["atlas"].shape == (42, 60, 3)
    edit(tab)
    got, guards = _paste_launch(paste_data, tab)
    _paste_check(paste_data, sel, 3, got, guards, untouched=(1,))


# a strong trapezoid (parallel sides 2 : 1: its vanishing line is the vertical one width to its left) where that line runs between the page's origin
# and the region, and where it runs THROUGH the origin
TRAPEZOIDS = (("line between origin and region", [(200, 40), (300, 30), (300, 70), (200, 60)]),
              ("line through the origin", [(100, 40), (200, 30), (200, 70), (100, 60)]))


@pytest.mark.parametrize("name,q", TRAPEZOIDS, ids=[t[0] for t in TRAPEZOIDS])
def test_strong_perspective_is_cropped_and_pasted_wherever_its_vanishing_line_runs(name, q):
    """both kernels on a region whose vanishing line crosses the page: the host's bytes, and the paste covers the polygon (its area up to its
    perimeter) — whether a region is restored does not depend on where it lies relative to page pixel (0, 0)"""
    rng = np.random.default_rng(70)
    page = rng.integers(0, 256, (80, 320, 3), dtype=np.uint8)
    rw, rh = quads.crop_size(q)
    M = quads.quad_map(q, rw, rh)
    page_d = torch.from_numpy(page).to(DEV)
    crops, offsets = quads.crop_quads(page_d, [M], [(rw, rh)])
    want_crop = quads.warp_crop_host(page, M, rw, rh)
    assert offsets == [0] and np.array_equal(crops.cpu().numpy().reshape(rh, rw, 3), want_crop)
    assert len(np.unique(want_crop.reshape(-1, 3), axis=0)) > rw * rh // 2                     # a real crop, not a fill
    fg = rng.integers(0, 256, (rh, rw, 3), dtype=np.uint8)
    xs, ys = [p[0] for p in q], [p[1] for p in q]
    rec = dict(out_quad=q, rw=rw, rh=rh, bbox=(min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys)))
    area, perimeter = 3000.0, 20.0 + 40.0 + 2 * math.hypot(100, 10)
    for F in (0, 3):
        want = quads.warp_paste_host(page.copy(), fg, quads.inverse_map(M), rw, rh, F)
        got = ops.quad_paste_u8(torch.from_numpy(fg).to(DEV), ops.table_to_device(quads.paste_table([rec], F, [(0, 0)]), DEV), rec["bbox"][2], rec["bbox"][3],
                                page_d.clone()).cpu().numpy()
        assert np.array_equal(got, want), F
        if F == 0:
            changed = int((got != page).any(axis=2).sum())
            assert abs(changed - area) <= perimeter, changed


@pytest.mark.parametrize("scale", (1, 4))
def test_compose_page_quads_equals_compose_quads_host(scale):
    """compose_page_quads (the background, the atlas and the tables made here) at the product's shape: rows = 128, one region without a line"""
    rng = np.random.default_rng(50 + scale)
    page = rng.integers(0, 256, (50, 120, 3), dtype=np.uint8)
    widths = [333, None, 400, 77]
    qs = [GENERAL, quads.box_quad([0, 0, 120, 50]), _orientations(2, 2, 14, 48)[1], [(30.5, 41.0), (110.0, 42.5), (109.0, 49.5), (30.0, 49.0)]]
    joined = rng.integers(0, 256, (3, 128, 400, 3), dtype=np.uint8)
    lines = [joined[0, :, :333], None, joined[1], joined[2, :, :77]]
    want = quads.compose_quads_host(page, lines, qs, scale, 8)
    assert not np.array_equal(want, lq_io.resize_cubic(page, scale, scale))
    for src in (page, torch.from_numpy(page).to(DEV)):                                        # a host page and a page that is on the device already
        out = quads.compose_page_quads(src, torch.from_numpy(joined).to(DEV), widths, qs, scale, 8)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (50 * scale, 120 * scale, 3)
        assert np.array_equal(out.cpu().numpy(), want)
    none = quads.compose_page_quads(page, None, [None] * 4, qs, scale, 8, device=DEV)
    assert np.array_equal(none.cpu().numpy(), lq_io.resize_cubic(page, scale, scale))


def test_prepare_packed_equals_prepare_strips():
    """the encoder's input from pixels on the device: the bits prepare_strips makes of the same images, previews included"""
    from marconet_amd import lq_device
    rng = np.random.default_rng(60)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((24, 101), (32, 300), (7, 9))]
    flat = np.concatenate([np.full((5,), 9, np.uint8)] + [i.reshape(-1) for i in imgs])
    offs = [5, 5 + imgs[0].size, 5 + imgs[0].size + imgs[1].size]
    a = lq_device.prepare_strips(imgs, DEV, preview=True)
    b = lq_device.prepare_packed(torch.from_numpy(flat).to(DEV), [i.shape[:2] for i in imgs], offs, preview=True)
    assert torch.equal(a.lq, b.lq) and torch.equal(a.preview, b.preview)
    assert (a.content_w, a.show_w, a.index, a.skipped) == (b.content_w, b.show_w, b.index, b.skipped)


# ---------------------------------------------------------------------------------------------------------------- through the networks
@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    return MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")


@pytest.fixture(scope="module")
def scene():
    """tests/test_pages_gpu.py's scene: a noise page carrying the 1321-px line of tests/long_lines_cases.py and the reference's two labelled strips
    at disjoint positions, and a fourth region whose text has a character outside the alphabet"""
    line, text = golden_line()
    strips = [(lq_io.load_png(os.path.join(cases_png.PNG_DIR, n)), lq_io.manual_text(n)) for n in cases_png.SR_STRIPS.values()]
    page = np.random.default_rng(7).integers(0, 256, (110, 1340, 3), dtype=np.uint8)
    boxes, texts = [], []
    for img, t, (x, y) in ((line, text, (11, 5)), (strips[0][0], strips[0][1], (3, 44)), (strips[1][0], strips[1][1], (700, 70))):
        page[y:y + img.shape[0], x:x + img.shape[1]] = img
        boxes.append([x, y, x + img.shape[1], y + img.shape[0]])
        texts.append(t)
    boxes.append([200, 45, 420, 66])
    texts.append(strips[0][1][:2] + " " + strips[0][1][2:])
    return page, boxes, texts


def test_boxes_as_quads_give_restore_page(pipe, scene):
    """axis-aligned integer boxes given as their four corners: restore_page's bytes, plans and widths — at scale 4 / feather 8 and at scale 1"""
    page, boxes, texts = scene
    qs = [quads.box_quad(b) for b in boxes]
    want, regions = pipe.restore_page(page, boxes, texts, scale=4, feather=8, details=True)
    got, info = pipe.restore_page_quads(page, qs, texts, scale=4, feather=8, details=True)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert info[3] is None and regions[3] is None and len(info[0]["plan"]) >= 3
    for r, i, b in zip(regions[:3], info[:3], boxes[:3]):
        assert i["plan"] == r["plan"] and i["out_w"] == r["out_w"] and i["size"] == r["rect"][2:]
        assert i["quad"] == [(4 * x, 4 * y) for x, y in quads.box_quad(b)]
    assert not np.array_equal(got, lq_io.resize_cubic(page, 4, 4))
    one = pipe.restore_page(page, boxes, texts, scale=1, feather=8)
    x1, y1, x2, y2 = boxes[1]                                                                   # scale 1, one region with its (evenly spaced) character boxes in page pixels, as boxes and as corners
    cb = [[c[0] + x1, c[1] + y1, c[2] + x1, c[3] + y1] for c in lq_io.evenly_spaced_boxes(len(texts[1]), x2 - x1, y2 - y1)]
    cb = [c if k % 2 else quads.box_quad(c) for k, c in enumerate(cb)]
    assert np.array_equal(pipe.restore_page_quads(page, qs, texts, char_boxes=[None, cb, None, None], scale=1, feather=8), one)


def test_rotated_page_gives_rotated_regions(pipe, scene):
    """the page and the quadrilaterals rotated by 90 degrees, feather 0: the crops are byte-identical and in the same batch order, so every region's
    rectangle is np.rot90 of its rectangle from the unrotated run; every pixel outside the regions — the skipped region included — is the
    background of the rotated page"""
    page, boxes, texts = scene
    s, W = 2, page.shape[1]
    upright = pipe.restore_page_quads(page, [quads.box_quad(b) for b in boxes], texts, scale=s, feather=0)
    turned = np.ascontiguousarray(np.rot90(page))                                               # turned[i, j] = page[j, W - 1 - i]: (x, y) → (y, W - x)
    qs = [[(y, W - x) for x, y in quads.box_quad(b)] for b in boxes]
    got, info = pipe.restore_page_quads(turned, qs, texts, scale=s, feather=0, details=True)
    assert got.shape == (s * W, s * page.shape[0], 3) and info[3] is None
    bg = lq_io.resize_cubic(turned, s, s)
    outside = np.ones(got.shape[:2], bool)
    for (x1, y1, x2, y2), i in zip(boxes[:3], info[:3]):
        rect = got[s * (W - x2):s * (W - x1), s * y1:s * y2]
        assert np.array_equal(rect, np.rot90(upright[s * y1:s * y2, s * x1:s * x2]))
        assert not np.array_equal(rect, bg[s * (W - x2):s * (W - x1), s * y1:s * y2])
        assert i["size"] == (s * (x2 - x1), s * (y2 - y1))
        outside[s * (W - x2):s * (W - x1), s * y1:s * y2] = False
    assert np.array_equal(got[outside], bg[outside])


def test_slanted_regions_equal_the_host_composition(pipe, scene):
    """restore_page_quads is compose_quads_host of what restore_lines gives for the host's rectified crops in the same order (the same batch, so the
    same network bytes) — with two regions slanted, one of them (the long line: several windows) reaching beyond the page's edge"""
    page, boxes, texts = scene
    qs = [quads.box_quad(b) for b in boxes]
    (x1, y1, x2, y2) = boxes[0]
    qs[0] = [[x1 + 0.25, y1 - 7.5], [x2 + 2.0, y1 + 1.75], [x2 - 0.5, y2 + 1.0], [x1, y2 - 6.25]]
    (x1, y1, x2, y2) = boxes[2]
    qs[2] = [[x1 + 0.5, y1 + 2.25], [x2 - 1.0, y1], [x2, y2 - 2.5], [x1, y2]]
    sizes = [quads.crop_size(q) for q in qs]
    crops = [quads.warp_crop_host(page, quads.quad_map(q, cw, ch), cw, ch) for q, (cw, ch) in zip(qs, sizes)]
    assert min(p[1] for p in qs[0]) < 0 and np.array_equal(crops[1], page[boxes[1][1]:boxes[1][3], boxes[1][0]:boxes[1][2]])
    lines, plans = pipe.restore_lines(crops, texts, details=True)
    assert len(plans[0]) >= 3 and lines[3] is None
    got, info = pipe.restore_page_quads(page, qs, texts, scale=2, feather=5, details=True)
    assert [i["plan"] for i in info[:3]] == plans[:3] and info[3] is None
    assert [i["size"] for i in info[:3]] == [(2 * cw, 2 * ch) for cw, ch in sizes[:3]]
    assert np.array_equal(got, quads.compose_quads_host(page, lines, qs, 2, 5))


def test_restore_page_quads_without_restored_regions_is_the_background(pipe, scene):
    page = scene[0][:40, :90]
    assert np.array_equal(pipe.restore_page_quads(page, [], [], scale=2), lq_io.resize_cubic(page, 2, 2))
    assert np.array_equal(pipe.restore_page_quads(page, [quads.box_quad([5, 5, 60, 30])], [""], scale=2), lq_io.resize_cubic(page, 2, 2))


def test_example_script_takes_quad_regions(tmp_path, scene):
    """examples/restore_page.py on the scene with one region given as a slanted "quad" and the others as boxes: the PNG's decoded pixels are
    restore_page_quads', computed in this process"""
    from PIL import Image
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    page, boxes, texts = scene
    regions = [dict(box=b, text=t) for b, t in zip(boxes, texts)]
    x1, y1, x2, y2 = boxes[2]
    slanted = [[x1 + 0.5, y1 + 2.25], [x2 - 1.0, y1], [x2, y2 - 2.5], [x1, y2]]
    regions[2] = dict(quad=slanted, text=texts[2])
    src, reg, out = str(tmp_path / "page.png"), str(tmp_path / "regions.json"), str(tmp_path / "out.png")
    Image.fromarray(page).save(src)
    with open(reg, "w", encoding="utf8") as f:
        json.dump(regions, f)
    env = dict(os.environ)
    env.pop("MARCONET_CKPT_DIR", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "restore_page.py"), "-i", src, "-r", reg, "-o", out, "--scale", "2", "--feather", "5",
                        "--precision", "fp32"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sde, sdg, sds, _ = checkpoints.load_state_dicts("")
    p = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, DEV), precision="fp32")
    qs = [quads.box_quad(b) for b in boxes]
    qs[2] = slanted
    want = p.restore_page_quads(page, qs, texts, scale=2, feather=5)
    assert want.shape == (2 * page.shape[0], 2 * page.shape[1], 3) and np.array_equal(lq_io.load_png(out), want), r.stdout[-1500:]
    assert "Region 3 keeps the page's pixels" in r.stdout and "Region 2: " in r.stdout and "quadrilateral" in r.stdout
