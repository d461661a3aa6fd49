"""-m gpu: the curved page path on the device (mnet_curve_crop_u8, mnet_curve_paste_u8, curves.compose_page_curves,
MarconetPipeline.restore_page_curves) against the pure-host definition curves.warp_crop_host / warp_paste_host / compose_curves_host — byte for
byte: every comparison is np.array_equal.  The device's fp64 square root and divisions are compared with numpy's correctly rounded ones through
these bytes.  The host references are computed once per module."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from marconet_amd import _lib, curves, lq_io, ops, quads
from tests.golden import cases_png
from tests.long_lines_cases import golden_line

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE_H, PAGE_W, GUARD = 120, 200, 4096


def arc(cx, cy, r_in, r_out, deg0, deg1, K):
    a = [math.radians(d) for d in np.linspace(deg0, deg1, K)]
    top = [(cx + r_out * math.cos(t), cy - r_out * math.sin(t)) for t in a]
    bot = [(cx + r_in * math.cos(t), cy - r_in * math.sin(t)) for t in a]
    return top + bot[::-1]


# four disjoint regions of the 200 x 120 page
ARC = arc(100.0, 112.0, 61.0, 83.0, 150.0, 30.0, 6)                               # 5 segments of 30: 150 x 22
FINE = arc(100.0, 112.0, 20.0, 38.0, 160.0, 20.0, 33)                             # 32 segments of 2 to 3 px, in the hollow of ARC
BEYOND = arc(200.0, 60.0, 18.0, 34.0, 150.0, 30.0, 5)                             # centred on the page's right edge: half of it outside
TAPERED = [(163.5, 85.75), (169.35, 86.35), (177.5, 88.0), (187.5, 108.0), (172.25, 110.0), (158.5, 116.0)]     # its first segment: a1 changes sign inside
NARROW = [(20.5, 80.25), (40.5, 78.0), (41.5, 77.875), (70.0, 79.0), (70.0, 97.0), (41.5, 95.875), (40.5, 96.0), (20.5, 98.25)]   # a 1-pixel-wide segment
PARALLELOGRAM = [(20.25, 8.5), (100.5, 14.75), (97.25, 40.0), (17.0, 33.75)]


def _page():
    """a 120 x 200 page made of the golden strips, its low bits stirred so that no two neighbouring pixels are alike"""
    rows = [lq_io.load_png(os.path.join(cases_png.PNG_DIR, n)) for n in ("real_lq13.png", "w1.png", "w2.png")]
    tiles = np.concatenate([rows[0][:, :200], rows[0][:, 188:388], rows[1][:, :200], rows[2][:, :200]], axis=0)[:PAGE_H]
    assert tiles.shape == (PAGE_H, PAGE_W, 3)
    return tiles ^ np.random.default_rng(20241030).integers(0, 16, tiles.shape, dtype=np.uint8)


def _region(poly, scale=1):
    return curves.check_curves(PAGE_H, PAGE_W, [poly], [True], scale, 0)[0]


def _crop_case(name, poly, c0=0, w=None):
    r = _region(poly)
    return dict(name=name, segs=r["segs"], w=r["cw"] - c0 if w is None else w, h=r["ch"], c0=c0)


# ------------------------------------------------------------------------------------------------------------------------ the gather in
CROPS = [
    _crop_case("the arc: 150 x 22, 5 segments, over tile column 63|64 and tile row 15|16", ARC),
    _crop_case("a window with c0 > 0 that starts and ends mid-segment", ARC, c0=37, w=70),
    _crop_case("a 1-pixel-wide segment", NARROW),
    _crop_case("32 segments of 2 to 3 px", FINE),
    _crop_case("half outside the page", BEYOND),
    _crop_case("the tapered chain", TAPERED),
    _crop_case("a parallelogram", PARALLELOGRAM),
]
CROPS[1]["segs"] = CROPS[0]["segs"]              # two windows of one region share its segments


@pytest.fixture(scope="module")
def crop_data():
    page = _page()
    want = [curves.warp_crop_host(page, c["segs"], c["w"], c["h"], c["c0"]) for c in CROPS]
    assert (CROPS[0]["w"], CROPS[0]["h"], len(CROPS[0]["segs"])) == (150, 22, 5) and [s["w"] for s in CROPS[2]["segs"]] == [20, 1, 29]
    assert len(CROPS[3]["segs"]) == 32 and {s["w"] for s in CROPS[3]["segs"]} <= {2, 3} and max(p[0] for p in BEYOND) > PAGE_W + 25
    assert np.array_equal(want[1], want[0][:, 37:107]) and all(len(np.unique(w.reshape(-1, 3), axis=0)) > w.shape[0] * w.shape[1] // 3 for w in want)
    return dict(page=page, page_d=torch.from_numpy(page).to(DEV), want=want)


def _crop_tables(sel):
    """the cases ``sel`` packed with a gap of 1, 2, 3 ... bytes before each, so that the offsets are odd and even and no multiple of a pixel"""
    tab, segs, _ = curves.crop_table([CROPS[r]["segs"] for r in sel], [(CROPS[r]["w"], CROPS[r]["h"]) for r in sel], [CROPS[r]["c0"] for r in sel])
    off = 0
    for j, r in enumerate(sel):
        off += j + 1
        tab["offset"][j] = off
        off += 3 * CROPS[r]["w"] * CROPS[r]["h"]
    return tab, segs, off + 5


def _crop_launch(d, tab, segs, size, n_segs=None):
    buf = torch.full((size + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    dst = buf[GUARD:GUARD + size]
    segs_d = ops.table_to_device(segs, DEV)
    ops.curve_crop_u8(d["page_d"], ops.table_to_device(tab, DEV), segs_d if n_segs is None else segs_d[:n_segs], int(max(tab["w"].max(), 1)),
                      int(max(tab["h"].max(), 1)), dst)
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
    tab, segs, size = _crop_tables(sel)
    assert any(o % 2 for o in tab["offset"]) and any(o % 3 for o in tab["offset"]) and tab["seg0"][1] == tab["seg0"][0]
    got, guards = _crop_launch(crop_data, tab, segs, size)
    _crop_check(crop_data, sel, tab, size, got, guards)


def test_crop_is_batch_invariant(crop_data):
    for r in range(len(CROPS)):
        tab, segs, size = _crop_tables([r])
        got, guards = _crop_launch(crop_data, tab, segs, size)
        _crop_check(crop_data, [r], tab, size, got, guards)


def test_one_segment_parallelogram_equals_the_quad_kernel(crop_data):
    cw, ch = quads.crop_size(PARALLELOGRAM)
    assert (cw, ch) == (CROPS[6]["w"], CROPS[6]["h"])
    a, _ = curves.crop_curves(crop_data["page_d"], [CROPS[6]["segs"]], [(cw, ch)])
    b, _ = quads.crop_quads(crop_data["page_d"], [quads.quad_map(PARALLELOGRAM, cw, ch)], [(cw, ch)])
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy().reshape(ch, cw, 3), crop_data["want"][6])


# crop 1 of the launch (the tapered chain: 2 segments, segs[5:7] of the 12 in the table) made unfollowable
def _seg_edit(field, index, value):
    def edit(tab, segs, size):
        segs[field][index] = value
    return edit


def _nan_coefficient(tab, segs, size):
    segs["c"][6][5] = float("nan")


CROP_BAD = (
    ("nseg = 0", lambda tab, segs, size: tab["nseg"].__setitem__(1, 0)),
    ("nseg = 33", lambda tab, segs, size: tab["nseg"].__setitem__(1, 33)),
    ("negative seg0", lambda tab, segs, size: tab["seg0"].__setitem__(1, -1)),
    ("seg0 + nseg beyond n_segs", lambda tab, segs, size: tab["seg0"].__setitem__(1, 11)),
    ("seg0 + nseg beyond 32 bits", lambda tab, segs, size: tab["seg0"].__setitem__(1, 2 ** 31 - 1)),
    ("a NaN coefficient", _nan_coefficient),
    ("a broken u0 chain", _seg_edit("u0", 6, 5)),
    ("a first segment that does not start at 0", _seg_edit("u0", 5, 1)),
    ("a segment of width 0", _seg_edit("w", 6, 0)),
    ("the window beyond the strip", lambda tab, segs, size: tab["c0"].__setitem__(1, 1)),
    ("an offset past dst", lambda tab, segs, size: tab["offset"].__setitem__(1, size + 1)),
    ("the crop's end past dst_bytes", lambda tab, segs, size: tab["offset"].__setitem__(1, size - 10)),
    ("negative offset", lambda tab, segs, size: tab["offset"].__setitem__(1, -1)),
    ("w = 0", lambda tab, segs, size: tab["w"].__setitem__(1, 0)),
    ("negative c0", lambda tab, segs, size: tab["c0"].__setitem__(1, -1)),
)


@pytest.mark.parametrize("name,edit", CROP_BAD, ids=[b[0] for b in CROP_BAD])
def test_unfollowable_crop_leaves_its_bytes_and_its_neighbours_stand(crop_data, name, edit):
    """descriptors the kernel declines by its own checks: nothing here can take it out of its buffers"""
    sel = [0, 5, 4]
    tab, segs, size = _crop_tables(sel)
    assert (tab["seg0"].tolist(), tab["nseg"].tolist(), len(segs)) == ([0, 5, 7], [5, 2, 4], 11)
    segs = np.concatenate([segs, segs[-1:]])                                      # 12 segments: the last one belongs to nobody
    edit(tab, segs, size)
    got, guards = _crop_launch(crop_data, tab, segs, size)
    _crop_check(crop_data, sel, _crop_tables(sel)[0], size, got, guards, untouched=(1,))


# ----------------------------------------------------------------------------------------------------------------------- the gather out
S = 2                                            # the regions of the enlarged 400 x 240 page: their boxes are larger than one 64 x 16 tile
REGIONS = (("the arc", ARC), ("32 segments", FINE), ("clipped by the page's right edge", BEYOND), ("the tapered chain", TAPERED))
FEATHERS = (0, 1, 3, 40)


@pytest.fixture(scope="module")
def paste_data():
    """a random page and a random atlas holding the regions' upright foregrounds at odd places; per feather the host result of every region alone"""
    rng = np.random.default_rng(20241031)
    page = rng.integers(0, 256, (S * PAGE_H, S * PAGE_W, 3), dtype=np.uint8)
    recs = curves.check_curves(PAGE_H, PAGE_W, [p for _, p in REGIONS], [True] * len(REGIONS), S, 0)
    assert recs[0]["bbox"][2] > 256 and recs[0]["bbox"][3] > 64 and recs[2]["bbox"][0] + recs[2]["bbox"][2] == S * PAGE_W and recs[3]["rh"] < 2 * 40
    assert any(sg["box"][2] == 0 for sg in recs[2]["out_segs"])                    # a segment wholly outside the page claims nothing
    xy, y = [], 3
    for k, r in enumerate(recs):
        xy.append((5 * k, y))
        y += r["rh"] + 2
    atlas = rng.integers(0, 256, (y, max(r["rw"] for r in recs) + 20, 3), dtype=np.uint8)
    fgs = [np.ascontiguousarray(atlas[y0:y0 + r["rh"], x0:x0 + r["rw"]]) for r, (x0, y0) in zip(recs, xy)]
    want = {F: [curves.warp_paste_host(page.copy(), fg, r["out_segs"], r["rw"], r["rh"], F) for r, fg in zip(recs, fgs)] for F in FEATHERS}
    masks = [(w != page).any(axis=2) for w in want[0]]
    assert sum(m.astype(np.int64) for m in masks).max() == 1 and all(m.sum() > 1500 for m in masks)
    return dict(page=page, atlas=torch.from_numpy(atlas).to(DEV), recs=recs, xy=xy, want=want)


def _paste_tables(d, sel, F):
    return curves.paste_table([d["recs"][r] for r in sel], F, [d["xy"][r] for r in sel])


def _paste_launch(d, tab, segs, atlas=None):
    H, W = S * PAGE_H, S * PAGE_W
    size = H * W * 3
    buf = torch.full((size + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    dst = buf[GUARD:GUARD + size].view(H, W, 3)
    dst.copy_(torch.from_numpy(d["page"]))
    got = ops.curve_paste_u8(d["atlas"] if atlas is None else atlas, ops.table_to_device(tab, DEV), ops.table_to_device(segs, DEV), int(max(tab["bw"].max(), 1)),
                             int(max(tab["bh"].max(), 1)), dst)
    assert got.data_ptr() == dst.data_ptr()
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + size].reshape(H, W, 3), (host[:GUARD], host[GUARD + size:])


def _paste_check(d, sel, F, got, guards, untouched=()):
    expect = d["page"].copy()
    for j, r in enumerate(sel):
        if j not in untouched:
            changed = (d["want"][F][r] != d["page"]).any(axis=2)
            expect[changed] = d["want"][F][r][changed]
    for r in sel:                                                                 # (one region's box may hold another region: the arc's holds the 32 segments)
        bx0, by0, bw, bh = d["recs"][r]["bbox"]
        assert np.array_equal(got[by0:by0 + bh, bx0:bx0 + bw], expect[by0:by0 + bh, bx0:bx0 + bw]), REGIONS[r][0]
    assert np.array_equal(got, expect)                                            # and outside the regions the page is untouched
    assert all((g == 0xCD).all() for g in guards)


@pytest.mark.parametrize("feather", FEATHERS)
def test_paste_batch_equals_host_and_is_batch_invariant(paste_data, feather):
    sel = list(range(len(REGIONS)))
    got, guards = _paste_launch(paste_data, *_paste_tables(paste_data, sel, feather))
    _paste_check(paste_data, sel, feather, got, guards)
    for r in sel:                                                                 # each region launched alone gives the bytes it gives in the batch
        got, guards = _paste_launch(paste_data, *_paste_tables(paste_data, [r], feather))
        _paste_check(paste_data, [r], feather, got, guards)


def _set(field, value):
    def edit(tab, segs):
        tab[field][1] = value
    return edit


def _seg_set(field, index, value):
    def edit(tab, segs):
        segs[field][index] = value
    return edit


def _nan_c(tab, segs):
    segs["c"][6][2] = float("nan")


def _box_left_of_region(tab, segs):
    segs["bx0"][5] = tab["bx0"][1] - 1


def _box_below_region(tab, segs):
    segs["bh"][6] = tab["by0"][1] + tab["bh"][1] - segs["by0"][6] + 1


# region 1 of the launch (the tapered chain: 2 segments, segs[5:7]) made unfollowable
PASTE_BAD = (
    ("nseg = 0", _set("nseg", 0)),
    ("nseg = 33", _set("nseg", 33)),
    ("negative seg0", _set("seg0", -1)),
    ("seg0 + nseg beyond n_segs", _set("seg0", 10)),
    ("a NaN coefficient", _nan_c),
    ("a broken u0 chain", _seg_set("u0", 6, 7)),
    ("a segment of width 0", _seg_set("w", 5, 0)),
    ("the widths do not sum to rw", _set("rw", 43)),
    ("a segment box left of the region box", _box_left_of_region),
    ("a segment box below the region box", _box_below_region),
    ("a segment box of negative width", _seg_set("bw", 5, -1)),
    ("the foreground beyond the atlas's bottom", _set("ay0", 10 ** 6)),
    ("the bounding box beyond the page's right edge", _set("bx0", 2 * PAGE_W - 10)),
    ("rh of 0", _set("rh", 0)),
    ("feather beyond 1024", _set("feather", 1025)),
)


@pytest.mark.parametrize("name,edit", PASTE_BAD, ids=[b[0] for b in PASTE_BAD])
def test_unfollowable_region_keeps_the_background_and_its_neighbours_stand(paste_data, name, edit):
    """descriptors the kernel declines by its own checks: nothing here can take it out of its buffers"""
    sel = [0, 3, 2]
    tab, segs = _paste_tables(paste_data, sel, 3)
    assert (tab["seg0"].tolist(), tab["nseg"].tolist(), len(segs), int(tab["rw"][1])) == ([0, 5, 7], [5, 2, 4], 11, 44)
    edit(tab, segs)
    got, guards = _paste_launch(paste_data, tab, segs)
    _paste_check(paste_data, sel, 3, got, guards, untouched=(1,))


@pytest.mark.parametrize("scale", (1, 4))
def test_compose_page_curves_equals_compose_curves_host(scale):
    """compose_page_curves (the background, the atlas and the tables made here) at the product's shape: rows = 128, one region without a line"""
    rng = np.random.default_rng(80 + scale)
    page = _page()
    widths = [333, None, 400, 77]
    polys = [ARC, FINE, BEYOND, TAPERED]
    joined = rng.integers(0, 256, (3, 128, 400, 3), dtype=np.uint8)
    lines = [joined[0, :, :333], None, joined[1], joined[2, :, :77]]
    want = curves.compose_curves_host(page, lines, polys, scale, 8)
    assert not np.array_equal(want, lq_io.resize_cubic(page, scale, scale))
    for src in (page, torch.from_numpy(page).to(DEV)):                                        # a host page and a page that is on the device already
        out = curves.compose_page_curves(src, torch.from_numpy(joined).to(DEV), widths, polys, scale, 8)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (PAGE_H * scale, PAGE_W * scale, 3)
        assert np.array_equal(out.cpu().numpy(), want)
    none = curves.compose_page_curves(page, None, [None] * 4, polys, scale, 8, device=DEV)
    assert np.array_equal(none.cpu().numpy(), lq_io.resize_cubic(page, scale, scale))


# ---------------------------------------------------------------------------------------------------------------- through the networks
@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    return MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")


@pytest.fixture(scope="module")
def scene():
    """tests/test_quads_gpu.py's scene: a noise page carrying the 1321-px line of tests/long_lines_cases.py and the reference's two labelled strips
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


def _cuts(box, n):
    """n - 2 integer abscissae inside the box: n points a side"""
    return [int(v) for v in np.linspace(box[0], box[2], n)[1:-1]]


def _bent(box, sag, n):
    """the box bent upwards: n points a side on a parabola that rises by ``sag`` in the middle"""
    x1, y1, x2, y2 = box
    xs = np.linspace(x1, x2, n)
    dy = [sag * (1.0 - (2.0 * (x - x1) / (x2 - x1) - 1.0) ** 2) for x in xs]
    return [[float(x), y1 - d] for x, d in zip(xs, dy)] + [[float(x), y2 - d] for x, d in zip(xs[::-1], dy[::-1])]


def test_boxes_as_polygons_give_restore_page(pipe, scene):
    """axis-aligned integer boxes given as polygons with 2, 3 and 5 points a side: restore_page's bytes, plans and widths — at scale 4 / feather 8
    and at scale 1"""
    page, boxes, texts = scene
    polys = [curves.box_polygon(b, _cuts(b, n)) for b, n in zip(boxes, (5, 2, 3, 2))]
    want, regions = pipe.restore_page(page, boxes, texts, scale=4, feather=8, details=True)
    got, info = pipe.restore_page_curves(page, polys, texts, scale=4, feather=8, details=True)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert info[3] is None and regions[3] is None and len(info[0]["plan"]) >= 3
    for r, i, p in zip(regions[:3], info[:3], polys[:3]):
        assert i["plan"] == r["plan"] and i["out_w"] == r["out_w"] and i["size"] == r["rect"][2:]
        assert i["polygon"] == [(4 * x, 4 * y) for x, y in p]
    assert not np.array_equal(got, lq_io.resize_cubic(page, 4, 4))
    one = pipe.restore_page(page, boxes, texts, scale=1, feather=8)
    x1, y1, x2, y2 = boxes[1]                                                                   # scale 1, one region with its (evenly spaced) character boxes in page pixels, as boxes and as corners
    cb = [[c[0] + x1, c[1] + y1, c[2] + x1, c[3] + y1] for c in lq_io.evenly_spaced_boxes(len(texts[1]), x2 - x1, y2 - y1)]
    cb = [c if k % 2 else quads.box_quad(c) for k, c in enumerate(cb)]
    polys[1] = curves.box_polygon(boxes[1], _cuts(boxes[1], 3))
    assert np.array_equal(pipe.restore_page_curves(page, polys, texts, char_boxes=[None, cb, None, None], scale=1, feather=8), one)


def test_curved_regions_equal_the_host_composition(pipe, scene):
    """restore_page_curves is compose_curves_host of what restore_lines gives for the host's rectified strips in the same order (the same batch, so
    the same network bytes) — the long line bent over 8 segments (several windows, its crest above the page's edge), one strip bent over 2"""
    page, boxes, texts = scene
    polys = [_bent(boxes[0], 5.25, 9), curves.box_polygon(boxes[1]), _bent(boxes[2], 2.25, 3), curves.box_polygon(boxes[3], _cuts(boxes[3], 4))]
    recs = curves.check_curves(page.shape[0], page.shape[1], polys, [True] * 4, 2, 5)
    crops = [curves.warp_crop_host(page, r["segs"], r["cw"], r["ch"]) for r in recs]
    assert min(p[1] for p in polys[0]) < 0 and np.array_equal(crops[1], page[boxes[1][1]:boxes[1][3], boxes[1][0]:boxes[1][2]])
    lines, plans = pipe.restore_lines(crops, texts, details=True)
    assert len(plans[0]) >= 2 and lines[3] is None
    got, info = pipe.restore_page_curves(page, polys, texts, scale=2, feather=5, details=True)
    assert [i["plan"] for i in info[:3]] == plans[:3] and info[3] is None
    assert [i["size"] for i in info[:3]] == [(r["rw"], r["rh"]) for r in recs[:3]]
    assert np.array_equal(got, curves.compose_curves_host(page, lines, polys, 2, 5))
    assert not np.array_equal(got, lq_io.resize_cubic(page, 2, 2))


def test_restore_page_curves_without_restored_regions_is_the_background(pipe, scene):
    page = scene[0][:40, :90]
    assert np.array_equal(pipe.restore_page_curves(page, [], [], scale=2), lq_io.resize_cubic(page, 2, 2))
    assert np.array_equal(pipe.restore_page_curves(page, [curves.box_polygon([5, 5, 60, 30], (20,))], [""], scale=2), lq_io.resize_cubic(page, 2, 2))


def test_example_script_takes_polygon_regions(tmp_path, scene):
    """examples/restore_page.py on the scene with one region given as a bent "polygon" and the others as boxes: the PNG's decoded pixels are
    restore_page_curves', computed in this process"""
    from PIL import Image
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    page, boxes, texts = scene
    regions = [dict(box=b, text=t) for b, t in zip(boxes, texts)]
    bent = _bent(boxes[2], 2.25, 3)
    regions[2] = dict(polygon=bent, text=texts[2])
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
    polys = [quads.box_quad(b) for b in boxes]
    polys[2] = bent
    want = p.restore_page_curves(page, polys, texts, scale=2, feather=5)
    assert want.shape == (2 * page.shape[0], 2 * page.shape[1], 3) and np.array_equal(lq_io.load_png(out), want), r.stdout[-1500:]
    assert "Region 3 keeps the page's pixels" in r.stdout and "Region 2: " in r.stdout and "6-point polygon" in r.stdout
