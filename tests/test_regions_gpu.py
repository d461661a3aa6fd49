"""-m gpu: regions of every kind of a page, overlapping, pasted in the caller's order by ONE launch whose workgroups own page tiles
(mnet_paste_mixed_u8, regions.bin_items / paste_tables, MarconetPipeline.restore_page_regions) against the pure-host definition — the existing
host paste of each kind applied one after another in list order — byte for byte: every comparison is np.array_equal.  The scene is
tests/regions_scene.py's; its host references are computed once per module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from marconet_amd import _lib, curves, lq_io, ops, pages, quads, regions
from tests import regions_scene as rs
from tests.golden import cases_png

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
PAGE_H, PAGE_W = rs.PAGE_H, rs.PAGE_W


def _guarded(array, fill=0xCD):
    """a guarded copy of ``array`` on the device → (the whole buffer, the array's view of it)"""
    buf = torch.full((array.size + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
    view = buf[GUARD:GUARD + array.size].view(array.shape)
    view.copy_(torch.from_numpy(array))
    return buf, view


def _intact(buf, size, fill=0xCD):
    host = buf.cpu().numpy()
    assert (host[:GUARD] == fill).all() and (host[GUARD + size:] == fill).all()                  # the guards are untouched
    return host[GUARD:GUARD + size]


@pytest.fixture(scope="module")
def data():
    page, lines = rs.data()
    things = rs.scene()
    lines_buf, lines_d = _guarded(lines)
    d = dict(page=page, lines=lines, things=things, lines_buf=lines_buf, lines_d=lines_d, want=rs.host(page, lines, things))
    # the scene holds what the tests are about: three kinds three deep in one tile, a vanished twin, a clipped region
    depth = np.zeros((PAGE_H, PAGE_W), np.int64)
    for t in things[:3]:
        depth += (rs.host(page, lines, [dict(t, F=0)]) != page).any(axis=2)
    assert (depth[16:32, 0:64] == 3).any()
    assert things[4]["rec"]["bbox"][0] + things[4]["rec"]["bbox"][2] == PAGE_W and max(p[0] for p in things[4]["rec"]["quad"]) > PAGE_W
    assert {t["F"] for t in things} == {0, 1, 3, 40} and len(things[3]["rec"]["out_segs"]) == 32 and len(things[2]["rec"]["out_segs"]) == 6
    assert np.array_equal(d["want"], rs.host(page, lines, things[:7] + things[8:]))               # the first twin has vanished under the second
    assert not np.array_equal(d["want"], rs.host(page, lines, things[::-1]))                      # the order shows
    return d


def _launch(d, tabs, spans=None, order=None, page=None):
    """the atlas by one mnet_paste_u8 launch, then one mnet_paste_mixed_u8 launch on a guarded page → the page's bytes on the host"""
    page = d["page"] if page is None else page
    if spans is None:
        spans, order = regions.bin_items(tabs["entries"], tabs["entry_item"], page.shape[0], page.shape[1])
    buf, dst = _guarded(page)
    up = lambda t: ops.table_to_device(t, DEV) if len(t) else None
    atlas, atlas_buf = None, None
    if tabs["fg"] is not None:
        atlas_buf, atlas = _guarded(np.zeros(tuple(tabs["atlas_hw"]) + (3,), np.uint8))
        ops.paste_u8(d["lines_d"], ops.table_to_device(tabs["fg"], DEV), atlas)
    got = ops.paste_mixed_u8(d["lines_d"] if len(tabs["cells"]) else None, atlas, up(tabs["cells"]), up(tabs["quads"]), up(tabs["curves"]), up(tabs["segs"]),
                             ops.table_to_device(tabs["items"], DEV), ops.table_to_device(spans, DEV), torch.from_numpy(order).to(DEV), dst)
    assert got.data_ptr() == dst.data_ptr()
    torch.cuda.synchronize()
    if atlas_buf is not None:
        _intact(atlas_buf, atlas.numel())
    assert np.array_equal(_intact(d["lines_buf"], d["lines"].size).reshape(d["lines"].shape), d["lines"])
    return _intact(buf, page.size).reshape(page.shape)


# ------------------------------------------------------------------------------------------------------------------------ the kernel
def test_the_whole_scene_equals_the_host_item_after_item(data):
    d = data
    got = _launch(d, rs.tables(d["things"]))
    assert np.array_equal(got, d["want"]) and not np.array_equal(got, d["page"])
    assert np.array_equal(_launch(d, rs.tables(d["things"][::-1])), rs.host(d["page"], d["lines"], d["things"][::-1]))


@pytest.mark.parametrize("sel", [list(range(m)) for m in range(1, 10)] + [[0, 2, 5, 9], [9, 3, 1], [8, 7, 6, 2]], ids=str)
def test_every_prefix_and_a_sub_selection_equal_the_host(data, sel):
    d = data
    things = [d["things"][i] for i in sel]
    assert np.array_equal(_launch(d, rs.tables(things)), rs.host(d["page"], d["lines"], things))


def test_only_cells_gives_the_bytes_of_the_ordered_kernel(data):
    d = data
    things = [t for t in d["things"] if t["kind"] in ("line", "column")] + [rs.line((30, 10, 40, 20), 3, 50, 2), rs.line((0, 0, 9, 4), 4, 35, 1)]
    tabs = rs.tables(things)
    spans, order = pages.bin_tiles(tabs["cells"], PAGE_H, PAGE_W)
    old = ops.paste_ordered_u8(d["lines_d"], ops.table_to_device(tabs["cells"], DEV), ops.table_to_device(spans, DEV), torch.from_numpy(order).to(DEV),
                               torch.from_numpy(d["page"]).to(DEV)).cpu().numpy()
    assert np.array_equal(_launch(d, tabs), old) and np.array_equal(old, rs.host(d["page"], d["lines"], things)) and not np.array_equal(old, d["page"])


def _atlas(d, tabs):
    atlas = torch.zeros(tuple(tabs["atlas_hw"]) + (3,), dtype=torch.uint8, device=DEV)
    return ops.paste_u8(d["lines_d"], ops.table_to_device(tabs["fg"], DEV), atlas)


def test_only_disjoint_quads_gives_the_bytes_of_the_quad_kernel(data):
    d = data
    things = [d["things"][1], d["things"][4], d["things"][7], rs.quad([(100, 40), (130, 44), (128, 66), (98, 62)], 0, 60, 40)]
    tabs = rs.tables(things)
    old = ops.quad_paste_u8(_atlas(d, tabs), ops.table_to_device(tabs["quads"], DEV), int(tabs["quads"]["bw"].max()), int(tabs["quads"]["bh"].max()),
                            torch.from_numpy(d["page"]).to(DEV)).cpu().numpy()
    assert np.array_equal(_launch(d, tabs), old) and np.array_equal(old, rs.host(d["page"], d["lines"], things)) and not np.array_equal(old, d["page"])


def test_only_disjoint_curves_gives_the_bytes_of_the_curve_kernel(data):
    d = data
    things = [d["things"][2], d["things"][3], rs.curve(rs.arc(20.0, 20.0, 6.0, 18.0, 170.0, 30.0, 4), 1, 50, 1)]
    tabs = rs.tables(things)
    old = ops.curve_paste_u8(_atlas(d, tabs), ops.table_to_device(tabs["curves"], DEV), ops.table_to_device(tabs["segs"], DEV), int(tabs["curves"]["bw"].max()),
                             int(tabs["curves"]["bh"].max()), torch.from_numpy(d["page"]).to(DEV)).cpu().numpy()
    assert np.array_equal(_launch(d, tabs), old) and np.array_equal(old, rs.host(d["page"], d["lines"], things)) and not np.array_equal(old, d["page"])


def test_an_item_listed_twice_is_pasted_twice(data):
    """two items that name one descriptor, a feathered one: the second blends into the first's result, as two host pastes do"""
    d = data
    for k in (0, 1, 2):                                                                         # a line, a quad, a curve (feathers 40, 1, 3)
        things = [d["things"][k]]
        tabs = rs.tables(things)
        tabs["items"] = np.concatenate([tabs["items"], tabs["items"]])
        n = len(tabs["entries"])
        tabs["entries"] = np.concatenate([tabs["entries"], tabs["entries"]])
        tabs["entry_item"] = np.concatenate([tabs["entry_item"], tabs["entry_item"] + 1])
        assert len(tabs["entries"]) == 2 * n
        once, twice = rs.host(d["page"], d["lines"], things), rs.host(d["page"], d["lines"], things * 2)
        assert not np.array_equal(once, twice)
        assert np.array_equal(_launch(d, tabs), twice)


# ------------------------------------------------------------------------------------------------------------- what the kernel skips
STACK = (0, 1, 2, 5, 9)          # a line, the quad over it, the arc over both, the column under the arc's end, the tapered chain: items 0, 1, 2, 3..5, 6


def _item(field, value):
    def edit(tabs, i):
        tabs["items"][field][i] = value
    return edit


def _desc(table, field, value, sub=None):
    def edit(tabs, i):
        index = int(tabs["items"]["index"][i])
        if table == "segs":
            index = int(tabs["curves"]["seg0"][index]) + 1
        if sub is None:
            tabs[table][field][index] = value
        else:
            tabs[table][field][index][sub] = value
    return edit


# (name, the index in STACK of the thing whose item is made unfollowable, the edit)
SKIPPED = (
    ("kind 3", 1, _item("kind", 3)),
    ("kind -1", 2, _item("kind", -1)),
    ("index -1 of a cell", 0, _item("index", -1)),
    ("index = n of a quad", 1, _item("index", 1)),
    ("index = n of a curve", 2, _item("index", 2)),
    ("index -1 of a curve", 4, _item("index", -1)),
    ("a NaN coefficient of a quad", 1, _desc("quads", "n", float("nan"), 4)),
    ("a NaN coefficient of a segment", 2, _desc("segs", "c", float("nan"), 3)),
    ("an infinite coefficient of a segment", 4, _desc("segs", "c", float("inf"), 0)),
    ("nseg 33", 2, _desc("curves", "nseg", 33)),
    ("nseg 0", 4, _desc("curves", "nseg", 0)),
    ("widths that do not chain to rw", 2, _desc("curves", "rw", 1)),
    ("a segment that does not chain", 2, _desc("segs", "u0", 0)),
    ("a quad's foreground outside the atlas", 1, _desc("quads", "ax0", 4000)),
    ("a curve's box outside the page", 4, _desc("curves", "bw", 4000)),
    ("a cell's line outside the lines", 0, _desc("cells", "line_index", rs.N_LINES)),
    ("feather beyond 1024", 1, _desc("quads", "feather", 1025)),
)


@pytest.mark.parametrize("name,which,edit", SKIPPED, ids=[s[0] for s in SKIPPED])
def test_an_unfollowable_item_alone_keeps_what_the_page_held(data, name, which, edit):
    """the spans are those of the sound tables, so the item stays listed in its tiles: the kernel's own checks skip it, and the items before and
    after it in the sequence stand"""
    d = data
    things = [d["things"][i] for i in STACK]
    tabs = rs.tables(things)
    spans, order = regions.bin_items(tabs["entries"], tabs["entry_item"], PAGE_H, PAGE_W)
    item = [0, 1, 2, 3, 6][which]
    assert tabs["items"]["kind"].tolist() == [0, 1, 2, 0, 0, 0, 2]
    edit(tabs, item)
    expect = rs.host(d["page"], d["lines"], things[:which] + things[which + 1:])
    assert not np.array_equal(expect, rs.host(d["page"], d["lines"], things))
    assert np.array_equal(_launch(d, tabs, spans, order), expect)


def test_a_span_past_the_order_keeps_its_tile_and_a_stray_listing_is_skipped(data):
    d = data
    things = [d["things"][i] for i in STACK]
    tabs = rs.tables(things)
    want = rs.host(d["page"], d["lines"], things)
    spans, order = regions.bin_items(tabs["entries"], tabs["entry_item"], PAGE_H, PAGE_W)
    t = 4                                                                                       # tile (1, 1): the line, the quad, the arc
    assert spans["count"][t] >= 3
    for first, count in ((len(order) - int(spans["count"][t]) + 1, None), (None, len(order) + 1), (-1, None), (2 ** 31 - 1, 2 ** 31 - 1)):
        bad = spans.copy()
        bad["first"][t] = bad["first"][t] if first is None else first
        bad["count"][t] = bad["count"][t] if count is None else count
        expect = want.copy()
        expect[16:32, 64:128] = d["page"][16:32, 64:128]
        assert not np.array_equal(expect, want) and np.array_equal(_launch(d, tabs, bad, order), expect)
    # every item listed in every tile, whether it touches it or not: the kernel skips the strays, so the bytes are the sound launch's
    n_items, n_tiles = len(tabs["items"]), len(spans)
    every = np.zeros((n_tiles,), dtype=np.dtype(_lib.TileSpan))
    every["count"] = n_items
    every["first"] = np.arange(n_tiles) * n_items
    assert np.array_equal(_launch(d, tabs, every, np.tile(np.arange(n_items, dtype=np.int32), n_tiles)), want)
    # entries outside the item table among them
    junk = np.tile(np.concatenate([np.asarray([-1, n_items, -2 ** 31, 2 ** 31 - 1], np.int32), np.arange(n_items, dtype=np.int32)]), n_tiles)
    every["count"] = n_items + 4
    every["first"] = np.arange(n_tiles) * (n_items + 4)
    assert np.array_equal(_launch(d, tabs, every, junk), want)


@pytest.mark.parametrize("page_h,page_w", ((3, 5), (33, 129)), ids=("one partial tile", "one column and one row past a tile multiple"))
def test_launch_regimes(data, page_h, page_w):
    d = data
    page = np.random.default_rng(page_h).integers(0, 256, (page_h, page_w, 3), dtype=np.uint8)
    if page_h == 3:
        things = [rs.line((0, 0, 5, 3), 0, 20, 1), rs.quad([(1, 0), (5, 0.5), (4.5, 3), (0.5, 2.5)], 1, 30, 0, page_h, page_w),
                  rs.curve(rs.arc(2.5, 4.0, 1.0, 4.0, 150.0, 30.0, 3), 2, 25, 1, page_h, page_w)]
    else:
        things = [rs.line((60, 10, 69, 23), 0, 96, 3), rs.quad([(100, 2), (129, 6), (127, 33), (98, 29)], 1, 80, 1, page_h, page_w),
                  rs.curve(rs.arc(64.0, 40.0, 14.0, 34.0, 170.0, 10.0, 6), 2, 96, 3, page_h, page_w), rs.line((128, 32, 1, 1), 3, 9, 0)]
    want = page.copy()
    for t in things:
        rs.paste_host(want, d["lines"], t)
    assert not np.array_equal(want, page)
    assert np.array_equal(_launch(d, rs.tables(things), page=page), want)


def test_compose_page_regions_equals_compose_regions_host(data):
    """the driver with one feather for all: regions.mixed_tables and paste_tables, 32-row lines so that the column goes through ``columns``"""
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    regs = [dict(box=[10, 5, 110, 45]), dict(quad=[(30, 12), (95, 20), (92, 36), (27, 28)]), dict(polygon=rs.arc(64.0, 60.0, 22.0, 38.0, 160.0, 20.0, 7)),
            dict(box=[88, 40, 100, 68], vertical=True), dict(box=[120, 2, 140, 12]), dict(polygon=rs.TAPERED)]
    cuts = [None, None, None, [40, 49, 59, 68], None, None]
    from marconet_amd import columns
    widths = columns.cell_widths(regs[3]["box"], cuts[3])
    out_ws = [96, 80, 96, sum(widths), None, 70]
    live = [i for i, w in enumerate(out_ws) if w is not None]
    joined = rng.integers(0, 256, (len(live), 32, 128, 3), dtype=np.uint8)
    lines = [None] * len(regs)
    for l, i in enumerate(live):
        lines[i] = joined[l, :, :out_ws[i]]
    for scale, feather in ((1, 3), (2, 0)):
        want = regions.compose_regions_host(page, lines, regs, scale=scale, feather=feather, overlap="order", cuts=cuts)
        got = regions.compose_page_regions(page, torch.from_numpy(joined).to(DEV), out_ws, regs, scale=scale, feather=feather, overlap="order", cuts=cuts)
        assert np.array_equal(got.cpu().numpy(), want) and not np.array_equal(want, lq_io.resize_cubic(page, scale, scale))
    with pytest.raises(ValueError, match="regions 0 and 1 overlap"):
        regions.compose_page_regions(page, torch.from_numpy(joined).to(DEV), out_ws, regs, scale=1, feather=3, cuts=cuts)


# ---------------------------------------------------------------------------------------------------------------- through the networks
@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    return MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")


@pytest.fixture(scope="module")
def mixed():
    """a 200 x 120 noise page carrying the reference's two labelled strips: a line, a column, a rotated quad and an arc whose end lies over the line"""
    strips = [(lq_io.load_png(os.path.join(cases_png.PNG_DIR, n)), lq_io.manual_text(n)) for n in cases_png.SR_STRIPS.values()]
    page = np.random.default_rng(9).integers(0, 256, (120, 200, 3), dtype=np.uint8)
    img, text = strips[0]
    h, w = min(img.shape[0], 28), min(img.shape[1], 120)
    page[8:8 + h, 6:6 + w] = img[:h, :w]
    t = text[:4]
    regs = [dict(box=[6, 8, 126, 36], text=t), dict(box=[170, 20, 190, 110], vertical=True, text=t),
            dict(quad=[[20, 60], [110, 72], [107, 92], [17, 80]], text=t), dict(polygon=[[float(x), float(y)] for x, y in rs.arc(120.0, 70.0, 26.0, 44.0, 200.0, 80.0, 6)], text=t),
            dict(box=[130, 100, 160, 115], text="")]
    return page, regs, [r["text"] for r in regs]


def _host_crops(page, recs):
    from marconet_amd import columns
    crops, boxes = [], []
    for r in recs:
        if r["kind"] == "column" and "cuts" in r:
            crops.append(columns.virtual_strip(page, r["box"], r["cuts"])[0])
            boxes.append(columns.virtual_boxes(r["widths"]))
        elif r["kind"] in ("line", "column"):
            b = r["box"]
            crops.append(page[b[1]:b[3], b[0]:b[2]])
            boxes.append(None)
        elif r["kind"] == "quad":
            crops.append(quads.warp_crop_host(page, quads.quad_map(r["quad"], r["cw"], r["ch"]), r["cw"], r["ch"]))
            boxes.append(None)
        else:
            crops.append(curves.warp_crop_host(page, r["segs"], r["cw"], r["ch"]))
            boxes.append(None)
    return crops, boxes


def test_a_mixed_page_equals_the_host_composition_and_refuse_raises_first(pipe, mixed):
    page, regs, texts = mixed
    restored = [bool(t) for t in texts]
    recs = regions.normalize_regions(page.shape[0], page.shape[1], regs, restored, texts, None, 2, 5, "order")
    assert [r["kind"] for r in recs] == ["line", "column", "quad", "curve", "line"]
    crops, boxes = _host_crops(page, recs)
    lines, plans = pipe.restore_lines(crops, texts, boxes, details=True)
    assert lines[4] is None and all(l is not None for l in lines[:4])
    got, info = pipe.restore_page_regions(page, regs, texts, scale=2, feather=5, details=True, overlap="order")
    want = regions.compose_regions_host(page, lines, regs, texts, None, 2, 5, "order")
    assert got.dtype == np.uint8 and np.array_equal(got, want) and not np.array_equal(got, lq_io.resize_cubic(page, 2, 2))
    assert [None if i is None else i["kind"] for i in info] == ["line", "column", "quad", "curve", None] and [i["plan"] for i in info[:4]] == plans[:4]
    # the arc's end lies over the line: the order shows there
    back = regions.compose_regions_host(page, lines[::-1], regs[::-1], texts[::-1], None, 2, 5, "order")
    assert not np.array_equal(want, back)
    with pytest.raises(ValueError, match="restore_page_regions: regions 0 and 3 overlap"):
        pipe.restore_page_regions(page, regs, texts, scale=2, feather=5)


def test_all_boxes_equal_restore_page_and_all_polygons_restore_page_curves(pipe, mixed):
    page, regs, texts = mixed
    boxes = [[6, 8, 126, 36], [20, 30, 150, 62], [100, 50, 190, 80], [130, 100, 160, 115]]
    tx = [texts[0], texts[1], texts[1], ""]
    want = pipe.restore_page(page, boxes, tx, scale=2, feather=6, overlap="order")
    assert np.array_equal(pipe.restore_page_regions(page, [dict(box=b) for b in boxes], tx, scale=2, feather=6, overlap="order"), want)
    assert not np.array_equal(want, lq_io.resize_cubic(page, 2, 2))
    polys = [regs[3]["polygon"], curves.box_polygon([6, 95, 70, 115], (40,)), [[150, 5], [195, 9], [194, 25], [149, 21]]]
    tx = [texts[1]] * 3
    want = pipe.restore_page_curves(page, polys, tx, scale=2, feather=4)
    assert np.array_equal(pipe.restore_page_regions(page, [dict(polygon=p) for p in polys], tx, scale=2, feather=4), want)
    assert not np.array_equal(want, lq_io.resize_cubic(page, 2, 2))


def test_no_live_region_is_the_background(pipe, mixed):
    page = mixed[0][:40, :90]
    assert np.array_equal(pipe.restore_page_regions(page, [], [], scale=2), lq_io.resize_cubic(page, 2, 2))
    assert np.array_equal(pipe.restore_page_regions(page, [dict(box=[5, 5, 60, 30]), dict(quad=[[5, 5], [60, 6], [60, 30], [5, 29]])], ["", ""], scale=2),
                          lq_io.resize_cubic(page, 2, 2))


def test_example_script_restores_a_mixed_file_in_one_call(tmp_path, mixed):
    from PIL import Image
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    page, regs, texts = mixed
    src, reg, out = str(tmp_path / "page.png"), str(tmp_path / "regions.json"), str(tmp_path / "out.png")
    Image.fromarray(page).save(src)
    with open(reg, "w", encoding="utf8") as f:
        json.dump(regs, f)
    env = dict(os.environ)
    env.pop("MARCONET_CKPT_DIR", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "restore_regions.py"), "-i", src, "-r", reg, "-o", out, "--scale", "2", "--feather", "5",
                        "--overlap", "order", "--precision", "fp32"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sde, sdg, sds, _ = checkpoints.load_state_dicts("")
    p = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, DEV), precision="fp32")
    want = p.restore_page_regions(page, regs, texts, scale=2, feather=5, overlap="order")
    assert np.array_equal(lq_io.load_png(out), want), r.stdout[-1500:]
    assert "Region 4 keeps the page's pixels" in r.stdout and "Region 1: a column" in r.stdout and "Region 3: a curve" in r.stdout
