"""not-gpu: a page that mixes kinds of region (marconet_amd/regions.py) — the refusals of normalize_regions, compose_regions_host against the four
single-kind definitions and against hand-written sequences of the kinds' host pastes, the item table and its binning against a brute-force loop
over the tiles, the C layout of mnet_page_item, the entry point's argument checks (the library loads without a GPU), the per-pixel header
compiled alone with the host compiler and compared with the numpy statements, and the build script's line.  Every comparison of pixels is
np.array_equal."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from marconet_amd import _lib, columns, curves, lq_io, pages, quads, regions
from tests import regions_scene as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marconet_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
PAGE_H, PAGE_W = 70, 150
ARC = rs.arc(64.0, 60.0, 22.0, 38.0, 160.0, 20.0, 7)


# ------------------------------------------------------------------------------------------------------------------- the refusals
def test_normalize_regions_refusals_name_the_region():
    line, col = dict(box=[10, 5, 110, 30]), dict(box=[88, 40, 100, 68], vertical=True)
    quad, arc = dict(quad=[(30, 12), (95, 20), (92, 36), (27, 28)]), dict(polygon=ARC)

    def norm(regs, overlap="refuse", texts=None, **kw):
        return regions.normalize_regions(PAGE_H, PAGE_W, regs, [True] * len(regs), ["abc"] * len(regs) if texts is None else texts, None, 1, 3, overlap, 32, **kw)
    with pytest.raises(ValueError, match='region 1: exactly one of "box", "quad" and "polygon"'):
        norm([line, dict(box=[0, 40, 20, 60], quad=quad["quad"])])
    with pytest.raises(ValueError, match="region 0: exactly one of"):
        norm([dict(text="no shape")])
    with pytest.raises(ValueError, match='region 1: "vertical" applies to a "box" only'):
        norm([line, dict(quad=quad["quad"], vertical=True)])
    with pytest.raises(ValueError, match='region 0: "vertical" applies to a "box" only'):
        norm([dict(polygon=ARC, vertical=True)])
    # a cross-kind overlap: a line under an arc, a quad over a column — both regions named
    with pytest.raises(ValueError, match=r"regions 0 and 1 overlap \(a line and a curve\)"):
        norm([dict(box=[10, 5, 110, 45]), arc])
    with pytest.raises(ValueError, match=r"regions 1 and 2 overlap \(a column and a quad\)"):
        norm([dict(box=[0, 0, 20, 10]), col, dict(quad=[(60, 44), (120, 48), (119, 62), (59, 58)])])
    recs = norm([dict(box=[10, 5, 110, 45]), arc, col, quad], "order")                    # the same pages accepted in order
    assert [r["kind"] for r in recs] == ["line", "curve", "column", "quad"] and [len(r["pieces"]) for r in recs] == [1, 6, 1, 1]
    assert recs[2]["cuts"] == columns.cell_cuts([88, 40, 100, 68], 3) and recs[2]["widths"] == columns.cell_widths([88, 40, 100, 68], recs[2]["cuts"])
    # a region that is not restored takes no part in the rule
    assert len(regions.normalize_regions(PAGE_H, PAGE_W, [dict(box=[10, 5, 110, 45]), arc], [True, False], None, None, 1, 3)) == 2
    # regions that only touch are not an overlap: a box against a box, a quad's edge on a box's edge, a column beside a line
    norm([dict(box=[0, 0, 60, 20]), dict(box=[60, 0, 150, 20]), dict(quad=[(0, 20), (60, 20), (60, 40), (0, 40)]), dict(box=[60, 20, 80, 60], vertical=True)])
    # every other refusal stands in order mode, under the region's own number
    for bad, match in ((dict(box=[5, 5, 5, 30]), "region 1: box .* is empty or lies outside"), (dict(quad=[(0, 0), (0, 10), (10, 10), (10, 0)]), "region 1: the corners run counter-clockwise"),
                       (dict(polygon=ARC[:5]), "region 1: an even number of points"), (dict(quad=[(200, 0), (300, 0), (300, 20), (200, 20)]), "region 1: its bounding box .* misses"),
                       (dict(box=[88, 40, 100, 42], vertical=True), "region 1: character \\d+: its cell is empty")):
        with pytest.raises(ValueError, match=match):
            norm([line, bad], "order")
    with pytest.raises(ValueError, match="region 1: its cuts .* do not run from"):
        norm([line, col], "order", cuts=[None, [41, 50, 68]])
    with pytest.raises(ValueError, match="overlap must be"):
        norm([line], "blend")
    with pytest.raises(ValueError, match="scale"):
        regions.normalize_regions(PAGE_H, PAGE_W, [line], [True], None, None, 9, 3)
    with pytest.raises(ValueError, match="one line .* per region"):
        regions.normalize_regions(PAGE_H, PAGE_W, [line], [True, True], None, None, 1, 3)


def test_entry_point_refuses_before_anything_runs():
    """the pipeline's host checks need neither weights on a device nor a launch"""
    from marconet_amd import networks
    from marconet_amd.pipeline import MarconetPipeline
    pipe = MarconetPipeline(networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet())
    page = np.zeros((120, 200, 3), np.uint8)
    a = lq_io.alphabet()[10]
    regs = [dict(box=[10, 5, 110, 45]), dict(polygon=ARC)]
    with pytest.raises(ValueError, match="restore_page_regions: regions 0 and 1 overlap"):
        pipe.restore_page_regions(page, regs, [a, a])
    with pytest.raises(ValueError, match="restore_page_regions: overlap must be"):
        pipe.restore_page_regions(page, regs, [a, a], overlap="blend")
    with pytest.raises(ValueError, match='restore_page_regions: region 1: exactly one of'):
        pipe.restore_page_regions(page, [regs[0], dict(text="x")], [a, a], overlap="order")
    with pytest.raises(ValueError, match="restore_page_regions: region 1: character \\d+: its cell is empty"):
        pipe.restore_page_regions(page, [regs[0], dict(box=[150, 5, 170, 25], vertical=True)], [a, a * 40], overlap="order")
    with pytest.raises(ValueError, match="restore_page_regions needs texts"):
        pipe.restore_page_regions(page, regs, None)
    with pytest.raises(ValueError, match="per region expected"):
        pipe.restore_page_regions(page, regs, [a])


# ------------------------------------------------------------------------------------------------------------------- the definition
def _lines(n, rows=32, seed=3, w=90):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8), [rng.integers(0, 256, (rows, w + 7 * i, 3), dtype=np.uint8) for i in range(n)]


@pytest.mark.parametrize("scale,feather", ((1, 3), (2, 0)))
def test_single_kind_pages_without_overlaps_are_the_four_definitions(scale, feather):
    page, lines = _lines(4)
    boxes = [[0, 0, 60, 20], [60, 0, 150, 20], [0, 20, 150, 45], [110, 45, 150, 70]]
    lines[3] = None
    assert np.array_equal(regions.compose_regions_host(page, lines, [dict(box=b) for b in boxes], scale=scale, feather=feather),
                          pages.compose_host(page, lines, boxes, scale, feather))
    cboxes, cuts = [[88, 4, 100, 64], [10, 20, 80, 44]], [[4, 20, 44, 64], None]
    widths = columns.cell_widths(cboxes[0], cuts[0])
    clines = [np.random.default_rng(4).integers(0, 256, (32, sum(widths), 3), dtype=np.uint8), lines[0]]
    want = columns.compose_columns_host(page, clines, cboxes, cuts, scale, feather)
    regs = [dict(box=cboxes[0], vertical=True), dict(box=cboxes[1], vertical=False)]
    assert np.array_equal(regions.compose_regions_host(page, clines, regs, scale=scale, feather=feather, cuts=cuts), want)
    qs = [[(30, 12), (95, 20), (92, 36), (27, 28)], [(135, 4), (160, 8), (158, 20), (133, 16)], [(5, 50), (40, 48), (41, 62), (6, 64)]]
    assert np.array_equal(regions.compose_regions_host(page, lines[:3], [dict(quad=q) for q in qs], scale=scale, feather=feather),
                          quads.compose_quads_host(page, lines[:3], qs, scale, feather))
    ps = [ARC, rs.TAPERED, curves.box_polygon([0, 0, 40, 12], (13,))]
    assert np.array_equal(regions.compose_regions_host(page, lines[:3], [dict(polygon=p) for p in ps], scale=scale, feather=feather),
                          curves.compose_curves_host(page, lines[:3], ps, scale, feather))


def _bbox(rec, s):
    if "rect" in rec:
        x0, y0, rw, rh = rec["rect"]
    else:
        x0, y0, rw, rh = rec["bbox"]
    return x0, y0, x0 + rw, y0 + rh


def test_order_matters_only_inside_the_intersection_and_feather_0_hides_what_lies_under():
    page, lines = _lines(4)
    regs = [dict(box=[10, 5, 110, 45]), dict(polygon=ARC), dict(quad=[(30, 12), (95, 20), (92, 36), (27, 28)]), dict(box=[88, 40, 100, 68], vertical=True)]
    cuts = [None, None, None, [40, 49, 59, 68]]
    lines[3] = np.random.default_rng(5).integers(0, 256, (32, sum(columns.cell_widths(regs[3]["box"], cuts[3])), 3), dtype=np.uint8)
    s, F = 2, 4
    with pytest.raises(ValueError, match="regions 0 and 1 overlap"):
        regions.compose_regions_host(page, lines, regs, scale=s, feather=F, cuts=cuts)
    got = regions.compose_regions_host(page, lines, regs, scale=s, feather=F, overlap="order", cuts=cuts)
    recs = regions.normalize_regions(PAGE_H, PAGE_W, regs, [True] * 4, None, None, s, F, "order", 32, cuts)
    want = lq_io.resize_cubic(page, s, s)
    pages.paste_host(want, lines[0], recs[0]["rect"], F)
    curves.warp_paste_host(want, pages.line_to_rect(lines[1], recs[1]["rw"], recs[1]["rh"]), recs[1]["out_segs"], recs[1]["rw"], recs[1]["rh"], F)
    quads.warp_paste_host(want, pages.line_to_rect(lines[2], recs[2]["rw"], recs[2]["rh"]), quads.inverse_map(quads.quad_map(recs[2]["out_quad"], recs[2]["rw"], recs[2]["rh"])),
                          recs[2]["rw"], recs[2]["rh"], F)
    columns.paste_column_host(want, lines[3], recs[3]["rect"], cuts[3], recs[3]["widths"], F)
    assert np.array_equal(got, want)
    for a, b in ((0, 1), (1, 2), (1, 3), (0, 2)):                                       # a line and an arc, an arc and a quad, an arc and a column, ...
        perm = list(range(4))
        perm[a], perm[b] = b, a
        swapped = regions.compose_regions_host(page, [lines[i] for i in perm], [regs[i] for i in perm], scale=s, feather=F, overlap="order", cuts=[cuts[i] for i in perm])
        diff = (swapped != got).any(axis=2)
        assert diff.any()
        ys, xs = np.nonzero(diff)
        boxes = [_bbox(recs[i], s) for i in range(4)]
        others = [i for i in range(4) if i not in (a, b)]
        # a changed pixel lies in the two regions' boxes, or — where a third region lies between them in the order — in that one's and one of theirs
        for y, x in zip(ys, xs):
            inside = [i for i in range(4) if boxes[i][0] <= x < boxes[i][2] and boxes[i][1] <= y < boxes[i][3]]
            assert (a in inside and b in inside) or (len(set(inside) & {a, b}) >= 1 and any(o in inside and a < o < b for o in others)), (a, b, x, y, inside)
    # a later region with feather 0 over the same shape makes the earlier one vanish — for each kind that is warped
    for reg in (regs[1], regs[2]):
        two = regions.compose_regions_host(page, [lines[0], lines[1]], [reg, reg], scale=s, feather=0, overlap="order")
        assert np.array_equal(two, regions.compose_regions_host(page, [None, lines[1]], [reg, reg], scale=s, feather=0, overlap="order"))
        assert not np.array_equal(two, regions.compose_regions_host(page, [lines[0], None], [reg, reg], scale=s, feather=0, overlap="order"))


# ------------------------------------------------------------------------------------------------------------- the items and their bins
def _brute(rects, page_h, page_w):
    out = []
    for ty in range(-(-page_h // 16)):
        for tx in range(-(-page_w // 64)):
            X0, Y0, X1, Y1 = 64 * tx, 16 * ty, min(64 * tx + 64, page_w), min(16 * ty + 16, page_h)
            out.append([c for c, (x0, y0, rw, rh) in enumerate(rects) if x0 < X1 and X0 < x0 + rw and y0 < Y1 and Y0 < y0 + rh])
    return out


def test_item_table_and_binning_of_the_scene():
    things = rs.scene()
    tabs = rs.tables(things)
    items = tabs["items"]
    assert items.dtype == np.dtype(_lib.PageItem) and items["kind"].tolist() == [0, 1, 2, 2, 1, 0, 0, 0, 0, 1, 1, 2]
    assert items["index"].tolist() == [0, 0, 0, 1, 1, 1, 2, 3, 4, 2, 3, 2]               # per kind, in paste order; the column's three cells consecutive
    rects = [tuple(int(it[n]) for n in ("x0", "y0", "rw", "rh")) for it in items]
    assert rects[0] == (10, 5, 100, 40) and rects[1] == tuple(things[1]["rec"]["bbox"]) and rects[5:8] == [(88, 40, 12, 9), (88, 49, 12, 10), (88, 59, 12, 9)]
    # pages.bin_tiles bins the items as they are: their field names are its own
    spans, order = pages.bin_tiles(items, PAGE_H, PAGE_W)
    per_tile = [order[int(s["first"]):int(s["first"]) + int(s["count"])].tolist() for s in spans]
    assert per_tile == _brute(rects, PAGE_H, PAGE_W) and len(spans) == 15
    # the refinement: a curve is listed where one of its segments' boxes touches the tile — a subset of the above, everything else unchanged
    rspans, rorder = regions.bin_items(tabs["entries"], tabs["entry_item"], PAGE_H, PAGE_W)
    refined = [rorder[int(s["first"]):int(s["first"]) + int(s["count"])].tolist() for s in rspans]
    curve_items = [i for i, k in enumerate(items["kind"]) if k == 2]
    assert rorder.dtype == np.int32 and rspans.dtype == np.dtype(_lib.TileSpan) and rspans["first"].tolist() == (np.cumsum(rspans["count"]) - rspans["count"]).tolist()
    for full, part in zip(per_tile, refined):
        assert part == sorted(set(part)) and set(part) <= set(full) and [i for i in full if i not in curve_items] == [i for i in part if i not in curve_items]
    assert sum(len(p) for p in refined) < sum(len(p) for p in per_tile)                   # an arc leaves part of its bounding box empty
    # every tile that holds a claimed pixel of a curve lists it
    page, lines = rs.data()
    for item, t in zip(curve_items, [t for t in things if t["kind"] == "curve"]):
        claimed = (rs.host(np.zeros_like(page), 1 + lines // 2, [dict(t, F=0)]) != 0).any(axis=2)
        assert claimed.any()
        for ty, tx in {(y // 16, x // 64) for y, x in zip(*np.nonzero(claimed))}:
            assert item in refined[ty * 3 + tx], (item, ty, tx)
    # regions.mixed_tables states the same tables for one feather
    regs = [dict(box=[10, 5, 110, 45]), dict(quad=[(30, 12), (95, 20), (92, 36), (27, 28)]), dict(polygon=ARC), dict(box=[0, 50, 20, 60]), dict(box=[120, 30, 140, 66], vertical=True)]
    recs = regions.normalize_regions(PAGE_H, PAGE_W, regs, [True, True, True, False, True], ["ab"] * 5, None, 1, 3, "order", 32)
    widths = recs[4]["widths"]
    m = regions.mixed_tables(recs, [96, 80, 96, None, sum(widths)], 3, 32)
    assert m["items"]["kind"].tolist() == [0, 1, 2, 0, 0] and m["items"]["index"].tolist() == [0, 0, 0, 1, 2] and len(m["segs"]) == 6
    assert np.array_equal(m["cells"][:1], pages.as_cell(pages.build_table([recs[0]["rect"]], [96], 3, 32, [0])))
    assert np.array_equal(m["cells"][1:], columns.paste_table([(recs[4]["box"], recs[4]["cuts"], widths, None)], [3], [recs[4]["rect"]], 3, 32))
    assert np.array_equal(m["quads"], quads.paste_table([recs[1]], 3, [(0, 0)])) and m["fg"]["line_index"].tolist() == [1, 2]
    assert np.array_equal(m["curves"], curves.paste_table([recs[2]], 3, [(0, recs[1]["rh"])])[0]) and m["atlas_hw"] == (recs[1]["rh"] + recs[2]["rh"], max(recs[1]["rw"], recs[2]["rw"]))
    assert m["entry_item"].tolist() == [0, 1] + [2] * 6 + [3, 4]
    with pytest.raises(ValueError, match="ascending"):
        regions.bin_items(tabs["entries"], tabs["entry_item"][::-1].copy(), PAGE_H, PAGE_W)


def test_crop_tables_take_a_base_offset():
    maps, sizes = [quads.quad_map(quads.box_quad([1, 2, 11, 8]), 10, 6)] * 2, [(10, 6), (4, 6)]
    t0, n0 = quads.crop_table(maps, sizes, [0, 3])
    t1, n1 = quads.crop_table(maps, sizes, [0, 3], base=1000)
    assert n0 == 3 * 84 and n1 == n0 + 1000 and t1["offset"].tolist() == [1000, 1180] and t0["offset"].tolist() == [0, 180]
    segs = curves.check_curves(PAGE_H, PAGE_W, [ARC], [True], 1, 3, 16)[0]["segs"]
    c0, s0, m0 = curves.crop_table([segs, segs], [(10, 6), (4, 6)])
    c1, s1, m1 = curves.crop_table([segs, segs], [(10, 6), (4, 6)], base=77)
    assert m1 == m0 + 77 and c1["offset"].tolist() == [77, 257] and c0["offset"].tolist() == [0, 180] and np.array_equal(s0, s1)


# ---------------------------------------------------------------------------------------------------------------------------- the ABI
def test_mixed_header_declares_exactly_the_bound_symbol_and_the_item_layout(tmp_path):
    text = open(os.path.join(INCLUDE, "marconet_hip_mixed.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(mnet_\w+)\s*\(", code)) == set(_lib.MIXED_SYMBOLS) == {"mnet_paste_mixed_u8"}
    assert len(_lib.MIXED_SYMBOLS["mnet_paste_mixed_u8"][1]) == 25
    cpath, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    fields = ("kind", "index", "x0", "y0", "rw", "rh")
    with open(cpath, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "marconet_hip_mixed.h"\nint main(void) {\n'
                'printf("%d %d %d %d %d ' + "%d " * 6 + '\\n", (int)sizeof(mnet_page_item), MNET_ITEM_CELL, MNET_ITEM_QUAD, MNET_ITEM_CURVE, MNET_ABI_VERSION, '
                + ", ".join("(int)offsetof(mnet_page_item, %s)" % n for n in fields) + ');\nreturn 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, cpath])
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, cpath, "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    S = _lib.PageItem
    assert got == [ctypes.sizeof(S), _lib.ITEM_CELL, _lib.ITEM_QUAD, _lib.ITEM_CURVE, _lib.ABI_VERSION] + [getattr(S, n).offset for n in fields]
    assert got[:5] == [24, 0, 1, 2, 4] and [n for n, _ in S._fields_] == list(fields) and np.dtype(S).itemsize == 24 and ctypes.alignment(S) == 4
    lib = _lib.load()
    assert hasattr(lib, "mnet_paste_mixed_u8") and lib.mnet_abi_version() == 4 and len(_lib.SYMBOLS) == 45
    assert not set(_lib.MIXED_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.ORDERED_SYMBOLS) | set(_lib.QUAD_SYMBOLS) | set(_lib.CURVE_SYMBOLS) | set(_lib.COLUMN_SYMBOLS))


def test_entry_point_validates_arguments_without_device():
    lib = _lib.load()
    ok = dict(lines=16, n_lines=2, rows=128, line_w=300, atlas=32, atlas_h=40, atlas_w=200, cells=48, n_cells=3, quads=56, n_quads=2, curves=64, n_curves=1,
              segs=72, n_segs=5, items=80, n_items=6, spans=84, n_spans=15, order=88, n_order=7, page=96, page_h=70, page_w=150)
    names = ("lines", "n_lines", "rows", "line_w", "atlas", "atlas_h", "atlas_w", "cells", "n_cells", "quads", "n_quads", "curves", "n_curves", "segs", "n_segs",
             "items", "n_items", "spans", "n_spans", "order", "n_order", "page", "page_h", "page_w")

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mnet_paste_mixed_u8(*([a[n] for n in names] + [None]))
    for bad in ("items", "spans", "order", "page", "lines", "atlas", "cells", "quads", "curves", "segs"):
        assert call(**{bad: None}) == -1 and b"null" in lib.mnet_last_error(), bad
    # a table may be absent with count 0 — the next refusal is then another one (the spans): nothing is launched here
    for gone in (dict(cells=None, n_cells=0, lines=None, n_lines=0, rows=0, line_w=0), dict(quads=None, n_quads=0),
                 dict(quads=None, n_quads=0, curves=None, n_curves=0, segs=None, n_segs=0, atlas=None, atlas_h=0, atlas_w=0)):
        assert call(n_spans=14, **gone) == -1 and b"spans for a page of 15 tiles" in lib.mnet_last_error()
    for bad in (dict(n_cells=-1), dict(n_quads=-1), dict(n_curves=-2), dict(n_segs=-1), dict(n_items=0), dict(n_order=0), dict(n_order=-3), dict(page_h=0), dict(page_w=-7),
                dict(n_lines=0), dict(rows=0), dict(line_w=-5), dict(atlas_h=0), dict(atlas_w=0), dict(n_segs=0)):
        assert call(**bad) == -1 and b"bad shape" in lib.mnet_last_error(), bad
    for bad in (14, 16, 0, -1):                                                         # the page has 3 x 5 tiles
        assert call(n_spans=bad) == -1 and b"spans for a page of 15 tiles" in lib.mnet_last_error()
    assert call(page_h=16 * 65536, page_w=64 * 32768, n_spans=2 ** 31 - 1) == -1 and b"too large" in lib.mnet_last_error()
    assert call(page_h=16 * 4096, page_w=64 * 4096, n_spans=2 ** 24) == -1 and b"too large" in lib.mnet_last_error()      # 2^24 tiles
    for bad in (dict(cells=52), dict(quads=57), dict(curves=68), dict(segs=73)):
        assert call(**bad) == -2 and b"8-byte aligned" in lib.mnet_last_error()
    for bad in (dict(items=82), dict(spans=85), dict(order=90)):
        assert call(**bad) == -2 and b"4-byte aligned" in lib.mnet_last_error()


def test_ops_refuses_cpu_tensors():
    from marconet_amd import ops
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.paste_mixed_u8(u8(2, 128, 300, 3), None, u8(1, 72), None, None, None, u8(1, 24), u8(15, 8), torch.zeros((4,), dtype=torch.int32), u8(70, 150, 3))


# ------------------------------------------------------------------------------------------------------------ the header on the host
def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    pytest.skip("no host C++ compiler")


MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "warp_paste.h"
// argv: in out | in: int32 page_h page_w atlas_h atlas_w n_quads n_curves n_segs, then the tables, the atlas, the page
template <class T> static std::vector<T> take(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) exit(2); return v; }
int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    std::vector<int32_t> h = take<int32_t>(f, 7);
    const int PH = h[0], PW = h[1], AH = h[2], AW = h[3];
    std::vector<mnet_quad_region> Q = take<mnet_quad_region>(f, h[4]);
    std::vector<mnet_curve_region> C = take<mnet_curve_region>(f, h[5]);
    std::vector<mnet_curve_seg> G = take<mnet_curve_seg>(f, h[6]);
    std::vector<uint8_t> atlas = take<uint8_t>(f, (size_t)AH * AW * 3), page = take<uint8_t>(f, (size_t)PH * PW * 3);
    fclose(f);
    const size_t row = (size_t)AW * 3;
    for (const mnet_quad_region& R : Q) {
        if (!quad_region_followed(R, AH, AW, PH, PW)) continue;
        for (int Y = R.by0; Y < R.by0 + R.bh; ++Y)
            for (int X = R.bx0; X < R.bx0 + R.bw; ++X)
                quad_paste_pixel(R.n, R.rw, R.rh, (unsigned)R.feather, atlas.data() + ((size_t)R.ay0 * AW + R.ax0) * 3, row, X + 0.5, Y + 0.5, page.data() + ((size_t)Y * PW + X) * 3);
    }
    for (const mnet_curve_region& R : C) {
        if (!curve_region_followed(R, AH, AW, PH, PW, (int)G.size())) continue;
        CurveSegL S[CURVE_MAX_SEGS];
        bool good = true;
        for (int t = 0; t < R.nseg; ++t) { mnet_curve_seg g; good = curve_stage(S, G.data(), R.seg0, t, g) && curve_seg_in_region(g, R) && good; }
        if (!good || (long long)S[R.nseg - 1].u0 + S[R.nseg - 1].w != R.rw) continue;
        for (int Y = R.by0; Y < R.by0 + R.bh; ++Y)
            for (int X = R.bx0; X < R.bx0 + R.bw; ++X)
                curve_paste_pixel(S, R.nseg, R.rw, R.rh, (unsigned)R.feather, atlas.data() + ((size_t)R.ay0 * AW + R.ax0) * 3, row, X, Y, X + 0.5, Y + 0.5, page.data() + ((size_t)Y * PW + X) * 3);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(page.data(), 1, page.size(), f) != page.size()) return 3;
    fclose(f);
    return 0;
}
"""


def test_per_pixel_header_compiles_alone_on_the_host_and_gives_the_numpy_bytes(tmp_path):
    """warp_paste.h, with the headers it includes, through the host compiler alone (-ffp-contract=off, as the device build): the quadrilaterals and
    curves of the scene pasted pixel by pixel by quad_paste_pixel / curve_paste_pixel give quads.warp_paste_host's and curves.warp_paste_host's
    bytes; an unfollowable region is left out by the header's own lists"""
    src, exe = str(tmp_path / "main.cpp"), str(tmp_path / "main")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.check_call([_cxx(), "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I", CSRC, src, "-o", exe])
    page, lines = rs.data()
    things = [t for t in rs.scene() if t["kind"] in ("quad", "curve")]
    things = [t for t in things if t["kind"] == "quad"] + [t for t in things if t["kind"] == "curve"]      # the program's order: quads, then curves
    tabs = rs.tables(things)
    atlas = np.zeros(tuple(tabs["atlas_hw"]) + (3,), np.uint8)
    for r, t in zip(tabs["fg"], things):
        atlas[int(r["y0"]):int(r["y0"]) + int(r["rh"]), :int(r["rw"])] = pages.line_to_rect(lines[t["li"]][:, :t["src_w"]], int(r["rw"]), int(r["rh"]))
    for drop in (None, 1):
        quad_tab, curve_tab, kept = tabs["quads"].copy(), tabs["curves"].copy(), list(things)
        if drop is not None:
            quad_tab["feather"][drop] = 1025                                           # unfollowable: that region alone keeps the page
            curve_tab["nseg"][0] = 33
            kept = [t for i, t in enumerate(things) if i not in (drop, len(quad_tab))]
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.asarray([PAGE_H, PAGE_W, atlas.shape[0], atlas.shape[1], len(quad_tab), len(curve_tab), len(tabs["segs"])], np.int32).tobytes())
            for part in (quad_tab, curve_tab, tabs["segs"], atlas, page):
                f.write(np.ascontiguousarray(part).tobytes())
        subprocess.check_call([exe, inp, out])
        got = np.fromfile(out, np.uint8).reshape(page.shape)
        assert np.array_equal(got, rs.host(page, lines, kept)) and not np.array_equal(got, page)


# ---------------------------------------------------------------------------------------------------------------------- the build
def test_build_script_compiles_and_stamps_the_kernel_and_the_bodies_are_stated_once():
    sh = open(os.path.join(CSRC, "build.sh")).read()
    assert re.search(r'^SRCS="[^"]*\bmixed_kernels\b[^"]*"', sh, flags=re.M) and 'mixed_kernels) echo "-ffp-contract=off" ;;' in sh
    stamp = re.search(r'\[ "\$1" = mixed_kernels \] && cat ([^;]*);', sh).group(1)
    for name in ("cell_paste.h", "warp_paste.h", "curve_map.h", "quad_map.h", "lq_taps.h", "page_blend.h", "page_tile.h", "marconet_hip_columns.h",
                 "marconet_hip_ordered.h", "marconet_hip_quad.h", "marconet_hip_curve.h", "marconet_hip_mixed.h"):
        assert name in stamp, name
    assert "page_kernels.hip" not in stamp
    for unit in ("quad_kernels", "curve_kernels"):
        assert "warp_paste.h" in re.search(r'\[ "\$1" = %s \] && cat ([^;]*);' % unit, sh).group(1)
    src = {n: open(os.path.join(CSRC, n)).read() for n in ("mixed_kernels.hip", "quad_kernels.hip", "curve_kernels.hip", "page_kernels.hip", "warp_paste.h")}
    mixed = src["mixed_kernels.hip"]
    assert '#include "cell_paste.h"' in mixed and '#include "warp_paste.h"' in mixed and ".hip\"" not in mixed
    assert not any("MNET_PAGE_CELL_ONLY" in open(os.path.join(CSRC, n)).read() for n in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, n)))
    # ONE page-tile compositor, which both entry points launch
    assert mixed.count("__global__") == 1 and "mnet_paste_ordered_u8" in mixed and "mnet_paste_mixed_u8" in mixed
    # the per-pixel arithmetic is stated once: in cell_paste.h for a cell, in warp_paste.h for a quadrilateral and a curve
    for body in ("quad_pos(", "curve_inv(", "quad_mix(", "page_feather("):
        assert body not in mixed and src["warp_paste.h"].count(body) == 1, body
    assert "quad_pos(R.n" not in src["quad_kernels.hip"] and "curve_inv(" not in src["curve_kernels.hip"] and "page_feather(" not in src["quad_kernels.hip"] + src["curve_kernels.hip"]
    assert src["quad_kernels.hip"].count("quad_paste_pixel(") == 1 and src["curve_kernels.hip"].count("curve_paste_pixel(") == 1
    assert mixed.count("quad_paste_pixel(") == 1 and mixed.count("curve_paste_pixel(") == 1 and mixed.count("cell_foreground(") == 1 and mixed.count("cell_blend(") == 1
    assert mixed.count("cell_followed(") == 1
    assert "page_box_avg(" not in mixed and "pt_round_clip(" not in mixed and "asm" not in mixed and "asm" not in src["warp_paste.h"]
    assert mixed.count("__shared__") == 2 and "__shared__ PtTaps s;" in mixed and "__shared__ CurveSegL S[CURVE_MAX_SEGS];" in mixed
