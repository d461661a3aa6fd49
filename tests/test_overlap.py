"""not-gpu: overlapping regions of a page in the caller's order (overlap="order") — the host definition (pages.compose_host,
columns.compose_columns_host: painter's order, stated in pages.py's head) against hand-written sequences of paste_host / paste_column_host, the
binning of cells into page tiles (pages.bin_tiles) against a brute-force loop over the tiles, the host twin of the device's as_cell, the C layout
of the span record, the entry point's argument checks (the library loads without a GPU) and the build script's line.  Every comparison of pixels
is np.array_equal."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from marconet_amd import _lib, columns, lq_io, pages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marconet_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
PAGE_H, PAGE_W = 70, 150


# ------------------------------------------------------------------------------------------------------------------- the definition
# boxes of a 150 x 70 page; 0, 1 and 2 share the pixels of [30, 50) x [12, 20): three deep.  3 lies apart.
STACK = ([5, 5, 60, 30], [20, 10, 100, 40], [30, 0, 50, 60], [110, 45, 150, 70])
DISJOINT = ([0, 0, 60, 20], [60, 0, 150, 20], [0, 20, 150, 45], [110, 45, 150, 70])


def _scene(boxes, rows=16, seed=1):
    rng = np.random.default_rng(seed)
    page = rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    lines = [rng.integers(0, 256, (rows, 30 + 7 * i, 3), dtype=np.uint8) for i in range(len(boxes))]
    return page, lines


def _rect(b, s):
    return (s * b[0], s * b[1], s * (b[2] - b[0]), s * (b[3] - b[1]))


def _depth(rects, h, w):
    cover = np.zeros((h, w), np.int64)
    for x0, y0, rw, rh in rects:
        cover[y0:y0 + rh, x0:x0 + rw] += 1
    return int(cover.max())


@pytest.mark.parametrize("scale,feather", ((1, 3), (2, 8), (1, 0)))
def test_compose_host_in_order_is_the_sequence_of_paste_host(scale, feather):
    page, lines = _scene(STACK)
    lines[3] = None                                                                    # a region that keeps the background
    rects = [_rect(b, scale) for b in STACK]
    assert _depth(rects[:3], scale * PAGE_H, scale * PAGE_W) == 3
    with pytest.raises(ValueError, match="regions 0 and 1 overlap"):
        pages.compose_host(page, lines, STACK, scale, feather)
    with pytest.raises(ValueError, match="regions 0 and 1 overlap"):
        pages.compose_host(page, lines, STACK, scale, feather, overlap="refuse")
    got = pages.compose_host(page, lines, STACK, scale, feather, overlap="order")
    want = lq_io.resize_cubic(page, scale, scale)
    for i in (0, 1, 2):
        pages.paste_host(want, lines[i], rects[i], feather)
    assert np.array_equal(got, want)
    back = pages.compose_host(page, lines[::-1], STACK[::-1], scale, feather, overlap="order")
    want_back = lq_io.resize_cubic(page, scale, scale)
    for i in (2, 1, 0):
        pages.paste_host(want_back, lines[i], rects[i], feather)
    assert np.array_equal(back, want_back)
    assert not np.array_equal(got, back)                                               # the order shows: an order bug cannot hide
    x0, y0, rw, rh = rects[2]                                                          # with no feather the last region's rectangle is its own foreground
    if feather == 0:
        assert np.array_equal(got[y0:y0 + rh, x0:x0 + rw], pages.line_to_rect(lines[2], rw, rh))


def test_a_disjoint_scene_gives_the_bytes_of_refuse():
    page, lines = _scene(DISJOINT, seed=2)
    assert _depth([_rect(b, 2) for b in DISJOINT], 2 * PAGE_H, 2 * PAGE_W) == 1
    a = pages.compose_host(page, lines, DISJOINT, 2, 5)
    assert np.array_equal(pages.compose_host(page, lines, DISJOINT, 2, 5, overlap="order"), a)
    assert np.array_equal(pages.compose_host(page, lines[::-1], DISJOINT[::-1], 2, 5, overlap="order"), a)


def test_every_other_refusal_stands_in_order_mode():
    page, lines = _scene(STACK)
    for bad, match in (([5, 5, 5, 30], "empty or lies outside"), ([5, 5, 160, 30], "empty or lies outside"), ([5.5, 5, 60, 30], "integer box")):
        with pytest.raises(ValueError, match=match):
            pages.compose_host(page, lines, (bad,) + STACK[1:], 1, 3, overlap="order")
    with pytest.raises(ValueError, match="scale"):
        pages.compose_host(page, lines, STACK, 9, 3, overlap="order")
    with pytest.raises(ValueError, match="feather"):
        pages.compose_host(page, lines, STACK, 1, 1025, overlap="order")
    tall = [np.zeros((128, 40, 3), np.uint8)] * 4
    with pytest.raises(ValueError, match="region 0: its rectangle is 7 rows high"):
        pages.compose_host(page, tall, ([5, 5, 60, 12],) + STACK[1:], 1, 3, overlap="order")


# a column of three cells (rows 32: one line column per strip column) crossing a line, and a second line over both
COL_BOXES = ([40, 4, 60, 64], [10, 20, 140, 44], [30, 30, 70, 50])
COL_CUTS = ([4, 20, 44, 64], None, None)


def _column_scene():
    rng = np.random.default_rng(3)
    page = rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    widths = columns.cell_widths(COL_BOXES[0], COL_CUTS[0])
    lines = [rng.integers(0, 256, (32, sum(widths), 3), dtype=np.uint8), rng.integers(0, 256, (32, 90, 3), dtype=np.uint8),
             rng.integers(0, 256, (32, 41, 3), dtype=np.uint8)]
    return page, lines, widths


def _column_sequence(page, lines, widths, seq, scale, feather):
    out = lq_io.resize_cubic(page, scale, scale)
    for i in seq:
        if COL_CUTS[i] is None:
            pages.paste_host(out, lines[i], _rect(COL_BOXES[i], scale), feather)
        else:
            columns.paste_column_host(out, lines[i], _rect(COL_BOXES[i], scale), COL_CUTS[i], widths, feather)
    return out


@pytest.mark.parametrize("scale,feather", ((1, 4), (2, 0)))
def test_compose_columns_host_in_order_is_the_sequence_of_its_pastes(scale, feather):
    page, lines, widths = _column_scene()
    assert _depth([_rect(b, 1) for b in COL_BOXES], PAGE_H, PAGE_W) == 3
    with pytest.raises(ValueError, match="regions 0 and 1 overlap"):
        columns.compose_columns_host(page, lines, COL_BOXES, COL_CUTS, scale, feather)
    got = columns.compose_columns_host(page, lines, COL_BOXES, COL_CUTS, scale, feather, overlap="order")
    assert np.array_equal(got, _column_sequence(page, lines, widths, (0, 1, 2), scale, feather))
    back = columns.compose_columns_host(page, lines[::-1], COL_BOXES[::-1], COL_CUTS[::-1], scale, feather, overlap="order")
    assert np.array_equal(back, _column_sequence(page, lines, widths, (2, 1, 0), scale, feather))
    assert not np.array_equal(got, back)
    # disjoint: the column and a line beside it give the bytes of "refuse"
    boxes, cuts = (COL_BOXES[0], [70, 20, 140, 44]), (COL_CUTS[0], None)
    a = columns.compose_columns_host(page, lines[:2], boxes, cuts, scale, feather)
    assert np.array_equal(columns.compose_columns_host(page, lines[:2], boxes, cuts, scale, feather, overlap="order"), a)
    # the column's own refusals stand
    with pytest.raises(ValueError, match="do not run from"):
        columns.compose_columns_host(page, lines, COL_BOXES, ([5, 20, 44, 64], None, None), scale, feather, overlap="order")


def test_a_bad_overlap_value_is_a_value_error():
    page, lines = _scene(DISJOINT)
    for bad in ("painter", "", None, True, "ORDER"):
        with pytest.raises(ValueError, match="overlap must be"):
            pages.region_rects(PAGE_H, PAGE_W, DISJOINT, [True] * 4, 1, 3, overlap=bad)
        with pytest.raises(ValueError, match="overlap must be"):
            pages.compose_host(page, lines, DISJOINT, 1, 3, overlap=bad)
        with pytest.raises(ValueError, match="overlap must be"):
            pages.compose_page(page, None, [None] * 4, DISJOINT, 1, 3, device="cpu", overlap=bad)
        with pytest.raises(ValueError, match="overlap must be"):
            columns.check_columns(PAGE_H, PAGE_W, DISJOINT, [True] * 4, [None] * 4, 1, 3, overlap=bad)
        with pytest.raises(ValueError, match="overlap must be"):
            columns.compose_columns_host(page, lines, DISJOINT, [None] * 4, 1, 3, overlap=bad)
    assert pages.region_rects(PAGE_H, PAGE_W, STACK, [True] * 4, 2, 3, overlap="order") == [_rect(b, 2) for b in STACK]
    assert columns.check_columns(PAGE_H, PAGE_W, COL_BOXES, [True] * 3, COL_CUTS, 1, 3, 32, overlap="order") == [_rect(b, 1) for b in COL_BOXES]


def test_entry_points_take_the_mode_and_refuse_before_anything_runs():
    """the pipeline's host checks need neither weights on a device nor a launch"""
    from marconet_amd import networks
    from marconet_amd.pipeline import MarconetPipeline
    pipe = MarconetPipeline(networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet())
    page = np.zeros((60, 200, 3), np.uint8)
    a = lq_io.alphabet()[10]
    over = [[0, 0, 100, 30], [99, 29, 150, 50]]
    with pytest.raises(ValueError, match="restore_page: regions 0 and 1 overlap"):
        pipe.restore_page(page, over, [a, a], overlap="refuse")
    with pytest.raises(ValueError, match="restore_page_columns: regions 0 and 1 overlap"):
        pipe.restore_page_columns(page, over, [a, a], vertical=[False, True], overlap="refuse")
    with pytest.raises(ValueError, match="restore_page: overlap must be"):
        pipe.restore_page(page, over, [a, a], overlap="blend")
    with pytest.raises(ValueError, match="restore_page_columns: overlap must be"):
        pipe.restore_page_columns(page, over, [a, a], overlap="blend")
    with pytest.raises(ValueError, match="restore_page: region 1: .*empty or lies outside"):      # the other refusals stand
        pipe.restore_page(page, [over[0], [300, 10, 350, 50]], [a, a], overlap="order")
    with pytest.raises(ValueError, match="restore_page_columns: region 0: character \\d+: its cell is empty"):
        pipe.restore_page_columns(page, over, [a * 40, a], vertical=[True, False], overlap="order")


# ----------------------------------------------------------------------------------------------------------------------- the binning
def _cells(rects):
    return pages.as_cell(pages.build_table(rects, [40] * len(rects), 3, 16))


def _brute(rects, page_h, page_w):
    """per tile, row-major, the ascending indices of the rectangles that share a pixel with it"""
    out = []
    for ty in range(-(-page_h // 16)):
        for tx in range(-(-page_w // 64)):
            X0, Y0, X1, Y1 = 64 * tx, 16 * ty, min(64 * tx + 64, page_w), min(16 * ty + 16, page_h)
            out.append([c for c, (x0, y0, rw, rh) in enumerate(rects) if x0 < X1 and X0 < x0 + rw and y0 < Y1 and Y0 < y0 + rh])
    return out


# rectangles of the 150 x 70 page: tile columns 64 | 64 | 22, tile rows 16 x 4 + 6
BIN_RECTS = (
    (10, 5, 100, 40),            # over 63|64 and 15|16: tiles of two columns, three rows
    (0, 0, 64, 16),              # exactly tile 0: ends ON both edges, must not leak into tiles 1 and 3
    (64, 16, 64, 16),            # exactly the tile (1, 1)
    (63, 15, 2, 2),              # one pixel in each of four tiles
    (128, 64, 22, 6),            # the ragged last tile, exactly
    (140, 0, 10, 70),            # the last tile column, every tile row
    (10, 5, 100, 40),            # the first rectangle again: listed after it in every tile
    (20, 33, 1, 1),              # one pixel
    (0, 48, 128, 16),            # a full tile row but the ragged column
)


def test_bin_tiles_equals_a_loop_over_the_tiles():
    spans, order = pages.bin_tiles(_cells(BIN_RECTS), PAGE_H, PAGE_W)
    want = _brute(BIN_RECTS, PAGE_H, PAGE_W)
    assert spans.dtype == np.dtype(_lib.TileSpan) and spans.shape == (15,) and order.dtype == np.int32 and order.flags["C_CONTIGUOUS"]
    got = [order[int(s["first"]):int(s["first"]) + int(s["count"])].tolist() for s in spans]
    assert got == want
    assert all(l == sorted(l) for l in got)
    assert got[0] == [0, 1, 3, 6] and got[1] == [0, 3, 6] and got[3] == [0, 3, 6] and got[4] == [0, 2, 3, 6]       # (0, 0, 64, 16) only in tile 0
    assert got[14] == [4, 5] and got[12] == [] and spans["count"][12] == 0
    # the spans partition the order: first is the exclusive prefix sum of count
    assert spans["first"].tolist() == (np.cumsum(spans["count"]) - spans["count"]).tolist()
    assert int(spans["count"].sum()) == len(order) == sum(len(l) for l in want)
    # no cells: every tile is empty
    spans0, order0 = pages.bin_tiles(_cells(BIN_RECTS)[:0], PAGE_H, PAGE_W)
    assert spans0["count"].tolist() == [0] * 15 and spans0["first"].tolist() == [0] * 15 and len(order0) == 0
    # a rectangle that pokes out of the page is clipped to it; an empty one touches nothing
    cells = _cells(((1, 1, 1, 1),) * 3)
    for name, values in zip(("x0", "y0", "rw", "rh"), zip((140, 60, 40, 40), (10, 10, 0, 5), (-5, -5, 10, 10))):
        cells[name] = values
    spans1, order1 = pages.bin_tiles(cells, PAGE_H, PAGE_W)
    assert [order1[int(s["first"]):int(s["first"]) + int(s["count"])].tolist() for s in spans1] == [[2]] + [[]] * 10 + [[0]] + [[]] * 2 + [[0]]


def test_bin_tiles_on_other_pages_and_random_cells():
    rng = np.random.default_rng(4)
    for page_h, page_w in ((16, 64), (17, 65), (1, 1), (96, 200)):
        rects = []
        for _ in range(25):
            x0, y0 = int(rng.integers(0, page_w)), int(rng.integers(0, page_h))
            rects.append((x0, y0, int(rng.integers(1, page_w - x0 + 1)), int(rng.integers(1, page_h - y0 + 1))))
        spans, order = pages.bin_tiles(_cells(rects), page_h, page_w)
        assert [order[int(s["first"]):int(s["first"]) + int(s["count"])].tolist() for s in spans] == _brute(rects, page_h, page_w)


def test_bin_tiles_refuses_what_int32_cannot_hold():
    cells = _cells(((0, 0, 10, 10),))
    with pytest.raises(ValueError, match="tiles, more than 2147483647"):
        pages.bin_tiles(cells, 16 * 65536, 64 * 32768)                                  # 2^31 tiles
    with pytest.raises(ValueError, match="an order longer than 2147483647"):
        big = _cells(((0, 0, 64 * 32768, 16 * 32768),) * 3)                             # 2^30 tiles each: the page's tiles fit, three times them do not
        pages.bin_tiles(big, 16 * 32768, 64 * 32768)
    with pytest.raises(ValueError, match="empty page"):
        pages.bin_tiles(cells, 0, 10)


def test_as_cell_is_the_device_s_as_cell():
    reg = pages.build_table([(3, 5, 70, 70), (100, 10, 64, 30)], [75, 73], 5, 128, line_index=[1, 0])
    cells = pages.as_cell(reg)
    assert cells.dtype == np.dtype(_lib.ColumnPaste) and len(cells) == 2
    for r, c in zip(reg, cells):
        assert tuple(c) == (int(r["line_index"]), 0, int(r["src_w"]), int(r["x0"]), int(r["y0"]), int(r["rw"]), int(r["rh"]), 5, int(r["k"]),
                            int(r["x0"]), int(r["y0"]), int(r["rw"]), int(r["rh"]), 0, float(r["scale_x"]), float(r["scale_y"]))
    src = open(os.path.join(CSRC, "page_kernels.hip")).read()
    assert "return {R.line_index, 0, R.src_w, R.x0, R.y0, R.rw, R.rh, R.feather, R.k, R.x0, R.y0, R.rw, R.rh, 0, R.scale_x, R.scale_y};" in src
    with pytest.raises(TypeError):
        pages.as_cell(cells)


def test_mixed_table_holds_lines_and_cells_in_region_order():
    widths = columns.cell_widths(COL_BOXES[0], COL_CUTS[0])
    joined = torch.zeros((3, 128, 4 * sum(widths) + 400, 3), dtype=torch.uint8)
    col = (COL_BOXES[0], COL_CUTS[0], widths, None)
    rects = [_rect(b, 2) for b in COL_BOXES]
    tab = columns.mixed_table(joined, [(2, rects[1], 333), (0, rects[0], col), (1, rects[2], 77)], 6)
    assert tab.dtype == np.dtype(_lib.ColumnPaste) and len(tab) == 5
    assert np.array_equal(tab[:1], pages.as_cell(pages.build_table([rects[1]], [333], 6, 128, [2])))
    assert np.array_equal(tab[1:4], columns.paste_table([col], [0], [rects[0]], 6, 128))
    assert np.array_equal(tab[4:], pages.as_cell(pages.build_table([rects[2]], [77], 6, 128, [1])))
    assert len(columns.mixed_table(joined, [], 6)) == 0
    with pytest.raises(ValueError, match="does not lie inside the lines"):
        columns.mixed_table(joined, [(3, rects[0], col)], 6)


# ---------------------------------------------------------------------------------------------------------------------------- the ABI
def test_ordered_header_declares_exactly_the_bound_symbols_and_compiles_as_c99(tmp_path):
    text = open(os.path.join(INCLUDE, "marconet_hip_ordered.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(mnet_\w+)\s*\(", code)) == set(_lib.ORDERED_SYMBOLS) == {"mnet_paste_ordered_u8"}
    assert len(_lib.ORDERED_SYMBOLS["mnet_paste_ordered_u8"][1]) == 14
    cpath, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    with open(cpath, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "marconet_hip_ordered.h"\nint main(void) {\n'
                'int (*p)(const uint8_t*, int32_t, int32_t, int32_t, const mnet_column_paste*, int32_t, const mnet_tile_span*, int32_t, const int32_t*, '
                'int32_t, uint8_t*, int32_t, int32_t, void*) = mnet_paste_ordered_u8;\n(void)p;\n'
                'printf("%d %d %d %d %d\\n", (int)sizeof(mnet_tile_span), (int)offsetof(mnet_tile_span, first), (int)offsetof(mnet_tile_span, count), '
                '(int)sizeof(mnet_column_paste), MNET_ABI_VERSION);\nreturn 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, cpath])
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, cpath, "-o", exe, "-Wl,--unresolved-symbols=ignore-all"])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    S = _lib.TileSpan
    assert got == [ctypes.sizeof(S), S.first.offset, S.count.offset, ctypes.sizeof(_lib.ColumnPaste), _lib.ABI_VERSION] == [8, 0, 4, 72, 4]
    assert np.dtype(S).itemsize == 8 and [n for n, _ in S._fields_] == ["first", "count"] and ctypes.alignment(S) == 4


def test_the_library_exports_the_symbol_and_the_other_sets_are_unchanged():
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in _lib.ORDERED_SYMBOLS)
    assert len(_lib.SYMBOLS) == 45 and "mnet_paste_u8" in _lib.SYMBOLS and _lib.ABI_VERSION == 4 and lib.mnet_abi_version() == 4
    assert set(_lib.UPFOLD_SYMBOLS) == {"mnet_upfold3x3_nhwc"} and set(_lib.UPFOLD_F32Z_SYMBOLS) == {"mnet_upfold3x3_f32z_nhwc"}
    assert set(_lib.QUAD_SYMBOLS) == {"mnet_quad_crop_u8", "mnet_quad_paste_u8"}
    assert set(_lib.COLUMN_SYMBOLS) == {"mnet_column_gather_u8", "mnet_column_paste_u8"}
    assert set(_lib.CURVE_SYMBOLS) == {"mnet_curve_crop_u8", "mnet_curve_paste_u8"}
    others = set(_lib.SYMBOLS) | set(_lib.UPFOLD_SYMBOLS) | set(_lib.UPFOLD_F32Z_SYMBOLS) | set(_lib.QUAD_SYMBOLS) | set(_lib.COLUMN_SYMBOLS) | set(_lib.CURVE_SYMBOLS)
    assert not set(_lib.ORDERED_SYMBOLS) & others
    assert _lib.ORDERED_SYMBOLS["mnet_paste_ordered_u8"][1][:6] == _lib.COLUMN_SYMBOLS["mnet_column_paste_u8"][1][:6]


def test_entry_point_validates_arguments_without_device():
    lib = _lib.load()
    ok = dict(lines=16, n_lines=2, rows=128, line_w=300, cells=16, n_cells=3, spans=32, n_spans=15, order=64, n_order=7, page=16, page_h=70, page_w=150)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mnet_paste_ordered_u8(a["lines"], a["n_lines"], a["rows"], a["line_w"], a["cells"], a["n_cells"], a["spans"], a["n_spans"], a["order"],
                                         a["n_order"], a["page"], a["page_h"], a["page_w"], None)

    for bad in ("lines", "cells", "spans", "order", "page"):
        assert call(**{bad: None}) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(n_lines=0), dict(rows=0), dict(line_w=-5), dict(n_cells=0), dict(n_cells=-1), dict(n_order=0), dict(n_order=-3), dict(page_h=0),
                dict(page_w=-7)):
        assert call(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    for bad in (14, 16, 0, -1, 3, 5):                                                   # the page has 3 x 5 tiles
        assert call(n_spans=bad) == -1 and b"spans for a page of 15 tiles" in lib.mnet_last_error()
    for bad in (dict(page_h=81), dict(page_h=64), dict(page_w=193), dict(page_w=128)):  # 18, 12, 20 and 10 tiles
        assert call(**bad) == -1 and b"15 spans for a page of" in lib.mnet_last_error()
    assert call(page_h=16 * 65536, page_w=64 * 32768, n_spans=2 ** 31 - 1) == -1 and b"too large" in lib.mnet_last_error()
    # 2^24 tiles of 256 threads are 2^32 threads: a launch that would run only a part of its workgroups is refused
    assert call(page_h=16 * 4096, page_w=64 * 4096, n_spans=2 ** 24) == -1 and b"too large" in lib.mnet_last_error()
    for bad in (dict(cells=20), dict(cells=17)):
        assert call(**bad) == -2 and b"8-byte aligned" in lib.mnet_last_error()
    for bad in (dict(spans=34), dict(spans=33), dict(order=66), dict(order=65)):
        assert call(**bad) == -2 and b"4-byte aligned" in lib.mnet_last_error()


def test_ops_refuses_cpu_tensors_and_bad_tables():
    from marconet_amd import ops
    lines = torch.zeros((2, 128, 300, 3), dtype=torch.uint8)
    page = torch.zeros((70, 150, 3), dtype=torch.uint8)
    cells, spans, order = torch.zeros((1, 72), dtype=torch.uint8), torch.zeros((15, 8), dtype=torch.uint8), torch.zeros((4,), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.paste_ordered_u8(lines, cells, spans, order, page)
    assert ops.page_tiles(70, 150) == (3, 5) and ops.page_tiles(64, 64) == (1, 4) and ops.page_tiles(65, 65) == (2, 5)


# ---------------------------------------------------------------------------------------------------------------------- the build
def test_build_script_stamps_the_header_and_the_kernel_shares_the_paste_body():
    sh = open(os.path.join(CSRC, "build.sh")).read()
    assert ('[ "$1" = page_kernels ] && cat "$HERE/lq_taps.h" "$HERE/page_blend.h" "$HERE/page_tile.h" "$HERE/../../include/marconet_hip_columns.h" '
            '"$HERE/cell_paste.h"') in sh
    src, body = open(os.path.join(CSRC, "page_kernels.hip")).read(), open(os.path.join(CSRC, "cell_paste.h")).read()
    # the ordered compositor is an instantiation of the page-tile compositor, in mixed_kernels.hip (tests/test_regions.py)
    assert '#include "cell_paste.h"' in src and "marconet_hip_ordered.h" not in src and "mnet_paste_ordered_u8" not in src
    # one box average, one cubic gather, one blend: stated once, in cell_paste.h, called by paste_cell (the two per-descriptor kernels) and by the compositor
    assert body.count("page_box_avg(") == 1 and body.count("page_feather(") == 1 and body.count("pt_round_clip(") == 1
    assert "page_box_avg(" not in src and "page_feather(" not in src and "pt_round_clip(" not in src
    assert src.count("cell_foreground(") == 1 and src.count("cell_blend(") == 1 and src.count("cell_followed(") == 1
    assert body.count("cell_foreground(") == 1 and body.count("cell_blend(") == 1 and body.count("cell_followed(") == 1       # their definitions
    assert src.count("__shared__ PtTaps s;") == 2 and "__shared__" not in src.replace("__shared__ PtTaps s;", "")     # the kernels' LDS is one PtTaps
    assert "__shared__" not in body and "asm" not in src and "asm" not in body


# -------------------------------------------------------------------------------------------------------------------- the example
def test_example_script_refuses_order_for_quadrilaterals_and_polygons(tmp_path):
    """--overlap order with a "quad" or a "polygon" in the file: the script exits with a message before it looks for a GPU"""
    line = dict(box=[40, 5, 90, 25], text="cd")
    for other in (dict(quad=[[40, 40], [90, 42], [89, 60], [39, 58]], text="ef"),
                  dict(polygon=[[10, 70], [40, 64], [70, 70], [68, 88], [40, 82], [12, 88]], text="gh")):
        path = str(tmp_path / "regions.json")
        with open(path, "w", encoding="utf8") as f:
            json.dump([line, other], f)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "restore_page.py"), "-i", "none.png", "-r", path, "-o", str(tmp_path / "o.png"),
                            "--overlap", "order"], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "still refuse overlaps" in r.stderr and "--overlap order applies to" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "restore_page.py"), "-i", "none.png", "-r", path, "-o", "o.png", "--overlap", "blend"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "invalid choice" in r.stderr
