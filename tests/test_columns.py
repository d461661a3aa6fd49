"""not-gpu: the host side of the vertical-column page path (marconet_amd/columns.py, mnet_column_gather_u8, mnet_column_paste_u8) — the cuts, the
virtual strip, the one-ramp paste, the refusals, the tables against the C layout of the two descriptors, the entry points' argument checks (the library
loads without a GPU) and the build script's lines.  Every comparison of pixels is np.array_equal."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from marconet_amd import _lib, columns, long_lines, lq_io, pages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marconet_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")


# ------------------------------------------------------------------------------------------------------------------------------- cuts
@pytest.mark.parametrize("y1,ch,n", [(5, 37, 1), (5, 37, 37), (0, 37, 5), (11, 100, 7), (3, 64, 64), (0, 9, 2)])
def test_evenly_spaced_cuts_tile_the_column(y1, ch, n):
    cuts = columns.cell_cuts([4, y1, 20, y1 + ch], n)
    assert len(cuts) == n + 1 and cuts[0] == y1 and cuts[-1] == y1 + ch
    assert all(b > a for a, b in zip(cuts, cuts[1:]))
    assert cuts == [y1 + (2 * j * ch + n) // (2 * n) for j in range(n + 1)]
    h = np.diff(cuts)
    assert h.sum() == ch and h.max() - h.min() <= 1                                             # j ch / n rounded half up: the cells differ by a row at most


def test_character_box_cuts_follow_plan_windows_rule():
    box = [10, 20, 40, 120]
    cb = [[12, 22.7, 38, 49.9], [11, 55.2, 39, 80.0], [12, 80.0, 37, 97.5], [12, 101, 38, 118]]
    cuts = columns.cell_cuts(box, 4, cb)
    assert cuts == [20, (49 + 55) // 2, (80 + 80) // 2, (97 + 101) // 2, 120]
    # the same boxes turned by 90 degrees are a line's: plan_windows cuts it at the same places (windows of two characters that share one)
    line = [[b[1] - 20, 0, b[3] - 20, 30] for b in cb]
    plan = long_lines.plan_windows(30, 100, line, max_glyphs=2, overlap_glyphs=1)
    assert [(p.g0, p.g1) for p in plan] == [(0, 2), (1, 3), (2, 4)]
    assert [p.c0 for p in plan] + [p.c1 for p in plan[1:]] == [c - 20 for c in cuts]
    # a cut beyond the column is clamped into it — and then names an empty cell, as a cut at the column's end must
    with pytest.raises(ValueError, match="character 2: its cell is empty"):
        columns.cell_cuts(box, 3, [[0, 20, 1, 40], [0, 50, 1, 130], [0, 140, 1, 400]])


def test_cut_refusals_name_the_region_and_the_character():
    box = [10, 20, 40, 120]
    with pytest.raises(ValueError, match="region 3: a column without a character"):
        columns.cell_cuts(box, 0, region=3)
    with pytest.raises(ValueError, match="region 2: 3 character boxes for 2 characters"):
        columns.cell_cuts(box, 2, [[0, 0, 1, 1]] * 3, region=2)
    with pytest.raises(ValueError, match="region 1: character 0: its cell is empty"):                 # both boxes above the column: the cut clamps to y1
        columns.cell_cuts(box, 2, [[0, 0, 1, 5], [0, 6, 1, 10]], region=1)
    with pytest.raises(ValueError, match="region 0: character 1: its cell is empty"):                 # the boxes out of order
        columns.cell_cuts(box, 3, [[0, 20, 1, 60], [0, 100, 1, 110], [0, 30, 1, 40]], region=0)
    with pytest.raises(ValueError, match="region 4: character 0: its cell is empty"):                 # more characters than rows
        columns.cell_cuts([0, 0, 10, 5], 12, region=4)


def test_check_columns_refusals_name_the_region():
    boxes = [[10, 20, 40, 120], [50, 10, 150, 40]]
    cuts = [columns.cell_cuts(boxes[0], 4), None]

    def refused(match, boxes_=boxes, cuts_=cuts, restored=(True, True), scale=2, feather=3):
        with pytest.raises(ValueError, match=match):
            columns.check_columns(130, 160, boxes_, list(restored), cuts_, scale, feather)

    assert columns.check_columns(130, 160, boxes, [True, True], cuts, 2, 3) == [(20, 40, 60, 200), (100, 20, 200, 60)]
    refused("region 1: .*empty or lies outside", [boxes[0], [50, 10, 170, 40]])                     # pages.region_rects' own refusals
    refused("region 0: an integer box", [[10.5, 20, 40, 120], boxes[1]])
    refused("regions 0 and 1 overlap", [boxes[0], [30, 10, 150, 40]])                                # across both kinds of region
    refused("scale", scale=9)
    refused("feather", feather=1025)
    refused("one line", restored=(True,))
    refused("one list of cuts", cuts_=cuts[:1])
    refused("region 0: its cuts .* do not run from y1 = 20 to y2 = 120", cuts_=[[20, 50, 119], None])
    refused("region 0: its cuts .* do not run from y1 = 20 to y2 = 120", cuts_=[[20], None])
    refused("region 0: character 1: its cell is empty", cuts_=[[20, 50, 50, 120], None])
    refused("region 0: character 2: its cell is empty", cuts_=[[20, 50, 70, 60, 120], None])
    refused("region 0: character 1: its cell is 6 rows high at scale 2, under the 8", cuts_=[[20, 50, 53, 120], None])
    columns.check_columns(130, 160, boxes, [True, True], [[20, 50, 54, 120], None], 2, 3)             # 8 rows: accepted
    columns.check_columns(130, 160, boxes, [False, True], [[20, 50, 53, 120], None], 2, 3)            # not restored: only its box is checked


def test_entry_point_refuses_before_anything_runs():
    """the host checks of restore_page_columns need neither weights on a device nor a launch"""
    from marconet_amd import networks
    from marconet_amd.pipeline import MarconetPipeline
    pipe = MarconetPipeline(networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet())
    page = np.zeros((200, 260, 3), np.uint8)
    a = lq_io.alphabet()[10]
    col = [10, 20, 40, 120]
    with pytest.raises(ValueError, match="needs texts"):
        pipe.restore_page_columns(page, [col], None)
    with pytest.raises(ValueError, match="one text"):
        pipe.restore_page_columns(page, [col], [a, a])
    with pytest.raises(ValueError, match="one text"):
        pipe.restore_page_columns(page, [col], [a], vertical=[True, False])
    with pytest.raises(ValueError, match="restore_page_columns: regions 0 and 1 overlap"):           # a column and a line
        pipe.restore_page_columns(page, [col, [30, 100, 200, 130]], [a * 3, a * 4], vertical=[True, False])
    with pytest.raises(ValueError, match="restore_page_columns: region 1: .*empty or lies outside"):
        pipe.restore_page_columns(page, [col, [300, 10, 350, 50]], [a, a])
    with pytest.raises(ValueError, match="restore_page_columns: region 0: 2 character boxes for 3 characters"):
        pipe.restore_page_columns(page, [col], [a * 3], char_boxes=[[[10, 20, 40, 60], [10, 60, 40, 120]]])
    with pytest.raises(ValueError, match="restore_page_columns: region 1: character 0: its cell is empty"):
        pipe.restore_page_columns(page, [[100, 0, 130, 50], col], [a, a * 2], char_boxes=[None, [[10, 0, 40, 5], [10, 6, 40, 10]]])
    with pytest.raises(ValueError, match="restore_page_columns: region 0: character 0: its cell is 6 rows high at scale 1, under the 8"):
        pipe.restore_page_columns(page, [[10, 20, 40, 44]], [a * 4], scale=1)
    with pytest.raises(ValueError, match="restore_page_columns: region 0: .*character 0 does not fit a window"):      # 200 x 8 cells: 800 px at height 32
        pipe.restore_page_columns(page, [[10, 20, 210, 36]], [a * 2], scale=2)
    with pytest.raises(ValueError, match="scale"):
        pipe.restore_page_columns(page, [col], [a], scale=9)
    with pytest.raises(ValueError, match="feather"):
        pipe.restore_page_columns(page, [col], [a], feather=2000)
    with pytest.raises(TypeError):
        pipe.restore_page_columns(page.astype(np.float32), [col], [a])


# ------------------------------------------------------------------------------------------------------------------ the virtual strip
def test_virtual_strip_is_the_hstack_of_the_cells_resized_on_their_own():
    page = np.random.default_rng(1).integers(0, 256, (90, 60, 3), dtype=np.uint8)
    box = [7, 3, 40, 88]
    cuts = columns.cell_cuts(box, 4, [[7, 3, 40, 20], [7, 22, 40, 70], [7, 70, 40, 75], [7, 76, 40, 88]])
    V, widths = columns.virtual_strip(page, box, cuts)
    assert widths == [max(1, int(np.rint(33 * 32 / (b - a)))) for a, b in zip(cuts, cuts[1:])] == columns.cell_widths(box, cuts)
    assert V.dtype == np.uint8 and V.shape == (32, sum(widths), 3)
    o = columns.cell_offsets(widths)
    assert columns.virtual_boxes(widths) == [[o[j], 0, o[j + 1], 32] for j in range(4)] and o[-1] == sum(widths)
    for j in range(4):
        assert np.array_equal(V[:, o[j]:o[j + 1]], pages.resize_cubic_to(page[cuts[j]:cuts[j + 1], 7:40], widths[j], 32))
    # the taps clamp at the cell's border: a cell's columns do not change with the rows of the page beyond it
    other = page.copy()
    other[:cuts[1]] = 255 - other[:cuts[1]]
    other[cuts[2]:] = 255 - other[cuts[2]:]
    assert np.array_equal(columns.virtual_strip(other, box, cuts)[0][:, o[1]:o[2]], V[:, o[1]:o[2]])
    assert columns.cell_widths([0, 0, 1, 400], [0, 400]) == [1]                                    # at least one column


def test_a_column_of_32_x_32_cells_reaches_the_encoder_unchanged():
    rng = np.random.default_rng(2)
    page = rng.integers(0, 256, (200, 50, 3), dtype=np.uint8)
    box = [9, 4, 41, 4 + 5 * 32]
    cuts = columns.cell_cuts(box, 5)
    V, widths = columns.virtual_strip(page, box, cuts)
    assert widths == [32] * 5
    assert np.array_equal(V, np.hstack([page[4 + 32 * j:36 + 32 * j, 9:41] for j in range(5)]))
    assert np.array_equal(lq_io.resize_cubic(V, 1, 1), V)                                          # lq_device's height-32 resize of a height-32 crop: the identity
    assert lq_io.lq_from_image(V)[1:] == (160, 640)
    # at scale 4 a cell's foreground is its 128 x 128 slice of the line, channel-flipped — wherever it stands
    line = rng.integers(0, 256, (128, 640, 3), dtype=np.uint8)
    fg = columns.column_foreground(line, (36, 16, 128, 640), cuts, widths)
    for j in range(5):
        assert np.array_equal(fg[128 * j:128 * (j + 1)], line[:, 128 * j:128 * (j + 1), ::-1])
    # the layout identity: the same cells laid out as a row, restored to the same (fake) line, give the same 128 x 128 blocks
    row_page = np.zeros((40, 200, 3), np.uint8)
    row_page[3:35, 20:180] = V
    row_up = pages.compose_host(row_page, [line], [[20, 3, 180, 35]], 4, 0)
    col_up = columns.compose_columns_host(page, [line], [box], [cuts], 4, 0)
    for j in range(5):
        assert np.array_equal(col_up[4 * (4 + 32 * j):4 * (36 + 32 * j), 36:164], row_up[12:140, 80 + 128 * j:80 + 128 * (j + 1)])


def test_every_window_cut_of_a_long_column_falls_on_a_cell_boundary():
    box = [3, 1, 30, 1 + 1111]
    cuts = columns.cell_cuts(box, 40)
    widths = columns.cell_widths(box, cuts)
    Wv, o = sum(widths), columns.cell_offsets(widths)
    for max_glyphs, overlap in ((16, 2), (7, 3), (2, 1)):
        plan = long_lines.plan_windows(32, Wv, columns.virtual_boxes(widths), max_glyphs, overlap)
        assert len(plan) > 2 and all(p.c0 == o[p.g0] and p.c1 == o[p.g1] for p in plan)
        assert all(p.offset == 4 * p.c0 and p.show_w == 4 * (p.c1 - p.c0) for p in plan)
        assert long_lines.plan_out_w(plan) == 4 * Wv
        tab, shapes, offsets, nbytes = columns.gather_table([(box, cuts, widths, plan)], base=7)
        assert len(tab) == sum(p.g1 - p.g0 for p in plan) and shapes == [(32, p.c1 - p.c0) for p in plan]
        assert offsets[0] == 7 and nbytes == 7 + sum(3 * 32 * w for _, w in shapes)
    with pytest.raises(ValueError, match="not its cells"):
        columns.gather_table([(box, cuts, widths, [plan[0]._replace(c1=plan[0].c1 + 1)])])


# --------------------------------------------------------------------------------------------------------------------------- the paste
def test_a_column_of_one_cell_is_paste_host_of_the_whole_line():
    rng = np.random.default_rng(3)
    up = rng.integers(0, 256, (120, 90, 3), dtype=np.uint8)
    for (cw, ch, s, F) in ((20, 25, 2, 3), (9, 40, 1, 0), (5, 4, 4, 30)):
        cuts = [6, 6 + ch]
        widths = columns.cell_widths([2, 6, 2 + cw, 6 + ch], cuts)
        line = rng.integers(0, 256, (128, 4 * widths[0], 3), dtype=np.uint8)
        rect = (s * 2, s * 6, s * cw, s * ch)
        assert np.array_equal(columns.paste_column_host(up.copy(), line, rect, cuts, widths, F), pages.paste_host(up.copy(), line, rect, F))


def test_one_ramp_follows_the_columns_outer_edge_and_none_runs_between_cells():
    rng = np.random.default_rng(4)
    up = rng.integers(0, 64, (130, 70, 3), dtype=np.uint8)                                         # a dark page under a bright line: the ramp shows
    box, cuts, s, F = [5, 3, 25, 59], [3, 30, 59], 2, 6
    widths = columns.cell_widths(box, cuts)
    o = columns.cell_offsets(widths)
    line = rng.integers(192, 256, (128, 4 * o[-1], 3), dtype=np.uint8)
    rect = (10, 6, 40, 112)
    got = columns.paste_column_host(up.copy(), line, rect, cuts, widths, F)
    fgs = [pages.line_to_rect(line[:, 4 * o[j]:4 * o[j + 1]], 40, 2 * (cuts[j + 1] - cuts[j])) for j in range(2)]
    assert [f.shape for f in fgs] == [(54, 40, 3), (58, 40, 3)]
    want = up.copy()
    want[6:118, 10:50] = pages.feather_blend(up[6:118, 10:50], np.vstack(fgs), F)                  # the one-ramp definition
    assert np.array_equal(got, want)
    per_cell = up.copy()
    pages.paste_host(per_cell, line[:, :4 * o[1]], (10, 6, 40, 54), F)
    pages.paste_host(per_cell, line[:, 4 * o[1]:], (10, 60, 40, 58), F)
    seam = slice(60 - F, 60 + F)
    assert not np.array_equal(got[seam, 10 + F:50 - F], per_cell[seam, 10 + F:50 - F])             # two ramps meet at the inner seam; one ramp has none there
    assert np.array_equal(got[seam, 10 + F:50 - F], np.vstack(fgs)[54 - F:54 + F, F:40 - F])         # F pixels inside the column the line's weight is exactly 1
    assert np.array_equal(got[6:6 + 54 - F], per_cell[6:6 + 54 - F]) and np.array_equal(got[60 + F:], per_cell[60 + F:])
    mask = np.ones(up.shape[:2], bool)
    mask[6:118, 10:50] = False
    assert np.array_equal(got[mask], up[mask])
    assert np.array_equal(columns.paste_column_host(up.copy(), line, rect, cuts, widths, 0)[6:118, 10:50], np.vstack(fgs))
    with pytest.raises(ValueError, match="outside"):
        columns.paste_column_host(up.copy(), line, (40, 6, 40, 112), cuts, widths, F)
    with pytest.raises(ValueError, match="no multiple"):
        columns.paste_column_host(up.copy(), line, (10, 6, 40, 111), cuts, widths, F)
    with pytest.raises(ValueError, match="a line of"):
        columns.paste_column_host(up.copy(), line[:, 1:], rect, cuts, widths, F)


def test_compose_columns_host_mixes_columns_and_lines():
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, (70, 100, 3), dtype=np.uint8)
    boxes = [[4, 2, 20, 66], [30, 10, 95, 30], [30, 40, 60, 60]]
    cuts = [columns.cell_cuts(boxes[0], 3), None, columns.cell_cuts(boxes[2], 1)]
    widths = columns.cell_widths(boxes[0], cuts[0])
    lines = [rng.integers(0, 256, (128, 4 * sum(widths), 3), dtype=np.uint8), rng.integers(0, 256, (128, 416, 3), dtype=np.uint8), None]
    got = columns.compose_columns_host(page, lines, boxes, cuts, 2, 5)
    want = lq_io.resize_cubic(page, 2, 2)
    columns.paste_column_host(want, lines[0], (8, 4, 32, 128), cuts[0], widths, 5)
    pages.paste_host(want, lines[1], (60, 20, 130, 40), 5)
    assert np.array_equal(got, want) and not np.array_equal(got, lq_io.resize_cubic(page, 2, 2))
    assert np.array_equal(columns.compose_columns_host(page, [None, lines[1], None], boxes, [None] * 3, 2, 5), pages.compose_host(page, [None, lines[1], None], boxes, 2, 5))


# ------------------------------------------------------------------------------------------------------------- the tables and the ABI
CELL_FIELDS = ("offset", "win_w", "dx", "dw", "sx", "sy", "sw", "sh", "reserved", "scale_x", "scale_y")
PASTE_FIELDS = ("line_index", "src_x0", "src_w", "x0", "y0", "rw", "rh", "feather", "k", "fx0", "fy0", "fw", "fh", "reserved", "scale_x", "scale_y")


def test_descriptor_layouts_match_c_and_the_tables_carry_the_definition(tmp_path):
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "marconet_hip_columns.h"\nint main(void){\n'
    for name, fields in (("mnet_column_cell", CELL_FIELDS), ("mnet_column_paste", PASTE_FIELDS)):
        code += 'printf("%%zu %%zu", sizeof(%s), _Alignof(%s));\n' % (name, name)
        code += "".join('printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f in fields) + 'printf("\\n");\n'
    code += "return 0; }\n"
    cpath, exe = str(tmp_path / "column_probe.c"), str(tmp_path / "column_probe")
    with open(cpath, "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-std=c11", "-I", INCLUDE, cpath, "-o", exe])
    got = [[int(v) for v in l.split()] for l in subprocess.check_output([exe]).decode().strip().split("\n")]
    for row, S, fields in ((got[0], _lib.ColumnCell, CELL_FIELDS), (got[1], _lib.ColumnPaste, PASTE_FIELDS)):
        assert row == [ctypes.sizeof(S), ctypes.alignment(S)] + [getattr(S, f).offset for f in fields]
        assert np.dtype(S).itemsize == row[0] and [n for n, _ in S._fields_] == list(fields)
    assert got[0][:2] == [56, 8] and got[1][:2] == [72, 8]
    # a column of three cells, 20 px wide, in two windows of two characters that share the middle one
    box, cuts = [4, 10, 24, 90], [10, 30, 70, 90]
    widths = columns.cell_widths(box, cuts)
    assert widths == [32, 16, 32]
    plan = long_lines.plan_windows(32, 80, columns.virtual_boxes(widths), max_glyphs=2, overlap_glyphs=1)
    assert [(p.c0, p.c1, p.g0, p.g1) for p in plan] == [(0, 48, 0, 2), (32, 80, 1, 3)]
    tab, shapes, offsets, nbytes = columns.gather_table([(box, cuts, widths, plan)], base=5)
    assert shapes == [(32, 48), (32, 48)] and offsets == [5, 5 + 3 * 32 * 48] and nbytes == 5 + 2 * 3 * 32 * 48
    assert [tuple(r)[:9] for r in tab] == [(5, 48, 0, 32, 4, 10, 20, 20, 0), (5, 48, 32, 16, 4, 30, 20, 40, 0),
                                            (4613, 48, 0, 16, 4, 30, 20, 40, 0), (4613, 48, 16, 32, 4, 70, 20, 20, 0)]
    assert tab["scale_x"].tolist() == [1.0 / (32 / 20), 1.0 / (16 / 20), 1.0 / (16 / 20), 1.0 / (32 / 20)]
    assert tab["scale_y"].tolist() == [1.0 / (32 / 20), 1.0 / (32 / 40), 1.0 / (32 / 40), 1.0 / (32 / 20)]
    empty = columns.gather_table([], base=11)
    assert len(empty[0]) == 0 and empty[1:] == ([], [], 11)
    # its paste at scale 1, feather 3: cells of 20 / 40 / 20 rows take k = 4 / 2 / 4; every cell's feather rectangle is the column's
    reg = columns.paste_table([(box, cuts, widths, plan)], [2], [(4, 10, 20, 80)], 3)
    assert [tuple(r)[:14] for r in reg] == [(2, 0, 128, 4, 10, 20, 20, 3, 4, 4, 10, 20, 80, 0), (2, 128, 64, 4, 30, 20, 40, 3, 2, 4, 10, 20, 80, 0),
                                            (2, 192, 128, 4, 70, 20, 20, 3, 4, 4, 10, 20, 80, 0)]
    assert reg["scale_x"].tolist() == [1.0 / (20 / 32), 1.0 / (20 / 32), 1.0 / (20 / 32)]
    assert reg["scale_y"].tolist() == [1.0 / (20 / 32), 1.0 / (40 / 64), 1.0 / (20 / 32)]
    assert [pages.box_factor(h) for h in (20, 40, 20)] == [4, 2, 4]


def test_columns_header_compiles_as_c99(tmp_path):
    cpath = str(tmp_path / "probe.c")
    with open(cpath, "w") as f:
        f.write('#include "marconet_hip_columns.h"\nint main(void) {\n'
                'int (*g)(const uint8_t*, int32_t, int32_t, const mnet_column_cell*, int32_t, int32_t, int32_t, uint8_t*, int64_t, void*) = mnet_column_gather_u8;\n'
                'int (*p)(const uint8_t*, int32_t, int32_t, int32_t, const mnet_column_paste*, int32_t, uint8_t*, int32_t, int32_t, void*) = mnet_column_paste_u8;\n'
                '(void)g; (void)p; return MNET_ABI_VERSION == 4 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, cpath])
    assert set(_lib.COLUMN_SYMBOLS) == {"mnet_column_gather_u8", "mnet_column_paste_u8"}
    assert not set(_lib.COLUMN_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.QUAD_SYMBOLS)) and _lib.ABI_VERSION == 4


def test_entry_points_validate_arguments_without_device():
    lib = _lib.load()
    ok = dict(page=16, page_h=70, page_w=150, cells=16, n=3, max_dw=100, dst_h=32, dst=16, dst_bytes=1 << 20)

    def gather(**kw):
        a = dict(ok, **kw)
        return lib.mnet_column_gather_u8(a["page"], a["page_h"], a["page_w"], a["cells"], a["n"], a["max_dw"], a["dst_h"], a["dst"], a["dst_bytes"], None)

    for bad in ("page", "cells", "dst"):
        assert gather(**{bad: None}) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(page_h=0), dict(page_w=-3), dict(n=0), dict(n=-1), dict(max_dw=0), dict(dst_h=0), dict(dst_h=-2), dict(dst_bytes=0), dict(dst_bytes=-5)):
        assert gather(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    assert gather(n=1 << 20, max_dw=1 << 20, dst_h=1 << 20) == -1 and b"too large" in lib.mnet_last_error()
    assert gather(n=1, max_dw=(1 << 31) - 1, dst_h=(1 << 31) - 1) == -1 and b"too large" in lib.mnet_last_error()
    for bad in (dict(cells=20), dict(cells=17), dict(cells=2)):
        assert gather(**bad) == -2 and b"aligned" in lib.mnet_last_error()

    okp = dict(lines=16, n_lines=2, rows=128, line_w=300, cells=16, n=2, page=16, page_h=280, page_w=600)

    def paste(**kw):
        a = dict(okp, **kw)
        return lib.mnet_column_paste_u8(a["lines"], a["n_lines"], a["rows"], a["line_w"], a["cells"], a["n"], a["page"], a["page_h"], a["page_w"], None)

    for bad in ("lines", "cells", "page"):
        assert paste(**{bad: None}) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(n_lines=0), dict(rows=0), dict(line_w=-1), dict(n=0), dict(n=-4), dict(page_h=0), dict(page_w=0)):
        assert paste(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    assert paste(n=1 << 20, page_h=1 << 20, page_w=1 << 20) == -1 and b"too large" in lib.mnet_last_error()
    for bad in (dict(cells=20), dict(cells=17)):
        assert paste(**bad) == -2 and b"aligned" in lib.mnet_last_error()


def test_ops_refuse_cpu_tensors_and_bad_tables():
    from marconet_amd import ops
    page = torch.zeros((80, 180, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.column_gather_u8(page, torch.zeros((1, 56), dtype=torch.uint8), 10, 32, torch.zeros((3000,), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.column_paste_u8(torch.zeros((1, 128, 64, 3), dtype=torch.uint8), torch.zeros((1, 72), dtype=torch.uint8), page.clone())
    joined = torch.zeros((1, 128, 100, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="column 0: line 0 of 128 columns does not lie inside"):
        columns.paste_columns(page, joined, [0], [([0, 0, 10, 10], [0, 10], [32], None)], [(0, 0, 10, 10)], 0)
    with pytest.raises(ValueError, match="column 0: line 1 of"):
        columns.paste_columns(page, joined, [1], [([0, 0, 10, 10], [0, 10], [16], None)], [(0, 0, 10, 10)], 0)
    assert columns.paste_columns(page, joined, [], [], [], 0) is page


# ----------------------------------------------------------------------------------------------------------------------- the build
def test_build_script_compiles_and_stamps_the_kernels():
    sh = open(os.path.join(CSRC, "build.sh")).read()
    assert re.search(r'^SRCS="[^"]*\bcolumn_kernels\b[^"]*"', sh, flags=re.M)
    assert 'column_kernels) echo "-ffp-contract=off" ;;' in sh
    assert '[ "$1" = column_kernels ] && cat "$HERE/lq_taps.h" "$HERE/page_tile.h" "$HERE/../../include/marconet_hip_columns.h"' in sh
    src = open(os.path.join(CSRC, "column_kernels.hip")).read()
    assert '#include "page_tile.h"' in src and "marconet_hip_columns.h" in src and src.count("pt_stage_taps(") == 1 and "mnet_column_gather_u8" in src
    # the paste stands beside its twin in page_kernels.hip, which is built and stamped with the taps, the blend, the tile and this header
    assert 'page_kernels) echo "-ffp-contract=off" ;;' in sh
    assert '[ "$1" = page_kernels ] && cat "$HERE/lq_taps.h" "$HERE/page_blend.h" "$HERE/page_tile.h" "$HERE/../../include/marconet_hip_columns.h"' in sh
    src = open(os.path.join(CSRC, "page_kernels.hip")).read()
    assert '#include "page_tile.h"' in src and '#include "page_blend.h"' in src and "marconet_hip_columns.h" in src and "mnet_column_paste_u8" in src
    tile = open(os.path.join(CSRC, "page_tile.h")).read()
    assert '#include "lq_taps.h"' in tile and tile.count("lq_cubic_taps(") == 2
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in _lib.COLUMN_SYMBOLS)


def test_device_build_of_the_column_kernels_is_not_contracted(tmp_path):
    """the gfx950 ISA of column_kernels.hip under build.sh's own flags holds no floating-point fused multiply-add at all (its divisions are
    integer); integer v_mad_u* / v_mad_i* do not count.  The tap arithmetic is there, unfused, in fp32 and fp64."""
    sh = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', sh, flags=re.M).group(1).split()
    extra = re.search(r'column_kernels\) echo "([^"]*)"', sh).group(1).split()
    assert "-ffp-contract=off" in extra
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = str(tmp_path / "column_kernels.s")
    subprocess.check_call([hipcc] + flags + extra + ["-S", "--cuda-device-only", os.path.join(CSRC, "column_kernels.hip"), "-o", asm], stderr=subprocess.DEVNULL)
    ops_ = re.findall(r"^\s+(v_[a-z0-9_]+)", open(asm).read(), flags=re.M)
    assert any(o.startswith("v_mul_f32") for o in ops_) and any(o.startswith("v_mul_f64") for o in ops_)
    fused = [o for o in ops_ if re.match(r"v_(pk_)?(fma|fmac|fmaak|fmamk|mad|mac)_", o) and not o.startswith("v_mad_u") and not o.startswith("v_mad_i")]
    assert fused == [], sorted(set(fused))


# ----------------------------------------------------------------------------------------------------------------------- the example
def test_example_script_reads_vertical_regions_and_refuses_them_beside_a_quad(tmp_path):
    """examples/restore_page.py's region file: "vertical": true beside a "box" gives one flag per region; combined with a "quad" anywhere in the file,
    or given without a "box", the script exits with a message before it looks for a GPU"""
    import importlib.util
    import json
    import sys
    spec = importlib.util.spec_from_file_location("restore_page_example", os.path.join(ROOT, "examples", "restore_page.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = str(tmp_path / "regions.json")

    def load(regions):
        with open(path, "w", encoding="utf8") as f:
            json.dump(regions, f)
        return mod.load_regions(path)

    col, line = dict(box=[5, 5, 30, 90], text="ab", vertical=True), dict(box=[40, 5, 90, 25], text="cd")
    quad = dict(quad=[[40, 40], [90, 42], [89, 60], [39, 58]], text="ef")
    assert load([col, line])[4] == [True, False] and load([col, line])[3] is None
    assert load([line, dict(line, vertical=False)])[4] is None                                      # no column: restore_page, as before
    assert load([line, quad])[4] is None and load([line, quad])[3] is not None
    with pytest.raises(SystemExit, match='holds a "vertical" region \\(0\\) and a "quad" region \\(2\\)'):
        load([col, line, quad])
    with pytest.raises(SystemExit, match='"vertical": true or false beside a "box" only'):
        load([dict(quad, vertical=True)])
    with pytest.raises(SystemExit, match="must hold a list"):
        load([dict(col, vertical="yes")])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "restore_page.py"), "-i", "none.png", "-r", load_path(path, [col, quad]), "-o", "none"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'holds a "vertical" region (0) and a "quad" region (1)' in r.stderr


def load_path(path, regions):
    import json
    with open(path, "w", encoding="utf8") as f:
        json.dump(regions, f)
    return path
