"""-m gpu: overlapping regions and column cells of a page pasted in the caller's order by ONE launch whose workgroups own page tiles
(mnet_paste_ordered_u8, pages.bin_tiles / paste_ordered / compose_page(overlap="order"), MarconetPipeline.restore_page and restore_page_columns
with overlap="order") against the pure-host definition — pages.paste_host and columns' paste applied one after another in list order — byte for
byte: every comparison is np.array_equal.  The host references are computed once per module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from marconet_amd import _lib, columns, lq_io, ops, pages
from tests.golden import cases_png
from tests.long_lines_cases import golden_line
from tests.test_pages_gpu import REGIONS as DISJOINT_REGIONS, _table as disjoint_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LINES, ROWS, LINE_W, PAGE_H, PAGE_W, GUARD = 5, 16, 96, 70, 150, 4096
TILES_X, TILES_Y = 3, 5

# The scene, in paste order: (name, line_index, src_w, (x0, y0, rw, rh), feather) for a line; a column carries its cells' (slice start, slice
# width, height) in the place of src_w.  k follows from a cell's height at rows = 16: 9.. → 1, 5..8 → 2, 3..4 → 4, 1..2 → 8.
SCENE = (
    ("the large one, over tile column 63|64 and tile row 15|16; k = 1", 3, 37, (10, 5, 100, 40), 3),
    ("wholly inside the large one", 0, 50, (30, 10, 40, 20), 2),
    ("over both: three deep in [50, 70) x [10, 16); k = 2; x0 and y0 no tile multiples", 1, 96, (50, 8, 30, 8), 1),
    ("one column wide, under the twins", 0, 5, (112, 20, 1, 16), 1),
    ("the first twin, feathered", 2, 33, (100, 30, 40, 16), 5),
    ("the second twin: the same rectangle with feather 0, so the first must vanish", 4, 30, (100, 30, 40, 16), 0),
    ("the page's corner (0, 0); k = 4", 0, 35, (0, 0, 9, 4), 1),
    ("over it at the corner; k = 8", 4, 90, (0, 0, 6, 2), 1),
    ("ending at the page's bottom right corner", 2, 33, (125, 58, 25, 12), 3),
    ("over it, ending at the same corner; k = 4", 3, 80, (130, 66, 20, 4), 1),
    ("one column wide, over the large one and the three-deep stack", 1, 7, (60, 2, 1, 30), 0),
    ("a feather wider than half the rectangle on both axes; k = 2", 1, 95, (0, 50, 60, 8), 40),
    ("over its right end and the large one's last rows", 2, 40, (40, 44, 40, 16), 2),
    ("a column of three cells of 10 / 18 / 8 rows: one ramp along the column's edge; over the large one", 1, ((0, 30, 10), (30, 40, 18), (70, 26, 8)), (84, 30, 12, 36), 4),
    ("a line over the column's second and third cell", 0, 61, (80, 50, 30, 9), 2),
)
IS_COLUMN = [isinstance(r[2], tuple) for r in SCENE]


def _cells_of(r):
    """the scene's region r as records of mnet_column_paste: a line as pages.as_cell states it, a column cell by cell"""
    _, li, src, (x0, y0, rw, rh), F = SCENE[r]
    if not IS_COLUMN[r]:
        return pages.as_cell(pages.build_table([(x0, y0, rw, rh)], [src], F, ROWS, [li]))
    tab, y = np.zeros((len(src),), dtype=np.dtype(_lib.ColumnPaste)), y0
    for j, (sx0, sw, ch) in enumerate(src):
        k = pages.box_factor(ch, ROWS)
        tab[j] = (li, sx0, sw, x0, y, rw, ch, F, k, x0, y0, rw, rh, 0, pages.axis_scale(rw, -(-sw // k)), pages.axis_scale(ch, ROWS // k))
        y += ch
    assert y == y0 + rh
    return tab


def _table(sel=None):
    sel = range(len(SCENE)) if sel is None else sel
    return np.concatenate([_cells_of(r) for r in sel])


def _paste_cell_host(page, lines, c):
    """one cell on the host: pages.paste_host where the feather rectangle is the cell's own; else the cell's foreground (pages.line_to_rect of its
    slice) under the weights of ITS part of the feather rectangle's ramp — pages.feather_blend's arithmetic, checked in the fixture against one
    pages.feather_blend over the whole column"""
    li, sx0, sw, x0, y0, rw, rh, F = (int(c[n]) for n in ("line_index", "src_x0", "src_w", "x0", "y0", "rw", "rh", "feather"))
    fx0, fy0, fw, fh = (int(c[n]) for n in ("fx0", "fy0", "fw", "fh"))
    assert int(c["k"]) == pages.box_factor(rh, lines.shape[1])
    line = lines[li, :, sx0:sx0 + sw]
    if (fx0, fy0, fw, fh) == (x0, y0, rw, rh):
        return pages.paste_host(page, line, (x0, y0, rw, rh), F)
    view, fg = page[y0:y0 + rh, x0:x0 + rw], pages.line_to_rect(line, rw, rh)
    if F == 0:
        view[...] = fg
        return page
    m = (pages.feather_axis(fh, F)[y0 - fy0:y0 - fy0 + rh, None] * pages.feather_axis(fw, F)[None, x0 - fx0:x0 - fx0 + rw])[:, :, None]
    D = 4 * F * F
    view[...] = ((view.astype(np.int64) * (D - m) + fg.astype(np.int64) * m + D // 2) // D).astype(np.uint8)
    return page


def _host(d, cells):
    out = d["page"].copy()
    for c in cells:
        _paste_cell_host(out, d["lines"], c)
    return out


@pytest.fixture(scope="module")
def data():
    """random lines and a random page, the scene's table, and the host results of the table in its order and reversed, computed once; asserts
    that the scene holds what the tests are about"""
    rng = np.random.default_rng(20260301)
    lines = rng.integers(0, 256, (N_LINES, ROWS, LINE_W, 3), dtype=np.uint8)
    page = rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    d = dict(lines=lines, lines_d=torch.from_numpy(lines).to(DEV), page=page)
    cells = _table()
    rects = [r[3] for r in SCENE]
    cover = np.zeros((PAGE_H, PAGE_W), np.int64)
    for x0, y0, rw, rh in rects:
        cover[y0:y0 + rh, x0:x0 + rw] += 1
    assert ((cover[:, 63] >= 2) & (cover[:, 64] >= 2)).any() and ((cover[15] >= 2) & (cover[16] >= 2)).any()      # overlaps across 63|64 and 15|16
    assert cover.max() >= 3 and (cover[10:16, 50:70] >= 3).all()                                                 # three deep
    (ax, ay, aw, ah), (bx, by, bw, bh) = rects[0], rects[1]
    assert ax < bx and ay < by and bx + bw < ax + aw and by + bh < ay + ah                                        # wholly inside
    assert rects[4] == rects[5] and SCENE[4][4] > 0 and SCENE[5][4] == 0                                          # the twins
    assert cover[0, 0] >= 2 and cover[-1, -1] >= 2                                                                # both corners, in pairs
    assert any(x0 % 64 and y0 % 16 for x0, y0, _, _ in rects)
    assert sum(rw == 1 for _, _, rw, _ in rects) >= 2
    for r, (x0, y0, rw, rh) in enumerate(rects):                                                                  # every region overlaps another
        assert (cover[y0:y0 + rh, x0:x0 + rw] >= 2).any(), SCENE[r][0]
    assert set(cells["k"].tolist()) == {1, 2, 4, 8}
    assert any(2 * r[4] > max(r[3][2], r[3][3]) for r in SCENE)                                                   # a feather wider than half a rectangle
    col = cells[13:16]
    assert IS_COLUMN.index(True) == 13 and sum(IS_COLUMN) == 1 and len(cells) == 17 and col["k"].tolist() == [1, 1, 2]
    assert all((int(c["fx0"]), int(c["fy0"]), int(c["fw"]), int(c["fh"])) == rects[13] != (int(c["x0"]), int(c["y0"]), int(c["rw"]), int(c["rh"])) for c in col)
    # the column's cells pasted one by one are the column's definition: the vstack of the cells' foregrounds under ONE feather_blend
    x0, y0, rw, rh = rects[13]
    fg = np.vstack([pages.line_to_rect(lines[1, :, sx0:sx0 + sw], rw, ch) for sx0, sw, ch in SCENE[13][2]])
    whole = page.copy()
    whole[y0:y0 + rh, x0:x0 + rw] = pages.feather_blend(page[y0:y0 + rh, x0:x0 + rw], fg, SCENE[13][4])
    assert np.array_equal(_host(d, col), whole)
    d.update(cells=cells, rects=rects, cover=cover, want=_host(d, cells), want_back=_host(d, np.concatenate([_cells_of(r) for r in reversed(range(len(SCENE)))])))
    assert not np.array_equal(d["want"], d["want_back"])                                                          # the order shows
    assert np.array_equal(d["want"][30:46, 100:140], pages.line_to_rect(lines[4, :, :30], 40, 16))               # the first twin has vanished
    return d


def _page_buf(page):
    """a guarded copy of the page on the device → (the whole buffer, the page's view of it)"""
    size = page.size
    buf = torch.full((size + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    dst = buf[GUARD:GUARD + size].view(page.shape)
    dst.copy_(torch.from_numpy(page))
    return buf, dst


def _read(buf, shape):
    host, size = buf.cpu().numpy(), int(np.prod(shape))
    assert (host[:GUARD] == 0xCD).all() and (host[GUARD + size:] == 0xCD).all()                                   # the guards are untouched
    return host[GUARD:GUARD + size].reshape(shape)


def _paste(d, dst, cells, spans=None, order=None):
    if spans is None:
        spans, order = pages.bin_tiles(cells, int(dst.shape[0]), int(dst.shape[1]))
    got = ops.paste_ordered_u8(d["lines_d"], ops.table_to_device(cells, DEV), ops.table_to_device(spans, DEV), torch.from_numpy(order).to(DEV), dst)
    assert got.data_ptr() == dst.data_ptr()


def _launch(d, cells, spans=None, order=None):
    buf, dst = _page_buf(d["page"])
    _paste(d, dst, cells, spans, order)
    return _read(buf, d["page"].shape)


# ------------------------------------------------------------------------------------------------------------------------ the kernel
def test_one_launch_equals_the_host_sequence(data):
    d = data
    got = _launch(d, d["cells"])
    for r, (x0, y0, rw, rh) in enumerate(d["rects"]):
        assert np.array_equal(got[y0:y0 + rh, x0:x0 + rw], d["want"][y0:y0 + rh, x0:x0 + rw]), SCENE[r][0]
    assert np.array_equal(got, d["want"])
    assert np.array_equal(got[d["cover"] == 0], d["page"][d["cover"] == 0]) and (d["cover"] == 0).any()           # outside all rectangles: the page's bytes
    back = _launch(d, np.concatenate([_cells_of(r) for r in reversed(range(len(SCENE)))]))
    assert np.array_equal(back, d["want_back"])
    assert np.array_equal(_launch(d, d["cells"][::-1].copy()), d["want_back"])                                    # the column's cells reversed too: they are disjoint


@pytest.mark.parametrize("m", (1, 2, 5, 14, 15, 16))                                                            # 14 and 15 split the column
def test_two_launches_over_a_split_table_give_the_bytes_of_one(data, m):
    d = data
    buf, dst = _page_buf(d["page"])
    _paste(d, dst, d["cells"][:m])
    _paste(d, dst, d["cells"][m:])
    assert np.array_equal(_read(buf, d["page"].shape), d["want"])


def test_a_disjoint_line_table_gives_the_bytes_of_paste_u8(data):
    """tests/test_pages_gpu.py's disjoint regions (the same page shape, 16-row lines): mnet_paste_u8's bytes, in any order of the table"""
    d = data
    reg = disjoint_table(range(len(DISJOINT_REGIONS)), ROWS)
    old = ops.paste_u8(d["lines_d"], ops.table_to_device(reg, DEV), torch.from_numpy(d["page"]).to(DEV)).cpu().numpy()
    cells = pages.as_cell(reg)
    assert np.array_equal(_launch(d, cells), old) and np.array_equal(_launch(d, cells[::-1].copy()), old)
    assert np.array_equal(old, _host(d, cells)) and not np.array_equal(old, d["page"])


def test_a_disjoint_column_table_gives_the_bytes_of_column_paste_u8():
    """tests/test_columns_gpu.py's disjoint columns at 128 rows: mnet_column_paste_u8's bytes on the same cell table"""
    from tests.test_columns_gpu import PASTE
    rng = np.random.default_rng(20260302)
    cols = [(box, cuts, columns.cell_widths(box, cuts), None) for _, box, cuts, _, _ in PASTE]
    lines = rng.integers(0, 256, (3, 128, 4 * max(sum(c[2]) for c in cols), 3), dtype=np.uint8)
    page = rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    rects = [(s * box[0], s * box[1], s * (box[2] - box[0]), s * (box[3] - box[1])) for _, box, _, s, _ in PASTE]
    d = dict(lines=lines, lines_d=torch.from_numpy(lines).to(DEV), page=page)
    for F in (0, 8, 40):
        tab = columns.paste_table(cols, [p[4] for p in PASTE], rects, F, 128)
        old = ops.column_paste_u8(d["lines_d"], ops.table_to_device(tab, DEV), torch.from_numpy(page).to(DEV)).cpu().numpy()
        assert np.array_equal(_launch(d, tab), old) and not np.array_equal(old, page)
        want = page.copy()
        for c, rect, p in zip(cols, rects, PASTE):
            columns.paste_column_host(want, lines[p[4], :, :4 * sum(c[2])], rect, c[1], c[2], F)
        assert np.array_equal(old, want)


# ------------------------------------------------------------------------------------------------------------- unfollowable inputs
def _tile_area(t):
    ty, tx = divmod(t, TILES_X)
    return slice(16 * ty, min(16 * ty + 16, PAGE_H)), slice(64 * tx, min(64 * tx + 64, PAGE_W))


def _span_edit(first=None, count=None):
    def edit(spans, order, t):
        n = len(order)
        f, c = int(spans["first"][t]), int(spans["count"][t])
        spans["first"][t] = f if first is None else first(f, c, n)
        spans["count"][t] = c if count is None else count(f, c, n)
    return edit


BAD_SPANS = (
    ("negative first", _span_edit(first=lambda f, c, n: -1)),
    ("first at -2^31", _span_edit(first=lambda f, c, n: -2 ** 31)),
    ("negative count", _span_edit(count=lambda f, c, n: -1)),
    ("count at -2^31", _span_edit(count=lambda f, c, n: -2 ** 31)),
    ("first + count one beyond n_order", _span_edit(first=lambda f, c, n: n - c + 1)),
    ("count beyond n_order", _span_edit(first=lambda f, c, n: 0, count=lambda f, c, n: n + 1)),
    ("first at 2^31 - 1", _span_edit(first=lambda f, c, n: 2 ** 31 - 1)),
    ("first and count at 2^31 - 1: their 32-bit sum is negative", _span_edit(first=lambda f, c, n: 2 ** 31 - 1, count=lambda f, c, n: 2 ** 31 - 1)),
)


@pytest.mark.parametrize("name,edit", BAD_SPANS, ids=[b[0] for b in BAD_SPANS])
def test_an_unfollowable_span_keeps_the_tile_s_background_and_the_other_tiles_stand(data, name, edit):
    d = data
    spans, order = pages.bin_tiles(d["cells"], PAGE_H, PAGE_W)
    t = 4                                                                                # tile (1, 1): the large one, the stack, the column
    assert spans["count"][t] >= 4
    edit(spans, order, t)
    expect = d["want"].copy()
    expect[_tile_area(t)] = d["page"][_tile_area(t)]
    assert not np.array_equal(expect, d["want"])
    assert np.array_equal(_launch(d, d["cells"], spans, order), expect)


@pytest.mark.parametrize("entry", (-1, 17, -2 ** 31, 2 ** 31 - 1), ids=("-1", "n_cells", "-2^31", "2^31 - 1"))
def test_an_order_entry_outside_the_table_is_skipped_and_its_neighbours_stand(data, entry):
    """tile 0's second entry (the cell wholly inside the large one, under the stack's third) replaced: the tile composites the others, in order"""
    d = data
    spans, order = pages.bin_tiles(d["cells"], PAGE_H, PAGE_W)
    f, c = int(spans["first"][0]), int(spans["count"][0])
    assert order[f:f + c].tolist()[:3] == [0, 1, 2] and len(d["cells"]) == 17
    order[f + 1] = entry
    expect = d["want"].copy()
    expect[_tile_area(0)] = _host(d, np.delete(d["cells"], 1))[_tile_area(0)]
    assert not np.array_equal(expect, d["want"])
    assert np.array_equal(_launch(d, d["cells"], spans, order), expect)


def _set(field, value):
    def edit(tab):
        tab[field][1] = value
    return edit


# cell 1 (line 0, src_w 50, rectangle (30, 10, 40, 20), k = 1, feather 2: wholly inside cell 0, under cell 2) made unfollowable
BAD_CELLS = (
    ("negative line_index", _set("line_index", -1)),
    ("line_index = n_lines", _set("line_index", N_LINES)),
    ("negative src_x0", _set("src_x0", -1)),
    ("the slice beyond line_w", _set("src_x0", LINE_W - 49)),
    ("src_x0 + src_w beyond 32 bits", _set("src_x0", 2 ** 31 - 1)),
    ("src_w = 0", _set("src_w", 0)),
    ("src_w beyond line_w", _set("src_w", LINE_W + 1)),
    ("rw = 0", _set("rw", 0)),
    ("negative rw", _set("rw", -40)),
    ("rh = 0", _set("rh", 0)),
    ("negative rh", _set("rh", -20)),
    ("negative x0", _set("x0", -1)),
    ("negative y0", _set("y0", -1)),
    ("the cell beyond the page's right edge", _set("rw", PAGE_W - 29)),
    ("the cell beyond the page's bottom", _set("rh", PAGE_H - 9)),
    ("x0 + rw beyond 32 bits", _set("x0", 2 ** 31 - 1)),
    ("y0 + rh beyond 32 bits", _set("y0", 2 ** 31 - 1)),
    ("negative feather", _set("feather", -1)),
    ("feather beyond 1024", _set("feather", 1025)),
    ("k = 0", _set("k", 0)),
    ("k = 3", _set("k", 3)),
    ("k = 16", _set("k", 16)),
    ("k = 32", _set("k", 32)),
    ("negative k", _set("k", -2)),
    ("fw = 0", _set("fw", 0)),
    ("negative fh", _set("fh", -20)),
    ("the feather rectangle starts right of the cell", _set("fx0", 31)),
    ("the feather rectangle starts below the cell", _set("fy0", 11)),
    ("the feather rectangle ends left of the cell's end", _set("fw", 39)),
    ("the feather rectangle ends above the cell's end", _set("fh", 19)),
    ("fx0 at -2^31", _set("fx0", -2 ** 31)),
)


@pytest.mark.parametrize("name,edit", BAD_CELLS, ids=[b[0] for b in BAD_CELLS])
def test_an_unfollowable_cell_of_a_stack_is_skipped_and_its_neighbours_stand(data, name, edit):
    """the spans are those of the sound table, so the cell stays listed in its tiles: the kernel's own checks skip it"""
    d = data
    if "without1" not in d:
        d["without1"] = _host(d, np.delete(d["cells"], 1))
        assert not np.array_equal(d["without1"], d["want"])
    spans, order = pages.bin_tiles(d["cells"], PAGE_H, PAGE_W)
    tab = d["cells"].copy()
    assert tuple(tab[1])[:14] == (0, 0, 50, 30, 10, 40, 20, 2, 1, 30, 10, 40, 20, 0)
    edit(tab)
    assert np.array_equal(_launch(d, tab, spans, order), d["without1"])


def test_a_cell_listed_in_a_tile_it_does_not_touch_is_skipped(data):
    """tile 0's list with cells of other tiles put into it (the bottom right corner's, the column's last, the twins'): the page's bytes do not move"""
    d = data
    spans, order = pages.bin_tiles(d["cells"], PAGE_H, PAGE_W)
    f, c = int(spans["first"][0]), int(spans["count"][0])
    own = order[f:f + c].tolist()
    foreign = [8, 15, 5, 4]
    assert not set(foreign) & set(own)
    listed = [foreign[0]] + own[:1] + foreign[1:3] + own[1:] + foreign[3:]
    spans["first"][0], spans["count"][0] = len(order), len(listed)
    order = np.concatenate([order, np.asarray(listed, np.int32)])
    assert np.array_equal(_launch(d, d["cells"], spans, order), d["want"])
    # every tile lists every cell: the same page
    spans["count"][:] = len(d["cells"])
    spans["first"][:] = 0
    assert np.array_equal(_launch(d, d["cells"], spans, np.arange(len(d["cells"]), dtype=np.int32)), d["want"])


def test_a_wrong_span_count_is_refused_with_nothing_written(data):
    d = data
    spans, order = pages.bin_tiles(d["cells"], PAGE_H, PAGE_W)
    buf, dst = _page_buf(d["page"])
    cells_d, spans_d, order_d = ops.table_to_device(d["cells"], DEV), ops.table_to_device(spans, DEV), torch.from_numpy(order).to(DEV)
    for bad in (spans_d[:-1], torch.cat([spans_d, spans_d[:1]])):
        with pytest.raises(ValueError, match="spans for a page of 3 x 5 tiles"):
            ops.paste_ordered_u8(d["lines_d"], cells_d, bad.contiguous(), order_d, dst)
    lib = _lib.load()
    for n_spans in (14, 16, 0):
        status = lib.mnet_paste_ordered_u8(d["lines_d"].data_ptr(), N_LINES, ROWS, LINE_W, cells_d.data_ptr(), len(d["cells"]), spans_d.data_ptr(), n_spans,
                                           order_d.data_ptr(), len(order), dst.data_ptr(), PAGE_H, PAGE_W, None)
        assert status == -1 and b"spans for a page of 15 tiles" in lib.mnet_last_error()
    with pytest.raises(TypeError):
        ops.paste_ordered_u8(d["lines_d"], cells_d, spans_d, order_d.to(torch.int64), dst)
    with pytest.raises(TypeError):
        ops.paste_ordered_u8(d["lines_d"], cells_d[:, :48].contiguous(), spans_d, order_d, dst)
    torch.cuda.synchronize()
    assert np.array_equal(_read(buf, d["page"].shape), d["page"])


# ----------------------------------------------------------------------------------------------------------- past 2^32 bytes
def test_a_page_past_2_32_bytes(data):
    """a 62 300 x 23 000 page (4 298 700 000 bytes) of zeros with a random window at its bottom right corner and two overlapping regions there:
    the window's bytes are the host's on the window alone (a paste is local to its rectangle), everything else is still zero, and only the tiles
    the two rectangles touch are given work"""
    H, W, wh, ww = 23000, 62300, 40, 100
    nbytes = H * W * 3
    assert nbytes > 2 ** 32
    free = torch.cuda.mem_get_info()[0]
    if free < 1.25 * nbytes:
        pytest.skip("the page needs %d bytes (x 1.25 = %d), the device has %d free" % (nbytes, int(1.25 * nbytes), free))
    d = data
    window = np.random.default_rng(20260303).integers(0, 256, (wh, ww, 3), dtype=np.uint8)
    local = [(10, 5, 80, 30), (50, 20, 50, 20)]                                          # in the window; the second ends at the page's corner
    regs = [(3, 37, 4), (2, 33, 0)]                                                      # line, src_w, feather
    want = window.copy()
    for (li, sw, F), rect in zip(regs, local):
        pages.paste_host(want, d["lines"][li, :, :sw], rect, F)
    assert np.array_equal(want[20:, 50:], pages.line_to_rect(d["lines"][2, :, :33], 50, 20)) and not np.array_equal(want[5:35, 10:50], window[5:35, 10:50])
    cells = np.concatenate([pages.as_cell(pages.build_table([(W - ww + x0, H - wh + y0, rw, rh)], [sw], F, ROWS, [li]))
                            for (li, sw, F), (x0, y0, rw, rh) in zip(regs, local)])
    spans, order = pages.bin_tiles(cells, H, W)
    tiles_x, tiles_y = ops.page_tiles(H, W)
    assert len(spans) == tiles_x * tiles_y == 974 * 1438
    busy = np.flatnonzero(spans["count"])
    assert len(busy) <= 3 * 3 and (busy // tiles_x >= tiles_y - 3).all() and (busy % tiles_x >= tiles_x - 3).all()      # only the touched tiles do work
    assert order.tolist().count(1) >= 1 and int(spans["count"].max()) == 2
    page_d = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    page_d[H - wh:, W - ww:] = torch.from_numpy(window).to(DEV)
    ops.paste_ordered_u8(d["lines_d"], ops.table_to_device(cells, DEV), ops.table_to_device(spans, DEV), torch.from_numpy(order).to(DEV), page_d)
    assert np.array_equal(page_d[H - wh:, W - ww:].cpu().numpy(), want)
    page_d[H - wh:, W - ww:] = 0
    for r0 in range(0, H, 4000):                                                          # under 2^31 elements per reduction
        assert not bool(page_d[r0:r0 + 4000].any())
    del page_d


# ----------------------------------------------------------------------------------------------------------------- the page driver
@pytest.mark.parametrize("scale", (1, 4))
def test_compose_page_in_order_equals_compose_host(scale):
    """compose_page(overlap="order") at the product's shape: rows = 128, one region without a line, regions 0 / 2 / 3 overlapping"""
    rng = np.random.default_rng(15 + scale)
    page = rng.integers(0, 256, (50, 120, 3), dtype=np.uint8)
    widths = [333, None, 400, 77]
    boxes = [[3, 2, 90, 12], [0, 0, 120, 50], [10, 10, 110, 34], [60, 1, 120, 13]]
    joined = rng.integers(0, 256, (3, 128, 400, 3), dtype=np.uint8)
    lines = [joined[0, :, :333], None, joined[1], joined[2, :, :77]]
    want = pages.compose_host(page, lines, boxes, scale, 8, overlap="order")
    back = pages.compose_host(page, lines[::-1], boxes[::-1], scale, 8, overlap="order")
    assert not np.array_equal(want, back)
    joined_d = torch.from_numpy(joined).to(DEV)
    with pytest.raises(ValueError, match="regions 0 and 2 overlap"):
        pages.compose_page(page, joined_d, widths, boxes, scale, 8)
    for src in (page, torch.from_numpy(page).to(DEV)):                                        # a host page and a page that is on the device already
        out = pages.compose_page(src, joined_d, widths, boxes, scale, 8, overlap="order")
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (50 * scale, 120 * scale, 3)
        assert np.array_equal(out.cpu().numpy(), want)
    out = pages.compose_page(page, joined_d.flip(0).contiguous(), widths[::-1], boxes[::-1], scale, 8, overlap="order")
    assert np.array_equal(out.cpu().numpy(), back)
    none = pages.compose_page(page, None, [None] * 4, boxes, scale, 8, device=DEV, overlap="order")
    assert np.array_equal(none.cpu().numpy(), lq_io.resize_cubic(page, scale, scale))
    # an overlap-free page takes the same path and gives the bytes of "refuse"
    apart = [[3, 2, 90, 12], [0, 0, 120, 50], [10, 14, 110, 34], [95, 1, 120, 13]]
    a = pages.compose_page(page, joined_d, widths, apart, scale, 8).cpu().numpy()
    assert np.array_equal(pages.compose_page(page, joined_d, widths, apart, scale, 8, overlap="order").cpu().numpy(), a)


# ---------------------------------------------------------------------------------------------------------------- through the networks
@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    return MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")


@pytest.fixture(scope="module")
def scene():
    """tests/test_pages_gpu.py's scene with the first strip moved up under the long line and both boxes fractional, as a detector gives them (the
    line's rows end at 36.2, the strip's start at 35.7): their outward-rounded boxes, rows [5, 37) and [35, 54), share two rows"""
    line, text = golden_line()
    strips = [(lq_io.load_png(os.path.join(cases_png.PNG_DIR, n)), lq_io.manual_text(n)) for n in cases_png.SR_STRIPS.values()]
    page = np.random.default_rng(7).integers(0, 256, (110, 1340, 3), dtype=np.uint8)
    for img, (x, y) in ((line, (11, 5)), (strips[0][0], (3, 35)), (strips[1][0], (700, 70))):
        page[y:y + img.shape[0], x:x + img.shape[1]] = img
    h0, (h1, w1), (h2, w2) = line.shape[0], strips[0][0].shape[:2], strips[1][0].shape[:2]
    boxes = [[11, 5, 11 + line.shape[1], 5 + h0 - 0.8], [3, 35.7, 3 + w1, 35 + h1 - 0.5], [700, 70, 700 + w2, 70 + h2], [200, 60, 420, 81]]
    texts = [text, strips[0][1], strips[1][1], strips[0][1][:2] + " " + strips[0][1][2:]]
    rounded = [pages.round_box(b, 110, 1340) for b in boxes]
    assert rounded[0][1::2] == [5, 37] and rounded[1][1::2] == [35, 54] and rounded[0][0] < rounded[1][2]
    return page, boxes, texts, rounded


def test_restore_page_in_order_equals_the_host_composition(pipe, scene):
    page, boxes, texts, rounded = scene
    with pytest.raises(ValueError, match="restore_page: regions 0 and 1 overlap"):
        pipe.restore_page(page, boxes, texts, scale=4, feather=8)
    crops = [page[b[1]:b[3], b[0]:b[2]] for b in rounded]
    lines = pipe.restore_lines(crops, texts)
    assert lines[3] is None and all(l is not None for l in lines[:3])
    got, regions = pipe.restore_page(page, boxes, texts, scale=4, feather=8, details=True, overlap="order")
    want = pages.compose_host(page, lines, rounded, 4, 8, overlap="order")
    assert got.dtype == np.uint8 and got.shape == (440, 5360, 3) and np.array_equal(got, want)
    assert regions[3] is None and [r["rect"] for r in regions[:3]] == [(4 * b[0], 4 * b[1], 4 * (b[2] - b[0]), 4 * (b[3] - b[1])) for b in rounded[:3]]
    back = pages.compose_host(page, lines[::-1], rounded[::-1], 4, 8, overlap="order")
    assert not np.array_equal(want, back)                                                     # the two shared rows show the order
    rev = pipe.restore_page(page, boxes[::-1], texts[::-1], scale=4, feather=8, overlap="order")
    assert np.array_equal(rev, pages.compose_host(page, pipe.restore_lines(crops[::-1], texts[::-1]), rounded[::-1], 4, 8, overlap="order"))
    # an overlap-free page: the bytes of the default mode
    apart = [boxes[0], boxes[2], boxes[3]]
    assert np.array_equal(pipe.restore_page(page, apart, [texts[0], texts[2], texts[3]], scale=2, feather=5, overlap="order"),
                          pipe.restore_page(page, apart, [texts[0], texts[2], texts[3]], scale=2, feather=5))


def _text(n, start=10):
    a = lq_io.alphabet()
    return "".join(a[start + 7 * k] for k in range(n))


def test_restore_page_columns_in_order_equals_the_host_composition(pipe):
    """a column of five characters with a line across it, the line first and the line last"""
    page = np.random.default_rng(8).integers(0, 256, (120, 200, 3), dtype=np.uint8)
    col, line = [36, 4, 60, 4 + 5 * 21], [10, 40, 190, 64]
    for boxes, texts, vertical in (([col, line], [_text(5), _text(6, 300)], [True, False]), ([line, col], [_text(6, 300), _text(5)], [False, True])):
        cuts = [columns.cell_cuts(b, len(t)) if v else None for b, t, v in zip(boxes, texts, vertical)]
        imgs, bxs = [], []
        for b, c in zip(boxes, cuts):
            if c is None:
                imgs.append(page[b[1]:b[3], b[0]:b[2]])
                bxs.append(None)
            else:
                V, widths = columns.virtual_strip(page, b, c)
                imgs.append(V)
                bxs.append(columns.virtual_boxes(widths))
        lines = pipe.restore_lines(imgs, texts, boxes=bxs)
        assert all(l is not None for l in lines)
        with pytest.raises(ValueError, match="restore_page_columns: regions 0 and 1 overlap"):
            pipe.restore_page_columns(page, boxes, texts, vertical=vertical, scale=3, feather=8)
        got, info = pipe.restore_page_columns(page, boxes, texts, vertical=vertical, scale=3, feather=8, details=True, overlap="order")
        want = columns.compose_columns_host(page, lines, boxes, cuts, 3, 8, overlap="order")
        assert np.array_equal(got, want)
        assert not np.array_equal(want, columns.compose_columns_host(page, lines[::-1], boxes[::-1], cuts[::-1], 3, 8, overlap="order"))
        assert [("cuts" in i) for i in info] == vertical


def test_example_script_pastes_overlapping_regions_in_order(tmp_path, scene):
    """examples/restore_page.py --overlap order on the scene: the PNG's decoded pixels are restore_page(overlap="order")'s, computed in this
    process; the same call without the mode is the overlap refusal"""
    from PIL import Image
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    page, boxes, texts, _ = scene
    page, boxes, texts = page[:60, :400], [[11, 5, 390, 36.2], boxes[1]], [texts[0][:11], texts[1]]
    src, reg, out = str(tmp_path / "page.png"), str(tmp_path / "regions.json"), str(tmp_path / "out.png")
    Image.fromarray(page).save(src)
    with open(reg, "w", encoding="utf8") as f:
        json.dump([dict(box=b, text=t) for b, t in zip(boxes, texts)], f)
    env = dict(os.environ)
    env.pop("MARCONET_CKPT_DIR", None)
    cmd = [sys.executable, os.path.join(ROOT, "examples", "restore_page.py"), "-i", src, "-r", reg, "-o", out, "--scale", "2", "--feather", "5", "--precision", "fp32"]
    r = subprocess.run(cmd + ["--overlap", "order"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sde, sdg, sds, _ = checkpoints.load_state_dicts("")
    p = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, DEV), precision="fp32")
    want = p.restore_page(page, boxes, texts, scale=2, feather=5, overlap="order")
    assert want.shape == (120, 800, 3) and np.array_equal(lq_io.load_png(out), want), r.stdout[-1500:]
    assert "Region 0: " in r.stdout and "Region 1: " in r.stdout
    with pytest.raises(ValueError, match="regions 0 and 1 overlap"):
        p.restore_page(page, boxes, texts, scale=2, feather=5)
