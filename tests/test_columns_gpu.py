"""-m gpu: the vertical-column page path on the device (mnet_column_gather_u8, mnet_column_paste_u8, MarconetPipeline.restore_page_columns) against
the pure-host definition columns.virtual_strip / paste_column_host / compose_columns_host — byte for byte: every comparison is np.array_equal.  The
host references are computed once per module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from marconet_amd import columns, long_lines, lq_io, ops, pages

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE_H, PAGE_W, GUARD = 70, 150, 4096


# -------------------------------------------------------------------------------------------------------------------------- the gather
# (name, box, cuts, (max_glyphs, overlap_glyphs)) — columns of the 70 x 150 page
GATHER = (
    ("a 20-row cell 96 px wide (over tile column 63|64), then a 40-row cell at dx = 96: shorter and taller than 32", [5, 2, 65, 62], [2, 22, 62], (16, 2)),
    ("a 1 x 1 cell in the page's last pixel", [149, 69, 150, 70], [69, 70], (16, 2)),
    ("three 10-row cells in the page's top left corner", [0, 0, 20, 30], [0, 10, 20, 30], (16, 2)),
    ("two cells in the page's bottom right corner", [130, 40, 150, 70], [40, 55, 70], (16, 2)),
    ("three cells in two windows: the second starts at cell 1, its cells at dx = 0 and dx > 0", [70, 5, 101, 64], [5, 25, 36, 64], (2, 1)),
)


def _gather_columns():
    cols = []
    for _, box, cuts, (mg, og) in GATHER:
        widths = columns.cell_widths(box, cuts)
        cols.append((box, cuts, widths, long_lines.plan_windows(32, sum(widths), columns.virtual_boxes(widths), mg, og)))
    return cols


@pytest.fixture(scope="module")
def gather_data():
    """a random page on the host and on the device; the windows of every case, each a slice of its column's virtual strip, and the table of all
    windows with a gap of 1, 2, 3 ... bytes before each, so that the offsets are odd and even and no multiple of a pixel"""
    page = np.random.default_rng(20251020).integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    cols = _gather_columns()
    tab, shapes, offsets, _ = columns.gather_table(cols)
    strips = [columns.virtual_strip(page, box, cuts)[0] for box, cuts, _, _ in cols]
    want = [strips[c][:, p.c0:p.c1] for c, col in enumerate(cols) for p in col[3]]
    assert [w.shape[:2] for w in want] == shapes and len(want) == 6
    assert cols[0][2] == [96, 48] and cols[1][2] == [32] and cols[2][2] == [64, 64, 64] and [len(c[3]) for c in cols] == [1, 1, 1, 1, 2]
    assert int(tab["dx"].max()) > 0 and cols[4][3][1].c0 > 0
    # clamping to the page instead of the cell shows: the corner cells are NOT the slices of their whole column resized at once
    assert not np.array_equal(strips[2][:, :64], pages.resize_cubic_to(page[0:30, 0:20], 64, 96)[:32])
    assert not np.array_equal(strips[3][:, 43:], pages.resize_cubic_to(page[40:70, 130:150], 43, 64)[32:])
    win_of = np.searchsorted(np.asarray(offsets), tab["offset"], side="right") - 1               # descriptor → its window
    new, off = [], 0
    for w, (h, ww) in enumerate(shapes):
        off += w + 1
        new.append(off)
        off += 3 * h * ww
    tab["offset"] = [new[w] for w in win_of]
    assert any(o % 2 for o in new) and any(o % 3 for o in new)
    return dict(page=page, page_d=torch.from_numpy(page).to(DEV), tab=tab, win_of=win_of, offsets=new, shapes=shapes, want=want, size=off + 5)


def _cell_image(d, r):
    """the contract of one descriptor, from the record alone: its page rectangle resized on its own to dw x 32"""
    return pages.resize_cubic_to(d["page"][int(r["sy"]):int(r["sy"]) + int(r["sh"]), int(r["sx"]):int(r["sx"]) + int(r["sw"])], int(r["dw"]), 32)


def _gather_launch(d, tab, max_dw=None):
    buf = torch.full((d["size"] + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    dst = buf[GUARD:GUARD + d["size"]]
    got = ops.column_gather_u8(d["page_d"], ops.table_to_device(tab, DEV), int(max(tab["dw"].max(), 1)) if max_dw is None else max_dw, 32, dst)
    assert got.data_ptr() == dst.data_ptr()
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + d["size"]], (host[:GUARD], host[GUARD + d["size"]:])


def _gather_expect(d, sel, untouched=()):
    """the whole buffer: 0xCD but for the columns of the descriptors ``sel`` of the fixture's table"""
    expect = np.full((d["size"],), 0xCD, np.uint8)
    for j, k in enumerate(sel):
        if j in untouched:
            continue
        r, w = d["tab"][k], int(d["win_of"][k])
        h, ww = d["shapes"][w]
        img = expect[d["offsets"][w]:d["offsets"][w] + 3 * h * ww].reshape(h, ww, 3)
        img[:, int(r["dx"]):int(r["dx"]) + int(r["dw"])] = _cell_image(d, r)
    return expect


def test_gather_batch_equals_virtual_strip(gather_data):
    d = gather_data
    got, guards = _gather_launch(d, d["tab"])
    for w, (want, off) in enumerate(zip(d["want"], d["offsets"])):
        assert np.array_equal(got[off:off + want.size].reshape(want.shape), want), w
    assert np.array_equal(got, _gather_expect(d, range(len(d["tab"]))))                             # and the bytes between the images are untouched
    assert all((g == 0xCD).all() for g in guards)


def test_gather_is_batch_invariant(gather_data):
    d = gather_data
    for w in range(len(d["want"])):                                                               # one window per launch
        sel = [k for k in range(len(d["tab"])) if d["win_of"][k] == w]
        got, guards = _gather_launch(d, d["tab"][sel])
        assert np.array_equal(got, _gather_expect(d, sel)), w
        assert all((g == 0xCD).all() for g in guards)
    for k in range(len(d["tab"])):                                                                # one cell per launch: its columns only
        got, guards = _gather_launch(d, d["tab"][[k]])
        assert np.array_equal(got, _gather_expect(d, [k])), k


def _gset(field, value):
    def edit(tab, size):
        tab[field][1] = value
    return edit


# descriptor 1 of the launch (the 40-row cell at dx = 96 of the first window: win_w 144, dw 48, page rectangle (5, 22, 60, 40)) made unfollowable
GATHER_BAD = (
    ("negative offset", _gset("offset", -1)),
    ("the window's end past dst_bytes", lambda tab, size: tab["offset"].__setitem__(1, size - 10)),
    ("an offset past dst_bytes", lambda tab, size: tab["offset"].__setitem__(1, size + 1)),
    ("an offset near 2^63", _gset("offset", 2 ** 63 - 2)),
    ("win_w = 0", _gset("win_w", 0)),
    ("win_w near 2^31", _gset("win_w", 2 ** 31 - 1)),
    ("dw = 0", _gset("dw", 0)),
    ("negative dw", _gset("dw", -48)),
    ("dw beyond max_dw = 96, inside the window", lambda tab, size: (tab["dx"].__setitem__(1, 0), tab["dw"].__setitem__(1, 97))),
    ("negative dx", _gset("dx", -1)),
    ("the columns beyond the window", _gset("dx", 97)),
    ("dx + dw beyond 32 bits", _gset("dx", 2 ** 31 - 1)),
    ("negative sx", _gset("sx", -1)),
    ("negative sy", _gset("sy", -1)),
    ("the cell beyond the page's right edge", _gset("sx", 91)),
    ("the cell beyond the page's bottom", _gset("sy", 31)),
    ("sx + sw beyond 32 bits", _gset("sx", 2 ** 31 - 1)),
    ("sw = 0", _gset("sw", 0)),
    ("negative sh", _gset("sh", -40)),
    ("a NaN scale_x", _gset("scale_x", float("nan"))),
    ("an infinite scale_y", _gset("scale_y", float("inf"))),
)


@pytest.mark.parametrize("name,edit", GATHER_BAD, ids=[b[0] for b in GATHER_BAD])
def test_unfollowable_cell_leaves_its_bytes_and_its_neighbours_stand(gather_data, name, edit):
    d = gather_data
    sel = [0, 1, 2, 3]                                                                            # both cells of the first window, the 1 x 1 cell, a corner cell
    tab = d["tab"][sel].copy()
    assert tuple(tab[1])[1:8] == (144, 96, 48, 5, 22, 60, 40)
    edit(tab, d["size"])
    got, guards = _gather_launch(d, tab, max_dw=96)
    assert np.array_equal(got, _gather_expect(d, sel, untouched=(1,)))
    assert all((g == 0xCD).all() for g in guards)


# --------------------------------------------------------------------------------------------------------------------------- the paste
ROWS, N_LINES = 128, 3
# (name, box in page pixels, cuts, scale, line_index): disjoint columns of the 150 x 70 enlarged page.  At 128 rows a cell of 8..16 output rows takes
# k = 8, 17..32 k = 4, 33..64 k = 2, more k = 1.
PASTE = (
    ("70 px wide, over tile column 63|64; cells of 10 / 18 / 38 rows, over tile rows 15|16: k = 8, 4, 2", [3, 2, 73, 68], [2, 12, 30, 68], 1, 2),
    ("one cell of 66 rows at scale 2: k = 1, the first cell and the last", [40, 1, 50, 34], [1, 34], 2, 0),
    ("cells of 9 / 9 / 19 rows, the 9-row ones 85 px wide in the strip: a ragged slice under k = 8", [105, 3, 129, 40], [3, 12, 21, 40], 1, 1),
)
FEATHERS = (0, 1, 8, 40)                                                                          # 40: more than half of every column's width


@pytest.fixture(scope="module")
def paste_data():
    """random lines and a random page; per feather the host result of every column alone"""
    rng = np.random.default_rng(20251021)
    cols = [(box, cuts, columns.cell_widths(box, cuts), None) for _, box, cuts, _, _ in PASTE]
    assert [c[2] for c in cols] == [[224, 124, 59], [10], [85, 85, 40]]
    line_w = 4 * max(sum(c[2]) for c in cols)
    lines = rng.integers(0, 256, (N_LINES, ROWS, line_w, 3), dtype=np.uint8)
    page = rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    rects = [(s * box[0], s * box[1], s * (box[2] - box[0]), s * (box[3] - box[1])) for _, box, _, s, _ in PASTE]
    assert rects == [(3, 2, 70, 66), (80, 2, 20, 66), (105, 3, 24, 37)]
    want = {F: [columns.paste_column_host(page.copy(), lines[li, :, :4 * sum(c[2])], rect, c[1], c[2], F) for c, rect, (_, _, _, _, li) in zip(cols, rects, PASTE)]
            for F in FEATHERS}
    tabs = {F: columns.paste_table(cols, [p[4] for p in PASTE], rects, F, ROWS) for F in FEATHERS}
    assert tabs[0]["k"].tolist() == [8, 4, 2, 1, 8, 8, 4] and tabs[0]["src_w"].tolist()[4] == 340 and 340 % 8
    col_of = [0, 0, 0, 1, 2, 2, 2]                                                                 # descriptor → its column
    return dict(page=page, lines_d=torch.from_numpy(lines).to(DEV), rects=rects, want=want, tabs=tabs, col_of=col_of)


def _paste_launch(d, tab):
    size = PAGE_H * PAGE_W * 3
    buf = torch.full((size + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    dst = buf[GUARD:GUARD + size].view(PAGE_H, PAGE_W, 3)
    dst.copy_(torch.from_numpy(d["page"]))
    got = ops.column_paste_u8(d["lines_d"], ops.table_to_device(tab, DEV), dst)
    assert got.data_ptr() == dst.data_ptr()
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + size].reshape(PAGE_H, PAGE_W, 3), (host[:GUARD], host[GUARD + size:])


def _paste_expect(d, F, sel, untouched=()):
    """the page with the cells ``sel`` (descriptors of the feather's table) pasted: each cell's rectangle taken from its column's host result"""
    expect = d["page"].copy()
    for j, k in enumerate(sel):
        if j in untouched:
            continue
        r = d["tabs"][F][k]
        x0, y0, rw, rh = int(r["x0"]), int(r["y0"]), int(r["rw"]), int(r["rh"])
        expect[y0:y0 + rh, x0:x0 + rw] = d["want"][F][d["col_of"][k]][y0:y0 + rh, x0:x0 + rw]
    return expect


@pytest.mark.parametrize("feather", FEATHERS)
def test_paste_batch_equals_host_and_is_batch_invariant(paste_data, feather):
    d, tab = paste_data, paste_data["tabs"][feather]
    got, guards = _paste_launch(d, tab)
    for c, (x0, y0, rw, rh) in enumerate(d["rects"]):
        assert np.array_equal(got[y0:y0 + rh, x0:x0 + rw], d["want"][feather][c][y0:y0 + rh, x0:x0 + rw]), PASTE[c][0]
        assert not np.array_equal(got[y0:y0 + rh, x0:x0 + rw], d["page"][y0:y0 + rh, x0:x0 + rw])
    assert np.array_equal(got, _paste_expect(d, feather, range(len(tab))))                          # and outside the columns the page is untouched
    assert all((g == 0xCD).all() for g in guards)
    for k in range(len(tab)):                                                                     # each cell alone — first, middle and last — gives the bytes it gives in the batch
        got, guards = _paste_launch(d, tab[[k]])
        assert np.array_equal(got, _paste_expect(d, feather, [k])), k
        assert all((g == 0xCD).all() for g in guards)


def _pset(field, value):
    def edit(tab):
        tab[field][1] = value
    return edit


# descriptor 1 of the launch (the middle cell of the first column: slice [896, 896 + 496) of line 2, rectangle (3, 12, 70, 18), k = 4, feather
# rectangle (3, 2, 70, 66)) made unfollowable
PASTE_BAD = (
    ("negative line_index", _pset("line_index", -1)),
    ("line_index = n_lines", _pset("line_index", N_LINES)),
    ("negative src_x0", _pset("src_x0", -1)),
    ("the slice beyond line_w", _pset("src_x0", 1133)),
    ("src_x0 + src_w beyond 32 bits", _pset("src_x0", 2 ** 31 - 1)),
    ("src_w = 0", _pset("src_w", 0)),
    ("rw = 0", _pset("rw", 0)),
    ("negative rh", _pset("rh", -18)),
    ("negative x0", _pset("x0", -1)),
    ("negative y0", _pset("y0", -1)),
    ("the cell beyond the page's right edge", _pset("x0", 81)),
    ("the cell beyond the page's bottom", _pset("y0", 53)),
    ("x0 + rw beyond 32 bits", _pset("x0", 2 ** 31 - 1)),
    ("negative feather", _pset("feather", -1)),
    ("feather beyond 1024", _pset("feather", 1025)),
    ("k = 0", _pset("k", 0)),
    ("k = 3", _pset("k", 3)),
    ("k = 16", _pset("k", 16)),
    ("fw = 0", _pset("fw", 0)),
    ("negative fh", _pset("fh", -66)),
    ("the feather rectangle starts right of the cell", _pset("fx0", 4)),
    ("the feather rectangle starts below the cell", _pset("fy0", 13)),
    ("the feather rectangle ends left of the cell's end", _pset("fw", 69)),
    ("the feather rectangle ends above the cell's end", _pset("fh", 27)),
    ("fx0 at -2^31", _pset("fx0", -2 ** 31)),
)


@pytest.mark.parametrize("name,edit", PASTE_BAD, ids=[b[0] for b in PASTE_BAD])
def test_unfollowable_paste_cell_keeps_the_background_and_its_neighbours_stand(paste_data, name, edit):
    d = paste_data
    sel = [0, 1, 2, 3]
    tab = d["tabs"][8][sel].copy()
    assert tuple(tab[1])[:13] == (2, 896, 496, 3, 12, 70, 18, 8, 4, 3, 2, 70, 66) and d["lines_d"].shape[2] == 1628
    edit(tab)
    got, guards = _paste_launch(d, tab)
    assert np.array_equal(got, _paste_expect(d, 8, sel, untouched=(1,)))
    assert all((g == 0xCD).all() for g in guards)


# ------------------------------------------------------------------------------------------------- the kernels and their twins
# (rectangle (x0, y0, rw, rh) in the 150-row x 200-column page, src_w, line): disjoint.  Heights 70 / 30 / 16 take k = 1 / 4 / 8; 73 and 70 columns
# are ragged under k = 4 and 8; widths 70 / 64 / 9: two x tiles, an exact tile edge, a sliver
TWIN_REGIONS = (((3, 5, 70, 70), 75, 0), ((100, 10, 64, 30), 73, 1), ((180, 100, 9, 16), 70, 0))


@pytest.mark.parametrize("feather", (0, 3, 40))                                                   # 40: more than half of every rectangle
def test_a_paste_region_is_a_column_cell_with_a_trivial_slice_and_its_own_feather_rectangle(feather):
    """mnet_paste_u8 and mnet_column_paste_u8 share one body: a ``PasteRegion`` table and the ``ColumnPaste`` table with src_x0 = 0 and the feather
    rectangle = the cell's own give identical pages, and both give ``pages.paste_host``'s"""
    from marconet_amd import _lib
    rng = np.random.default_rng(20251022)
    page = rng.integers(0, 256, (150, 200, 3), dtype=np.uint8)
    lines = rng.integers(0, 256, (2, 128, 75, 3), dtype=np.uint8)
    rects = [r for r, _, _ in TWIN_REGIONS]
    reg = pages.build_table(rects, [w for _, w, _ in TWIN_REGIONS], feather, 128, line_index=[l for _, _, l in TWIN_REGIONS])
    assert reg["k"].tolist() == [1, 4, 8] and reg["line_index"].tolist() == [0, 1, 0] and reg["src_w"].tolist() == [75, 73, 70]
    cells = np.zeros((len(reg),), dtype=np.dtype(_lib.ColumnPaste))
    for n, (r, (x0, y0, rw, rh)) in enumerate(zip(reg, rects)):
        cells[n] = (int(r["line_index"]), 0, int(r["src_w"]), x0, y0, rw, rh, feather, int(r["k"]), x0, y0, rw, rh, 0, float(r["scale_x"]), float(r["scale_y"]))
    want = page.copy()
    for (rect, src_w, l) in TWIN_REGIONS:
        pages.paste_host(want, lines[l, :, :src_w], rect, feather)
    lines_d = torch.from_numpy(lines).to(DEV)
    as_regions = ops.paste_u8(lines_d, ops.table_to_device(reg, DEV), torch.from_numpy(page).to(DEV)).cpu().numpy()
    as_cells = ops.column_paste_u8(lines_d, ops.table_to_device(cells, DEV), torch.from_numpy(page).to(DEV)).cpu().numpy()
    assert np.array_equal(as_regions, as_cells)
    assert np.array_equal(as_regions, want) and np.array_equal(as_cells, want)
    for x0, y0, rw, rh in rects:
        assert not np.array_equal(want[y0:y0 + rh, x0:x0 + rw], page[y0:y0 + rh, x0:x0 + rw])


def test_a_gather_cell_over_a_whole_image_at_one_step_is_the_preview_resize():
    """mnet_column_gather_u8 and mnet_lq_from_u8 share one cubic: one cell that covers a 20 x 70 image at the step 1 / 2 on both axes gives the
    preview form's bytes, and both give ``lq_io.resize_cubic(img, 2, 2)`` (= ``pages.resize_cubic_to(img, 140, 40)``: checked first, on the host)"""
    from marconet_amd import _lib
    img = np.random.default_rng(20251023).integers(0, 256, (20, 70, 3), dtype=np.uint8)
    want = lq_io.resize_cubic(img, 2, 2)
    assert want.shape == (40, 140, 3) and np.array_equal(pages.resize_cubic_to(img, 140, 40), want)
    img_d = torch.from_numpy(img).to(DEV)
    cell = np.zeros((1,), dtype=np.dtype(_lib.ColumnCell))
    cell[0] = (0, 140, 0, 140, 0, 0, 70, 20, 0, 1.0 / 2, 1.0 / 2)
    dst = torch.full((3 * 40 * 140,), 0xCD, dtype=torch.uint8, device=DEV)
    gathered = ops.column_gather_u8(img_d, ops.table_to_device(cell, DEV), 140, 40, dst).cpu().numpy().reshape(40, 140, 3)
    desc = np.zeros((1,), dtype=np.dtype(_lib.LqImage))
    desc[0] = (0, 20, 70, 140, 0, 0.5)
    preview = ops.lq_from_u8(img_d.reshape(-1), ops.table_to_device(desc, DEV), 40, 140, preview=True)[0].cpu().numpy()
    assert np.array_equal(gathered, preview)
    assert np.array_equal(gathered, want) and np.array_equal(preview, want)


# ---------------------------------------------------------------------------------------------------------------- through the networks
@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    return MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")


def _text(n, start=10):
    a = lq_io.alphabet()
    return "".join(a[start + 7 * k] for k in range(n))


@pytest.fixture(scope="module")
def scene():
    """a noise page with a column of 5 characters (one window), a column of 20 characters with its character boxes (several windows), a horizontal
    line, and a column whose text has a character outside the alphabet"""
    page = np.random.default_rng(8).integers(0, 256, (230, 200, 3), dtype=np.uint8)
    boxes = [[6, 4, 30, 4 + 5 * 21], [50, 3, 61, 3 + 20 * 11], [80, 20, 190, 44], [100, 60, 120, 160]]
    texts = [_text(5), _text(20, 40), _text(6, 300), _text(2) + " " + _text(2)]
    cb = [[50, 3 + 11 * j + (j % 3 == 1), 61, 3 + 11 * (j + 1) - (j % 2)] for j in range(20)]       # boxes with gaps of 0..2 rows between them
    return page, boxes, texts, [None, cb, None, None]


def _lines_of(pipe, page, boxes, texts, cuts):
    """what restore_lines gives for the virtual strips of the columns and the crops of the lines, as ONE batch in the regions' order"""
    imgs, bxs = [], []
    for b, c in zip(boxes, cuts):
        if c is None:
            imgs.append(page[b[1]:b[3], b[0]:b[2]])
            bxs.append(None)
        else:
            V, widths = columns.virtual_strip(page, b, c)
            imgs.append(V)
            bxs.append(columns.virtual_boxes(widths))
    return pipe.restore_lines(imgs, texts, boxes=bxs, details=True)


def test_columns_equal_the_host_composition(pipe, scene):
    page, boxes, texts, cb = scene
    sel = [0, 1, 3]                                                                               # the three columns
    b3, t3 = [boxes[i] for i in sel], [texts[i] for i in sel]
    cuts = [columns.cell_cuts(b3[0], 5), columns.cell_cuts(b3[1], 20, cb[1]), columns.cell_cuts(b3[2], 5)]
    lines, plans = _lines_of(pipe, page, b3, t3, cuts)
    assert len(plans[0]) == 1 and len(plans[1]) >= 2 and lines[2] is None and lines[0].shape == (128, 4 * sum(columns.cell_widths(b3[0], cuts[0])), 3)
    got, info = pipe.restore_page_columns(page, b3, t3, char_boxes=[None, cb[1], None], scale=2, feather=5, details=True)
    assert got.dtype == np.uint8 and got.shape == (460, 400, 3)
    assert np.array_equal(got, columns.compose_columns_host(page, lines, b3, cuts[:2] + [None], 2, 5))
    assert not np.array_equal(got, lq_io.resize_cubic(page, 2, 2))
    assert info[2] is None and [i["plan"] for i in info[:2]] == plans[:2] and [i["cuts"] for i in info[:2]] == cuts[:2]
    assert [i["widths"] for i in info[:2]] == [columns.cell_widths(b, c) for b, c in zip(b3[:2], cuts[:2])]
    assert [i["rect"] for i in info[:2]] == [(12, 8, 48, 210), (100, 6, 22, 440)] and info[0]["out_w"] == lines[0].shape[1]


def test_a_mixed_page_equals_the_host_composition(pipe, scene):
    page, boxes, texts, _ = scene
    b2, t2 = [boxes[2], boxes[0]], [texts[2], texts[0]]                                           # a line, then a column
    cuts = [None, columns.cell_cuts(b2[1], 5)]
    lines, plans = _lines_of(pipe, page, b2, t2, cuts)
    got, info = pipe.restore_page_columns(page, b2, t2, vertical=[False, True], scale=3, feather=8, details=True)
    assert np.array_equal(got, columns.compose_columns_host(page, lines, b2, cuts, 3, 8))
    assert [i["plan"] for i in info] == plans and "cuts" not in info[0] and info[1]["cuts"] == cuts[1]


def test_vertical_all_false_gives_restore_page(pipe, scene):
    page, boxes, texts, _ = scene
    b2, t2 = [boxes[2], [5, 200, 195, 226]], [texts[2], _text(12, 90)]
    want, regions = pipe.restore_page(page, b2, t2, scale=2, feather=5, details=True)
    got, info = pipe.restore_page_columns(page, b2, t2, vertical=[False, False], scale=2, feather=5, details=True)
    assert np.array_equal(got, want) and info == regions and not np.array_equal(got, lq_io.resize_cubic(page, 2, 2))


def test_a_column_and_the_row_of_the_same_cells_restore_to_the_same_characters(pipe):
    """the layout identity: a column of 32 x 32 cells reaches the encoder as the row of the same cells does (one window each: the same batch), so at
    scale 4 with feather 0 every restored cell is the matching 128 x 128 block of restore_page's line"""
    rng = np.random.default_rng(9)
    cells = rng.integers(0, 256, (5, 32, 32, 3), dtype=np.uint8)
    text = _text(5, 60)
    col_page = rng.integers(0, 256, (170, 50, 3), dtype=np.uint8)
    row_page = rng.integers(0, 256, (40, 200, 3), dtype=np.uint8)
    for j in range(5):
        col_page[4 + 32 * j:36 + 32 * j, 9:41] = cells[j]
        row_page[3:35, 20 + 32 * j:52 + 32 * j] = cells[j]
    row = pipe.restore_page(row_page, [[20, 3, 180, 35]], [text], scale=4, feather=0)
    col = pipe.restore_page_columns(col_page, [[9, 4, 41, 164]], [text], scale=4, feather=0)
    for j in range(5):
        assert np.array_equal(col[4 * (4 + 32 * j):4 * (36 + 32 * j), 36:164], row[12:140, 80 + 128 * j:80 + 128 * (j + 1)]), j
    assert not np.array_equal(col[16:656, 36:164], lq_io.resize_cubic(col_page, 4, 4)[16:656, 36:164])


def test_restore_page_columns_without_restored_regions_is_the_background(pipe, scene):
    page = scene[0][:40, :90]
    assert np.array_equal(pipe.restore_page_columns(page, [], [], scale=2), lq_io.resize_cubic(page, 2, 2))
    assert np.array_equal(pipe.restore_page_columns(page, [[5, 5, 30, 38]], [""], scale=2), lq_io.resize_cubic(page, 2, 2))
    assert np.array_equal(pipe.restore_page_columns(page, [[5, 5, 30, 38], [40, 5, 80, 30]], ["a b", ""], vertical=[True, False], scale=2),
                          lq_io.resize_cubic(page, 2, 2))


def test_example_script_takes_a_vertical_region(tmp_path, scene):
    """examples/restore_page.py on a page with one "vertical" region and one line: the PNG's decoded pixels are restore_page_columns', computed in
    this process"""
    from PIL import Image
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    page, boxes, texts, _ = scene
    page = page[:120]
    regions = [dict(box=boxes[0], text=texts[0], vertical=True), dict(box=boxes[2], text=texts[2]), dict(box=[100, 60, 120, 110], text="a b", vertical=True)]
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
    want = p.restore_page_columns(page, [r_["box"] for r_ in regions], [r_["text"] for r_ in regions], vertical=[True, False, True], scale=2, feather=5)
    assert want.shape == (240, 400, 3) and np.array_equal(lq_io.load_png(out), want), r.stdout[-1500:]
    assert "Region 0: a column of 5 cell(s)" in r.stdout and "Region 1: " in r.stdout and "Region 2 keeps the page's pixels" in r.stdout
