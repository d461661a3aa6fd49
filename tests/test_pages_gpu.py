"""-m gpu: the page path on the device (mnet_paste_u8, pages.compose_page, MarconetPipeline.restore_page) against the pure-host definition
pages.paste_host / pages.compose_host — byte for byte: every comparison is np.array_equal.  The host references are computed once per module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from marconet_amd import _lib, lq_io, ops, pages
from tests.golden import cases_png
from tests.long_lines_cases import golden_line

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LINES, ROWS, LINE_W, PAGE_H, PAGE_W, GUARD = 5, 16, 96, 70, 150, 4096

# (name, line_index, src_w, (x0, y0, rw, rh), feather): disjoint rectangles of a 150 x 70 page; k follows from rh at rows = 16
REGIONS = (
    ("enlarging, over tile column 63|64 and tile row 15|16", 3, 37, (10, 5, 100, 40), 3),
    ("the page's corner (0, 0); k = 4, src_w = 35 not divisible by it", 0, 35, (0, 0, 9, 4), 1),
    ("the line's own size, no feather", 4, 30, (115, 2, 30, 16), 0),
    ("k = 2 at the full line width; a feather larger than half the rectangle on both axes", 1, 96, (0, 50, 60, 8), 40),
    ("ending at the page's bottom right corner; shrinking with k = 1", 2, 33, (125, 58, 25, 12), 3),
    ("one column wide", 0, 5, (112, 20, 1, 16), 1),
    ("k = 4, src_w divisible by it", 3, 80, (70, 50, 20, 4), 0),
    ("k = 2, odd src_w", 1, 95, (0, 60, 50, 8), 2),
    ("k = 8", 4, 90, (115, 30, 20, 2), 0),
)
KS = (1, 4, 1, 2, 1, 1, 4, 2, 8)


def _table(sel, rows=ROWS):
    tab = np.zeros((len(sel),), dtype=np.dtype(_lib.PasteRegion))
    for j, r in enumerate(sel):
        _, line_index, src_w, rect, feather = REGIONS[r]
        tab[j] = pages.build_table([rect], [src_w], feather, rows)[0]
        tab["line_index"][j] = line_index
    return tab


@pytest.fixture(scope="module")
def data():
    """random lines and a random page on the host and the lines on the device + the host result of every region alone, computed once"""
    assert [pages.box_factor(r[3][3], ROWS) for r in REGIONS] == list(KS) and _table(range(len(REGIONS)))["k"].tolist() == list(KS)
    rng = np.random.default_rng(20240903)
    lines = rng.integers(0, 256, (N_LINES, ROWS, LINE_W, 3), dtype=np.uint8)      # the columns beyond src_w are random too: they must not show
    page = rng.integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    cover = np.zeros((PAGE_H, PAGE_W), np.int64)
    want = []
    for _, line_index, src_w, (x0, y0, rw, rh), feather in REGIONS:
        cover[y0:y0 + rh, x0:x0 + rw] += 1
        full = pages.paste_host(page.copy(), lines[line_index, :, :src_w], (x0, y0, rw, rh), feather)
        want.append(full[y0:y0 + rh, x0:x0 + rw].copy())
    assert cover.max() == 1 and cover[0, 0] == 1 and cover[-1, -1] == 1          # disjoint; both corners taken
    assert np.array_equal(want[2], lines[4, :, :30, ::-1])                        # the identity-size region is the line, flipped to RGB
    return dict(lines=lines, lines_d=torch.from_numpy(lines).to(DEV), page=page, want=want)


def _launch(d, tab, lines_d=None):
    """one launch over a guarded copy of the page → (the page on the host, the two guards)"""
    size = PAGE_H * PAGE_W * 3
    buf = torch.full((size + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    dst = buf[GUARD:GUARD + size].view(PAGE_H, PAGE_W, 3)
    dst.copy_(torch.from_numpy(d["page"]))
    got = ops.paste_u8(d["lines_d"] if lines_d is None else lines_d, ops.table_to_device(tab, DEV), dst)
    assert got.data_ptr() == dst.data_ptr()
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + size].reshape(PAGE_H, PAGE_W, 3), (host[:GUARD], host[GUARD + size:])


def _check(d, sel, got, guards, untouched=()):
    expect = d["page"].copy()
    for j, r in enumerate(sel):
        x0, y0, rw, rh = REGIONS[r][3]
        if j not in untouched:
            expect[y0:y0 + rh, x0:x0 + rw] = d["want"][r]
        assert np.array_equal(got[y0:y0 + rh, x0:x0 + rw], expect[y0:y0 + rh, x0:x0 + rw]), REGIONS[r][0]
    assert np.array_equal(got, expect)                                            # and nothing outside the rectangles has changed
    assert all((g == 0xCD).all() for g in guards)


def test_paste_batch_equals_host(data):
    """all regions in ONE launch: the host's bytes in every rectangle, the page's own bytes outside them, the guards around the page untouched"""
    sel = list(range(len(REGIONS)))
    got, guards = _launch(data, _table(sel))
    _check(data, sel, got, guards)


def test_paste_is_batch_invariant(data):
    """each region launched alone gives the bytes it gives inside the batch"""
    for r in range(len(REGIONS)):
        got, guards = _launch(data, _table([r]))
        _check(data, [r], got, guards)


def _set(field, value):
    def edit(tab):
        tab[field][1] = value
    return edit


# region 1 of the launch (REGIONS[3]: x0 = 0, y0 = 50, 60 x 8, k = 2) made unfollowable; regions 0 and 2 (REGIONS[0], REGIONS[4]) are its neighbours
BAD = (
    ("line_index below the tensor", _set("line_index", -1)),
    ("line_index beyond the tensor", _set("line_index", N_LINES)),
    ("src_w of 0", _set("src_w", 0)),
    ("src_w beyond the line width", _set("src_w", LINE_W + 1)),
    ("negative x0", _set("x0", -1)),
    ("negative y0", _set("y0", -1)),
    ("the rectangle beyond the page's right edge", _set("x0", PAGE_W - 59)),
    ("the rectangle beyond the page's bottom", _set("y0", PAGE_H - 7)),
    ("x0 + rw beyond 32 bits", _set("x0", 2 ** 31 - 1)),
    ("y0 + rh beyond 32 bits", _set("y0", 2 ** 31 - 1)),
    ("rw of 0", _set("rw", 0)),
    ("negative rw", _set("rw", -60)),
    ("rh of 0", _set("rh", 0)),
    ("negative rh", _set("rh", -8)),
    ("negative feather", _set("feather", -1)),
    ("feather beyond 1024", _set("feather", 1025)),
    ("k of 0", _set("k", 0)),
    ("k of 3", _set("k", 3)),
    ("k of 16", _set("k", 16)),
    ("negative k", _set("k", -2)),
)


@pytest.mark.parametrize("name,edit", BAD, ids=[b[0] for b in BAD])
def test_unfollowable_region_keeps_the_background_and_its_neighbours_stand(data, name, edit):
    sel = [0, 3, 4]
    tab = _table(sel)
    edit(tab)
    got, guards = _launch(data, tab)
    _check(data, sel, got, guards, untouched=(1,))


def test_rows_not_divisible_by_k_keeps_the_background(data):
    """lines of 12 rows: a region with k = 8 (12 % 8 != 0) is not followed; its neighbours (k = 1 and k = 2, which divide 12) stand"""
    lines12 = np.ascontiguousarray(data["lines"][:, :12])
    sel = [0, 3, 6]
    tab = _table(sel, rows=12)
    assert tab["k"].tolist() == [1, 1, 2]
    tab["k"][1] = 8
    got, guards = _launch(data, tab, torch.from_numpy(lines12).to(DEV))
    expect = data["page"].copy()
    for r in (0, 6):
        _, line_index, src_w, rect, feather = REGIONS[r]
        pages.paste_host(expect, lines12[line_index, :, :src_w], rect, feather)
    assert np.array_equal(got, expect) and all((g == 0xCD).all() for g in guards)


@pytest.mark.parametrize("scale", (1, 4))
def test_compose_page_equals_compose_host(scale):
    """compose_page (the background and the table made here, one launch each) at the product's shape: rows = 128, one region without a line"""
    rng = np.random.default_rng(5 + scale)
    page = rng.integers(0, 256, (50, 120, 3), dtype=np.uint8)
    widths = [333, None, 400, 77]
    boxes = [[3, 2, 90, 12], [0, 0, 120, 50], [10, 14, 110, 34], [95, 1, 120, 13]]           # rh = 10, 20, 12 page rows: k = 8, 4, 8 at scale 1; 2, 1, 2 at 4
    joined = rng.integers(0, 256, (3, 128, 400, 3), dtype=np.uint8)
    lines = [joined[0, :, :333], None, joined[1], joined[2, :, :77]]
    want = pages.compose_host(page, lines, boxes, scale, 8)
    for src in (page, torch.from_numpy(page).to(DEV)):                                        # a host page and a page that is on the device already
        out = pages.compose_page(src, torch.from_numpy(joined).to(DEV), widths, boxes, scale, 8)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (50 * scale, 120 * scale, 3)
        assert np.array_equal(out.cpu().numpy(), want)
    none = pages.compose_page(page, None, [None] * 4, boxes, scale, 8, device=DEV)
    assert np.array_equal(none.cpu().numpy(), lq_io.resize_cubic(page, scale, scale))


# ---------------------------------------------------------------------------------------------------------------- through the networks
@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    return MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")


@pytest.fixture(scope="module")
def scene():
    """a noise page carrying the 1321-px line of tests/long_lines_cases.py and the reference's two labelled strips at disjoint positions, and a
    fourth region whose text has a character outside the alphabet"""
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


def test_restore_page_equals_the_host_composition(pipe, scene):
    """restore_page is compose_host of what restore_lines gives for the same crops in the same order (the same batch, so the same network bytes);
    the region that restore_lines skips keeps the background; scale 1 holds too"""
    page, boxes, texts = scene
    crops = [page[b[1]:b[3], b[0]:b[2]] for b in boxes]
    lines, plans = pipe.restore_lines(crops, texts, details=True)
    assert len(plans[0]) >= 3 and lines[3] is None and all(l is not None for l in lines[:3])
    got, regions = pipe.restore_page(page, boxes, texts, scale=4, feather=8, details=True)
    H, W = page.shape[:2]
    assert got.dtype == np.uint8 and got.shape == (4 * H, 4 * W, 3)
    assert np.array_equal(got, pages.compose_host(page, lines, boxes, 4, 8))
    assert regions[3] is None and [r["plan"] for r in regions[:3]] == plans[:3]
    assert [r["out_w"] for r in regions[:3]] == [l.shape[1] for l in lines[:3]]
    assert [r["rect"] for r in regions[:3]] == [(4 * b[0], 4 * b[1], 4 * (b[2] - b[0]), 4 * (b[3] - b[1])) for b in boxes[:3]]
    x1, y1, x2, y2 = (4 * v for v in boxes[3])
    bg = lq_io.resize_cubic(page, 4, 4)
    assert np.array_equal(got[y1:y2, x1:x2], bg[y1:y2, x1:x2])                               # the skipped region: the background's bytes
    x0, y0, rw, rh = regions[0]["rect"]
    assert not np.array_equal(got[y0:y0 + rh, x0:x0 + rw], bg[y0:y0 + rh, x0:x0 + rw])       # a restored one: not the background
    one = pipe.restore_page(page, boxes, texts, scale=1, feather=8)
    assert one.shape == page.shape and np.array_equal(one, pages.compose_host(page, lines, boxes, 1, 8))


def test_restore_page_without_restored_regions_is_the_background(pipe, scene):
    page = scene[0][:40, :90]
    assert np.array_equal(pipe.restore_page(page, [], [], scale=2), lq_io.resize_cubic(page, 2, 2))
    assert np.array_equal(pipe.restore_page(page, [[5, 5, 60, 30]], [""], scale=2), lq_io.resize_cubic(page, 2, 2))


def test_example_script_writes_the_page(tmp_path, scene):
    """examples/restore_page.py on the scene, with one region's character boxes given in page pixels (the evenly spaced ones, so that the page must
    be the one restore_page makes without them): the PNG's decoded pixels are restore_page's, computed in this process"""
    from PIL import Image
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    page, boxes, texts = scene
    regions = [dict(box=b, text=t) for b, t in zip(boxes, texts)]
    x1, y1, x2, y2 = boxes[1]
    regions[1]["char_boxes"] = [[c[0] + x1, c[1] + y1, c[2] + x1, c[3] + y1] for c in lq_io.evenly_spaced_boxes(len(texts[1]), x2 - x1, y2 - y1)]
    regions[2]["box"] = [boxes[2][0] + 0.25, boxes[2][1] + 0.5, boxes[2][2] - 0.75, boxes[2][3] - 0.01]       # rounded outward: the same box
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
    want = p.restore_page(page, boxes, texts, scale=2, feather=5)
    assert want.shape == (2 * page.shape[0], 2 * page.shape[1], 3) and np.array_equal(lq_io.load_png(out), want), r.stdout[-1500:]
    assert "Region 3 keeps the page's pixels" in r.stdout and "Region 0: " in r.stdout
