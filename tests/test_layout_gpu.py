"""-m gpu: finding a page's text lines on the device (marconet_amd/layout.py, mnet_box_ink_u8, MarconetPipeline.find_lines / restore_page_auto) on the
seeded synthetic weights.  Nothing here is about the QUALITY of the finding or of the reading, only about the definition: the kernel returns
``layout.box_ink`` with ``==`` whatever the order of its atomic additions, the device path returns ``layout.find_lines_host``'s dict with ``==``, and a
call that finds its lines gives, byte for byte, the call that is GIVEN those boxes.  The encoder's locations are pinned as tests/test_blind_gpu.py
pins them (its head says why)."""
import numpy as np
import pytest
import torch

from marconet_amd import _lib, blind_columns as bc, layout, lq_io, ops
from tests import layout_scene as ls

pytestmark = pytest.mark.gpu
DEV = "cuda"
TW, TH = _lib.BOXINK_TILE_W, _lib.BOXINK_TILE_H                                                     # 256 x 32: the kernel's tile
PAIRS = [v for k in range(16) for v in ((k + 0.1) * 0.046, (k + 0.9) * 0.046)]                     # tests/test_blind_gpu.py's
BASE = 7                                                                                            # what dst holds before the kernel adds


# ------------------------------------------------------------------------------------------------------------------- mnet_box_ink_u8
def _table(rows):
    tab = np.zeros((len(rows),), dtype=np.dtype(_lib.BoxInkBox))
    for k, r in enumerate(rows):
        tab[k] = tuple(r) + (0,)
    return tab


def _kernel_case():
    """the flat source — a random page of colours, behind it a page with ONE vertical edge between its columns TW - 1 and TW — and boxes of every
    width and height around the tile's edges as views of it (odd x1, pitch > 3 w), two boxes over the same pixels, the edge page as a whole;
    3 guard elements before, between and behind all output ranges → (src uint8 [bytes], pages, boxes [(page index, box)], table rows, dst_len)"""
    rng = np.random.default_rng(20250302)
    H, W = 2 * TH + 6, 2 * TW + 8
    page = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    page[:, :W // 2] = (page[:, :W // 2] // 16) * 3 + 100                                           # half of it: differences around the floor of 24
    page[TH + 2:TH + 5, W // 2 + 10:W // 2 + 50:2], page[TH + 2:TH + 5, W // 2 + 11:W // 2 + 51:2] = 0, 255          # differences of 255: the floor's upper end
    edge = np.full((TH + 1, 2 * TW + 1, 3), 100, np.uint8)
    edge[:, TW:] = (180, 220, 90)
    boxes = []
    for w in (1, 2, 63, 64, 65, TW - 1, TW, TW + 1, 2 * TW + 1):
        for h in (1, TH - 1, TH, TH + 1, 2 * TH + 1):
            x1, y1 = int(rng.integers(0, (W - w) // 2 + 1)) * 2 + 1, int(rng.integers(0, H - h + 1))
            boxes.append((0, [min(x1, W - w), y1, min(x1, W - w) + w, y1 + h]))
    boxes += [(0, [11, 3, 311, 40]), (0, [11, 3, 311, 40]), (0, [0, 0, W, H]), (1, [0, 0, 2 * TW + 1, TH + 1])]
    pages_, bases = [page, edge], [0, page.size]
    rows, out = [], 3
    for k, (x1, y1, x2, y2) in boxes:
        pw = pages_[k].shape[1]
        rows.append((bases[k] + (y1 * pw + x1) * 3, 3 * pw, y2 - y1, x2 - x1, out, out + (y2 - y1) + 3))
        out += (y2 - y1) + (x2 - x1) + 6
    src = np.concatenate([page.reshape(-1), edge.reshape(-1)])
    return src, pages_, boxes, rows, out


def _want(pages_, boxes, rows, dst_len, floor):
    want = np.full((dst_len,), BASE, np.int64)
    for (k, b), r in zip(boxes, rows):
        ink_r, ink_c = layout.box_ink(pages_[k], b, floor)
        want[r[4]:r[4] + r[2]] += ink_r
        want[r[5]:r[5] + r[3]] += ink_c
    return want


@pytest.fixture(scope="module")
def kernel_case():
    src, pages_, boxes, rows, dst_len = _kernel_case()
    return dict(src=torch.from_numpy(src).to(DEV), pages=pages_, boxes=boxes, rows=rows, dst_len=dst_len, tab=ops.table_to_device(_table(rows), DEV),
                max_h=max(r[2] for r in rows), max_w=max(r[3] for r in rows))


def _launch(c, floor, tab=None, src=None):
    dst = torch.full((c["dst_len"],), BASE, dtype=torch.int32, device=DEV)
    got = ops.box_ink_u8(c["src"] if src is None else src, c["tab"] if tab is None else tab, c["max_h"], c["max_w"], floor, dst=dst)
    assert got is dst
    return dst.cpu().numpy()


def test_box_ink_kernel_is_box_ink_in_one_launch(kernel_case):
    c = kernel_case
    assert len(c["boxes"]) == 49 and c["max_h"] == 2 * TH + 6 and c["max_w"] == 2 * TW + 8
    wants = {floor: _want(c["pages"], c["boxes"], c["rows"], c["dst_len"], floor) for floor in (0, 1, 24, 255)}
    assert np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[1], wants[24]) and not np.array_equal(wants[24], wants[255])
    assert (wants[255] > BASE).sum() > 20                                                           # the floor's upper end still counts something
    for floor, want in wants.items():
        got = _launch(c, floor)
        assert got.dtype == np.int32 and np.array_equal(got, want), floor
    want = wants[24]
    guards = np.ones(c["dst_len"], bool)
    for r in c["rows"]:
        guards[r[4]:r[4] + r[2]] = guards[r[5]:r[5] + r[3]] = False
    assert guards.sum() == 3 + 6 * len(c["rows"]) and (want[guards] == BASE).all()
    # the single edge between columns TW - 1 and TW: once in cols[TW - 1], once per row
    r = c["rows"][-1]
    step = int(bc.luma(np.array([180, 220, 90]))) - 100
    assert step > 24 and want[r[4]:r[4] + r[2]].tolist() == [BASE + step] * (TH + 1)
    assert want[r[5]:r[5] + r[3]].tolist() == [BASE] * (TW - 1) + [BASE + (TH + 1) * step] + [BASE] * (TW + 1)
    # two boxes over the same pixels, separate outputs
    a, b = c["rows"][45], c["rows"][46]
    assert a[:4] == b[:4] and a[4] != b[4] and np.array_equal(want[a[4]:a[4] + a[2]], want[b[4]:b[4] + b[2]]) and want[a[4]:a[4] + a[2]].min() > BASE
    # the wrapper's own tensor of zeros
    zeros = ops.box_ink_u8(c["src"], c["tab"], c["max_h"], c["max_w"], 24, dst_len=c["dst_len"])
    assert zeros.dtype == torch.int32 and np.array_equal(zeros.cpu().numpy(), want - BASE)
    # floor <= 1: the row profiles are mnet_row_ink_u8's on the same boxes
    ink_tab = np.zeros((len(c["rows"]),), dtype=np.dtype(_lib.RowInkBox))
    for k, r in enumerate(c["rows"]):
        ink_tab[k] = r[:5]
    ink = torch.full((c["dst_len"],), BASE, dtype=torch.int32, device=DEV)
    ops.row_ink_u8(c["src"], ops.table_to_device(ink_tab, DEV), c["max_h"], ink)
    ink = ink.cpu().numpy()
    for r in c["rows"]:
        assert np.array_equal(ink[r[4]:r[4] + r[2]], wants[1][r[4]:r[4] + r[2]] - BASE)


def test_box_ink_kernel_bad_descriptors_between_good_ones(kernel_case):
    c = kernel_case
    assert np.array_equal(_launch(c, 24), _want(c["pages"], c["boxes"], c["rows"], c["dst_len"], 24))      # the good-only case first
    n_src, L = int(c["src"].numel()), c["dst_len"]
    keep = [0, 20, 44, 47, 48]                                                                      # good ones, the whole page and the edge page among them
    free = c["rows"][22]                                                                            # box 22 (65 x TH) is left out: its output ranges are free
    h, w = free[2], free[3]
    bad = [(n_src - 3 * w - (h - 1) * 3 * w + 1, 3 * w, h, w, free[4], free[5]),                    # its last row ends one byte past src_bytes: -1
           (0, 3 * 4, 3, 4, -1, 10), (0, 3 * 4, 3, 4, 10, L - 3), (0, 3 * 4, 3, 4, L - 2, 10), (0, 3 * 4, 3, 4, 2 ** 31 - 2, 10),   # an output range fails
           (0, 3 * 4, 0, 4, 10, 20), (0, 3 * 4, 3, -1, 10, 20)]                                     # no box at all
    rows = [c["rows"][keep[0]], bad[0], c["rows"][keep[1]], bad[1], bad[2], c["rows"][keep[2]], bad[3], bad[4], bad[5], c["rows"][keep[3]], bad[6],
            c["rows"][keep[4]]]
    got = _launch(c, 24, tab=ops.table_to_device(_table(rows), DEV))
    want = _want(c["pages"], [c["boxes"][k] for k in keep], [c["rows"][k] for k in keep], L, 24)
    want[free[4]:free[4] + h] = -1
    want[free[5]:free[5] + w] = -1
    assert (h, w) == (TH, 65)
    assert np.array_equal(got, want) and (want == -1).sum() == h + w
    # the same box one byte further in: followed
    ok = (bad[0][0] - 1,) + bad[0][1:]
    got = _launch(c, 24, tab=ops.table_to_device(_table([ok]), DEV))
    assert (got[free[4]:free[4] + h] >= BASE).all() and (got[free[5]:free[5] + w] >= BASE).all()


def test_box_ink_wrapper_refusals(kernel_case):
    c = kernel_case
    dst = torch.full((c["dst_len"],), BASE, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError, match="either dst_len"):
        ops.box_ink_u8(c["src"], c["tab"], c["max_h"], c["max_w"], 24)
    with pytest.raises(TypeError, match="either dst_len"):
        ops.box_ink_u8(c["src"], c["tab"], c["max_h"], c["max_w"], 24, dst_len=10, dst=dst)
    with pytest.raises(TypeError, match="uint8 .bytes. pixels"):
        ops.box_ink_u8(c["src"].reshape(-1, 3), c["tab"], c["max_h"], c["max_w"], 24, dst=dst)
    with pytest.raises(TypeError, match="int32 .len. dst"):
        ops.box_ink_u8(c["src"], c["tab"], c["max_h"], c["max_w"], 24, dst=dst.float())
    with pytest.raises(TypeError, match="box table"):
        ops.box_ink_u8(c["src"], c["tab"][:, :24].contiguous(), c["max_h"], c["max_w"], 24, dst=dst)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.box_ink_u8(c["src"].cpu(), c["tab"], c["max_h"], c["max_w"], 24, dst=dst)
    for kw in (dict(floor=256), dict(floor=-1), dict(max_h=0), dict(max_w=2 ** 23)):
        a = dict(max_h=c["max_h"], max_w=c["max_w"], floor=24)
        a.update(kw)
        with pytest.raises(_lib.MarconetHipError, match="box_ink_u8"):
            ops.box_ink_u8(c["src"], c["tab"], a["max_h"], a["max_w"], a["floor"], dst=dst)
    torch.cuda.synchronize()
    assert dst.cpu().tolist() == [BASE] * c["dst_len"]                                              # nothing was enqueued


# ------------------------------------------------------------------------------------------------------------------------- find_lines
@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    p = MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")
    forward, pinned = p.encoder.forward, torch.tensor(PAIRS, dtype=torch.float32).reshape(1, 32)

    def pinned_forward(lq, **kw):
        logits, locs, w = forward(lq, **kw)
        return logits, pinned.to(locs.device).expand(locs.shape[0], 32).contiguous(), w
    p.encoder.forward = pinned_forward
    return p


def test_find_lines_is_find_lines_host(pipe):
    page, lines = ls.two_columns()
    found = pipe.find_lines(page, text_h=ls.TEXT_H)
    assert found == layout.find_lines_host(page, text_h=ls.TEXT_H) and found["tight"] == ls.expected_tight(lines) and found["passes"] == 6
    page, _ = ls.two_columns(gutter=2 * ls.TEXT_H - 1, wide=False)
    assert pipe.find_lines(page, text_h=ls.TEXT_H) == layout.find_lines_host(page, text_h=ls.TEXT_H)
    page, _ = ls.specks_and_figure()
    for kw in (dict(text_h=12), dict(text_h=12, min_h=0, min_w=0, max_h=49, pad=1000), dict(), dict(floor=0), dict(floor=255)):
        got = pipe.find_lines(page, **kw)
        assert got == layout.find_lines_host(page, **kw), kw
    blank = ls.paper(np.random.default_rng(3), 120, 90)
    assert pipe.find_lines(blank) == layout.find_lines_host(blank) == dict(boxes=[], tight=[], skipped=[], passes=3)
    ink = np.random.default_rng(4).integers(0, 2, (40, 90, 1), dtype=np.uint8).repeat(3, axis=2) * 200
    assert pipe.find_lines(ink, text_h=10) == layout.find_lines_host(ink, text_h=10)
    for seed in range(5):
        page = ls.random_page(seed)
        kw = dict(text_h=(8, 12, 5)[seed % 3], floor=(24, 0, 1, 60)[seed % 4], min_h=0, min_w=0)
        assert pipe.find_lines(page, **kw) == layout.find_lines_host(page, **kw), seed
    with pytest.raises(ValueError, match="find_lines: floor must be"):
        pipe.find_lines(blank, floor=300)
    with pytest.raises(TypeError):
        pipe.find_lines(blank.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ restore_page_auto
def _small_page():
    """four short lines 12 rows high — two side by side — and a strip 3 rows high that is a line to the cut but too low to paste at scale 2"""
    rng = np.random.default_rng(20250303)
    page = ls.paper(rng, 110, 260)
    lines = [[10, 8, ls.draw_line(rng, page, 10, 8, 100, 20), 20], [140, 8, ls.draw_line(rng, page, 140, 8, 240, 20), 20],
             [10, 40, ls.draw_line(rng, page, 10, 40, 180, 52), 52], [10, 60, ls.draw_line(rng, page, 10, 60, 90, 72), 72]]
    strip = [10, 90, ls.draw_line(rng, page, 10, 90, 120, 93), 93]
    return page, lines, strip


def test_restore_page_auto_is_restore_page_given_its_boxes(pipe):
    page, lines, strip = _small_page()
    kw = dict(text_h=12, pad=0)
    found = pipe.find_lines(page, **kw)
    assert found["tight"] == ls.expected_tight(lines + [strip]) and found["skipped"] == []
    got, det = pipe.restore_page_auto(page, scale=2, feather=3, details=True, **kw)
    assert det["boxes"] == found["boxes"][:4] and det["tight"] == found["tight"][:4] and det["passes"] == found["passes"]
    assert [s["box"] for s in det["skipped"]] == [found["boxes"][4]] and "under the 8 output rows" in det["skipped"][0]["reason"]
    assert len(det["regions"]) == len(det["text"]) == 4
    assert det["text"] == [None if r is None else r["text"] for r in det["regions"]] and any(t for t in det["text"])
    want, regions = pipe.restore_page(page, det["boxes"], texts=None, scale=2, feather=3, details=True)
    assert got.shape == (220, 520, 3) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert [None if r is None else (r["text"], r["rect"], r["out_w"]) for r in regions] == [None if r is None else (r["text"], r["rect"], r["out_w"]) for r in det["regions"]]
    assert not np.array_equal(got, lq_io.resize_cubic(page, 2, 2))                                  # something was pasted
    assert np.array_equal(pipe.restore_page_auto(page, scale=2, feather=3, **kw), got)              # without details: the page alone
    # the default pad: the same lines, grown, and the strip grown enough to be pasted
    got_pad, det_pad = pipe.restore_page_auto(page, scale=2, feather=3, details=True, text_h=12)
    assert det_pad["tight"] == found["tight"] and det_pad["skipped"] == [] and det_pad["boxes"] == pipe.find_lines(page, text_h=12)["boxes"]
    assert np.array_equal(got_pad, pipe.restore_page(page, det_pad["boxes"], texts=None, scale=2, feather=3))


def test_restore_page_auto_on_a_blank_page_and_its_refusals(pipe):
    from marconet_amd import pages, restore
    blank = ls.paper(np.random.default_rng(3), 60, 90)
    got, det = pipe.restore_page_auto(blank, scale=2, details=True)
    assert np.array_equal(got, pages.enlarge(restore.page_to_device(blank, DEV), 2).cpu().numpy()) and np.array_equal(got, lq_io.resize_cubic(blank, 2, 2))
    assert det == dict(boxes=[], tight=[], skipped=[], passes=3, regions=[], text=[])
    with pytest.raises(ValueError, match="restore_page_auto: scale must be an integer"):
        pipe.restore_page_auto(blank, scale=9)
    with pytest.raises(ValueError, match="restore_page_auto: feather must be an integer"):
        pipe.restore_page_auto(blank, feather=-1)
    with pytest.raises(ValueError, match="restore_page_auto: floor must be"):
        pipe.restore_page_auto(blank, floor=-1)
    with pytest.raises(TypeError, match="restore_page_auto: uint8 RGB"):
        pipe.restore_page_auto(blank[..., 0])
