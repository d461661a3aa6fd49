"""-m gpu: a skewed page's slope and text lines on the device (marconet_amd/skew.py, mnet_skew_ink_u8, MarconetPipeline.estimate_skew /
find_lines_skewed / restore_page_auto(deskew=True)) on the seeded synthetic weights.  Nothing here is about the QUALITY of the estimate or of the
reading, only about the definition: the kernel returns ``skew.frame_ink`` with ``==`` whatever the order of its atomic additions, the device paths
return the host definitions' dicts with ``==``, and a call that finds its lines gives, byte for byte, the call that is GIVEN those quadrilaterals.
The encoder's locations are pinned as tests/test_blind_gpu.py pins them (its head says why)."""
import numpy as np
import pytest
import torch

from marconet_amd import _lib, layout, lq_io, ops, skew
from tests import layout_scene as ls, skew_scene as ss

pytestmark = pytest.mark.gpu
DEV = "cuda"
TW, TH = _lib.SKEWINK_TILE_W, _lib.SKEWINK_TILE_H                                                   # 256 x 32: the kernel's tile
H, W = 2 * TH + 6, TW + 44                                                                          # 70 x 300: 3 row tiles, the last ragged; 2 column tiles
SLOPES = (0, 1, -1, 32, -32, 2048, -2048, 8192, -8192)
PAIRS = [v for k in range(16) for v in ((k + 0.1) * 0.046, (k + 0.9) * 0.046)]                     # tests/test_blind_gpu.py's
BASE = 7                                                                                            # what dst holds before the kernel adds


# ------------------------------------------------------------------------------------------------------------------ mnet_skew_ink_u8
def _pages():
    """a page of uniform noise (with floor 0 every pair adds) and a sparse one: paper, two short lines and a few specks"""
    rng = np.random.default_rng(20250404)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    noise[TH + 1, TW - 20:TW + 20:2], noise[TH + 1, TW - 19:TW + 21:2] = 0, 255                      # differences of 255: the floor's upper end
    sparse = ls.paper(rng, H, W)
    ls.draw_line(rng, sparse, 20, 10, 280, 22)
    ls.draw_line(rng, sparse, 200, 40, 290, 52)
    sparse[33, 250:262], sparse[63:66, 255:258], sparse[69, 299], sparse[0, 0] = 20, 0, 0, 0
    return noise, sparse


def _records():
    """(frame box, slope, columns wanted) of ONE launch: per slope the frame box, boxes that straddle the tile edges at column 256 and rows 32 and
    64, a 1 x 2 box and a 1-row box, boxes partly outside the page, two records over the same pixels, records with out_cols = -1"""
    out = []
    for m in SLOPES:
        fb = skew.frame_box(H, W, m)
        out += [(fb, m, True), (fb, m, False), ([TW - 9, TH - 5, TW + 7, TH + 4], m, True), ([TW - 1, 2 * TH - 3, TW + 1, 2 * TH + 2], m, True),
                ([100, 40, 102, 41], m, True), ([5, TH, W - 3, TH + 1], m, True), ([-20, -9, 40, 12], m, True), ([W - 30, H - 8, W + 25, H + 14], m, True),
                ([TW - 40, 20, TW + 30, 50], m, True), ([TW - 40, 20, TW + 30, 50], m, True), ([TW - 40, 20, TW + 30, 50], m, False)]
    return out


def _table(records, rects=None, guard=3):
    """``skew.ink_table`` with ``guard`` free elements before, between and behind all output ranges → (table, per record (rows, cols or None), length)"""
    tab, starts, total = skew.ink_table(records, H, W, np.dtype(_lib.SkewInkBox))
    at, placed = guard, []
    for k, (box, m, cols) in enumerate(records):
        h, w = box[3] - box[1], box[2] - box[0]
        tab[k]["out_rows"], tab[k]["out_cols"] = at, at + h + guard if cols else -1
        placed.append((at, at + h + guard if cols else None))
        at += h + guard + (w + guard if cols else 0)
        if rects is not None:
            tab[k]["px1"], tab[k]["py1"], tab[k]["px2"], tab[k]["py2"] = rects[k]
    return tab, placed, at


def _want(page, records, placed, length, floor):
    want = np.full((length,), BASE, np.int64)
    e = skew.pair_ink(page, floor)
    for (box, m, cols), (sr, sc) in zip(records, placed):
        rows_, cols_ = skew.profiles_of(e, box, m)
        want[sr:sr + rows_.size] += rows_
        if sc is not None:
            want[sc:sc + cols_.size] += cols_
    return want


def _launch(page_d, tab, length, floor):
    dst = torch.full((length,), BASE, dtype=torch.int32, device=DEV)
    rect_h, rect_w = max(1, int((tab["py2"] - tab["py1"]).max())), max(1, int((tab["px2"] - tab["px1"]).max()))
    got = ops.skew_ink_u8(page_d, ops.table_to_device(tab, DEV), rect_h, rect_w, floor, dst=dst)
    assert got is dst
    return dst.cpu().numpy()


@pytest.fixture(scope="module")
def case():
    noise, sparse = _pages()
    records = _records()
    tab, placed, length = _table(records)
    return dict(pages=dict(noise=noise, sparse=sparse), dev={k: torch.from_numpy(v).to(DEV) for k, v in (("noise", noise), ("sparse", sparse))},
                records=records, tab=tab, placed=placed, length=length)


@pytest.mark.parametrize("name", ["noise", "sparse"])
def test_skew_ink_kernel_is_frame_ink_in_one_launch(case, name):
    c, page = case, case["pages"][name]
    assert len(c["records"]) == 11 * len(SLOPES) and int((c["tab"]["py2"] - c["tab"]["py1"]).max()) == H and int((c["tab"]["px2"] - c["tab"]["px1"]).max()) == W
    wants = {floor: _want(page, c["records"], c["placed"], c["length"], floor) for floor in (0, 1, 24, 255)}
    assert np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[1], wants[24]) and not np.array_equal(wants[24], wants[255])
    assert (wants[255] > BASE).sum() > (20 if name == "noise" else -1)                              # the floor's upper end still counts something
    for floor, want in wants.items():
        got = _launch(c["dev"][name], c["tab"], c["length"], floor)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, floor)
    want = wants[0]
    guards = np.ones(c["length"], bool)
    for (box, m, cols), (sr, sc) in zip(c["records"], c["placed"]):
        guards[sr:sr + box[3] - box[1]] = False
        if sc is not None:
            guards[sc:sc + box[2] - box[0]] = False
    assert guards.sum() == 3 + 3 * len(c["records"]) + 3 * sum(r[2] for r in c["records"]) and (want[guards] == BASE).all()
    if name == "noise":                                                                             # with floor 0 every pair of the page adds to its frame box
        total = int(skew.pair_ink(page, 0).sum())
        for k in range(0, len(c["records"]), 11):
            (box, m, _), (sr, sc) = c["records"][k], c["placed"][k]
            assert (want[sr:sr + box[3] - box[1]] - BASE).sum() == total == (want[sc:sc + box[2] - box[0]] - BASE).sum()
    # two records over the same pixels, separate outputs
    (a, _, _), (ar, ac), (br, bc) = c["records"][8], c["placed"][8], c["placed"][9]
    assert c["records"][9][0] == a and ar != br and np.array_equal(want[ar:ar + 30], want[br:br + 30]) and np.array_equal(want[ac:ac + 70], want[bc:bc + 70])
    assert want[ar:ar + 30].max() > BASE
    # the wrapper's own tensor of zeros
    zeros = ops.skew_ink_u8(c["dev"][name], ops.table_to_device(c["tab"], DEV), H, W, 0, dst_len=c["length"])
    assert zeros.dtype == torch.int32 and np.array_equal(zeros.cpu().numpy(), want - BASE)


def test_slope_0_records_are_box_ink(case):
    c = case
    recs = [r for r in c["records"] if r[1] == 0 and r[2] and 0 <= r[0][0] and r[0][2] <= W and 0 <= r[0][1] and r[0][3] <= H]
    assert len(recs) == 7
    tab, placed, length = _table(recs)
    box_tab = np.zeros((len(recs),), dtype=np.dtype(_lib.BoxInkBox))
    for k, ((x1, y1, x2, y2), _, _) in enumerate(recs):
        box_tab[k] = ((y1 * W + x1) * 3, 3 * W, y2 - y1, x2 - x1, placed[k][0], placed[k][1], 0)
    for name in ("noise", "sparse"):
        for floor in (0, 24):
            dst = torch.full((length,), BASE, dtype=torch.int32, device=DEV)
            ops.box_ink_u8(c["dev"][name].reshape(-1), ops.table_to_device(box_tab, DEV), H, W, floor, dst=dst)
            assert np.array_equal(_launch(c["dev"][name], tab, length, floor), dst.cpu().numpy()), (name, floor)


def test_whole_page_scan_rectangles_give_the_same(case):
    c = case
    tab, placed, length = _table(c["records"], rects=[(0, 0, W, H)] * len(c["records"]))
    assert placed == c["placed"] and not np.array_equal(tab["px2"], c["tab"]["px2"])
    for name in ("noise", "sparse"):
        assert np.array_equal(_launch(c["dev"][name], tab, length, 24), _want(c["pages"][name], c["records"], placed, length, 24)), name


def test_skew_ink_kernel_bad_records_between_good_ones(case):
    c, page = case, case["pages"]["noise"]
    good = [c["records"][k] for k in (0, 2, 13, 40, 98)]
    box = [10, 5, 50, 25]                                                                           # 20 rows, 40 columns
    recs = [good[0], (box, 8193, True), good[1], ([10, 5, 10, 25], 0, True), ([10, 25, 50, 25], 0, True), good[2], (box, 2048, True), (box, -8193, False),
            good[3], (box, 0, True), (box, 0, True), (box, 0, True), good[4], (box, 0, True), (box, 0, True)]
    tab, placed, length = _table(recs)
    tab[6]["px2"] = W + 1                                                                           # the scan rectangle leaves the page
    tab[9]["py1"] = -1
    tab[10]["px1"], tab[10]["px2"] = 30, 20                                                         # px1 > px2
    tab[11]["out_cols"] = length - 39                                                               # the column range ends one past dst_len: rows -1, cols nothing
    tab[13]["out_rows"] = -2                                                                        # below -1: the row range fails: cols -1, rows nothing
    tab[14]["out_rows"], tab[14]["out_cols"] = 2 ** 31 - 10, -1                                     # far outside, nothing else wanted: nothing
    got = _launch(c["dev"]["noise"], tab, length, 24)
    keep = [0, 2, 5, 8, 12]
    want = _want(page, [recs[k] for k in keep], [placed[k] for k in keep], length, 24)
    marked = 0
    for k, rows_too, cols_too in ((1, True, True), (6, True, True), (7, True, False), (9, True, True), (10, True, True), (11, True, False), (13, False, True)):
        if rows_too:
            want[placed[k][0]:placed[k][0] + 20] = -1
            marked += 20
        if cols_too:
            want[placed[k][1]:placed[k][1] + 40] = -1
            marked += 40
    assert np.array_equal(got, want) and (want == -1).sum() == marked == 6 * 20 + 5 * 40             # the empty boxes (3, 4) and record 14 write nothing
    # the same box, followed: its profiles are exact
    tab, placed, length = _table([(box, 8192, True)])
    assert np.array_equal(_launch(c["dev"]["noise"], tab, length, 24), _want(page, [(box, 8192, True)], placed, length, 24))


def test_skew_ink_wrapper_refusals(case):
    c = case
    page_d, tab_d = c["dev"]["noise"], ops.table_to_device(c["tab"], DEV)
    dst = torch.full((c["length"],), BASE, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError, match="either dst_len"):
        ops.skew_ink_u8(page_d, tab_d, H, W, 24)
    with pytest.raises(TypeError, match="either dst_len"):
        ops.skew_ink_u8(page_d, tab_d, H, W, 24, dst_len=10, dst=dst)
    with pytest.raises(TypeError, match="page must be uint8"):
        ops.skew_ink_u8(page_d.reshape(-1), tab_d, H, W, 24, dst=dst)
    with pytest.raises(TypeError, match="int32 .len. dst"):
        ops.skew_ink_u8(page_d, tab_d, H, W, 24, dst=dst.float())
    with pytest.raises(TypeError, match="record table"):
        ops.skew_ink_u8(page_d, tab_d[:, :32].contiguous(), H, W, 24, dst=dst)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.skew_ink_u8(page_d.cpu(), tab_d, H, W, 24, dst=dst)
    for kw in (dict(floor=256), dict(floor=-1), dict(max_h=0), dict(max_w=2 ** 17)):
        a = dict(max_h=H, max_w=W, floor=24)
        a.update(kw)
        with pytest.raises(_lib.MarconetHipError, match="skew_ink_u8"):
            ops.skew_ink_u8(page_d, tab_d, a["max_h"], a["max_w"], a["floor"], dst=dst)
    torch.cuda.synchronize()
    assert dst.cpu().tolist() == [BASE] * c["length"]                                               # nothing was enqueued


# ------------------------------------------------------------------------------------------------- estimate_skew, find_lines_skewed
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


@pytest.mark.parametrize("deg", [2.5, -3.0])
def test_the_device_paths_are_the_host_definitions(pipe, deg):
    page, _, _ = ss.skewed(deg)
    est = pipe.estimate_skew(page)
    assert est == skew.estimate_host(page) and len(est["scores"]) == 49 + 17 and all(isinstance(s, int) for _, s in est["scores"])
    found = pipe.find_lines_skewed(page, text_h=ls.TEXT_H)
    assert found == skew.find_lines_host(page, text_h=ls.TEXT_H) and len(found["quads"]) == 24 and found["slope"] == est["slope"]
    for kw in (dict(slope=0), dict(slope=est["slope"], pad=0, floor=30), dict(slope=-8192, text_h=8, min_h=0, min_w=0), dict(floor=0, max_h=10 ** 6)):
        assert pipe.find_lines_skewed(page, **kw) == skew.find_lines_host(page, **kw), kw
    assert pipe.estimate_skew(page, floor=0, max_slope=8192) == skew.estimate_host(page, floor=0, max_slope=8192)


def test_the_device_paths_on_other_pages_and_their_refusals(pipe):
    blank = ls.paper(np.random.default_rng(3), 120, 90)
    assert pipe.estimate_skew(blank) == skew.estimate_host(blank) and pipe.estimate_skew(blank)["slope"] == 0
    assert pipe.find_lines_skewed(blank) == skew.find_lines_host(blank) and pipe.find_lines_skewed(blank)["quads"] == []
    for seed in range(3):
        page = ls.random_page(seed)
        kw = dict(slope=(700, -4000, 8192)[seed], text_h=(8, 12, 5)[seed], floor=(24, 0, 60)[seed], min_h=0, min_w=0)
        assert pipe.find_lines_skewed(page, **kw) == skew.find_lines_host(page, **kw), seed
    page, _ = ls.two_columns()
    assert pipe.find_lines_skewed(page, slope=0, text_h=ls.TEXT_H)["tight"] == pipe.find_lines(page, text_h=ls.TEXT_H)["tight"]
    with pytest.raises(ValueError, match="find_lines_skewed: slope must be"):
        pipe.find_lines_skewed(blank, slope=8193)
    with pytest.raises(ValueError, match="estimate_skew: floor must be"):
        pipe.estimate_skew(blank, floor=300)
    with pytest.raises(TypeError):
        pipe.estimate_skew(blank.astype(np.float32))


# ------------------------------------------------------------------------------------------------------ restore_page_auto(deskew=True)
def _small_skewed_page():
    """``test_layout_gpu``'s small page — four short lines 12 rows high, two of them side by side, and a strip, here 2 rows high: 3 in the frame, too
    low to paste at scale 2 — rotated by 3 degrees"""
    rng = np.random.default_rng(20250303)
    page = ls.paper(rng, 110, 260)
    for x1, y1, x2, y2 in ([10, 8, 100, 20], [140, 8, 240, 20], [10, 40, 180, 52], [10, 60, 90, 72], [10, 90, 120, 92]):
        ls.draw_line(rng, page, x1, y1, x2, y2)
    return page, ss.rotate_nearest(page, 3.0)


def test_restore_page_auto_deskew_is_restore_page_quads_given_its_quads(pipe):
    upright, page = _small_skewed_page()
    kw = dict(text_h=12, pad=0)
    got, det = pipe.restore_page_auto(page, scale=2, feather=3, details=True, deskew=True, **kw)
    found = pipe.find_lines_skewed(page, **kw)
    assert len(found["quads"]) == 5 and abs(det["slope"] - 3435) <= 900 and det["slope"] == found["slope"] and det["scores"] == found["scores"]
    assert det["quads"] == found["quads"][:4] and det["frame_boxes"] == found["frame_boxes"][:4] and det["tight"] == found["tight"][:4]
    assert [s["box"] for s in det["skipped"]] == [found["frame_boxes"][4]] and "under the 8 output rows" in det["skipped"][0]["reason"]
    assert len(det["regions"]) == len(det["text"]) == 4 and any(t for t in det["text"])
    want, regions = pipe.restore_page_quads(page, det["quads"], texts=None, scale=2, feather=3, details=True)
    assert got.shape == (220, 520, 3) and got.dtype == np.uint8 and np.array_equal(got, want)
    pick = lambda rs: [None if r is None else (r["text"], r["quad"], r["out_w"]) for r in rs]
    assert pick(regions) == pick(det["regions"])
    assert not np.array_equal(got, lq_io.resize_cubic(page, 2, 2))                                  # something was pasted
    assert np.array_equal(pipe.restore_page_auto(page, scale=2, feather=3, deskew=True, **kw), got)  # without details: the page alone
    blank = ls.paper(np.random.default_rng(3), 60, 90)
    got, det = pipe.restore_page_auto(blank, scale=2, details=True, deskew=True)
    assert np.array_equal(got, lq_io.resize_cubic(blank, 2, 2))
    assert det == dict(slope=0, frame_boxes=[], tight=[], quads=[], skipped=[], passes=3, scores=skew.estimate_host(blank)["scores"], regions=[], text=[])


def test_restore_page_auto_without_the_keyword_is_as_it_was(pipe):
    upright, page = _small_skewed_page()
    for image in (upright, page):
        kw = dict(text_h=12)
        found = pipe.find_lines(image, **kw)
        keep = [b for b in found["boxes"] if 2 * (b[3] - b[1]) * 16 >= 128]
        got, det = pipe.restore_page_auto(image, scale=2, feather=3, details=True, **kw)
        assert det["boxes"] == keep and sorted(det) == ["boxes", "passes", "regions", "skipped", "text", "tight"]
        assert np.array_equal(got, pipe.restore_page(image, det["boxes"], texts=None, scale=2, feather=3))
        assert np.array_equal(got, pipe.restore_page_auto(image, scale=2, feather=3, deskew=False, **kw))
