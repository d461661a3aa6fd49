"""-m gpu: reading vertical columns blind (marconet_amd/blind_columns.py, mnet_row_ink_u8, MarconetPipeline.read_columns, restore_page_columns /
restore_page_regions with blind_columns=True) on the seeded synthetic weights.  Nothing here is about the QUALITY of the segmentation or of the
reading — no trained checkpoint exists — only about the definition: the kernel returns ``blind_columns.row_ink`` with ``==``, the device path returns
``blind_columns.read_columns_host``'s reading with ``==``, and a call that reads gives, byte for byte, the call that is GIVEN that reading.

The encoder's locations are pinned as tests/test_blind_gpu.py pins them (its head says why): every probe reports the same 16 evenly spaced pairs.
The columns of the scene are 16 px wide with a flat gap of 2 rows every 16 rows, so the first-pass cuts are the grid and every cell is 32 px wide in
the virtual strip: 18 cells are 2 probes, 25 cells are 4."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from marconet_amd import _lib, blind, blind_columns as bc, columns, lq_device, lq_io, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [v for k in range(16) for v in ((k + 0.1) * 0.046, (k + 0.9) * 0.046)]          # tests/test_blind_gpu.py's
BLANK = 6735


# ------------------------------------------------------------------------------------------------------------------- mnet_row_ink_u8
def _table(rows):
    tab = np.zeros((len(rows),), dtype=np.dtype(_lib.RowInkBox))
    for k, r in enumerate(rows):
        tab[k] = r
    return tab


def _view(W, box, out):
    x1, y1, x2, y2 = box
    return ((y1 * W + x1) * 3, 3 * W, y2 - y1, x2 - x1, out)


def test_row_ink_kernel_is_row_ink_in_one_launch():
    """every width around the 64-lane stride and every height around the 4-row workgroup inside one page (pitch > 3 w), boxes that overlap, the
    box that ends at the page's last byte, sentinel gaps in dst, descriptors that fail their source check (-1) or their dst range (nothing)"""
    rng = np.random.default_rng(20250122)
    H, W = 64, 320
    page = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    boxes = []
    for w in (1, 2, 63, 64, 65, 129, 300):
        for h in (1, 3, 4, 5, 37):
            x1, y1 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
            boxes.append([x1, y1, x1 + w, y1 + h])
    boxes += [[10, 10, 110, 30], [50, 20, 150, 40], [50, 20, 150, 40]]                    # overlapping, and the same box twice
    boxes += [[W - 65, H - 5, W, H], [0, 0, W, H]]                                        # ends at the page's last byte; the whole page (h = 64 > max_h: see below)
    rows, out, starts = [], 2, []
    for b in boxes:
        rows.append(_view(W, b, out))
        starts.append(out)
        out += b[3] - b[1] + 3                                                            # 3 sentinels between two boxes' ranges
    n_good, nbytes = len(rows), page.size
    bad_src = [(-3, 3 * W, 4, 10), (0, 29, 4, 10), (nbytes - 3 * W * 3 - 29, 3 * W, 4, 10), (0, 2 ** 31 - 1, 2, 2 ** 23), (0, 3 * W, 3, 0),
               (nbytes + 1, 3 * W, 1, 1), (nbytes - 2, 3, 1, 1)]
    for off, pitch, h, w in bad_src:
        rows.append((off, pitch, h, w, out))
        starts.append(out)
        out += h + 3
    dst_len = out
    bad_dst = [(0, 3 * W, 5, 10, -1), (0, 3 * W, 5, 10, dst_len - 4), (0, 3 * W, 5, 10, dst_len), (0, 3 * W, 5, 10, 2 ** 31 - 3), (0, 3 * W, 0, 10, 0),
               (0, 3 * W, -4, 10, 0)]
    rows += bad_dst
    dst = torch.full((dst_len,), -7, dtype=torch.int32, device=DEV)
    page_d = torch.from_numpy(page).to(DEV)
    max_h = 37 + 27                                                                       # 64: the whole page's height
    ops.row_ink_u8(page_d.reshape(-1), ops.table_to_device(_table(rows), DEV), max_h, dst)
    got = dst.cpu().numpy()
    want = np.full((dst_len,), -7, np.int32)
    for b, s in zip(boxes, starts):
        want[s:s + b[3] - b[1]] = bc.row_ink(page, b)
    for (off, pitch, h, w), s in zip(bad_src, starts[n_good:]):
        want[s:s + h] = -1
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (want == -7).sum() >= 3 * len(starts) and (want > 0).sum() > 300
    # max_h below a box's height: its rows beyond are not computed, nothing else changes
    dst2 = torch.full((dst_len,), -7, dtype=torch.int32, device=DEV)
    ops.row_ink_u8(page_d.reshape(-1), ops.table_to_device(_table(rows), DEV), 37, dst2)
    want2 = want.copy()
    want2[starts[n_good - 1] + 40:starts[n_good - 1] + 64] = -7                            # ceil(37 / 4) workgroups of 4 rows: 40 rows
    assert np.array_equal(dst2.cpu().numpy(), want2)


def test_row_ink_kernel_refusals():
    page_d = torch.zeros((3000,), dtype=torch.uint8, device=DEV)
    tab = ops.table_to_device(_table([(0, 30, 4, 10, 0)]), DEV)
    dst = torch.full((16,), -7, dtype=torch.int32, device=DEV)
    lib, stream = _lib.load(), ops._stream()
    call = lambda **kw: lib.mnet_row_ink_u8(*[kw.get(k, v) for k, v in (("src", ops._p(page_d)), ("src_bytes", 3000), ("boxes", ops._p(tab)), ("n", 1),
                                                                          ("max_h", 4), ("dst", ops._p(dst)), ("dst_len", 16), ("stream", stream))])
    for kw in (dict(src=None), dict(boxes=None), dict(dst=None), dict(n=0), dict(max_h=0), dict(src_bytes=0), dict(dst_len=0), dict(n=65536),
               dict(n=8192, max_h=8192), dict(n=-1)):
        assert call(**kw) == -1, kw                                                        # MNET_E_ARG
    assert call(boxes=tab.data_ptr() + 4) == -2 and call(dst=dst.data_ptr() + 2) == -2    # MNET_E_ALIGN
    torch.cuda.synchronize()
    assert dst.cpu().tolist() == [-7] * 16                                                # nothing was enqueued
    with pytest.raises(_lib.MarconetHipError, match="row_ink_u8"):
        ops.row_ink_u8(page_d, tab, 0, dst)
    with pytest.raises(TypeError):
        ops.row_ink_u8(page_d, tab, 4, dst.float())
    with pytest.raises(TypeError):
        ops.row_ink_u8(page_d, tab[:, :20].contiguous(), 4, dst)
    assert call() == 0 and dst.cpu().tolist() == [0] * 4 + [-7] * 12


def test_row_ink_kernel_past_2_31_bytes():
    """one box whose first byte lies past 2^31: the offset is 64 bits all the way; only the tail of the buffer is initialised"""
    base, tail_n = 2 ** 31, 4096
    buf = torch.empty((base + tail_n,), dtype=torch.uint8, device=DEV)
    tail = np.random.default_rng(5).integers(0, 256, tail_n, dtype=np.uint8)
    buf[base:].copy_(torch.from_numpy(tail))
    h, w, pitch = 8, 30, 120
    dst = torch.full((h + 2,), -7, dtype=torch.int32, device=DEV)
    ops.row_ink_u8(buf, ops.table_to_device(_table([(base + 5, pitch, h, w, 1)]), DEV), h, dst)
    page = tail[5:5 + h * pitch].reshape(h, pitch // 3, 3)
    assert dst.cpu().tolist() == [-7] + bc.row_ink(page, [0, 0, w, h]).tolist() + [-7]
    dst.fill_(-7)                                                                         # one byte short of the last row's end: -1
    ops.row_ink_u8(buf[:base + 5 + (h - 1) * pitch + 3 * w - 1], ops.table_to_device(_table([(base + 5, pitch, h, w, 1)]), DEV), h, dst)
    assert dst.cpu().tolist() == [-7] + [-1] * h + [-7]


# ------------------------------------------------------------------------------------------------------------------------ the readings
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


ONE = ([60, 5, 76, 53], [60, 70, 76, 150], [60, 170, 76, 298])                             # 3, 5 and 8 cells: one probe each
MULTI = ([4, 3, 20, 291], [30, 10, 46, 410])                                              # 18 and 25 cells, 16 px wide: 2 and 4 probes
LINE = [90, 20, 190, 44]


def _page():
    rng = np.random.default_rng(20250123)
    page = rng.integers(0, 256, (420, 200, 3), dtype=np.uint8)
    for x1, y1, x2, y2 in ONE + MULTI:                                                    # a flat gap of 2 rows around every 16th row of a column
        for t in range(y1, y2 + 1, 16):
            page[max(t - 1, y1):min(t + 1, y2), x1:x2] = 200
    return page


@pytest.fixture(scope="module")
def scene(pipe):
    """the page, the reading of its columns by both paths — computed once — and the precondition: every multi-probe column is read with >= 2 probes
    and loses at least one character to ownership; the first-pass cuts are the grid"""
    page = _page()
    boxes = list(ONE + MULTI)
    read = pipe.read_columns(page, boxes, scale=2)
    host = bc.read_columns_host(pipe, page, boxes, scale=2)
    for box, r in zip(boxes, host):
        assert r is not None and r["first_cuts"] == list(range(box[1], box[3] + 1, 16)), (box, r and r["first_cuts"])
    assert [len(r["probes"]) for r in host] == [1, 1, 1, 2, 4]
    for box, r in zip(MULTI, host[len(ONE):]):
        cuts = r["first_cuts"]
        strip, widths = columns.virtual_strip(page, box, cuts)
        assert widths == [32] * (len(cuts) - 1)
        crops = [np.ascontiguousarray(strip[:, p[2]:p[3]]) for p in r["probes"]]
        rows, locs = blind.encode(pipe, lq_device.prepare_strips(crops, DEV).lq)
        seen = sum(len(blind.read_probe(rows[k], locs[k], (p[2], p[3], -10 ** 9, 10 ** 9), 32)[0]) for k, p in enumerate(r["probes"]))
        owned = sum(len(blind.read_probe(rows[k], locs[k], p[2:], 32)[0]) for k, p in enumerate(r["probes"]))
        assert len(r["probes"]) >= 2 and owned < seen, (box, seen, owned)
    return dict(page=page, boxes=boxes, read=read, host=host)


def test_read_columns_is_read_columns_host(pipe, scene):
    assert scene["read"] == scene["host"]
    for box, r in zip(scene["boxes"], scene["host"]):
        n = len(r["labels"])
        assert n == len(r["char_boxes"]) == len(r["text"]) >= 1 and len(r["cuts"]) == n + 1 and r["cuts"][0] == box[1] and r["cuts"][-1] == box[3]
        assert all(b[0] == float(box[0]) and b[2] == float(box[2]) and box[1] <= b[1] < b[3] <= box[3] for b in r["char_boxes"])
        assert all(p[3] <= q[1] for p, q in zip(r["char_boxes"], r["char_boxes"][1:]))                        # top to bottom, disjoint
        assert all(16 * 2 * (b - a) >= 128 for a, b in zip(r["cuts"], r["cuts"][1:]))                         # settled for scale 2
    assert pipe.read_columns(scene["page"], [], scale=2) == []
    with pytest.raises(ValueError, match="region 1: box .* is empty or lies outside"):
        pipe.read_columns(scene["page"], [ONE[0], [300, 0, 310, 50]], scale=2)


# ---------------------------------------------------------------------------------------------------------------- the page entry points
def _given(det, idx):
    return [det[i]["text"] for i in idx], [det[i]["char_boxes"] for i in idx]


def test_restore_page_columns_blind_is_the_call_given_the_reading(pipe, scene):
    page, boxes = scene["page"], [MULTI[0], ONE[1], ONE[2]]
    got, det = pipe.restore_page_columns(page, boxes, None, scale=2, feather=3, details=True, blind_columns=True)
    assert all(d is not None and d["text"] and len(d["char_boxes"]) == len(d["text"]) and "first_cuts" in d and "overflow" in d for d in det)
    host = {tuple(b): r for b, r in zip(scene["boxes"], scene["host"])}
    assert [(d["text"], d["char_boxes"], d["first_cuts"], d["cuts"]) for d in det] == \
           [(host[tuple(b)]["text"], host[tuple(b)]["char_boxes"], host[tuple(b)]["first_cuts"], host[tuple(b)]["cuts"]) for b in boxes]
    texts, cbs = _given(det, range(3))
    want, det2 = pipe.restore_page_columns(page, boxes, texts, char_boxes=cbs, scale=2, feather=3, details=True)
    assert np.array_equal(got, want) and [d["plan"] for d in det] == [d["plan"] for d in det2] and "text" not in det2[0]
    assert not np.array_equal(got, lq_io.resize_cubic(page, 2, 2))                                            # something was pasted
    mixed = pipe.restore_page_columns(page, boxes, [None, texts[1], None], char_boxes=[None, cbs[1], None], scale=2, feather=3, blind_columns=True)
    assert np.array_equal(mixed, want)


def test_a_horizontal_line_that_is_read_beside_blind_columns(pipe, scene):
    page, boxes, vertical = scene["page"], [MULTI[1], LINE, ONE[0]], [True, False, True]
    got, det = pipe.restore_page_columns(page, boxes, None, vertical=vertical, scale=2, feather=3, details=True, blind_columns=True)
    assert all(d is not None for d in det) and "boxes" in det[1] and "char_boxes" in det[0] and "char_boxes" in det[2]
    want = pipe.restore_page_columns(page, boxes, [det[0]["text"], None, det[2]["text"]], vertical=vertical,
                                     char_boxes=[det[0]["char_boxes"], None, det[2]["char_boxes"]], scale=2, feather=3)
    assert np.array_equal(got, want)


def test_restore_page_regions_blind_column_over_a_line(pipe, scene):
    page = scene["page"]
    line_text = lq_io.alphabet()[100:106]
    regions = [dict(box=[40, 300, 160, 324]), dict(box=[60, 170, 76, 330], vertical=True), dict(box=MULTI[0], vertical=True)]      # the column crosses the line
    with pytest.raises(ValueError, match="restore_page_regions: regions 0 and 1 overlap"):
        pipe.restore_page_regions(page, regions, [line_text, None, None], scale=2, feather=3, blind_columns=True)   # refused before anything is read
    got, det = pipe.restore_page_regions(page, regions, [line_text, None, None], scale=2, feather=3, overlap="order", details=True, blind_columns=True)
    assert [d["kind"] for d in det] == ["line", "column", "column"] and "text" not in det[0] and det[1]["text"] and det[2]["first_cuts"]
    want = pipe.restore_page_regions(page, regions, [line_text, det[1]["text"], det[2]["text"]],
                                     char_boxes=[None, det[1]["char_boxes"], det[2]["char_boxes"]], scale=2, feather=3, overlap="order")
    assert np.array_equal(got, want)
    swapped = pipe.restore_page_regions(page, regions[:2][::-1], [None, line_text], scale=2, feather=3, overlap="order", blind_columns=True)
    assert not np.array_equal(swapped, pipe.restore_page_regions(page, regions[:2], [line_text, None], scale=2, feather=3, overlap="order", blind_columns=True))


def test_refusals_that_need_no_pixel_and_the_unchanged_default(pipe, scene):
    page = scene["page"]
    with pytest.raises(ValueError, match=r"restore_page_columns: region 0: a column needs its text \(its cells are cut from it, one per character\): only "
                                         "horizontal lines, quadrilaterals and curves are read where the text is None"):
        pipe.restore_page_columns(page, [ONE[0]], None, scale=2, feather=3)
    with pytest.raises(ValueError, match=r"restore_page_regions: region 0: a column needs its text \(its cells are cut from it, one per character\)"):
        pipe.restore_page_regions(page, [dict(box=ONE[0], vertical=True)], None, scale=2, feather=3)
    with pytest.raises(ValueError, match="restore_page_columns: scale must be an integer"):
        pipe.restore_page_columns(page, [ONE[0]], None, scale=9, blind_columns=True)
    with pytest.raises(ValueError, match="restore_page_columns: feather must be an integer"):
        pipe.restore_page_columns(page, [ONE[0]], None, scale=2, feather=-1, blind_columns=True)
    with pytest.raises(ValueError, match="restore_page_columns: region 1: box .* is empty or lies outside"):
        pipe.restore_page_columns(page, [ONE[0], [250, 0, 260, 40]], None, scale=2, blind_columns=True)
    with pytest.raises(ValueError, match="restore_page_columns: regions 0 and 1 overlap"):
        pipe.restore_page_columns(page, [ONE[0], ONE[0]], None, scale=2, blind_columns=True)
    with pytest.raises(ValueError, match="restore_page_regions: scale must be an integer"):
        pipe.restore_page_regions(page, [dict(box=ONE[0], vertical=True)], None, scale=0, blind_columns=True)


def test_a_blank_reading_keeps_the_background(pipe, scene):
    page, forward = scene["page"], pipe.encoder.forward

    def blank_forward(lq, **kw):
        logits, locs, w = forward(lq, **kw)
        logits = torch.zeros_like(logits)
        logits[..., BLANK] = 1.0
        return logits, locs, w
    pipe.encoder.forward = blank_forward
    try:
        assert pipe.read_columns(page, [MULTI[0], ONE[0]], scale=2) == [None, None]
        got, det = pipe.restore_page_columns(page, [MULTI[0], ONE[0]], None, scale=2, feather=3, details=True, blind_columns=True)
        regs = pipe.restore_page_regions(page, [dict(box=MULTI[0], vertical=True)], None, scale=2, feather=3, blind_columns=True)
    finally:
        pipe.encoder.forward = forward
    assert det == [None, None] and np.array_equal(got, lq_io.resize_cubic(page, 2, 2)) and np.array_equal(regs, got)


def test_example_script_reads_a_column_with_blind_columns(tmp_path, scene):
    from PIL import Image
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    page = scene["page"]
    regs = [dict(box=LINE, text=lq_io.alphabet()[200:205]), dict(box=MULTI[0], vertical=True), dict(box=ONE[2], vertical=True, text=lq_io.alphabet()[300:308])]
    src, reg, out = str(tmp_path / "page.png"), str(tmp_path / "regions.json"), str(tmp_path / "out.png")
    Image.fromarray(page).save(src)
    with open(reg, "w", encoding="utf8") as f:
        json.dump(regs, f)
    env = dict(os.environ)
    env.pop("MARCONET_CKPT_DIR", None)
    cmd = [sys.executable, os.path.join(ROOT, "examples", "restore_regions.py"), "-i", src, "-r", reg, "-o", out, "--scale", "2", "--feather", "5", "--precision", "fp32"]
    r = subprocess.run(cmd + ["--blind-columns"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sde, sdg, sds, _ = checkpoints.load_state_dicts("")
    p = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, DEV), precision="fp32")
    want, det = p.restore_page_regions(page, regs, [g.get("text") for g in regs], scale=2, feather=5, details=True, blind_columns=True)
    assert np.array_equal(lq_io.load_png(out), want), r.stdout[-1500:]
    if det[1] is None:
        assert "Region 1 keeps the page's pixels" in r.stdout
    else:
        assert "Region 1: a column" in r.stdout and "(read" in r.stdout
