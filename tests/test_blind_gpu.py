"""-m gpu: reading lines and pages blind (marconet_amd/blind.py, MarconetPipeline.read_lines, restore_lines / restore_page* with texts=None) on the
seeded synthetic weights.  Nothing here is about reading QUALITY — no trained checkpoint exists — only about the definition: the device path returns
``blind.read_host``'s reading with ``==``, and a call that reads gives, byte for byte, the call that is GIVEN that reading.

The encoder's locations are pinned: every probe reports the same 16 evenly spaced (left, right) pairs, whatever its random labels are, so that every
reading has sane, monotone boxes that ``plan_windows`` can plan (the precondition is asserted in the fixture).  The pairs are put in place of the
encoder's second output and not into ``linear_locs``' last Linear: that Linear(256, 2) is shared by the 16 location slots — its bias holds ONE pair.

A line of ONE probe takes the encoder's ``preds_locs`` as they are (``restore_images(texts=None)``'s bytes, checked at equal batch below); given as
boxes, the same locations go through ``locs_from_boxes``' own rounding, so the blind-against-given comparisons use lines of several probes.

``restore_lines`` reads a line whose ENTRY of ``texts`` is None; ``texts=None`` itself stays the refusal it always was there
(tests/test_long_lines_gpu.py keeps it), while the page entry points take ``texts=None`` as a None per region."""
import numpy as np
import pytest
import torch

from marconet_amd import blind, long_lines, lq_device

pytestmark = pytest.mark.gpu
DEV = "cuda"
# 16 pairs over the first 0.736 of the canvas: inside a probe of 384 of its 512 columns; a character 0.8 of its pitch wide
PAIRS = [v for k in range(16) for v in ((k + 0.1) * 0.046, (k + 0.9) * 0.046)]
ONE = ((24, 200), (24, 384), (40, 300))                          # one probe each; 384 is the widest at height 24
MULTI = ((24, 400), (24, 500), (24, 600), (24, 750), (40, 700), (40, 800), (40, 1250))
N_PROBES = (2, 3, 4, 5, 2, 3, 5)


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


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y))


@pytest.fixture(scope="module")
def scene(pipe):
    """the lines, their reading by both paths and the blind restoration of the multi-probe lines, computed once; the precondition: every multi-probe
    line is read with >= 2 probes, loses at least one character to ownership and is planned into >= 2 windows"""
    images = _images(ONE + MULTI, 20250118)
    read = pipe.read_lines(images)
    multi = images[len(ONE):]
    lines, plans, readings = pipe.restore_lines(multi, [None] * len(multi), details=True)
    crops = [np.ascontiguousarray(img[:, p[0]:p[1]]) for img in multi for p in blind.plan_probes(img.shape[0], img.shape[1])]
    rows, locs = blind.encode(pipe, lq_device.prepare_strips(crops, DEV).lq)
    j = 0
    for i, img in enumerate(multi):
        h, w = img.shape[:2]
        probes = blind.plan_probes(h, w)
        assert len(probes) == N_PROBES[i] >= 2 and read[len(ONE) + i]["probes"] == probes
        seen = sum(len(blind.read_probe(rows[j + k], locs[j + k], (p[0], p[1], -10 ** 9, 10 ** 9), h)[0]) for k, p in enumerate(probes))
        owned = sum(len(blind.read_probe(rows[j + k], locs[j + k], p, h)[0]) for k, p in enumerate(probes))
        j += len(probes)
        assert owned < seen and lines[i] is not None and len(plans[i]) >= 2, (i, seen, owned, plans[i])
    assert all(len(blind.plan_probes(h, w)) == 1 for h, w in ONE)
    return dict(images=images, read=read, multi=multi, lines=lines, plans=plans, readings=readings)


def test_read_lines_is_read_host(pipe, scene):
    want = blind.read_host(pipe, scene["images"])
    assert scene["read"] == want and all(r is not None for r in want)
    for r, img in zip(want, scene["images"]):
        assert len(r["labels"]) == len(r["boxes"]) == len(r["text"]) >= 1
        assert all(b[1] == 0.0 and b[3] == float(img.shape[0]) and 0.0 <= b[0] < b[2] <= float(img.shape[1]) for b in r["boxes"])
        assert all(p[2] <= q[0] for p, q in zip(r["boxes"], r["boxes"][1:]))
    assert pipe.read_lines([]) == []


def test_restore_lines_blind_is_restore_lines_given_the_reading(pipe, scene):
    multi, read = scene["multi"], scene["read"][len(ONE):]
    assert [dict(text=r["text"], boxes=r["boxes"], overflow=r["overflow"]) for r in read] == scene["readings"]
    texts, boxes = [r["text"] for r in read], [r["boxes"] for r in read]
    given, plans = pipe.restore_lines(multi, texts, boxes, details=True)
    assert plans == scene["plans"]
    _same(scene["lines"], given)
    for line, plan in zip(given, plans):
        assert line.shape == (128, long_lines.plan_out_w(plan), 3)
    # given and None mixed: the lines of 4, 5 and 5 probes are read, the others take the reading as given
    some = [3, 2, 6]
    mixed = pipe.restore_lines(multi, [None if i in some else t for i, t in enumerate(texts)], [None if i in some else b for i, b in enumerate(boxes)])
    _same(mixed, given)


def test_one_probe_lines_are_restore_images_blind(pipe, scene):
    """at equal batch: both calls run the encoder and the three networks on the same three strips"""
    ones = scene["images"][:len(ONE)]
    want = pipe.restore_images(ones, texts=None)
    got, plans, readings = pipe.restore_lines(ones, [None] * len(ones), details=True)
    assert all(w is not None for w in want) and all(len(p) == 1 for p in plans)
    _same(got, want)
    assert [r["text"] for r in readings] == [s["text"] for s in pipe.restore_images(ones, texts=None, details=True)[1]]


@pytest.fixture(scope="module")
def page():
    return np.random.default_rng(20250119).integers(0, 256, (160, 400, 3), dtype=np.uint8)


def test_restore_page_blind_is_restore_page_given_the_reading(pipe, page):
    boxes = [[0, 10, 400, 34], [6, 50, 398, 73]]                                       # 400 and 392 px at heights 24 and 23: two probes each
    got, det = pipe.restore_page(page, boxes, None, scale=2, feather=3, details=True)
    assert all(d is not None and len(d["plan"]) >= 2 and len(d["boxes"]) == len(d["text"]) for d in det)
    assert all(b[1] == float(box[1]) and b[3] == float(box[3]) and box[0] <= b[0] < b[2] <= box[2] for d, box in zip(det, boxes) for b in d["boxes"])
    want, det2 = pipe.restore_page(page, boxes, [d["text"] for d in det], char_boxes=[d["boxes"] for d in det], scale=2, feather=3, details=True)
    assert np.array_equal(got, want) and [d["plan"] for d in det] == [d["plan"] for d in det2] and "text" not in det2[0]
    mixed = pipe.restore_page(page, boxes, [None, det[1]["text"]], char_boxes=[None, det[1]["boxes"]], scale=2, feather=3)
    assert np.array_equal(mixed, want)
    assert not np.array_equal(got, pipe.restore_page(page, boxes, ["", ""], scale=2, feather=3))      # something was pasted


def test_restore_page_regions_blind_reads_every_kind_but_a_column(pipe, page):
    regions = [dict(box=[3, 10, 397, 34]),
               dict(quad=[[5, 60], [395, 66], [394, 88], [4, 82]]),
               dict(polygon=[[5, 125], [200, 120], [395, 125], [395, 145], [200, 140], [5, 145]])]
    got, det = pipe.restore_page_regions(page, regions, None, scale=2, feather=3, details=True)
    assert [d["kind"] for d in det] == ["line", "quad", "curve"] and all(len(d["plan"]) >= 2 and d["text"] for d in det)
    char_boxes = [det[0]["boxes"], dict(crop=det[1]["boxes"]), dict(crop=det[2]["boxes"])]     # a line's in page pixels, the others' in their crops
    want = pipe.restore_page_regions(page, regions, [d["text"] for d in det], char_boxes=char_boxes, scale=2, feather=3)
    assert np.array_equal(got, want)
    assert np.array_equal(pipe.restore_page_quads(page, [regions[1]["quad"]], None, scale=2, feather=3),
                          pipe.restore_page_quads(page, [regions[1]["quad"]], [det[1]["text"]], char_boxes=[char_boxes[1]], scale=2, feather=3))
    assert np.array_equal(pipe.restore_page_curves(page, [regions[2]["polygon"]], [None], scale=2, feather=3),
                          pipe.restore_page_curves(page, [regions[2]["polygon"]], [det[2]["text"]], char_boxes=[char_boxes[2]], scale=2, feather=3))
    column = dict(box=[380, 40, 398, 118], vertical=True)
    with pytest.raises(ValueError, match="restore_page_regions: region 3: a column needs its text"):
        pipe.restore_page_regions(page, regions + [column], None, scale=2, feather=3)
    with pytest.raises(ValueError, match="restore_page_columns: region 1: a column needs its text"):
        pipe.restore_page_columns(page, [regions[0]["box"], column["box"]], [None, None], vertical=[False, True], scale=2, feather=3)
    got = pipe.restore_page_columns(page, [regions[0]["box"]], [None], vertical=[False], scale=2, feather=3)      # a horizontal line among columns is read
    assert np.array_equal(got, pipe.restore_page(page, [regions[0]["box"]], None, scale=2, feather=3))
