"""-m gpu: the launches of the five ``restore_page*`` entry points, pinned: every kernel wrapper of ``marconet_amd.ops`` that the page path calls
is wrapped so that a call appends its name to a list, each entry point restores one small page once per overlap mode it has, and the recorded
sequence equals a literal.  The literals are what the entry points did before they shared one driver; a refactor of the page path keeps them.

The blind paths (a text that is None, ``read_lines``, ``read_columns``) are pinned the same way, on tests/test_blind_gpu.py's page, regions and
pinned encoder locations; their literals are a run of these tests before the probes and the planned windows shared one packer
(``restore.page_layout`` / ``page_windows_lq``).  Since then the probes of a page's lines are made AFTER its quadrilaterals' and curves' probes
are cropped, where ``mnet_lq_windows_u8`` used to be launched first: the kernels are independent and on one stream, the bytes are the same.  It
is the one reorder, and it shows in ``test_restore_page_regions_blind`` only."""
import numpy as np
import pytest
import torch

from marconet_amd import curves, lq_io, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
WATCHED = ("lq_from_u8", "stitch_u8", "paste_u8", "column_paste_u8", "column_gather_u8", "quad_crop_u8", "quad_paste_u8", "curve_crop_u8",
           "curve_paste_u8", "paste_ordered_u8", "paste_mixed_u8", "lq_windows_u8", "row_ink_u8")       # the last two: launched only where something is read
# one window per region: the background, at most one gather / crop launch per kind present, the encoder's input, the join, the paste(s)
FRONT, FORWARD = ["lq_from_u8"], ["lq_from_u8", "stitch_u8"]


@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    return MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")


@pytest.fixture(scope="module")
def scene():
    """a 200 x 100 noise page with two disjoint regions of every kind, three characters each (one window per region), and per kind a last
    region whose text has a character outside the alphabet"""
    a = lq_io.alphabet()
    text, bad = a[10] + a[17] + a[24], a[10] + " " + a[17]
    page = np.random.default_rng(11).integers(0, 256, (100, 200, 3), dtype=np.uint8)
    return dict(page=page, text=text, bad=bad,
                lines=[[4, 4, 64, 18], [4, 22, 64, 36], [4, 80, 64, 94]],
                columns=[[180, 4, 194, 60], [160, 4, 174, 60], [140, 4, 154, 60]],
                quads=[[[70, 6], [130, 10], [129, 24], [69, 20]], [[70, 30], [130, 34], [129, 48], [69, 44]], [[70, 80], [130, 80], [130, 94], [70, 94]]],
                polygons=[curves.box_polygon([4, 44, 64, 58], (30,)), [[70, 56], [130, 60], [129, 74], [69, 70]], [[4, 62], [64, 62], [64, 76], [4, 76]]])


@pytest.fixture
def calls(monkeypatch):
    seen = []
    for name in WATCHED:
        def wrapped(*args, _name=name, _fn=getattr(ops, name), **kw):
            seen.append(_name)
            return _fn(*args, **kw)
        monkeypatch.setattr(ops, name, wrapped)
    return seen


def _texts(scene, n):
    return [scene["text"]] * (n - 1) + [scene["bad"]]


@pytest.mark.parametrize("overlap,want", [("refuse", ["lq_from_u8", "lq_from_u8", "stitch_u8", "paste_u8"]),
                                          ("order", ["lq_from_u8", "lq_from_u8", "stitch_u8", "paste_ordered_u8"])])
def test_restore_page(pipe, scene, calls, overlap, want):
    """the same launches as before the shared driver; the background's launch, which followed the forward, now precedes it as in the other four"""
    got = pipe.restore_page(scene["page"], scene["lines"], _texts(scene, 3), scale=2, overlap=overlap)
    assert got.shape == (200, 400, 3) and calls == want


def test_restore_page_quads(pipe, scene, calls):
    pipe.restore_page_quads(scene["page"], scene["quads"], _texts(scene, 3), scale=2)
    assert calls == FRONT + ["quad_crop_u8"] + FORWARD + ["paste_u8", "quad_paste_u8"]


def test_restore_page_curves(pipe, scene, calls):
    pipe.restore_page_curves(scene["page"], scene["polygons"], _texts(scene, 3), scale=2)
    assert calls == FRONT + ["curve_crop_u8"] + FORWARD + ["paste_u8", "curve_paste_u8"]


@pytest.mark.parametrize("overlap,want", [("refuse", ["paste_u8", "column_paste_u8"]), ("order", ["paste_ordered_u8"])])
def test_restore_page_columns(pipe, scene, calls, overlap, want):
    boxes = scene["lines"][:2] + scene["columns"]
    pipe.restore_page_columns(scene["page"], boxes, [scene["text"]] * 4 + [scene["bad"]], vertical=[False, False, True, True, True], scale=2, overlap=overlap)
    assert calls == FRONT + ["column_gather_u8"] + FORWARD + want


@pytest.mark.parametrize("overlap", ["refuse", "order"])
def test_restore_page_regions(pipe, scene, calls, overlap):
    regs = [dict(box=b) for b in scene["lines"][:2]] + [dict(box=b, vertical=True) for b in scene["columns"][:2]] + \
           [dict(quad=q) for q in scene["quads"][:2]] + [dict(polygon=p) for p in scene["polygons"][:2]] + [dict(box=scene["lines"][2])]
    pipe.restore_page_regions(scene["page"], regs, _texts(scene, 9), scale=2, overlap=overlap)
    assert calls == FRONT + ["column_gather_u8", "quad_crop_u8", "curve_crop_u8"] + FORWARD + ["paste_u8", "paste_mixed_u8"]


# ------------------------------------------------------------------------------------------------------------------------ the blind paths
PAIRS = [v for k in range(16) for v in ((k + 0.1) * 0.046, (k + 0.9) * 0.046)]          # tests/test_blind_gpu.py's
REGIONS = [dict(box=[3, 10, 397, 34]), dict(quad=[[5, 60], [395, 66], [394, 88], [4, 82]]),
           dict(polygon=[[5, 125], [200, 120], [395, 125], [395, 145], [200, 140], [5, 145]])]
COLUMN = [380, 40, 398, 118]
# a page that is read: the probes, the background, the planned windows (the lines' as views of the page), the join
READ_LINES, PLANNED_LINES = ["lq_windows_u8"], ["lq_from_u8", "lq_windows_u8", "stitch_u8"]


@pytest.fixture(scope="module")
def blind_pipe(ckpts):
    """tests/test_blind_gpu.py's pipe: every probe reports the same 16 evenly spaced (left, right) pairs"""
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    p = MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")
    forward, pinned = p.encoder.forward, torch.tensor(PAIRS, dtype=torch.float32).reshape(1, 32)

    def pinned_forward(lq, **kw):
        logits, locs, w = forward(lq, **kw)
        return logits, pinned.to(locs.device).expand(locs.shape[0], 32).contiguous(), w
    p.encoder.forward = pinned_forward
    return p


@pytest.fixture(scope="module")
def blind_page():
    return np.random.default_rng(20250119).integers(0, 256, (160, 400, 3), dtype=np.uint8)


def test_restore_page_blind(blind_pipe, blind_page, calls):
    got, det = blind_pipe.restore_page(blind_page, [[0, 10, 400, 34], [6, 50, 398, 73]], None, scale=2, feather=3, details=True)
    assert got.shape == (320, 800, 3) and all(d is not None for d in det)
    assert calls == READ_LINES + PLANNED_LINES + ["paste_u8"]


def test_restore_page_regions_blind(blind_pipe, blind_page, calls):
    """the probes: one crop launch per warped kind, then the line's views (before the shared packer: the views first); the planned windows alike"""
    got, det = blind_pipe.restore_page_regions(blind_page, REGIONS, None, scale=2, feather=3, details=True)
    assert [d["kind"] for d in det if d is not None] == ["line", "quad", "curve"]
    crops = ["quad_crop_u8", "curve_crop_u8", "lq_windows_u8", "lq_from_u8"]
    assert calls == crops + ["lq_from_u8"] + crops + ["stitch_u8", "paste_u8", "paste_mixed_u8"]


def test_restore_page_columns_blind_column_beside_a_line_that_is_read(blind_pipe, blind_page, calls):
    got, det = blind_pipe.restore_page_columns(blind_page, [COLUMN, REGIONS[0]["box"]], None, vertical=[True, False], scale=2, feather=3, details=True,
                                               blind_columns=True)
    assert all(d is not None for d in det) and det[0]["first_cuts"] and det[1]["boxes"]
    assert calls == ["row_ink_u8", "column_gather_u8", "lq_from_u8"] + READ_LINES + ["lq_from_u8", "column_gather_u8", "lq_windows_u8", "lq_from_u8", "stitch_u8",
                                                                                      "paste_u8", "column_paste_u8"]


def test_read_lines(blind_pipe, calls):
    rng = np.random.default_rng(20250118)
    read = blind_pipe.read_lines([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((24, 200), (24, 600), (40, 700))])
    assert all(r is not None for r in read) and calls == ["lq_windows_u8"]


def test_read_columns(blind_pipe, blind_page, calls):
    read = blind_pipe.read_columns(blind_page, [COLUMN, [350, 40, 366, 150]], scale=2)
    assert all(r is not None for r in read) and calls == ["row_ink_u8", "column_gather_u8", "lq_from_u8"]
