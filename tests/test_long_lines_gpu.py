"""-m gpu: the long-line path on the device (mnet_stitch_u8, long_lines.compose_lines, MarconetPipeline.restore_lines) against the pure-host
definition long_lines.stitch_host — byte for byte: every comparison is np.array_equal.  The host references are computed once per module."""
import os

import numpy as np
import pytest
import torch

from marconet_amd import long_lines, lq_io, ops
from tests.golden import cases_png
from tests.long_lines_cases import golden_line

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, SR_W, GUARD = 5, 96, 4096


def _w(offset, show_w):
    return long_lines.Window(0, 0, 0, 0, offset, show_w)


# (offset, show_w) per window
LINES = (
    ((0, 70),),                                   # one window only: a copy
    ((0, 50), (49, 60)),                          # D = 1: the one shared column is the mean, rounded half up
    ((0, 40), (33, 50)),                          # odd D = 7
    ((0, 40), (30, 96)),                          # even D = 10; a window of the full SR width
    ((0, 50), (40, 60), (50, 80)),                # three windows whose overlaps touch: B_0 = 50 = A_1, every column of the middle window is shared
    ((0, 65), (60, 5)),                           # 65 columns: the tile edge 63 | 64 falls inside the overlap [60, 65)
    ((0, 1),),                                    # one column
)
PLANS = [[_w(*w) for w in line] for line in LINES]
N_WIN = sum(len(p) for p in PLANS)
OUT_W = max(long_lines.plan_out_w(p) for p in PLANS)


@pytest.fixture(scope="module")
def data():
    """random windows on the host and on the device + the host lines, computed once and left unchanged.  Window j of the batch reads SR image
    PERM[j]: the index is followed, not assumed"""
    assert OUT_W == 130 and OUT_W % 64 and [long_lines.plan_out_w(p) for p in PLANS] == [70, 109, 83, 126, 130, 65, 1]
    rng = np.random.default_rng(20240902)
    sr = rng.integers(0, 256, (N_WIN, ROWS, SR_W, 3), dtype=np.uint8)           # the columns beyond show_w are random too: they must not show
    perm = [int(v) for v in rng.permutation(N_WIN)]
    sr[perm[1], :, 49] = 255
    sr[perm[2], :, 0] = 0                                                       # (255 + 0 + 1) // 2 = 128 at the D = 1 column
    want, starts, j = [], [], 0
    for plan in PLANS:
        starts.append(j)
        want.append(long_lines.stitch_host([sr[perm[j + k], :, :p.show_w] for k, p in enumerate(plan)], plan))
        j += len(plan)
    return dict(sr=torch.from_numpy(sr).to(DEV), perm=perm, want=want, starts=starts)


def _tables(sel, perm_of, edit=None):
    lines, wins = long_lines.build_tables([PLANS[k] for k in sel], sr_index=[p for k in sel for p in perm_of(k)])
    if edit is not None:
        edit(lines, wins)
    return (torch.from_numpy(lines.view(np.uint8).reshape(len(lines), 16)).to(DEV), torch.from_numpy(wins.view(np.uint8).reshape(len(wins), 16)).to(DEV))


def _launch(d, sel, out_w, edit=None):
    """the lines ``sel`` in one launch into a guarded destination → (host result [len(sel),ROWS,out_w,3], the two guards)"""
    lines_d, wins_d = _tables(sel, lambda k: d["perm"][d["starts"][k]:d["starts"][k] + len(PLANS[k])], edit)
    size = len(sel) * ROWS * out_w * 3
    buf = torch.full((size + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    out = buf[GUARD:GUARD + size].view(len(sel), ROWS, out_w, 3)
    got = ops.stitch_u8(d["sr"], lines_d, wins_d, out_w=out_w, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + size].reshape(len(sel), ROWS, out_w, 3), (host[:GUARD], host[GUARD + size:])


def _check(d, sel, got, guards, filled=()):
    for j, k in enumerate(sel):
        w = 0 if j in filled else d["want"][k].shape[1]
        assert np.array_equal(got[j, :, :w], d["want"][k][:, :w]), (j, LINES[k])
        assert not got[j, :, w:].any(), (j, LINES[k])                            # 0 beyond the line: the 0xCD fill is gone everywhere
    assert all((g == 0xCD).all() for g in guards)


def test_stitch_batch_equals_host(data):
    """all lines in ONE launch: the host's bytes, 0 at the columns beyond each line's width, the guards around dst untouched"""
    sel = list(range(len(LINES)))
    got, guards = _launch(data, sel, OUT_W)
    _check(data, sel, got, guards)
    assert (got[1, :, 49] == 128).all()                                          # the D = 1 column


def test_stitch_is_batch_invariant(data):
    """each line alone, in a destination of its own width, gives the bytes it gives inside the batch"""
    sel = list(range(len(LINES)))
    batch, _ = _launch(data, sel, OUT_W)
    for k in sel:
        w = data["want"][k].shape[1]
        alone, guards = _launch(data, [k], w)
        assert np.array_equal(alone[0], batch[k, :, :w]), LINES[k]
        assert all((g == 0xCD).all() for g in guards)


def _set(*changes):
    def edit(lines, wins):
        for table, row, field, value in changes:
            (lines if table == "line" else wins)[field][row] = value
    return edit


# line 1 of the launch (PLANS[4], three windows: rows 2..4 of the window table) made unfollowable; lines 0 and 2 (PLANS[3], PLANS[1]) are its neighbours
BAD = (
    ("sr_index below the tensor", _set(("win", 3, "sr_index", -1))),
    ("sr_index beyond the tensor", _set(("win", 4, "sr_index", N_WIN))),
    ("show_w of 0", _set(("win", 2, "show_w", 0))),
    ("show_w beyond the SR width", _set(("win", 4, "show_w", SR_W + 1))),
    ("negative offset", _set(("win", 2, "offset", -1))),
    ("equal offsets", _set(("win", 3, "offset", 0))),
    ("decreasing offsets", _set(("win", 4, "offset", 39))),
    ("a column in three windows", _set(("win", 4, "offset", 49), ("win", 4, "show_w", 81))),
    ("a column in no window, inside", _set(("win", 2, "show_w", 39))),
    ("column 0 in no window", _set(("win", 2, "offset", 1))),
    ("the last column in no window", _set(("line", 1, "out_w", 131))),
    ("no window", _set(("line", 1, "n_win", 0))),
    ("a negative window count", _set(("line", 1, "n_win", -3))),
    ("a negative first window", _set(("line", 1, "win0", -1))),
    ("a negative width", _set(("line", 1, "out_w", -1))),
    ("a width beyond the destination", _set(("line", 1, "out_w", 133))),
)


@pytest.mark.parametrize("name,edit", BAD, ids=[b[0] for b in BAD])
def test_unfollowable_line_is_filled_and_its_neighbours_stand(data, name, edit):
    sel = [3, 4, 1]
    got, guards = _launch(data, sel, 132, edit)
    _check(data, sel, got, guards, filled=(1,))


def test_compose_lines_equals_host(data):
    """compose_lines (tables built and copied here, one launch; window j reads SR image j)"""
    rng = np.random.default_rng(3)
    sr = rng.integers(0, 256, (N_WIN, 128, 2048, 3), dtype=np.uint8)
    wide = [_w(0, 2048), _w(2000, 2048), _w(4000, 100)]                           # a line wider than any single SR image
    plans = PLANS[:4] + [wide]
    sr = sr[:sum(len(p) for p in plans)]
    out = long_lines.compose_lines(torch.from_numpy(sr).to(DEV), plans)
    assert out.shape == (len(plans), 128, 4100, 3) and out.dtype == torch.uint8 and out.is_cuda
    out, j = out.cpu().numpy(), 0
    for l, plan in enumerate(plans):
        want = long_lines.stitch_host([sr[j + k, :, :p.show_w] for k, p in enumerate(plan)], plan)
        j += len(plan)
        assert np.array_equal(out[l, :, :want.shape[1]], want) and not out[l, :, want.shape[1]:].any(), l


# ---------------------------------------------------------------------------------------------------------------- through the networks
@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    return MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")


def test_restore_lines_equals_the_stitched_windows(pipe):
    """a 1321-px line of the reference's strips and a short strip in one call: the line is stitch_host of what restore_images gives for the same
    crops in the same batch order (the same launch regime, so the network's bytes agree); the short strip is restore_images' own result"""
    line, text = golden_line()
    name = cases_png.SR_STRIPS["lqe01"]
    short, short_text = lq_io.load_png(os.path.join(cases_png.PNG_DIR, name)), lq_io.manual_text(name)
    h, w = line.shape[:2]
    boxes = lq_io.evenly_spaced_boxes(len(text), w, h)
    plan = long_lines.plan_windows(h, w, boxes)
    assert len(plan) >= 3 and not long_lines.too_wide(*short.shape[:2])
    got, plans = pipe.restore_lines([line, short], [text, short_text], details=True)
    assert plans[0] == plan and len(plans[1]) == 1
    crops = [np.ascontiguousarray(line[:, p.c0:p.c1]) for p in plan] + [short]
    crop_texts = [text[p.g0:p.g1] for p in plan] + [short_text]
    crop_boxes = [[[b[0] - p.c0, b[1], b[2] - p.c0, b[3]] for b in boxes[p.g0:p.g1]] for p in plan] + [None]
    res = pipe.restore_images(crops, texts=crop_texts, boxes=crop_boxes)
    assert all(r is not None for r in res)
    want = long_lines.stitch_host(res[:len(plan)], plan)
    assert got[0].dtype == np.uint8 and got[0].shape == (128, long_lines.plan_out_w(plan), 3) and np.array_equal(got[0], want)
    assert abs(got[0].shape[1] - 4 * w) <= 1 and got[0].shape[1] > 2048                       # wider than the SR canvas itself
    assert got[1].shape == res[-1].shape and np.array_equal(got[1], res[-1])
    plain = pipe.restore_lines([line, short], [text, short_text])
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])


def test_restore_lines_needs_texts_and_skips_what_restore_strips_skips(pipe):
    line, text = golden_line()
    with pytest.raises(ValueError, match="cut characters in half"):
        pipe.restore_lines([line], None)
    name = cases_png.SR_STRIPS["lqe02"]
    short, short_text = lq_io.load_png(os.path.join(cases_png.PNG_DIR, name)), lq_io.manual_text(name)
    got, plans = pipe.restore_lines([line, short, line], [text[:20] + " " + text[21:], short_text, ""], details=True)
    assert got[0] is None and plans[0] is None and got[2] is None and plans[2] is None      # a blank is outside the alphabet; no character
    assert np.array_equal(got[1], pipe.restore_images([short], [short_text])[0])
    assert pipe.restore_lines([line], [""]) == [None]
    assert pipe.restore_images([line], [text]) == [None]                                    # untouched: a wide strip is still skipped there
