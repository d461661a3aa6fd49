"""-m gpu: the device LQ path (mnet_lq_from_u8, marconet_amd/lq_device.py, MarconetPipeline.restore_images) against the pure-host definition
lq_io — bit for bit: every comparison is torch.equal / np.array_equal.  Host references are computed once per module."""
import functools
import os

import numpy as np
import pytest
import torch

from marconet_amd import lq_device, lq_io, ops
from tests.golden import cases_png

pytestmark = pytest.mark.gpu
DEV = "cuda"
PNGS = ("real_lq13.png",) + tuple(cases_png.SR_STRIPS.values()) + tuple(cases_png.W_STRIPS)


SIZES = ((32, 512), (32, 1), (8, 3), (1, 7), (2, 31), (64, 5), (64, 7), (33, 528), (100, 1600), (100, 1601), (251, 1999), (19, 109), (15, 128))
NAMES = ["%dx%d" % s for s in SIZES] + ["47x300_checker", "all0_40x200", "all255_40x200"] + list(PNGS)
LQ_NAMES = [n for n in NAMES if n != "100x1601"]          # 100x1601 is the preview-width case (show_w 2049)


@functools.lru_cache(maxsize=None)
def _images():
    """name -> uint8 RGB image; seeded random unless named otherwise"""
    rng = np.random.default_rng(20240607)
    out = {}
    for h, w in SIZES:
        out["%dx%d" % (h, w)] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:47, 0:300]
    out["47x300_checker"] = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)      # both clip ends are hit
    out["all0_40x200"] = np.zeros((40, 200, 3), np.uint8)
    out["all255_40x200"] = np.full((40, 200, 3), 255, np.uint8)
    for f in PNGS:
        out[f] = lq_io.load_png(os.path.join(cases_png.PNG_DIR, f))
    assert list(out) == NAMES
    return out


@pytest.fixture(scope="module")
def host():
    """name -> (lq [1,3,32,512], content_w, show_w, preview) from lq_io, computed once and left unchanged"""
    ref = {}
    for name, img in _images().items():
        lq, cw, sw = lq_io.lq_from_image(img)
        ref[name] = (lq, cw, sw, lq_io.show_lq(img))
    assert ref["100x1601"][2] == 2049 and ref["33x528"][1] == 512 and ref["64x5"][1] == 2 and ref["64x7"][1] == 4
    ck = ref["47x300_checker"][3]
    assert ck.min() == 0 and ck.max() == 255
    return ref


@pytest.fixture(scope="module")
def singles(host):
    """every image through prepare_strips on its own → name -> (lq, preview) on the device"""
    out = {}
    for name, img in _images().items():
        p = lq_device.prepare_strips([img], DEV, preview=True)
        assert p.index == [0] and p.skipped == []
        assert p.content_w == [host[name][1]] and p.show_w == [host[name][2]]
        assert p.lq.shape == (1, 3, 32, 512) and p.lq.dtype == torch.float32
        assert p.preview.shape == (1, 128, host[name][2], 3) and p.preview.dtype == torch.uint8
        out[name] = (p.lq, p.preview)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", LQ_NAMES)
def test_lq_one_strip_equals_host(name, host, singles):
    lq = singles[name][0].cpu()
    assert torch.equal(lq, host[name][0])
    assert bool((lq[:, :, :, host[name][1]:] == -1.0).all())


@pytest.mark.parametrize("name", NAMES)
def test_preview_one_strip_equals_host(name, host, singles):
    assert np.array_equal(singles[name][1][0].cpu().numpy(), host[name][3])


def _ragged(names, preview):
    geoms = [lq_device.strip_geometry(_images()[n]) for n in names]
    sizes = [g.h * g.w * 3 for g in geoms]
    offsets = [int(v) for v in np.cumsum([0] + sizes[:-1])]
    assert any(o % 2 for o in offsets)                                   # per-image offsets are odd in general
    tab = lq_device.build_table(geoms, offsets, preview)
    src = torch.from_numpy(np.concatenate([_images()[n].reshape(-1) for n in names])).to(DEV)
    table = torch.from_numpy(tab.view(np.uint8).reshape(tab.shape[0], len(names), 32)).to(DEV)
    return geoms, src, table


def test_lq_ragged_batch_equals_host_and_singles(host, singles):
    """all strips in ONE launch into a NaN-filled destination: the host's bits, the one-at-a-time bits, the whole canvas defined, -1 beyond dw"""
    geoms, src, table = _ragged(LQ_NAMES, False)
    out = torch.full((len(LQ_NAMES), 3, 32, 512), float("nan"), dtype=torch.float32, device=DEV)
    got = ops.lq_from_u8(src, table[0], 32, 512, out=out)
    assert got.data_ptr() == out.data_ptr()
    out = out.cpu()
    assert not bool(torch.isnan(out).any())
    for k, name in enumerate(LQ_NAMES):
        assert geoms[k].dw == host[name][1] and geoms[k].show_w == host[name][2]
        assert torch.equal(out[k:k + 1], host[name][0]), name
        assert torch.equal(out[k:k + 1], singles[name][0].cpu()), name
        assert bool((out[k, :, :, geoms[k].dw:] == -1.0).all()), name


def test_preview_ragged_batch_equals_host_and_singles(host, singles):
    geoms, src, table = _ragged(NAMES, True)
    wmax = max(g.show_w for g in geoms)
    assert wmax == 2049
    out = torch.full((len(NAMES), 128, wmax, 3), 0xCD, dtype=torch.uint8, device=DEV)
    ops.lq_from_u8(src, table[1], 128, wmax, preview=True, out=out)
    out = out.cpu().numpy()
    for k, name in enumerate(NAMES):
        sw = host[name][2]
        assert geoms[k].show_w == sw
        assert np.array_equal(out[k, :, :sw], host[name][3]), name
        assert np.array_equal(out[k, :, :sw], singles[name][1][0].cpu().numpy()), name
        assert not out[k, :, sw:].any(), name                              # 0 beyond the strip: the 0xCD fill is gone everywhere


def test_prepare_strips_batch_skips_too_wide_and_keeps_order(host):
    names = ["19x109", "251x1999", "real_lq13.png"]
    wide = np.zeros((33, 529, 3), np.uint8)
    batch = [_images()[names[0]], wide, _images()[names[1]], _images()[names[2]]]
    with pytest.raises(lq_io.StripTooWide):                                # the host path's error, unchanged, unless the caller asks to skip
        lq_device.prepare_strips(batch, DEV, preview=True)
    p = lq_device.prepare_strips(batch, DEV, preview=True, skip_too_wide=True)
    assert p.index == [0, 2, 3] and [i for i, _ in p.skipped] == [1] and isinstance(p.skipped[0][1], lq_io.StripTooWide)
    assert p.preview.shape[2] == max(host[n][2] for n in names)
    for k, n in enumerate(names):
        assert torch.equal(p.lq[k:k + 1].cpu(), host[n][0])
        assert np.array_equal(p.preview[k, :, :host[n][2]].cpu().numpy(), host[n][3])
    with pytest.raises(ValueError, match="empty output"):
        lq_device.prepare_strips([np.zeros((64, 1, 3), np.uint8)], DEV)
    empty = lq_device.prepare_strips([wide], DEV, skip_too_wide=True)
    assert empty.lq.shape == (0, 3, 32, 512) and empty.index == [] and len(empty.skipped) == 1



# heights and steps whose sample positions are NOT dyadic (at dst_h = 32 / 128 every product of the weights is exact, so a fused multiply-add
# would go unnoticed): (h, w, fx) -> resize_cubic(img, fx, fx); the kernel gets dst_h = rint(h fx), dw = rint(w fx), scale = 1 / fx
GENERAL = ((47, 61, 37 / 47), (100, 333, 0.37), (19, 109, 100 / 19), (53, 97, 1.7), (251, 640, 0.113), (7, 11, 3.3), (33, 200, 0.731))


@pytest.mark.parametrize("h,w,fx", GENERAL)
def test_any_height_and_step_equals_resize_cubic(h, w, fx):
    """mnet_lq_from_u8 takes any dst_h and any step: the uint8 form against lq_io.resize_cubic, the fp32 form against ToTensor + Normalize of it"""
    img = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    ref = lq_io.resize_cubic(img, fx, fx)
    dh, dw = ref.shape[:2]
    assert (dh, dw) == (int(np.rint(h * fx)), int(np.rint(w * fx)))
    canvas = dw + 3                                                        # a few fill columns, not a multiple of the tile
    tab = lq_device.build_table([lq_device.Geometry(h, w, dw, 1.0 / fx, dw, 1.0 / fx)], [1], False)      # odd offset
    src = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), img.reshape(-1)])).to(DEV)
    table = torch.from_numpy(tab.view(np.uint8).reshape(1, 1, 32)).to(DEV)
    u8 = ops.lq_from_u8(src, table[0], dh, canvas, preview=True).cpu().numpy()[0]
    assert np.array_equal(u8[:, :dw], ref) and not u8[:, dw:].any()
    f32 = ops.lq_from_u8(src, table[0], dh, canvas).cpu()[0]
    want = torch.from_numpy(u8.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255).sub_(0.5).div_(0.5)
    assert torch.equal(f32, want)


@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    return MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_restore_images_equals_restore_strips(pipe):
    """raw arrays + the text of the file names through restore_images == strip_from_png + restore_strips: the same uint8 SR rows and the same
    structure-prior rows; a strip with a character outside the alphabet and a strip wider than 512 px come back as None"""
    paths = [os.path.join(cases_png.PNG_DIR, f) for f in cases_png.SR_STRIPS.values()]
    strips = [lq_io.strip_from_png(p) for p in paths]
    want = pipe.restore_strips(strips, with_prior=True)
    images = [lq_io.load_png(p) for p in paths]
    texts = [lq_io.manual_text(p) for p in paths]
    got, det = pipe.restore_images([images[0], images[1], images[0], np.zeros((33, 529, 3), np.uint8)], texts=texts + ["a b", texts[0]],
                                   with_prior=True, details=True)
    assert got[2] is None and got[3] is None and det[3] is None and int(det[2]["labels"].min()) == -1
    for k in range(2):
        assert want[k] is not None and _same(got[k], want[k])
        assert got[k][0].dtype == np.uint8 and got[k][0].shape == (128, strips[k]["show_w"], 3)
        assert torch.equal(det[k]["lq"].cpu(), strips[k]["lq"]) and torch.equal(det[k]["labels"], strips[k]["labels"])
        assert torch.equal(det[k]["locs"], strips[k]["locs"]) and det[k]["show_w"] == strips[k]["show_w"] and det[k]["text"] == strips[k]["text"]
        assert np.array_equal(det[k]["show"], lq_io.show_lq(images[k]))
    plain = pipe.restore_images(images, texts=texts)
    assert all(np.array_equal(plain[k], want[k][0]) for k in range(2))


def test_restore_entry_points_skip_the_same_strips(pipe):
    """one batch through restore_images, restore_panels and restore_lines: a restorable strip, a text with a character outside the alphabet,
    an empty text, and a strip wider than 512 px at height 32 — which only restore_lines restores; the restorable strip's bytes agree"""
    from marconet_amd import long_lines
    name = cases_png.SR_STRIPS["lqe01"]
    strip, text = lq_io.load_png(os.path.join(cases_png.PNG_DIR, name)), lq_io.manual_text(name)[:3]
    wide = np.random.default_rng(5).integers(0, 256, (32, 600, 3), dtype=np.uint8)
    images, texts = [strip, strip, strip, wide], [text, text[0] + " ", "", text]
    assert len(text) == 3 and min(lq_io.labels_from_text(text)) >= 0 and min(lq_io.labels_from_text(texts[1])) == -1
    assert not long_lines.too_wide(*strip.shape[:2]) and long_lines.too_wide(*wide.shape[:2])
    singles, panels = pipe.restore_images(images, texts), pipe.restore_panels(images, texts)
    lines = pipe.restore_lines(images, texts, overlap_glyphs=1)              # 3 characters in windows of 2: one shared character
    show_w = lq_device.strip_geometry(strip).show_w
    assert singles[1:] == [None] * 3 and singles[0].dtype == np.uint8 and singles[0].shape == (128, show_w, 3)
    assert panels[1:] == [None] * 3 and panels[0].dtype == np.uint8 and panels[0].shape == (512, show_w, 3)
    assert lines[1] is None and lines[2] is None
    assert lines[3].dtype == np.uint8 and lines[3].shape[0] == 128 and abs(lines[3].shape[1] - 4 * 600) <= 1
    assert lines[0].dtype == np.uint8 and np.array_equal(lines[0], singles[0])


def test_restore_images_blind_equals_the_host_prepared_path(pipe):
    """texts=None: labels and locations from the encoder, as forward_blind's sources — the same bytes as the host-prepared strips give"""
    from marconet_amd.pipeline import clear_labels_batch, locs_from_left_right
    images = [lq_io.load_png(os.path.join(cases_png.PNG_DIR, f)) for f in cases_png.W_STRIPS]
    pre = [lq_io.lq_from_image(img) for img in images]
    with torch.no_grad():
        logits, locs_lr, _ = pipe.encoder(torch.cat([p[0] for p in pre]).to(DEV))
    labels, locs = clear_labels_batch(logits), locs_from_left_right(locs_lr).float().cpu()
    strips = []
    for k, p in enumerate(pre):
        lab = labels[k][:4]
        n = int(lab.shape[0])
        strips.append(dict(lq=p[0], labels=lab, locs=locs[k:k + 1, :2 * n].contiguous(), show_w=p[2]))
    live = [k for k, s in enumerate(strips) if s["labels"].numel() > 0]
    want = [None] * len(strips)
    for k, r in zip(live, pipe.restore_strips([strips[k] for k in live])):
        want[k] = r
    got = pipe.restore_images(images, max_glyphs=4)
    assert len(live) > 0
    for g, w in zip(got, want):
        assert (g is None and w is None) or np.array_equal(g, w)
