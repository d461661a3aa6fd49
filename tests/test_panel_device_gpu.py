"""-m gpu: the device panel path (mnet_panel_u8, marconet_amd/panel_device.py, MarconetPipeline.restore_panels, examples/restore_strips.py
--device-panel) against the pure-host definition lq_io.panel_rgb_u8(lq_io.panel(...)) — bit for bit: every comparison is np.array_equal.  The
host references of the kernel tests are computed once per module."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from marconet_amd import lq_io, ops, panel_device
from tests.golden import cases_png

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (characters, show_w): one column; the identity width; a strong shrink; one column past a tile edge; enlarging (both border clamps);
# a width that is no multiple of anything; the full canvas
STRIPS = ((1, 1), (1, 128), (3, 37), (16, 65), (2, 700), (5, 641), (16, 2048))
GUARD = 4096


def _locs(rng, n, show_w, k):
    loc = np.empty(2 * n, np.float32)
    loc[0::2] = rng.uniform(-0.02, 1.05, n) * (show_w / 2048)
    loc[1::2] = rng.uniform(0.0, 0.03, n)
    if k == 4:
        loc[:4] = (-0.002, 0.0005, 1.2, 0.1)            # the negative-stop wrap (red on columns 0..show_w-4) and an edge beyond 2048
    if k == 3:
        loc[:6] = (66 / 2048, 2 / 2048, -0.5, 0.1, 0.0, 0.0)   # an edge at show_w; all left of the canvas; zero half-width at column 0
    return loc


@pytest.fixture(scope="module")
def data():
    """inputs on the host and on the device + the host panels, computed once and left unchanged"""
    rng = np.random.default_rng(20240611)
    n = len(STRIPS)
    counts, show_w = [c for c, _ in STRIPS], [w for _, w in STRIPS]
    G = sum(counts)
    preview = rng.integers(0, 256, (n, 128, 2048, 3), dtype=np.uint8)          # the columns beyond show_w are random too: they must not show
    sr = rng.integers(0, 256, (n, 128, 2048, 3), dtype=np.uint8)
    prior = rng.uniform(-1.0, 1.0, (G, 128, 128, 4)).astype(np.float32)
    special = np.float32([1.0, -1.0, 0.0, -0.0, 1e-40, -1e-40, np.float32(2.0 ** -149), 1.0 - 2.0 ** -24, -1.0 + 2.0 ** -24, 1 / 255, -1 / 255])
    flat = prior.reshape(-1)
    flat[rng.choice(flat.size, 40000, replace=False)] = rng.choice(special, 40000)
    prior[:, :, :, 3] = np.nan                                                  # the fourth float of a pixel is padding: never read into a result
    prior[:, :, 0, :3] = np.float32(1.0)                                        # the left and right columns of every image: the border clamps
    prior[:, :, 127, :3] = np.float32(-1.0)                                     # land on exact 1.0 → 255 and 0.0 → 0
    locs = [_locs(rng, c, w, k) for k, (c, w) in enumerate(STRIPS)]
    want, g = [], 0
    for k in range(n):
        p = prior[g:g + counts[k], :, :, :3] * np.float32(0.5) + np.float32(0.5)                       # test_sr.py:208
        prior128 = p.transpose(1, 0, 2, 3).reshape(128, 128 * counts[k], 3)                           # :209-211
        assert prior128.dtype == np.float32
        want.append(lq_io.panel_rgb_u8(lq_io.panel(None, locs[k], counts[k], sr[k], prior128, show=preview[k, :, :show_w[k]])))
        assert want[-1].shape == (512, show_w[k], 3)
        g += counts[k]
    red = (want[4][128:192] == (255, 0, 0)).all(axis=(0, 2))
    assert red[:697].all() and not red[697:].any()                             # the wrap case is in the data
    dev = dict(preview=torch.from_numpy(preview).to(DEV), sr=torch.from_numpy(sr).to(DEV), prior=torch.from_numpy(prior).to(DEV))
    return dict(counts=counts, show_w=show_w, locs=locs, want=want, starts=[int(v) for v in np.cumsum([0] + counts[:-1])], **dev)


def _launch(d, sel, out_w, preview=None, index=None):
    """the strips ``sel`` of the data in one launch into a guarded destination → (host result [len(sel),512,out_w,3], the two guards)"""
    counts, show_w = [d["counts"][k] for k in sel], [d["show_w"][k] for k in sel]
    gsel = [g for k in sel for g in range(d["starts"][k], d["starts"][k] + d["counts"][k])]
    prior = d["prior"] if gsel == list(range(d["prior"].shape[0])) else d["prior"][torch.tensor(gsel, device=DEV)].contiguous()
    sr = d["sr"][torch.tensor(sel, device=DEV)].contiguous()
    tab, marks = panel_device.build_tables(sel if index is None else index, show_w, counts, [d["locs"][k] for k in sel])
    strips_d = torch.from_numpy(tab.view(np.uint8).reshape(len(sel), 24)).to(DEV)
    size = len(sel) * 512 * out_w * 3
    buf = torch.full((size + 2 * GUARD,), 0xCD, dtype=torch.uint8, device=DEV)
    out = buf[GUARD:GUARD + size].view(len(sel), 512, out_w, 3)
    got = ops.panel_u8(d["preview"] if preview is None else preview, sr, prior, strips_d, torch.from_numpy(marks).to(DEV), out_w=out_w, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    return host[GUARD:GUARD + size].reshape(len(sel), 512, out_w, 3), (host[:GUARD], host[GUARD + size:])


def _check(d, sel, got, guards):
    for j, k in enumerate(sel):
        w = d["show_w"][k]
        assert np.array_equal(got[j, :, :w], d["want"][k]), STRIPS[k]
        assert not got[j, :, w:].any(), STRIPS[k]                                # 0 beyond the strip: the 0xCD fill is gone everywhere
    assert all((g == 0xCD).all() for g in guards)


def test_panel_batch_equals_host(data):
    """all strips in ONE launch: the host's bytes, 0 at the columns >= show_w, the guards around dst untouched"""
    sel = list(range(len(STRIPS)))
    _check(data, sel, *_launch(data, sel, 2048))


def test_panel_batch_whose_width_is_no_multiple_of_the_tile(data):
    """out_w = 65 (preview_w stays 2048): the last tile has one live column"""
    sel = [0, 2, 3]
    assert max(data["show_w"][k] for k in sel) == 65
    _check(data, sel, *_launch(data, sel, 65))


def test_panel_with_permuted_preview_index(data):
    """the previews in another order than the strips (skipped strips leave such gaps): preview_index is followed"""
    sel = list(range(len(STRIPS)))
    perm = [3, 0, 6, 1, 5, 2, 4]                                                  # strip k's preview lives at row perm[k]
    shuffled = torch.empty_like(data["preview"])
    shuffled[torch.tensor(perm, device=DEV)] = data["preview"]
    _check(data, sel, *_launch(data, sel, 2048, preview=shuffled, index=perm))


def test_panel_is_batch_invariant(data):
    """each strip alone (its own descriptor, glyph0 = 0) gives the bytes it gives inside the batch"""
    sel = list(range(len(STRIPS)))
    batch, _ = _launch(data, sel, 2048)
    for k in sel:
        w = data["show_w"][k]
        alone, guards = _launch(data, [k], w, index=[k])
        assert np.array_equal(alone[0], batch[k, :, :w]), STRIPS[k]
        assert all((g == 0xCD).all() for g in guards)


def test_compose_panels_equals_host_and_refuses_2050(data):
    """compose_panels (tables built and copied here, one launch): the host's bytes; show_w = 2050 > the SR width raises before any launch"""
    out = panel_device.compose_panels(data["preview"], list(range(len(STRIPS))), data["show_w"], data["sr"], data["prior"], data["counts"], data["locs"])
    assert out.shape == (len(STRIPS), 512, 2048, 3) and out.dtype == torch.uint8 and out.is_cuda
    _check(data, list(range(len(STRIPS))), out.cpu().numpy(), ())
    wide = torch.zeros((1, 128, 2050, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="strip 0 is 2050 px wide"):
        panel_device.compose_panels(wide, [0], [2050], data["sr"][:1], data["prior"][:1], [1], [np.float32([0.5, 0.1])])


# ---------------------------------------------------------------------------------------------------------------- through the networks
@pytest.fixture(scope="module")
def pipe(ckpts):
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    return MarconetPipeline(*checkpoints.build_networks(ckpts[0], ckpts[1], ckpts[2], DEV), precision="fp32")


def _host_panels(pipe, images, texts, **kw):
    """the panels built on the host from restore_images(with_prior=True, details=True), as examples/restore_strips.py --device-prep builds them"""
    res, det = pipe.restore_images(images, texts=texts, with_prior=True, details=True, **kw)
    out = []
    for r, s in zip(res, det):
        if r is None:
            out.append(None)
            continue
        show_sr, prior128 = r
        out.append(lq_io.panel_rgb_u8(lq_io.panel(None, s["locs"][0], int(s["labels"].shape[0]), show_sr, prior128, show=s["show"])))
    return out, det


def _batch():
    names = sorted(os.listdir(cases_png.PNG_DIR))
    images = [lq_io.load_png(os.path.join(cases_png.PNG_DIR, f)) for f in names]
    texts = [lq_io.manual_text(f) for f in names]
    sr_names = list(cases_png.SR_STRIPS.values())
    first = images[names.index(sr_names[0])]
    images += [first, np.zeros((33, 529, 3), np.uint8), first]                   # a character outside the alphabet (the blank); too wide; no character
    texts += ["a b", texts[names.index(sr_names[0])], ""]
    return names, images, texts


def test_restore_panels_equals_the_host_panels(pipe):
    """raw strips + texts: restore_panels == the host panels, byte for byte; None where restore_images gives None"""
    names, images, texts = _batch()
    want, det = _host_panels(pipe, images, texts)
    got, strips = pipe.restore_panels(images, texts, details=True)
    live = [i for i, w in enumerate(want) if w is not None]
    assert live == list(range(len(names)))                                                # every strip of the directory gives a panel
    assert want[-3] is None and want[-2] is None and want[-1] is None and det[-2] is None and strips[-2] is None
    assert len(got) == len(images)
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, i
            continue
        assert g.dtype == np.uint8 and g.shape == (512, det[i]["show_w"], 3) and np.array_equal(g, w), i
        assert strips[i]["text"] == texts[i] and strips[i]["show_w"] == det[i]["show_w"]
    plain = pipe.restore_panels(images, texts)
    assert all((p is None and w is None) or np.array_equal(p, w) for p, w in zip(plain, want))


def test_restore_panels_blind_equals_the_host_panels(pipe):
    """texts=None: labels and locations from the encoder itself, as restore_images takes them"""
    _, images, _ = _batch()
    images = images[:-1]
    want, _ = _host_panels(pipe, images, None, max_glyphs=4)
    got = pipe.restore_panels(images, max_glyphs=4)
    assert sum(w is not None for w in want) > 0 and want[-1] is None
    for g, w in zip(got, want):
        assert (g is None and w is None) or (g.shape == w.shape and np.array_equal(g, w))


def test_example_script_device_panel_writes_the_host_panels(tmp_path):
    """examples/restore_strips.py -m --device-panel on the reference's own strips: per strip a PNG under the script's file name whose decoded
    pixels are the host panel computed in this process"""
    from marconet_amd import checkpoints
    from marconet_amd.pipeline import MarconetPipeline
    out = str(tmp_path / "panels")
    env = dict(os.environ)
    env.pop("MARCONET_CKPT_DIR", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "restore_strips.py"), "-i", cases_png.PNG_DIR, "-o", out, "-m", "--device-panel",
                        "--precision", "fp32"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    sde, sdg, sds, _ = checkpoints.load_state_dicts("")
    p = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, DEV), precision="fp32")
    names = sorted(os.listdir(cases_png.PNG_DIR))                                # every strip of the directory, as the script lists them
    images = [lq_io.load_png(os.path.join(cases_png.PNG_DIR, f)) for f in names]
    texts = [lq_io.manual_text(f) for f in names]
    want, _ = _host_panels(p, images, texts)
    assert len(names) >= 2 and all(w is not None for w in want)
    assert sorted(os.listdir(out)) == sorted("%s_%s.png" % (os.path.splitext(f)[0], t) for f, t in zip(names, texts)), r.stdout[-1500:]
    for f, t, w in zip(names, texts, want):
        assert np.array_equal(lq_io.load_png(os.path.join(out, "%s_%s.png" % (os.path.splitext(f)[0], t))), w), f
