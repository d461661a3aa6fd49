#!/usr/bin/env python
"""The figures of DESIGN.md §6 "output side": for ONE batch of strips (the two labelled strips under tests/golden/pngs, repeated; seeded synthetic
weights), the time from raw strips to the saved panels' pixels

    host panels    MarconetPipeline.restore_images(with_prior=True, details=True) + lq_io.panel + lq_io.panel_rgb_u8 per strip
                   (what examples/restore_strips.py --device-prep does before it encodes), and the per-strip panel part of it alone
    device panels  MarconetPipeline.restore_panels on the same batch (examples/restore_strips.py --device-panel)

— host clock around the call, a device synchronise before and after, median of ``--passes`` after one warm-up pass — and the panel kernel alone
(device events).  Prints one JSON document.  Needs the GPU:

    python tools/panel_time.py [--batch 256] [--passes 3] [--precision fp16x2]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from marconet_amd import checkpoints, lq_io, panel_device
from marconet_amd.pipeline import MarconetPipeline
from tests.golden import cases_png

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--precision", default="fp16x2")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("panel_time.py: no GPU visible - a time measured without one says nothing about the device path")
dev = "cuda"
names = list(cases_png.SR_STRIPS.values())
imgs = [lq_io.load_png(os.path.join(cases_png.PNG_DIR, f)) for f in names]
images = [imgs[i % len(imgs)] for i in range(a.batch)]
texts = [lq_io.manual_text(names[i % len(names)]) for i in range(a.batch)]
sde, sdg, sds, source = checkpoints.load_state_dicts("")
pipe = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, dev), precision=a.precision)
res = {"batch": a.batch, "glyphs": sum(len(t) for t in texts), "precision": a.precision, "weights": source, "passes": a.passes,
       "strip_shapes": [list(i.shape) for i in imgs], "torch_threads": torch.get_num_threads()}


def host_panels():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out, det = pipe.restore_images(images, texts=texts, with_prior=True, details=True)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    panels = [lq_io.panel_rgb_u8(lq_io.panel(None, s["locs"][0], int(s["labels"].shape[0]), r[0], r[1], show=s["show"])) for r, s in zip(out, det)]
    t2 = time.perf_counter()
    return panels, (t2 - t0) * 1e3, (t2 - t1) * 1e3


def device_panels():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    panels = pipe.restore_panels(images, texts=texts)
    torch.cuda.synchronize()
    return panels, (time.perf_counter() - t0) * 1e3


want, _, _ = host_panels()                           # warm-up passes: weights packed, kernels loaded; and the two paths agree
got, _ = device_panels()
res["device_equals_host"] = bool(all(np.array_equal(g, w) for g, w in zip(got, want)))
res["panel_bytes"] = int(sum(w.size for w in want))
host, part, devt = [], [], []
for _ in range(a.passes):
    _, t, p = host_panels(); host.append(t); part.append(p)
    _, t = device_panels(); devt.append(t)
stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
res["host_panels_ms_per_batch"] = stat(host)
res["host_panels_ms_per_batch_panel_part_alone"] = stat(part)
res["device_panels_ms_per_batch"] = stat(devt)

# the kernel alone: everything on the device already (random previews / SR / structure images of the batch's shapes)
counts, show_w = [len(t) for t in texts], [w.shape[1] for w in want]
g = torch.Generator(device=dev).manual_seed(1)
preview = torch.randint(0, 256, (a.batch, 128, max(show_w), 3), dtype=torch.uint8, device=dev, generator=g)
sr = torch.randint(0, 256, (a.batch, 128, 2048, 3), dtype=torch.uint8, device=dev, generator=g)
prior = torch.rand((sum(counts), 128, 128, 4), device=dev, generator=g) * 2 - 1
locs = [lq_io.locs_from_boxes(lq_io.evenly_spaced_boxes(c, 100, 20), 20)[0] for c in counts]
for _ in range(3):
    panel_device.compose_panels(preview, list(range(a.batch)), show_w, sr, prior, counts, locs)
torch.cuda.synchronize()
from marconet_amd import ops
tab, marks = panel_device.build_tables(list(range(a.batch)), show_w, counts, locs)
strips_d = torch.from_numpy(tab.view(np.uint8).reshape(a.batch, tab.dtype.itemsize)).to(dev)
marks_d = torch.from_numpy(marks).to(dev)
out = ops.panel_u8(preview, sr, prior, strips_d, marks_d, out_w=max(show_w))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    ops.panel_u8(preview, sr, prior, strips_d, marks_d, out_w=max(show_w), out=out)
e1.record(); torch.cuda.synchronize()
res["kernel_ms_per_batch"] = e0.elapsed_time(e1) / 20
res["kernel_out_bytes"] = int(out.numel())
print(json.dumps(res, indent=1))
