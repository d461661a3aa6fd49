#!/usr/bin/env python
"""The figures of DESIGN.md §6 "input side": host time per strip of lq_io.lq_from_image + lq_io.show_lq over the strips under tests/golden/pngs
(median of 7 passes after a warm-up pass), and the device path for a 256-strip batch of the same strips — lq_device.prepare_strips end to end
(host packing, both copies, launches; host clock around the call and a device synchronise, median of 20 after 3 warm-ups) and the kernels alone
(device events over 50 launches).  Prints one JSON document.  Needs the GPU:

    python tools/lq_prep_time.py
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from marconet_amd import lq_device, lq_io, ops
from tests.golden import cases_png

names = ("real_lq13.png",) + tuple(cases_png.SR_STRIPS.values()) + tuple(cases_png.W_STRIPS)
imgs = [lq_io.load_png(os.path.join(cases_png.PNG_DIR, f)) for f in names]
res = {"shapes": [list(i.shape) for i in imgs], "torch_threads": torch.get_num_threads()}
for img in imgs:                                   # warm-up
    lq_io.lq_from_image(img); lq_io.show_lq(img)
host = {n: {"lq": [], "show": []} for n in names}
for _ in range(7):
    for n, img in zip(names, imgs):
        t0 = time.perf_counter(); lq_io.lq_from_image(img); t1 = time.perf_counter(); lq_io.show_lq(img); t2 = time.perf_counter()
        host[n]["lq"].append((t1 - t0) * 1e3); host[n]["show"].append((t2 - t1) * 1e3)
res["host_ms_per_strip"] = {n: {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in d.items()} for n, d in host.items()}
res["host_ms_per_strip_mean_of_medians_lq_plus_show"] = float(np.mean([statistics.median(d["lq"]) + statistics.median(d["show"]) for d in host.values()]))

if not torch.cuda.is_available():
    raise SystemExit("lq_prep_time.py: no GPU visible - a time measured without one says nothing about the device path")
dev = "cuda"
batch = [imgs[i % len(imgs)] for i in range(256)]
for preview in (False, True):
    for _ in range(3):
        p = lq_device.prepare_strips(batch, dev, preview=preview); torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        p = lq_device.prepare_strips(batch, dev, preview=preview)
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    res["device_256_strips_ms_end_to_end_preview_%s" % preview] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
# kernel alone (pixels and table already on the device), device events
geoms = [lq_device.strip_geometry(i) for i in batch]
offs = [int(v) for v in np.cumsum([0] + [g.h * g.w * 3 for g in geoms[:-1]])]
tab = lq_device.build_table(geoms, offs, True)
src = torch.from_numpy(np.concatenate([i.reshape(-1) for i in batch])).to(dev)
table = torch.from_numpy(tab.view(np.uint8).reshape(2, 256, 32)).to(dev)
res["packed_bytes"] = int(src.numel())
wmax = max(g.show_w for g in geoms)
for label, args, kw in (("lq", (table[0], 32, 512), {}), ("preview", (table[1], 128, wmax), {"preview": True})):
    out = ops.lq_from_u8(src, *args, **kw)
    for _ in range(5):
        ops.lq_from_u8(src, *args, out=out, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        ops.lq_from_u8(src, *args, out=out, **kw)
    e1.record(); torch.cuda.synchronize()
    res["kernel_ms_256_strips_%s" % label] = e0.elapsed_time(e1) / 50
    res["out_bytes_%s" % label] = int(out.numel() * out.element_size())
print(json.dumps(res, indent=1))
