#!/usr/bin/env python
"""The figures of DESIGN.md §6 "precision margin guard":

    kernel     mnet_compare_stats on a 128-glyph prior64 pair (fp16+8 [128,64,64,256] against split half, one group per glyph): achieved bytes/s —
               both tensors' storage bytes once over the time of the two launches (device events) — next to mnet_nonfinite_flag's rate over the
               SAME number of bytes (an fp32 tensor: it reads no blocked storage) in the same process, rounds alternated
    calibrate  MarconetPipeline.calibrate on ``--strips`` strips x ``--glyphs`` glyphs (host clock, a device synchronise before and after; its
               one device→host copy included) next to the sum of the two plain forward_batch calls it contains (the configured mode, then the
               reference mode via set_precision), runs alternated, median of ``--passes`` after one warm-up pass

Seeded synthetic weights and inputs.  Prints one JSON document.  Needs the GPU:

    python tools/compare_time.py [--strips 8] [--glyphs 16] [--passes 5] [--precision fp16x2] [--reference fp16x3]
"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from marconet_amd import checkpoints, ops, synthetic
from marconet_amd.packing import MX_DTYPE, SPLIT_DTYPE
from marconet_amd.pipeline import MarconetPipeline

ap = argparse.ArgumentParser()
ap.add_argument("--strips", type=int, default=8)
ap.add_argument("--glyphs", type=int, default=16)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--precision", default="fp16x2")
ap.add_argument("--reference", default="fp16x3")
ap.add_argument("--kernel-glyphs", type=int, default=128)
ap.add_argument("--kernel-iters", type=int, default=50)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("compare_time.py: no GPU visible - a time measured without one says nothing about the device path")
dev = "cuda"
stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
res = {"precision": a.precision, "reference": a.reference, "passes": a.passes}

# ---- the kernel alone
G = a.kernel_glyphs
g = torch.Generator(device=dev).manual_seed(1)
x = torch.randn((G, 64, 64, 256), device=dev, generator=g)
pm, pr = ops.convert(x, MX_DTYPE), ops.convert((x + 1e-4 * torch.randn(x.shape, device=dev, generator=g)).contiguous(), SPLIT_DTYPE)
nbytes = 2 * x.numel() * 4
flat = torch.randn((nbytes // 4,), device=dev, generator=g)          # the finiteness flag over the same number of bytes
flag = torch.empty((1,), dtype=torch.int32, device=dev)
del x


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


for _ in range(3):
    ops.compare_stats(pm, pr); ops.nonfinite_flag(flat, out=flag)
torch.cuda.synchronize()
tc, tf = [], []
for _ in range(a.passes):
    tc.append(timed(lambda: ops.compare_stats(pm, pr), a.kernel_iters))
    tf.append(timed(lambda: ops.nonfinite_flag(flat, out=flag), a.kernel_iters))
res["kernel"] = {"shape": [G, 64, 64, 256], "pair": "fp16+8 vs split half", "groups": G, "bytes": nbytes, "iters": a.kernel_iters,
                 "compare_stats_ms": stat(tc), "compare_stats_GBps": nbytes / statistics.median(tc) / 1e6,
                 "nonfinite_flag_ms": stat(tf), "nonfinite_flag_GBps": nbytes / statistics.median(tf) / 1e6,
                 "note": "compare_stats: partial + fold launch and the wrapper's two allocations; nonfinite_flag: memset + one launch, fp32 tensor of the same bytes"}
del pm, pr, flat

# ---- calibrate next to the two forwards it contains
sde, sdg, sds, source = checkpoints.load_state_dicts("")
pipe = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, dev), precision=a.precision)
B, n = a.strips, a.glyphs
lq = synthetic.make_lq(151, B, [512] * B).to(dev)
labels = [synthetic.make_labels(160 + b, n) for b in range(B)]
locs = synthetic.make_locs([n] * B, [512] * B, max_glyphs=n)


def t_calibrate():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    rep = pipe.calibrate(lq, labels, locs, reference=a.reference, max_strips=B)
    torch.cuda.synchronize()
    return rep, (time.perf_counter() - t0) * 1e3


def t_forwards():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    pipe.forward_batch(lq, labels, locs)
    pipe.set_precision(a.reference)
    pipe.forward_batch(lq, labels, locs)
    pipe.set_precision(a.precision)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


rep, _ = t_calibrate(); t_forwards()                 # warm-up: weights packed in both modes, kernels loaded
cal, fwd = [], []
for _ in range(a.passes):
    cal.append(t_calibrate()[1]); fwd.append(t_forwards())
res["calibrate"] = {"strips": B, "glyphs_per_strip": n, "weights": source, "calibrate_ms": stat(cal), "two_forward_batch_ms": stat(fwd),
                    "report_ok": rep.ok, "sr_max_abs_diff": rep.sr.max_abs_diff, "report": str(rep).splitlines()}
print(json.dumps(res, indent=1))
