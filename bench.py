#!/usr/bin/env python
"""bench.py — SR images/sec of the MARCONet hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one pass of the whole hot path (ResNet-45 + TextViT encoder → TSPGAN over all glyphs → TSPSRNet) over one
batch of synthetic 32x512 LR strips per GPU — by default the configuration BASELINE.json's metric is quoted on: batch 256
per GPU, 16 glyphs per image, inputs resident in HBM, random-init seeded checkpoints of the reference's exact architecture.
The headline is measured in the fastest precision mode that MEETS the north-star parity bar (<= 1e-3 max-abs vs the reference's
CPU forward, character indices bit-exact): "fp16x2" — fp16+8 storage, every multiply evaluated as hi*hi on the fp16 MFMA plus
one block-scaled fp8 MFMA for both correction products, fp32 accumulation.
(`--batch 64` is BASELINE configs[1]; `--gpus 8 --batch 128` is configs[2].)  N>1: weak scaling, every rank processes its
own batch and the post-processed SR outputs (uint8 BGR, test_sr.py:198-200) are all-gathered over RCCL — the one collective
of the path.  Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set-up, --warmup steps, --steps timed steps, the outputs of the last timed step when
--dump-outputs DIR is given, and the line (`value`, `ms_per_step` and the configuration; `roofline` and `secondary` are null).
--dump-outputs DIR: rank 0 writes the arrays its last timed step returned as DIR/<name>.npy in float32; above 64 MB in all, a fixed seeded
sample of whole images (their indices in DIR/<name>_index.npy).  Inputs and weights are seeded, so two builds can be compared file for file.

--full adds everything else, after the timed steps: the roofline of the dominant kernel (a separate instrumented pass), and at N = 1 the
CPU baseline and "parity" (the oracle comparison, also of the TIMED batch itself: one strip per generator chunk, with and without the
generator's structure image, on TWO weight regimes — marconet_amd/synthetic.py: "tame" and "trained"-like — or on the reference's real
checkpoints when MARCONET_CKPT_DIR holds them, marconet_amd/checkpoints.py).  For the default config it also times, under "secondary", the
split-half mode fp16x3 (three f16 products, fp32-class accuracy), the plain fp16 storage mode (2x faster, ~1e-2 deviation), the exact
fp32 mode, and BASELINE configs[1] (batch 64), configs[3] (TSPGAN alone) and configs[4] (mixed widths) under "secondary.configs", each with
the roofline fraction of its dominant kernel and a parity sample.

Other BASELINE configs as stand-alone lines, each with its own roofline of its dominant kernel:
    --config gan     configs[3]: the test_w.py StyleGAN-prior path alone — 256 x 16 = 4096 glyphs of 128x128 through TSPGAN
    --config mixed   configs[4]: strips of content width 128..512 bucketed by padded width (MarconetPipeline.forward_mixed_widths),
                     work-balanced over the ranks for N>1
"""
import argparse
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F16_TFLOPS = 2500.0       # MI355X dense fp16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3        # fp32 matrix (v_mfma_f32_16x16x4_f32)
PEAK_F16X3_TFLOPS = PEAK_F16_TFLOPS / 3.0    # split-precision: three fp16 MFMA products per algorithmic product
PEAK_F16X2_TFLOPS = PEAK_F16_TFLOPS / 2.0    # fp16+8: one fp16 MFMA product + both corrections as one fp8 MFMA (twice the rate, twice the k): 2 units
GF_RESNET, GF_VIT, GF_SR_TRUNK = 108.01, 3.69, 484.12     # GFLOP / image
GF_GAN, GF_SR_PRIOR = 41.78, 47.25                         # GFLOP / glyph
GF_F16_FIXED = GF_RESNET + GF_SR_TRUNK
GF_F16_PER_GLYPH = GF_GAN + GF_SR_PRIOR
GF_GAN_IMAGE_LEVEL = 232.0 / 16.0                          # GFLOP / glyph of TSPGAN's 128-px level (232 of 668 GF per 16 glyphs): feeds only the structure image

# kernel id (mnet_conv2d_plan) → name as it appears in rocprofv3's kernel trace
KNAME = {1: "conv_igemm_kernel (register-staged)", 3: "conv_skinny_f32_kernel", 16: "conv_dma_kernel<256,256,4,4,2,16>", 17: "conv_dma_kernel<256,128,4,2,3,16>",
         18: "conv_dma_kernel<128,256,2,4,3,16>", 19: "conv_dma_kernel<64,256,1,8,3,16>", 20: "conv_dma_kernel<128,512,2,8,2,16>",
         21: "conv_dma_kernel<64,512,1,8,2,16>", 22: "conv_dma_kernel<256,256,2,4,2,16>", 26: "conv_dma_kernel<128,128,2,4,4,16>",
         24: "conv_dma_kernel<256,256,4,4,2,16,spread>", 25: "conv_dma_kernel<128,512,2,8,2,16,spread>",
         64: "conv_dma_kernel<256,256,2,4,2,16,spread,pipe>", 65: "conv_dma_kernel<128,512,2,4,2,16,spread,pipe>",
         32: "conv_strip_kernel<256,256,4,4>", 33: "conv_strip_kernel<64,512,1,8>", 34: "conv_strip_kernel<128,256,2,4>"}
KNAME_X3 = {33: "conv_strip_kernel<64,512,1,8,x3>", 22: "conv_dma_kernel<256,256,2,4,2,16>", 23: "conv_dma_kernel<128,512,2,4,2,16>",      # split-half ids 6 / 7: the 8-wave tiles
            24: "conv_dma_kernel<256,256,2,4,2,16,spread>", 25: "conv_dma_kernel<128,512,2,4,2,16,spread>",
            27: "conv_dma_kernel<256,256,2,4,2,16,spread,pipe>", 28: "conv_dma_kernel<128,512,2,4,2,16,spread,pipe>"}
KNAME_X2 = {16: "conv_dma_kernel<256,256,4,4,2,32,mx>", 17: "conv_dma_kernel<256,128,4,2,3,32,mx>", 18: "conv_dma_kernel<128,256,2,4,3,32,mx>",
            19: "conv_dma_kernel<64,256,1,8,3,32,mx>", 20: "conv_dma_kernel<128,512,2,8,2,32,mx>", 21: "conv_dma_kernel<64,512,1,8,2,32,mx>",
            22: "conv_dma_kernel<256,256,2,4,2,32,mx>", 23: "conv_dma_kernel<128,512,2,4,2,32,mx>", 24: "conv_dma_kernel<128,512,1,8,2,32,mx>",
            26: "conv_dma_kernel<128,128,2,4,4,32,mx>", 27: "conv_dma_kernel<256,256,2,4,2,32,mx,pipe>", 28: "conv_dma_kernel<128,512,1,8,2,32,mx,pipe>",
            29: "conv_dma_kernel<64,512,1,8,2,32,mx,pipe>", 31: "conv_dma_kernel<256,256,2,4,2,32,mx,swp>", 25: "conv_dma_kernel<128,512,1,8,2,32,mx,swp>",
            32: "conv_strip_kernel<256,256,2,4,mx>", 33: "conv_strip_kernel<64,512,1,8,mx>", 64: "conv_dma_w4_kernel"}
DTNAME = {0: "f32", 1: "f16", 2: "f16x3", 3: "f16x2"}
MFMA_UNITS = {0: 1.0, 1: 1.0, 2: 3.0, 3: 2.0}      # fp16-MFMA-equivalent time units per algorithmic product


def kname(kid, dt):
    return (KNAME_X3.get(kid) if dt == 2 else KNAME_X2.get(kid) if dt == 3 else None) or KNAME.get(kid, str(kid))

DTPEAK = {0: PEAK_F32_TFLOPS, 1: PEAK_F16_TFLOPS, 2: PEAK_F16X3_TFLOPS, 3: PEAK_F16X2_TFLOPS}
PDT = {"fp32": 0, "fp16": 1, "fp16x3": 2, "fp16x2": 3}
# sources whose content decides the dominant kernel's HBM traffic: the PMC figure in profiles/pmc_traffic.json is reported
# only while these files are the ones it was measured on (else it is stale and `traffic` is null)
KERNEL_SOURCES = ["marconet_amd/csrc/conv_igemm_dma.hip", "marconet_amd/csrc/conv_dma_w4.hip", "marconet_amd/csrc/conv_dma_common.h", "marconet_amd/csrc/conv_args.h"]


def kernel_sources_sha():
    h = hashlib.sha256()
    for f in KERNEL_SOURCES:
        with open(os.path.join(ROOT, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="sr", choices=["sr", "gan", "mixed"], help="sr: the headline path; gan: configs[3]; mixed: configs[4]")
    ap.add_argument("--batch", type=int, default=256, help="images per GPU (the metric's batch 256; configs[1]: 64; configs[2]: 128 on 8 GPUs)")
    ap.add_argument("--glyphs", type=int, default=16, help="glyphs per image (SURVEY.md §8d: n=16)")
    ap.add_argument("--precision", default="fp16x2", choices=["fp16x2", "fp16x3", "fp16", "fp32"],
                    help="fp16x2 (default): fp16+8 storage, x*w = hi*hi on the f16 MFMA + one block-scaled fp8 MFMA for both correction products — "
                         "the fastest mode that meets the 1e-3 parity bar; fp16x3: split-half storage (three f16 MFMA products, fp32-class accuracy); "
                         "fp16: BASELINE configs[1]'s storage type (secondary figure with its measured deviation); fp32: exact fp32 MFMA")
    ap.add_argument("--force-gather", action="store_true", help="N=1: initialise an RCCL process group of one rank and run the output "
                                                                 "all-gather inside the timed region anyway (its cost is reported)")
    ap.add_argument("--cpu-images", type=int, default=4, help="images timed on the host CPU oracle (0 = skip); ~3.5 s each on 32 threads")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary throughput measurements")
    ap.add_argument("--secondary-steps", type=int, default=3, help="timed steps of every secondary measurement (the headline uses --steps)")
    ap.add_argument("--glyph-chunk", type=int, default=0, help="glyphs per TSPGAN call inside the batched driver (0: MarconetPipeline's default, 1024)")
    ap.add_argument("--no-regimes", action="store_true", help="skip the parity sample on the trained-like weight regime")
    ap.add_argument("--cpu-threads", type=int, default=32, help="cap on host threads for the CPU baseline")
    ap.add_argument("--no-gather", action="store_true")
    ap.add_argument("--dry", action="store_true", help="plumbing check without a GPU: gloo process group, a stand-in forward (a deterministic function of each image "
                                                       "alone) through the same launch / shard / overlapped all-gather / barrier + max-over-ranks timing / JSON code; "
                                                       "the line says \"dry\": true and carries no throughput claim (tests/test_bench_launch.py)")
    ap.add_argument("--gather-format", default="u8", choices=["u8", "f32"], help="N>1: what is all-gathered — the post-processed uint8 BGR image (0.75 MiB/img) or the fp32 NCHW tensor (3 MiB/img)")
    ap.add_argument("--full", action="store_true", help="after the headline: roofline pass, secondary measurements, CPU baseline and parity "
                                                        "(--cpu-images, --no-secondary, --secondary-steps and --no-regimes shape these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the outputs of the last timed step (rank 0) as DIR/<name>.npy, float32, "
                                                                        "at most 64 MB in all (a fixed seeded sample of whole images above that)")
    return ap.parse_args()


DUMP_BYTES = 64 * 10 ** 6      # --dump-outputs: every file together, .npy headers included
DUMP_SEED = 20240601


def dump_outputs(d, name, images):
    """--dump-outputs: ``images`` — one tensor indexed by image (or glyph) along dim 0, or a list of per-image tensors of different shapes —
    → float32 <d>/<name>.npy (a list: <d>/<name>_<index>.npy per image) and the indices written, float64, in <d>/<name>_index.npy.  When all
    of them exceed DUMP_BYTES, whole images are taken in one fixed seeded order until the budget is reached, so every run writes the same ones."""
    os.makedirs(d, exist_ok=True)
    n = len(images)
    nbytes = [images[i].numel() * 4 for i in range(n)]
    keep = list(range(n))
    budget = DUMP_BYTES - (1 << 16)           # headers and the index file
    if sum(nbytes) > budget:
        keep, total = [], 0
        for i in torch.randperm(n, generator=torch.Generator().manual_seed(DUMP_SEED)).tolist():
            if total + nbytes[i] > budget:
                break
            keep.append(i)
            total += nbytes[i]
        keep.sort()
    import numpy as np
    if isinstance(images, torch.Tensor):
        idx = torch.tensor(keep, dtype=torch.long, device=images.device)
        np.save(os.path.join(d, name + ".npy"), images.index_select(0, idx).float().cpu().numpy())
    else:
        for i in keep:
            np.save(os.path.join(d, "%s_%04d.npy" % (name, i)), images[i].float().cpu().numpy())
    np.save(os.path.join(d, name + "_index.npy"), np.asarray(keep, dtype=np.float64))
    return keep


def host_threads(cap):
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return max(1, min(avail, cap))


def timed(step, fence, steps, world, dev):
    import torch.distributed as dist
    fence()
    t0 = time.perf_counter()
    y = None
    for _ in range(steps):
        y = step()
    fence()
    dt = time.perf_counter() - t0
    per_rank = [dt]
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        allt = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        per_rank = [float(v.item()) for v in allt]
        dt = max(per_rank)
    return dt, per_rank, y


def conv_roofline(ops, steps, alg_gf_step, prefer_dtype, batch=None, precision=None):
    """roofline of the dominant conv kernel from the live HIP events of the timed steps (events are recorded on the launch
    stream around every conv launch; the kernel each launch resolved to comes from mnet_conv2d_plan)"""
    per = {}
    for s_, e_, fl, dt_, kid in ops.stats.events:
        r = per.setdefault((kid, dt_), [0.0, 0.0, 0])
        r[0] += s_.elapsed_time(e_); r[1] += fl; r[2] += 1
    cand = {k: v for k, v in per.items() if k[1] == prefer_dtype} or per
    dom = max(cand, key=lambda k: cand[k][0])
    dom_ms, dom_fl, dom_n = cand[dom]
    peak = DTPEAK[dom[1]]
    achieved = dom_fl / max(dom_ms, 1e-9) / 1e9                        # FLOP/ms/1e9 == TFLOP/s (algorithmic FLOPs)
    main_ms = sum(v[0] for k, v in per.items() if k[1] == prefer_dtype) / max(steps, 1)
    all_ms = sum(v[0] for v in per.values()) / max(steps, 1)
    kn = kname(dom[0], dom[1])
    traffic, traffic_note = None, None
    # measured separately (rocprofv3 --pmc passes, tools/pmc_passes.sh), one file per precision mode; see DESIGN.md
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json" if precision in (None, "fp16") else "pmc_traffic_%s.json" % precision)
    if os.path.isfile(tpath):
        try:
            tj = json.load(open(tpath))
            ent = tj.get(kn + (" " + DTNAME[dom[1]] if dom[1] >= 2 else ""), {})
            if tj.get("kernel_sources_sha16") == kernel_sources_sha() and tj.get("batch") == batch and tj.get("precision") == precision:
                traffic = ent.get("hbm_bytes_per_launch")
                traffic_note = "rocprofv3 --pmc passes of this bench at %s (profiles/%s), kernel sources unchanged since" % (tj.get("measured_at", "?"), os.path.basename(tpath))
            else:
                traffic_note = ("profiles/%s was measured on other kernel sources or another batch / precision "
                                "(%s, batch %s, %s): not reported" % (os.path.basename(tpath), tj.get("measured_at", "round 1"), tj.get("batch", 64), tj.get("precision", "fp16")))
        except Exception as e:      # noqa: BLE001
            traffic_note = "profiles/%s unreadable: %s" % (os.path.basename(tpath), e)
    # north_star's unit: ALGORITHMIC TFLOP/s against the dense fp16 MFMA peak (2500; 157.3 for the exact-fp32 mode).  The ceiling of the
    # precision mode itself (peak / MFMA time units per product) is reported beside it, never as `frac`
    ns_peak = PEAK_F32_TFLOPS if dom[1] == 0 else PEAK_F16_TFLOPS
    tail = {}
    for s_, e_, nb, name in ops.stats.tail_events:
        r = tail.setdefault(name, [0.0, 0.0, 0])
        r[0] += s_.elapsed_time(e_); r[1] += nb; r[2] += 1
    tail_ms = sum(v[0] for v in tail.values()) / max(steps, 1)
    tail_bytes = sum(v[1] for v in tail.values()) / max(steps, 1)
    hbm_tail = {
        "bound": "hbm", "ms_per_step": round(tail_ms, 3), "bytes": round(tail_bytes, 1),
        "GB_per_s": round(tail_bytes / max(tail_ms, 1e-9) / 1e6, 1), "peak_GB_per_s": 8000.0,
        "frac": round(tail_bytes / max(tail_ms, 1e-9) / 1e6 / 8000.0, 4),
        "bytes_note": "algorithmic: every input and output tensor of a launch once, in its storage type (4 bytes per element in the fp16x2 / fp16x3 modes)",
        "copy_rate_note": "a pure copy with these kernels' access shape measured 5.76-5.79 TB/s on MI355X (profiles/r4n_stream_pattern_microbench.txt)",
        "by_kernel": {k: {"ms_per_step": round(v[0] / max(steps, 1), 3), "GB_per_s": round(v[1] / max(v[0], 1e-9) / 1e6, 1), "launches_per_step": v[2] // max(steps, 1)}
                      for k, v in sorted(tail.items(), key=lambda kv: -kv[1][0])},
    }
    return {
        "bound": "mfma", "achieved": round(achieved, 2), "peak": round(ns_peak, 1), "unit": "TFLOP/s",
        "frac": round(achieved / ns_peak, 4), "mode_peak": round(peak, 1), "frac_of_mode_peak": round(achieved / peak, 4),
        "executed_mfma_tflops": round(achieved * MFMA_UNITS[dom[1]], 1),
        "peak_note": "achieved = algorithmic FLOPs / kernel time; peak = 2500 TFLOP/s dense fp16 MFMA (north_star's unit; 157.3 in the fp32 mode); mode_peak = "
                     "peak / %.0f fp16-MFMA time units per algorithmic product in this mode; executed_mfma_tflops = achieved x units" % MFMA_UNITS[dom[1]],
        "hbm_tail": hbm_tail,
        "traffic": traffic, "traffic_source": traffic_note,
        "kernel": kn + " " + DTNAME[dom[1]],
        "launches_per_step": dom_n // max(steps, 1),
        "avg_launch_ms": round(dom_ms / max(dom_n, 1), 4),
        "flops_per_launch_avg": round(dom_fl / max(dom_n, 1), 1),
        "kernel_ms_per_step": round(dom_ms / max(steps, 1), 3),
        "all_conv_kernels": {
            "achieved": round(alg_gf_step / max(main_ms, 1e-9), 2), "frac": round(alg_gf_step / max(main_ms, 1e-9) / ns_peak, 4),
            "frac_of_mode_peak": round(alg_gf_step / max(main_ms, 1e-9) / peak, 4),
            "ms_per_step": round(main_ms, 3), "ms_per_step_all_dtypes": round(all_ms, 3),
            "algorithmic_gflop_per_step": round(alg_gf_step, 1),
            "launched_gflop_per_step": round(sum(v[1] for v in per.values()) / max(steps, 1) / 1e9, 1),
            "by_kernel_ms_per_step": {kname(k[0], k[1]) + " " + DTNAME[k[1]]: round(v[0] / max(steps, 1), 3)
                                      for k, v in sorted(per.items())},
        },
    }, ns_peak


def cpu_info():
    """(model string, logical cores of the host, cores this process may run on)"""
    model = "?"
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.lower().startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return model, os.cpu_count() or 1, avail


def flat_roofline(r):
    """the scalars of a roofline dict a reader needs first, without nesting (the driver's parsed record keeps only one level)"""
    return {"kernel": r["kernel"], "achieved_TFLOPs": r["achieved"], "frac_of_2500": r["frac"], "frac_of_mode_peak": r["frac_of_mode_peak"],
            "all_conv_TFLOPs": r["all_conv_kernels"]["achieved"], "hbm_tail_ms": r["hbm_tail"]["ms_per_step"], "hbm_tail_GB_per_s": r["hbm_tail"]["GB_per_s"]}


def self_launch(n):
    """`python bench.py --gpus N` from a plain shell (no WORLD_SIZE in the environment): re-execute under torch.distributed.run with one rank per GPU on
    127.0.0.1 — the command line the driver's contract spells out — and hand its exit status back.  Rank 0 of that job prints the one JSON line."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC only on this host driver (RCCL across processes)
    env.setdefault("OMP_NUM_THREADS", str(max(1, host_threads(32) // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def dry_main(a, world, rank):
    """--dry: everything of the N-rank bench that is not the HIP forward — process group, per-rank batch, overlapped all-gather of the uint8 outputs,
    barrier + max-over-ranks timing, per-rank rates, ONE JSON line from rank 0 — on CPU tensors over gloo with a stand-in forward"""
    import torch.distributed as dist
    from marconet_amd.pipeline import OverlappedGather
    dev = torch.device("cpu")
    if world > 1 or a.force_gather:
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29534")
            os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("gloo")
    B = min(a.batch, 8)
    gather = OverlappedGather() if (world > 1 or a.force_gather) and not a.no_gather else None

    def fence():
        if gather is not None:
            gather.flush()
        if world > 1:
            dist.barrier()

    def stand_in(i):                 # "SR output" of global image i: a function of i alone (uint8 BGR, a 1/64 thumbnail of [128,2048,3])
        g = torch.Generator().manual_seed(5000 + i)
        return torch.randint(0, 256, (16, 256, 3), generator=g, dtype=torch.uint8)

    def step():
        y = torch.stack([stand_in(rank * B + b) for b in range(B)])
        if gather is not None:
            gather.submit(y)
        return y
    for _ in range(a.warmup):
        step()
    dt, per_rank_dt, _ = timed(step, fence, a.steps, world, dev)
    ok = None
    if gather is not None:           # the collective's result: every rank's shard at its place
        gather.submit(step())
        full = gather.flush()
        ok = bool(torch.equal(full, torch.stack([stand_in(i) for i in range(world * B)])))
    if rank == 0:
        out = {"metric": "SR images/sec (32x512 LR -> 128x2048 SR)", "value": round(world * B * a.steps / dt, 3), "unit": "images/s", "n_gpus": world,
               "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "u8", "data": "DRY RUN: stand-in forward on CPU, no throughput claim", "dry": True,
               "config": {"workload": "dry run: %d stand-in images per rank, gloo" % B, "per_gpu_batch": B, "global_batch": world * B, "parallelism": "dp%d" % world,
                          "collective": "gloo world of %d: all_gather(uint8), asynchronous, overlapped with the next step" % world if gather is not None else "none"},
               "roofline": None, "cpu_baseline": None,
               "ranks": {"world_size": dist.get_world_size() if dist.is_initialized() else 1, "backend": dist.get_backend() if dist.is_initialized() else None,
                         "per_rank_images_per_s": [round(B * a.steps / t_, 2) for t_ in per_rank_dt], "gathered_equals_single_process": ok}}
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def main():
    a = parse()
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        raise SystemExit(self_launch(a.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.dry:
        return dry_main(a, world, rank)
    import torch.distributed as dist
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1 or a.force_gather:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=dev)
        # N ranks build the same seeded checkpoints on the host at the same time: do not oversubscribe its cores
        torch.set_num_threads(max(1, min(32, host_threads(1 << 30) // world)))

    from marconet_amd import checkpoints, ops, synthetic
    from marconet_amd.pipeline import MarconetPipeline, OverlappedGather, balance_shards

    # weights: the reference's real checkpoints when MARCONET_CKPT_DIR holds them (marconet_amd/checkpoints.py), else seeded synthetic ones
    sde, sdg, sds, weights_source = checkpoints.load_state_dicts()
    enc, gan, sr = checkpoints.build_networks(sde, sdg, sds, dev)
    # the product's defaults (check_finite included: on for the half-range modes, one flag read back per batch)
    pipe = MarconetPipeline(enc, gan, sr, precision=a.precision, **({"glyph_chunk": a.glyph_chunk} if a.glyph_chunk > 0 else {}))
    pdt = PDT[a.precision]

    B, n = a.batch, a.glyphs
    gather = OverlappedGather() if (world > 1 or a.force_gather) and not a.no_gather and a.config != "gan" else None
    u8 = gather is not None and a.gather_format == "u8"
    sec_steps = max(1, min(a.steps, a.secondary_steps))

    def fence():
        if gather is not None:
            gather.flush()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def rate(step_fn, steps, images):
        """warm-up + ``steps`` timed steps of a secondary measurement → (images/s over all ranks, ms per step)"""
        step_fn()
        dts, _, _ = timed(step_fn, fence, steps, world, dev)
        return round(images * steps / dts, 3), round(dts / steps * 1e3, 3)

    def instrumented(step_fn, steps, alg_gf, batch, precision):
        """a separate pass with HIP events around every conv launch and every streaming kernel → roofline dict"""
        ops.stats.reset()
        ops.stats.enabled = ops.stats.timing = True
        timed(step_fn, fence, steps, world, dev)
        ops.stats.enabled = ops.stats.timing = False
        r, pk = conv_roofline(ops, steps, alg_gf, PDT[precision], batch, precision)
        ops.stats.reset()
        return r, pk

    # ------------------------------------------------------------------ workloads (each: step(), images per step, algorithmic GFLOP per step)
    def sr_workload(Bq):
        widths = [512] * Bq
        lq_ = synthetic.make_lq(1234 + rank, Bq, widths).to(dev)
        # labels and glyph locations stay on the HOST, where the OCR / detector front-end leaves them (test_sr.py:121-149):
        # the forward then needs no device→host synchronisation at all
        labels_ = [synthetic.make_labels(1234 + 1000 * rank + b, n) for b in range(Bq)]
        locs_ = synthetic.make_locs([n] * Bq, widths)
        return lq_, labels_, locs_

    def gan_in_mode(st_, lab_):
        """TSPGAN in the precision mode's OWN arithmetic (what --config gan times): the module call with its fp16x3 image margin switched off"""
        gan.TextGenerator.module_call_fp16x3 = False
        try:
            return gan(styles=st_, labels=lab_, noise=None)
        finally:
            gan.TextGenerator.module_call_fp16x3 = True

    def gan_workload(N):
        styles_ = synthetic.make_styles(77 + rank, N).to(dev)
        glabels_ = synthetic.make_labels(78 + rank, N).to(dev)
        # configs[3] times the generator in the precision mode's OWN arithmetic (round 6: the module call alone would run it in fp16x3 when the mode is fp16x2, for the
        # margin of the returned image — TextGenerator.module_call_fp16x3)

        def step_():
            ys_ = []                                                  # the structure images of every chunk (what --dump-outputs writes)
            gan.TextGenerator.module_call_fp16x3 = False
            try:
                for s_ in range(0, N, pipe.glyph_chunk):              # bounded working set (8.6 GB of 128-px maps per 1024 glyphs)
                    ys_.append(gan(styles=styles_[s_:s_ + pipe.glyph_chunk], labels=glabels_[s_:s_ + pipe.glyph_chunk], noise=None)[0])
            finally:
                gan.TextGenerator.module_call_fp16x3 = True
            return ys_
        return styles_, glabels_, step_

    def mixed_workload(Bq):
        # configs[4]: content widths uniform in {128,192,...,512}; n_b = w_b / 32 glyphs; the GLOBAL batch (Bq x world strips,
        # same on every rank) is split by algorithmic work (pipeline.balance_shards), each rank runs its strips bucketed by width
        G = Bq * world
        wsel = synthetic.integers(4321, "mixed.w", (G,), 0, 7).tolist()
        widths_all = [128 + 64 * int(v) for v in wsel]
        counts_all = [w_ // 32 for w_ in widths_all]
        mine = balance_shards(widths_all, counts_all, world)[rank]
        widths_ = [widths_all[i] for i in mine]
        counts_ = [counts_all[i] for i in mine]
        lq_ = synthetic.make_lq(4000 + rank, len(mine), widths_).to(dev)
        labels_ = [synthetic.make_labels(4100 + i, c) for i, c in zip(mine, counts_)]
        locs_ = synthetic.make_locs(counts_, widths_, max_glyphs=16)
        gf = sum(GF_RESNET + GF_SR_TRUNK * w_ / 512.0 + GF_F16_PER_GLYPH * c for w_, c in zip(widths_, counts_))
        return lq_, widths_, counts_, labels_, locs_, gf

    secondary = None
    lq = labels = locs = styles = glabels = None
    if a.config == "sr":
        lq, labels, locs = sr_workload(B)
        images_per_step = B
        alg_gf_step = B * (GF_F16_FIXED + GF_F16_PER_GLYPH * n)       # algorithmic GFLOP of the non-ViT convs per step
        gf_image = GF_F16_FIXED + GF_F16_PER_GLYPH * n + GF_VIT
        workload = "metric config: batch %d x 32x512 LR, %d glyphs/img, enc+TSPGAN+TSPSRNet, %s" % (B, n, a.precision)

        def step():
            # N > 1: the all-gather of this step's outputs (the one collective of the path) is enqueued asynchronously and
            # overlaps the next step's compute; the fence waits for the last one, so every gather is inside the timed region
            y = pipe.forward_batch(lq, labels, locs, output="u8_bgr" if u8 else "nchw_f32")
            if gather is not None:
                gather.submit(y)
            return y
    elif a.config == "gan":
        N = B * n                                                     # configs[3]: 256 x 16 = 4096 glyph images per step
        gan.set_precision(a.precision)
        styles, glabels, step = gan_workload(N)
        images_per_step = N
        alg_gf_step = N * GF_GAN
        gf_image = GF_GAN
        workload = "configs[3]: TSPGAN alone, %d x %d = %d glyphs of 128x128 per GPU, chunks of %d, %s" % (B, n, N, pipe.glyph_chunk, a.precision)
    else:
        lq, widths, counts, labels, locs, alg_gf_step = mixed_workload(B)
        images_per_step = len(widths)
        gf_image = (alg_gf_step + GF_VIT * len(widths)) / max(len(widths), 1)
        workload = "configs[4]: %d strips/GPU, widths {128..512 step 64}, w/32 glyphs, 64-px buckets, %s" % (B, a.precision)

        def step():
            return pipe.forward_mixed_widths(lq, widths, labels, locs)

    for _ in range(a.warmup):
        step()
    # headline: the product's default configuration, un-instrumented
    dt, per_rank_dt, y = timed(step, fence, a.steps, world, dev)
    # HBM in use by the timed workload (inputs, weights, every live activation; torch's caching allocator is the only allocator on the path)
    hbm_peak_gb = round(torch.cuda.max_memory_allocated(dev) / 1e9, 1)
    if a.dump_outputs and rank == 0:
        # sr: [B,3,128,2048] fp32 (or [B,128,2048,3] uint8 BGR when that is what is gathered); gan: [B*n,3,128,128]; mixed: [3,128,4W'] per strip
        dump_outputs(a.dump_outputs, {"sr": "sr", "gan": "tspgan_image", "mixed": "sr_strip"}[a.config], torch.cat(y) if a.config == "gan" else y)
    roofline = y_timed = y_timed_noimg = None
    samp_idx = []
    if a.full:
        # roofline of the dominant kernel: a SEPARATE pass with HIP events around every conv launch (same stream)
        prof_steps = min(a.steps, 2)
        roofline, peak = instrumented(step, prof_steps, alg_gf_step, B if a.config == "sr" else None, a.precision)
        roofline["measured_in"] = "a separate instrumented pass of %d step(s) after the timed region (HIP events around every conv launch)" % prof_steps
        for t_ in (y if isinstance(y, list) else [y]):
            if t_.dtype.is_floating_point:
                assert torch.isfinite(t_).all()
        # the timed batch's OWN output, sampled: one strip per generator chunk (4096 glyphs / glyph_chunk 1024 = 4 chunks at the default
        # configuration) — compared with the oracle below (the batch-256 step is the only place where the glyph loop of
        # MarconetPipeline._core runs more than once)
        if a.config == "sr":
            samp_idx = sorted(set([0, B // 3, (2 * B) // 3, B - 1]))
            y_timed = y[samp_idx].float().cpu() if (y.dtype.is_floating_point and y.dim() == 4 and y.shape[1] == 3) else None
    del y
    total_images, per_rank_images = images_per_step, [images_per_step]
    if world > 1:
        t = torch.tensor([images_per_step], device=dev, dtype=torch.float64)
        allc = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allc, t)
        per_rank_images = [int(v.item()) for v in allc]
        total_images = sum(per_rank_images)

    # ---- secondary figures (reported separately, never the headline)
    if a.full and a.config == "sr" and not a.no_secondary:
        secondary = {"steps_each": sec_steps}
        # the same step without the generator's 128-px structure image, which only feeds test_sr.py's saved visualisation
        pipe.need_prior_image = False
        step()
        dt2, _, y2 = timed(step, fence, sec_steps, world, dev)
        pipe.need_prior_image = True
        if y_timed is not None:
            y_timed_noimg = y2[samp_idx].float().cpu()
        del y2
        secondary["images_per_s_without_prior_image"] = round(total_images * sec_steps / dt2, 3)
        secondary["note_without_prior_image"] = "opt-in MarconetPipeline(need_prior_image=False): TSPGAN stops at the 64-px level; SR output identical"
        if pipe._image_precision() not in (None, a.precision):
            # the default runs TSPGAN's image-only 128-px level (11.5 % of the algorithmic FLOPs; forward_batch drops that image unless return_prior=True) in plain
            # fp16: here the same step with EVERY level in the mode's own arithmetic (prior_image_precision=None)
            saved = pipe.prior_image_precision
            pipe.prior_image_precision = None
            secondary["images_per_s_all_levels_in_mode_precision"], _ = rate(step, sec_steps, total_images)
            pipe.prior_image_precision = saved
        if a.precision == "fp16x2":
            # opt-in per-layer precision plan (TSPSRNet.scale_branch_precision = "fp16": the conv_*_scale branches in plain fp16) —
            # not the default (over the bar on edge-clipped glyph windows), timed here with its deviation under parity
            pipe.sr.scale_branch_precision = "fp16"
            secondary["images_per_s_scale_branches_fp16"], _ = rate(step, sec_steps, total_images)
            pipe.sr.scale_branch_precision = None
        # the other precision modes on the same batch (fp32: a 16-image slice — 54 images/s): the mode that meets the parity bar
        # (fp16x3, or fp32) is always reported next to the fp16 storage mode, with its measured deviation under "parity" below
        for prec in ("fp16x2", "fp16x3", "fp16", "fp32"):
            if prec == a.precision:
                continue
            pipe.set_precision(prec)
            kk = min(B, 16) if prec == "fp32" else B
            step_k = (lambda: pipe.forward_batch(lq[:kk], labels[:kk], locs[:kk])) if kk != B else step
            n_steps = 1 if prec == "fp32" else sec_steps
            secondary["%s_mode_images_per_s" % prec], _ = rate(step_k, n_steps, total_images if kk == B else kk * world)
            secondary["%s_mode_batch_per_gpu" % prec] = kk
        pipe.set_precision(a.precision)
        secondary["modes"] = ("fp32: exact fp32 MFMA (parity mode); fp16x3: split-half storage, hi*hi + hi*lo + lo*hi on the fp16 MFMA (fp32-class "
                              "accuracy); fp16x2: fp16+8 storage, hi*hi on the f16 MFMA + one block-scaled fp8 MFMA for both correction products "
                              "(meets the 1e-3 bar, see parity); fp16: one half per element (BASELINE configs[1]'s storage type)")
        if gather is not None and world == 1:
            # --force-gather: what the collective costs when nothing hides it (a world of one: the gather is a device copy through RCCL)
            pipe_y = step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                gather.submit(pipe_y)
                gather.flush()
            torch.cuda.synchronize()
            secondary["forced_all_gather_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)

    units_fixed = {"fp16x2": ("fp16x3", "fp16x2"), "fp16x3": ("fp16x3", "fp16x3"), "fp16": ("fp16", "fp16"), "fp32": ("fp32", "fp32")}[a.precision]
    img_prec = (pipe._image_precision() or a.precision) if a.config != "gan" else a.precision
    arithmetic = {            # which algorithmic GFLOP per image run in which arithmetic (BENCH readers: this is what `value` times)
        "resnet45_%s" % units_fixed[0]: GF_RESNET, "textvit_fp32": GF_VIT,
        "sr_net_%s" % units_fixed[1]: round(GF_SR_TRUNK + GF_SR_PRIOR * n, 1),
        "tspgan_prior_levels_%s" % units_fixed[1]: round((GF_GAN - GF_GAN_IMAGE_LEVEL) * n, 1),
        "tspgan_image_only_level_%s" % img_prec: round(GF_GAN_IMAGE_LEVEL * n, 1),
    } if a.config == "sr" else None
    out = {
        "metric": {"sr": "SR images/sec (32x512 LR -> 128x2048 SR)", "gan": "TSPGAN glyph images/sec (128x128 structure prior)",
                   "mixed": "SR images/sec (mixed-width 32x{128..512} LR, bucketed)"}[a.config],
        "value": round(total_images * a.steps / dt, 3),
        "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": DTNAME[pdt],
        "data": "synthetic inputs; weights: %s" % weights_source,
        "config": {"workload": workload, "per_gpu_batch": B, "global_batch": total_images, "glyphs_per_image": n,
                   "parallelism": "dp%d" % world, "precision_mode": a.precision,
                   "need_prior_image": bool(pipe.need_prior_image) if a.config != "gan" else True,
                   "prior_image_precision": img_prec,
                   "prior_image_note": ("TSPGAN's 128-px level (%.0f of %.0f GF/img) feeds only the structure image, dropped here (return_prior=False): computed, in %s"
                                        % (GF_GAN_IMAGE_LEVEL * n, gf_image, img_prec)) if a.config == "sr" else None,
                   "gflop_per_image": round(gf_image, 1), "gflop_per_image_by_arithmetic": arithmetic,
                   "weights": weights_source, "hbm_peak_gb": hbm_peak_gb, "hbm_capacity_gb": 288,
                   "collective": (("RCCL world of %d: " % world) + "all_gather(%s), asynchronous, overlapped with the next step"
                                  % ("uint8 BGR post-processed SR [b,128,2048,3]" if u8 else "fp32 SR outputs [b,3,128,2048]"))
                   if gather is not None else "none"},
        "roofline": roofline,
        "secondary": secondary,
    }
    if roofline is not None:
        roofline.update({"all_conv_achieved": roofline["all_conv_kernels"]["achieved"], "all_conv_frac": roofline["all_conv_kernels"]["frac"],
                         "hbm_tail_ms_per_step": roofline["hbm_tail"]["ms_per_step"], "hbm_tail_GB_per_s": roofline["hbm_tail"]["GB_per_s"],
                         "hbm_tail_frac_of_8TBps": roofline["hbm_tail"]["frac"]})
        roofline["end_to_end_frac_of_peak"] = round(out["value"] / world * gf_image / 1e3 / peak, 4)      # of the dense fp16 (fp32-mode: fp32) MFMA peak
    if a.config == "sr" and secondary:
        # the two neighbours of `value` a reader of the parsed record needs beside it (also under `secondary`): the same step with EVERY generator
        # level in the mode's own arithmetic (what corresponds to "the script's outputs, all <= 1e-3": test_sr.py:207-211 consumes the structure image), and with the
        # structure image not computed at all (opt-in, skips work the reference does)
        out["value_all_levels_in_mode_precision"] = secondary.get("images_per_s_all_levels_in_mode_precision", out["value"])
        out["value_without_prior_image"] = secondary.get("images_per_s_without_prior_image")
        out["config"]["value_is"] = "defaults: structure image computed in %s, dropped; neighbours: value_all_levels_in_mode_precision, value_without_prior_image" % img_prec
    if a.full and a.config == "sr":
        out["headline_note"] = ("value: %s mode, product defaults (check_finite on, need_prior_image on, image-only TSPGAN level in %s), un-instrumented. fp16x2 "
                                "(fp16+8 storage: hi*hi on the f16 MFMA + w_lo8*x_hi8 + w_hi8*x_lo8 as one block-scaled fp8 MFMA) and fp16x3 (split-half, three "
                                "f16 MFMA products) meet the north-star bar (<= 1e-3, indices bit-exact; see parity); plain fp16 (~1e-2) and exact fp32 are "
                                "secondary.*_mode_images_per_s; secondary.images_per_s_all_levels_in_mode_precision = no level in a cheaper arithmetic" % (a.precision, img_prec))
    if world > 1 or a.force_gather:
        out["ranks"] = {"world_size": dist.get_world_size(), "backend": dist.get_backend(),
                        "per_rank_images_per_s": [round(c_ * a.steps / t_, 2) for c_, t_ in zip(per_rank_images, per_rank_dt)]}

    cpu_model, host_cores, affinity = cpu_info()
    # ---- CPU baseline (the oracle = port of the reference's CPU forward) + parity, rank 0 at N=1 only
    if a.full and rank == 0 and world == 1 and a.cpu_images > 0 and a.config == "sr":
        from oracle import marconet_oracle as O
        k = min(a.cpu_images, len(samp_idx))
        sel = samp_idx[:k]                       # the strips the oracle recomputes: spread over the timed batch (one per generator chunk)
        # the threads actually used: the affinity mask, capped (oneDNN convs at batch 1 stop scaling well before
        # that, and 256 oversubscribed threads on a cgroup-limited box measured 100x slower)
        threads = host_threads(a.cpu_threads)
        torch.set_num_threads(threads)
        lq_c, locs_c = lq[sel].cpu(), locs[sel]
        lab_c = [labels[i] for i in sel]
        O.end_to_end(sde, sdg, sds, lq_c[:1], [lab_c[0][:2]], locs_c[:1])          # warm-up (small)
        t0 = time.perf_counter()
        refs = [O.end_to_end(sde, sdg, sds, lq_c[i:i + 1], lab_c[i:i + 1], locs_c[i:i + 1]) for i in range(k)]  # batch 1, like test_sr.py:77
        cdt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(k / cdt, 4), "unit": "images/s", "cores": threads, "kind": "port",
                               "threads": threads, "host_cores": host_cores, "affinity_cores": affinity, "cpu_model": cpu_model,
                               "sample": "%d strips (batch 1 each, %d glyphs) of the timed batch through oracle/marconet_oracle.py, torch %s CPU fp32, %d threads of %d cores"
                                         % (k, n, torch.__version__, threads, host_cores)}
        # the same at batch 8 (one call) and per network (seconds per image at batch 1)
        k8 = min(8, B)
        if k8 > 1:
            t0 = time.perf_counter()
            O.end_to_end(sde, sdg, sds, lq[:k8].cpu(), labels[:k8], locs[:k8])
            out["cpu_baseline"]["batch8_images_per_s"] = round(k8 / (time.perf_counter() - t0), 4)
        with torch.no_grad():
            t0 = time.perf_counter(); lg_, _, w_ = O.encoder_forward(sde, lq_c[:1]); t_enc = time.perf_counter() - t0
            t0 = time.perf_counter(); g_ = O.tspgan_forward(sdg, w_[:1].repeat(lab_c[0].shape[0], 1), lab_c[0]); t_gan = time.perf_counter() - t0
            t0 = time.perf_counter(); O.tspsr_forward(sds, lq_c[:1], [g_[1]], [g_[2]], locs_c[:1]); t_sr = time.perf_counter() - t0
        out["cpu_baseline"]["seconds_per_image_by_net"] = {"encoder": round(t_enc, 3), "tspgan_%d_glyphs" % n: round(t_gan, 3), "tspsrnet": round(t_sr, 3)}
        ref_sr = torch.cat([r["sr"] for r in refs])
        ref_arg = torch.cat([r["logits"] for r in refs]).argmax(-1)
        par = {}
        for prec in ("fp16", "fp16x2", "fp16x3", "fp32"):
            try:
                pipe.set_precision(prec)
            except ValueError:
                continue
            yk = pipe.forward_batch(lq[sel].contiguous(), lab_c, locs_c)
            lg = pipe.encoder(lq[sel].contiguous())[0]
            par["sr_max_abs_%s" % prec] = round((yk.cpu() - ref_sr).abs().max().item(), 6)
            par["argmax_match_%s" % prec] = round(float((lg.argmax(-1).cpu() == ref_arg).float().mean()), 4)
        pipe.set_precision(a.precision)
        if a.precision == "fp16x2":
            pipe.sr.scale_branch_precision = "fp16"
            par["sr_max_abs_fp16x2_scale_branches_fp16"] = round((pipe.forward_batch(lq[sel].contiguous(), lab_c, locs_c).cpu() - ref_sr).abs().max().item(), 6)
            pipe.sr.scale_branch_precision = None
        if y_timed is not None:       # the timed batch itself (all B strips in one call, the generator in chunks), at the sampled strips
            par["sr_max_abs_%s_timed_batch" % a.precision] = round((y_timed[:k] - ref_sr).abs().max().item(), 6)
            if y_timed_noimg is not None:
                par["sr_max_abs_%s_timed_batch_without_prior_image" % a.precision] = round((y_timed_noimg[:k] - ref_sr).abs().max().item(), 6)
                par["timed_batch_without_prior_image_equals_default"] = bool(torch.equal(y_timed, y_timed_noimg))
            par["timed_batch_strips"] = sel
        par["weights"] = weights_source

        # ---- BASELINE configs[1] / [3] / [4], driver-timed in the same line (short: `sec_steps` steps each)
        if not a.no_secondary:
            cfgs = {}
            # configs[1]: batch 64 of the same strips (strip 0 is one the oracle has just recomputed)
            k64 = min(64, B)
            step64 = lambda: pipe.forward_batch(lq[:k64], labels[:k64], locs[:k64])       # noqa: E731
            v64, ms64 = rate(step64, sec_steps, k64)
            r64, _ = instrumented(step64, 1, k64 * (GF_F16_FIXED + GF_F16_PER_GLYPH * n), None, a.precision)
            y64 = step64()
            cfgs["configs1_batch64"] = dict(value=v64, unit="images/s", ms_per_step=ms64, steps=sec_steps, **flat_roofline(r64),
                                            parity_sr_max_abs_strip0=round((y64[:1].cpu() - ref_sr[:1]).abs().max().item(), 6))
            del y64
            # configs[3]: TSPGAN alone on B x n glyphs (TSPGAN.forward: every level in the mode's arithmetic, the image is returned)
            Ng = B * n
            gan.set_precision(a.precision)
            st_g, lab_g, step_g = gan_workload(Ng)
            vg, msg = rate(step_g, sec_steps, Ng)
            rg, _ = instrumented(step_g, 1, Ng * GF_GAN, None, a.precision)
            kg = min(16, Ng)
            t0 = time.perf_counter()
            ref_g = O.tspgan_forward(sdg, st_g[:kg].cpu(), lab_g[:kg].cpu())
            cg = time.perf_counter() - t0
            yg = gan_in_mode(st_g[:kg], lab_g[:kg])
            cfgs["configs3_gan_only"] = dict(value=vg, unit="glyph images/s", ms_per_step=msg, steps=sec_steps, glyphs_per_step=Ng, **flat_roofline(rg),
                                             parity_image_max_abs=round((yg[0].cpu() - ref_g[0]).abs().max().item(), 6),
                                             parity_prior64_max_abs=round((yg[1].cpu() - ref_g[1]).abs().max().item(), 6),
                                             cpu_glyph_images_per_s=round(kg / cg, 3))
            del st_g, lab_g, yg
            # configs[4]: mixed widths, bucketed; parity: the narrowest strip against the reference arithmetic at its bucket width
            lqm, wm, cm, labm, locm, gfm = mixed_workload(B)
            stepm = lambda: pipe.forward_mixed_widths(lqm, wm, labm, locm)                 # noqa: E731
            vm, msm = rate(stepm, sec_steps, len(wm))
            rm, _ = instrumented(stepm, 1, gfm, None, a.precision)
            outs = stepm()
            bsel = min(range(len(wm)), key=lambda i: (wm[i], i))
            wb = (wm[bsel] + 63) // 64 * 64
            t0 = time.perf_counter()
            with torch.no_grad():
                lqs = lqm[bsel:bsel + 1].cpu()
                _, _, w1 = O.encoder_forward(sde, lqs)
                _, a64, a32 = O.tspgan_forward(sdg, w1[:1].repeat(cm[bsel], 1), labm[bsel])
                c64 = torch.trunc(locm[bsel:bsel + 1] * 1024.0)      # the integer centres of the 512-padded run (tests/test_modules_gpu.py::test_config5_*)
                refm = O.tspsr_forward(sds, lqs[:, :, :, :wb], [a64], [a32], (c64 + 0.5) / (2.0 * wb))
            cmix = time.perf_counter() - t0
            cfgs["configs4_mixed_widths"] = dict(value=vm, unit="images/s", ms_per_step=msm, steps=sec_steps, strips=len(wm), **flat_roofline(rm),
                                                 parity_sr_max_abs_narrowest_strip=round((outs[bsel].cpu() - refm[0]).abs().max().item(), 6),
                                                 parity_strip_width=wm[bsel], cpu_images_per_s_that_strip=round(1.0 / cmix, 4))
            del outs, lqm
            secondary["configs"] = cfgs
            secondary["configs_note"] = ("BASELINE configs[1] (batch 64), [3] (TSPGAN alone, %d glyphs) and [4] (mixed widths) in this same run, %d timed steps "
                                         "each + 1 instrumented step for the dominant kernel's fraction of 2500 TFLOP/s" % (Ng, sec_steps))

        # ---- second weight regime: the trained-like synthetic checkpoints (marconet_amd/synthetic.py) through the same comparison
        if not a.no_regimes and not weights_source.startswith("synthetic:trained"):
            t_sde, t_sdg, t_sds, t_src = checkpoints.load_state_dicts(path="", regime="trained")
            t_nets = checkpoints.build_networks(t_sde, t_sdg, t_sds, dev)
            t_pipe = MarconetPipeline(*t_nets, precision=a.precision)
            kt = min(2, k)
            t_refs = [O.end_to_end(t_sde, t_sdg, t_sds, lq_c[i:i + 1], lab_c[i:i + 1], locs_c[i:i + 1]) for i in range(kt)]
            t_sr = torch.cat([r["sr"] for r in t_refs])
            t_arg = torch.cat([r["logits"] for r in t_refs]).argmax(-1)
            reg = {"strips": sel[:kt], "oracle_sr_abs_max": round(t_sr.abs().max().item(), 4)}
            for prec in ("fp16x2", "fp16x3", "fp32"):
                t_pipe.set_precision(prec)
                yk = t_pipe.forward_batch(lq[sel[:kt]].contiguous(), lab_c[:kt], locs_c[:kt])
                lg = t_pipe.encoder(lq[sel[:kt]].contiguous())[0]
                reg["sr_max_abs_%s" % prec] = round((yk.cpu() - t_sr).abs().max().item(), 6)
                reg["argmax_match_%s" % prec] = round(float((lg.argmax(-1).cpu() == t_arg).float().mean()), 4)
            par["regime_trained_like"] = reg
            par["sr_max_abs_%s_trained_like_regime" % a.precision] = reg.get("sr_max_abs_%s" % a.precision)
            del t_pipe, t_nets
        par["regimes"] = "tame (default synthetic, all sr_max_abs_* above) and trained_like (heavy-tailed weights, modulation spread 1e3, SN sigma in [0.1,10])"
        par["bar"] = "north_star: <= 1e-3 max-abs on the SR output, argmax bit-exact (argmax_match == 1.0)"
        par["oracle"] = ("oracle/marconet_oracle.py = CPU restatement of models/*.py, pinned against the real reference modules in the build container (<= 1e-6) and by "
                         "tests/golden; unpinned by the reference itself: basicsr fused_act (un-vendored; upstream semantics sqrt2*lrelu(x+b)); cv2 INTER_CUBIC is outside "
                         "this forward; cpu_baseline.kind = port (the oracle: /root/reference does not travel to the GPU box)")
        out["parity"] = par
    elif a.full and rank == 0 and world == 1 and a.cpu_images > 0 and a.config == "gan":
        from oracle import marconet_oracle as O
        threads = host_threads(a.cpu_threads)
        torch.set_num_threads(threads)
        k = min(16, styles.shape[0])
        st_c, lab_c = styles[:k].cpu(), glabels[:k].cpu()
        O.tspgan_forward(sdg, st_c[:2], lab_c[:2])
        t0 = time.perf_counter()
        ref = O.tspgan_forward(sdg, st_c, lab_c)
        cdt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(k / cdt, 4), "unit": "images/s", "cores": threads, "kind": "port",
                               "threads": threads, "host_cores": host_cores, "affinity_cores": affinity, "cpu_model": cpu_model,
                               "sample": "%d glyphs in one TSPGAN call through oracle/marconet_oracle.py, torch %s CPU fp32, %d threads of %d cores" % (k, torch.__version__, threads, host_cores)}
        yk = gan_in_mode(styles[:k], glabels[:k])
        ym = gan(styles=styles[:k], labels=glabels[:k], noise=None)       # the module call as test_w.py makes it (fp16x2 mode: whole generator in fp16x3, see TextGenerator.forward)
        out["parity"] = {"image_max_abs_%s" % a.precision: round((yk[0].cpu() - ref[0]).abs().max().item(), 6),
                         "prior64_max_abs_%s" % a.precision: round((yk[1].cpu() - ref[1]).abs().max().item(), 6),
                         "image_max_abs_module_call": round((ym[0].cpu() - ref[0]).abs().max().item(), 6)}
    elif a.full and rank == 0 and world == 1 and a.cpu_images > 0 and a.config == "mixed":
        # configs[4] stand-alone: the narrowest strip against the reference arithmetic at its bucket width, timed on the host
        from oracle import marconet_oracle as O
        threads = host_threads(a.cpu_threads)
        torch.set_num_threads(threads)
        outs = pipe.forward_mixed_widths(lq, widths, labels, locs)
        bsel = min(range(len(widths)), key=lambda i: (widths[i], i))
        wb = (widths[bsel] + 63) // 64 * 64
        t0 = time.perf_counter()
        with torch.no_grad():
            lqs = lq[bsel:bsel + 1].cpu()
            _, _, w1 = O.encoder_forward(sde, lqs)
            _, a64, a32 = O.tspgan_forward(sdg, w1[:1].repeat(counts[bsel], 1), labels[bsel])
            c64 = torch.trunc(locs[bsel:bsel + 1] * 1024.0)
            refm = O.tspsr_forward(sds, lqs[:, :, :, :wb], [a64], [a32], (c64 + 0.5) / (2.0 * wb))
        cdt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(1.0 / cdt, 4), "unit": "images/s", "cores": threads, "kind": "port",
                               "threads": threads, "host_cores": host_cores, "affinity_cores": affinity, "cpu_model": cpu_model,
                               "sample": "the narrowest strip of the batch (%d px, %d glyphs) through oracle/marconet_oracle.py at its bucket width, torch %s CPU fp32, %d threads of %d cores"
                                         % (widths[bsel], counts[bsel], torch.__version__, threads, host_cores)}
        out["parity"] = {"sr_max_abs_%s_narrowest_strip" % a.precision: round((outs[bsel].cpu() - refm[0]).abs().max().item(), 6), "strip_width": widths[bsel]}

    if rank == 0:
        print(json.dumps(out))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
