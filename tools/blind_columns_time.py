#!/usr/bin/env python
"""Times the blind reading of a page's vertical columns (marconet_amd/blind_columns.py, MarconetPipeline.read_columns): DESIGN.md §3's numbers.

    python tools/blind_columns_time.py [--reps 5] [--precision fp32]

The page is an A4 page at 300 dpi (2480 x 3508) of random pixels with the 40 columns of tools/ordered_paste_time.py's scene (a) — boxes of 50 x 3300
px, which that scene cuts into 30 cells of 50 x 110 px from a given text; read blind, the square-cell prior cuts each into 66 cells —, scale 4, on
the seeded synthetic weights with the encoder's locations pinned as in tests/test_blind_gpu.py: the figures are about cost, not about what is read.
Timed with device events, each as (median, min, max) in ms over ``reps`` repetitions after one warm-up:
    ink            the table's copy and the ONE mnet_row_ink_u8 launch over all columns as views of the page
    profiles_copy  the one device→host copy of all profiles
    gather         the table's copy and the ONE mnet_column_gather_u8 launch for every probe of every column
    forward        lq_device.prepare_packed and the encoder's forward on all probes
beside, on a host clock, numpy ``row_ink`` over the same boxes (the host's only way to the profiles), ``first_cuts`` + ``plan_cell_probes`` on
the host, and the whole ``read_columns`` call.  The device's profiles are compared with numpy's (==) before anything is timed.
One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from marconet_amd import blind_columns as bc, checkpoints, columns, lq_device, ops                # noqa: E402
from marconet_amd.pipeline import MarconetPipeline                                               # noqa: E402

PAGE_W, PAGE_H, SCALE = 2480, 3508, 4
PAIRS = [v for k in range(16) for v in ((k + 0.1) * 0.046, (k + 0.9) * 0.046)]


def stats(ms):
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def timed_events(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def timed_host(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="fp32")
    a = ap.parse_args()
    dev = "cuda"
    sde, sdg, sds, _ = checkpoints.load_state_dicts(path="", regime="trained")
    pipe = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, dev), precision=a.precision)
    forward, pinned = pipe.encoder.forward, torch.tensor(PAIRS, dtype=torch.float32).reshape(1, 32)

    def pinned_forward(lq, **kw):
        logits, locs, w = forward(lq, **kw)
        return logits, pinned.to(locs.device).expand(locs.shape[0], 32).contiguous(), w
    pipe.encoder.forward = pinned_forward

    page = np.random.default_rng(1).integers(0, 256, (PAGE_H, PAGE_W, 3), dtype=np.uint8)
    boxes = [[20 + 60 * c, 100, 70 + 60 * c, 100 + 30 * 110] for c in range(40)]
    page_d = torch.from_numpy(page).to(dev)
    tab, _, total = bc.ink_table(boxes, PAGE_W)
    ink_d = torch.empty((total,), dtype=torch.int32, device=dev)
    state = {}

    def ink():
        ops.row_ink_u8(page_d.reshape(-1), ops.table_to_device(tab, dev), int(tab["h"].max()), ink_d)

    def copy():
        state["ink"] = ink_d.cpu().numpy()

    def host_ink():
        state["host_ink"] = [bc.row_ink(page, b) for b in boxes]

    def plan():
        inks = [state["ink"][int(t["out"]):int(t["out"]) + int(t["h"])] for t in tab]
        state["plans"] = bc.plan_columns(boxes, inks)
        state["cols"] = [(p["box"], p["first_cuts"], p["widths"], bc.probe_windows(p["probes"])) for p in state["plans"]]

    def gather():
        state["packed"] = columns.gather_columns(page_d, state["cols"])

    def fwd():
        packed, shapes, offsets = state["packed"]
        state["out"] = pipe.encoder(lq_device.prepare_packed(packed, shapes, offsets).lq)

    with torch.no_grad():
        res = dict(page=[PAGE_W, PAGE_H], columns=len(boxes), column=[50, 3300], scale=SCALE, precision=a.precision, reps=a.reps)
        res["ink_ms"] = timed_events(ink, a.reps)
        res["profiles_copy_ms"] = timed_events(copy, a.reps)
        res["host_row_ink_ms"] = timed_host(host_ink, a.reps)
        assert np.array_equal(state["ink"], np.concatenate(state["host_ink"]))
        res["host_cuts_probes_ms"] = timed_host(plan, a.reps)
        res["cells"] = sum(len(p["widths"]) for p in state["plans"])
        res["probes"] = sum(len(p["probes"]) for p in state["plans"])
        res["gather_ms"] = timed_events(gather, a.reps)
        res["forward_ms"] = timed_events(fwd, a.reps)
        res["read_columns_ms"] = timed_host(lambda: state.update(read=pipe.read_columns(page, boxes, scale=SCALE)), a.reps)
        res["characters_read"] = sum(len(r["text"]) for r in state["read"] if r is not None)
        res["profile_bytes"] = int(4 * total)
        res["box_bytes"] = int(sum(3 * (b[2] - b[0]) * (b[3] - b[1]) for b in boxes))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
