#!/usr/bin/env python
"""Times the blind reading of a page (marconet_amd/blind.py, MarconetPipeline.restore_page(texts=None)): DESIGN.md §3's numbers.

    python tools/blind_read_time.py [--reps 5] [--lines 40] [--precision fp32]

The page is an A4 page at 300 dpi (2480 x 3508) of random pixels with ``lines`` text lines of 2080 x 60 px (five probes each at the default probe
width of 384), scale 4, feather 8, on the seeded synthetic weights.  No trained checkpoint exists here, so the encoder's locations are pinned to 16
evenly spaced pairs per probe, as in tests/test_blind_gpu.py: the labels are random, the boxes sane, and every line is planned into several
windows — the figures are about cost, not about what is read.
Timed, each as (median, min, max) in ms over ``reps`` repetitions on a host clock between two device synchronisations, after one warm-up:
    reading        the probes' launch (lq_device.prepare_windows over views of the page on the device: the table's copy and mnet_lq_windows_u8),
                   the encoder's forward on all probes, and the argmax + the one device→host copy + the merge on the host
    windows        the encoder input of the PLANNED windows: lq_device.prepare_windows over views of the page, beside the path they took before —
                   the crops cut on the host, lq_device.prepare_strips (their upload and mnet_lq_from_u8); the two results are compared with
                   torch.equal before anything is timed
    restore_page   the whole call with the texts read, and given the texts and boxes that were read (the same windows, the same bytes)
One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from marconet_amd import blind, checkpoints, lq_device          # noqa: E402
from marconet_amd.pipeline import MarconetPipeline              # noqa: E402

PAGE_W, PAGE_H, SCALE, FEATHER = 2480, 3508, 4, 8
PAIRS = [v for k in range(16) for v in ((k + 0.1) * 0.046, (k + 0.9) * 0.046)]


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lines", type=int, default=40)
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
    boxes = [[200, 60 + 85 * i, 2280, 120 + 85 * i] for i in range(a.lines)]
    view = lambda b, c0, c1: ((b[1] * PAGE_W + b[0] + c0) * 3, 3 * PAGE_W, b[3] - b[1], c1 - c0)      # noqa: E731
    sizes = [(b[3] - b[1], b[2] - b[0]) for b in boxes]
    probes = blind.line_probes(sizes)
    page_d = torch.from_numpy(page).to(dev).reshape(-1)
    probe_wins = [view(b, p[0], p[1]) for b, pr in zip(boxes, probes) for p in pr]
    res = dict(page=[PAGE_W, PAGE_H], lines=a.lines, line=[2080, 60], scale=SCALE, feather=FEATHER, precision=a.precision, reps=a.reps,
               probes=len(probe_wins))

    # the reading pass, stage by stage
    state = {}

    def launch():
        state["lq"] = lq_device.prepare_windows(page_d, probe_wins).lq

    def encode():
        state["out"] = pipe.encoder(state["lq"])

    def copy_merge():
        rows, locs = blind.encode(pipe, state["lq"])              # the forward again: its time is taken off below
        state["read"] = blind.decode(sizes, probes, rows, locs)

    with torch.no_grad():
        t_launch, t_enc, t_all = timed(launch, a.reps), timed(encode, a.reps), timed(copy_merge, a.reps)
        res["reading"] = dict(probe_windows_ms=t_launch, encoder_forward_ms=t_enc, forward_copy_merge_ms=t_all,
                              copy_merge_ms=t_all[0] - t_enc[0], total_ms=t_launch[0] + t_all[0])

        # the planned windows: views of the page on the device against host crops, their upload and mnet_lq_from_u8
        got, det = pipe.restore_page(page, boxes, None, scale=SCALE, feather=FEATHER, details=True)
        texts, char_boxes = [d["text"] for d in det], [d["boxes"] for d in det]
        plan_wins = [(b, p) for b, d in zip(boxes, det) for p in d["plan"]]
        res["planned_windows"] = len(plan_wins)
        res["characters_read"] = sum(len(t) for t in texts)
        views = [view(b, p.c0, p.c1) for b, p in plan_wins]

        def old():
            crops = [np.ascontiguousarray(page[b[1]:b[3], b[0] + p.c0:b[0] + p.c1]) for b, p in plan_wins]
            return lq_device.prepare_strips(crops, dev).lq

        new = lambda: lq_device.prepare_windows(page_d, views).lq                                   # noqa: E731
        assert torch.equal(old(), new())
        res["windows"] = dict(host_crops_upload_lq_from_u8_ms=timed(old, a.reps), views_lq_windows_u8_ms=timed(new, a.reps),
                              crop_bytes=int(sum(3 * (b[3] - b[1]) * (p.c1 - p.c0) for b, p in plan_wins)))

        # the whole call
        want = pipe.restore_page(page, boxes, texts, char_boxes=char_boxes, scale=SCALE, feather=FEATHER)
        assert np.array_equal(got, want)
        res["restore_page"] = dict(texts_read_ms=timed(lambda: pipe.restore_page(page, boxes, None, scale=SCALE, feather=FEATHER), a.reps),
                                   texts_given_ms=timed(lambda: pipe.restore_page(page, boxes, texts, char_boxes=char_boxes, scale=SCALE, feather=FEATHER),
                                                        a.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
