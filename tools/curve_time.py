#!/usr/bin/env python
"""Times the two kernels of the curved page path (mnet_curve_crop_u8, mnet_curve_paste_u8) with device events, beside the quadrilateral kernels
(mnet_quad_crop_u8, mnet_quad_paste_u8) on the same regions' bounding quadrilaterals: DESIGN.md §3's numbers.

    python tools/curve_time.py [--reps 7] [--launches 50]

The page is an A4 page at 300 dpi (2480 x 3508), scale 4, feather 8, with 40 arcs of 6 segments (4 columns x 10 rows; a line 60 px high bent over
120 degrees at a mean radius of 210 px).  Each figure is the median over ``reps`` repetitions of the time of ``launches`` back-to-back launches
between two events, divided by ``launches``, after a warm-up of as many launches.  One JSON line on stdout."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from marconet_amd import curves, ops, quads          # noqa: E402

PAGE_W, PAGE_H, SCALE, FEATHER = 2480, 3508, 4, 8


def arc(cx, cy, r_in, r_out, deg0, deg1, K):
    a = [math.radians(d) for d in np.linspace(deg0, deg1, K)]
    top = [(cx + r_out * math.cos(t), cy - r_out * math.sin(t)) for t in a]
    bot = [(cx + r_in * math.cos(t), cy - r_in * math.sin(t)) for t in a]
    return top + bot[::-1]


def timed(fn, reps, launches):
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / launches)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    dev = "cuda"
    polys = [arc(330.0 + 600.0 * i, 300.0 + 340.0 * j, 180.0, 240.0, 150.0, 30.0, 7) for j in range(10) for i in range(4)]
    recs = curves.check_curves(PAGE_H, PAGE_W, polys, [True] * len(polys), SCALE, FEATHER)
    boxes = []
    for p in polys:                                                               # the bounding quadrilateral: the polygon's outward-rounded box
        xs, ys = [q[0] for q in p], [q[1] for q in p]
        boxes.append([math.floor(min(xs)), math.floor(min(ys)), math.ceil(max(xs)), math.ceil(max(ys))])
    qrecs = quads.check_quads(PAGE_H, PAGE_W, [quads.box_quad(b) for b in boxes], [True] * len(boxes), SCALE, FEATHER)
    g = torch.Generator(device="cpu").manual_seed(1)
    page = torch.randint(0, 256, (PAGE_H, PAGE_W, 3), dtype=torch.uint8, generator=g).to(dev)
    out = torch.randint(0, 256, (SCALE * PAGE_H, SCALE * PAGE_W, 3), dtype=torch.uint8, generator=g).to(dev)
    res = dict(page=[PAGE_W, PAGE_H], scale=SCALE, feather=FEATHER, regions=len(polys), segments=len(recs[0]["segs"]), reps=a.reps, launches=a.launches)

    # the gather in
    tab, seg_tab, nbytes = curves.crop_table([r["segs"] for r in recs], [(r["cw"], r["ch"]) for r in recs])
    tab_d, seg_d, dst = ops.table_to_device(tab, dev), ops.table_to_device(seg_tab, dev), torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    mw, mh = max(r["cw"] for r in recs), max(r["ch"] for r in recs)
    res["curve_crop_ms"] = timed(lambda: ops.curve_crop_u8(page, tab_d, seg_d, mw, mh, dst), a.reps, a.launches)
    res["curve_crop_pixels"] = nbytes // 3
    qtab, qbytes = quads.crop_table([quads.quad_map(r["quad"], r["cw"], r["ch"]) for r in qrecs], [(r["cw"], r["ch"]) for r in qrecs])
    qtab_d, qdst = ops.table_to_device(qtab, dev), torch.empty((qbytes,), dtype=torch.uint8, device=dev)
    qmw, qmh = max(r["cw"] for r in qrecs), max(r["ch"] for r in qrecs)
    res["quad_crop_ms"] = timed(lambda: ops.quad_crop_u8(page, qtab_d, qmw, qmh, qdst), a.reps, a.launches)
    res["quad_crop_pixels"] = qbytes // 3

    # the gather out
    def atlas_for(rs):
        xy, y = [], 0
        for r in rs:
            xy.append((0, y))
            y += r["rh"]
        return torch.randint(0, 256, (y, max(r["rw"] for r in rs), 3), dtype=torch.uint8, generator=g).to(dev), xy

    atlas, xy = atlas_for(recs)
    ptab, pseg = curves.paste_table(recs, FEATHER, xy)
    ptab_d, pseg_d = ops.table_to_device(ptab, dev), ops.table_to_device(pseg, dev)
    bw, bh = max(r["bbox"][2] for r in recs), max(r["bbox"][3] for r in recs)
    before = out.clone()
    ops.curve_paste_u8(atlas, ptab_d, pseg_d, bw, bh, out)
    res["curve_paste_pixels"] = int((out != before).any(dim=2).sum().item())
    res["curve_paste_box_pixels"] = int(sum(r["bbox"][2] * r["bbox"][3] for r in recs))
    res["curve_paste_ms"] = timed(lambda: ops.curve_paste_u8(atlas, ptab_d, pseg_d, bw, bh, out), a.reps, a.launches)
    qatlas, qxy = atlas_for(qrecs)
    qptab_d = ops.table_to_device(quads.paste_table(qrecs, FEATHER, qxy), dev)
    qbw, qbh = max(r["bbox"][2] for r in qrecs), max(r["bbox"][3] for r in qrecs)
    res["quad_paste_pixels"] = int(sum(r["bbox"][2] * r["bbox"][3] for r in qrecs))
    res["quad_paste_ms"] = timed(lambda: ops.quad_paste_u8(qatlas, qptab_d, qbw, qbh, out), a.reps, a.launches)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
