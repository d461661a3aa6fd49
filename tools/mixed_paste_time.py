#!/usr/bin/env python
"""Times the page compositor for regions of every kind (mnet_paste_mixed_u8) with device events, beside the kernels it stands in for, on the same
tables in the same run: DESIGN.md §3's numbers.  The method is tools/ordered_paste_time.py's, whose helpers this script uses.

    python tools/mixed_paste_time.py [--reps 7] [--launches 50]

The page is an A4 page at 300 dpi (2480 x 3508), scale 4, feather 8, lines of 128 rows.  Scene (a): 40 disjoint lines of 1600 x 60 px — the mixed
kernel against mnet_paste_ordered_u8 on the same cells: the cost of the kind switch and of the larger kernel.  Scene (b): those lines plus 6 arcs of
6 segments and 4 rotated quadrilaterals beside them, all disjoint — the ONE mixed launch against the sum of mnet_paste_ordered_u8,
mnet_quad_paste_u8 and mnet_curve_paste_u8 on their own parts (three launches between the same two events).  Scene (c): scene (b) with every arc
laid over two lines and more — the mixed kernel alone: nothing else can paste it.  The atlas of upright foregrounds is made once, outside the
timed windows, for both sides.  Before anything is timed the pages of the two sides are compared byte for byte.  ``bin_items_ms`` is the host time
of regions.bin_items (a host clock).  One JSON line on stdout."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from marconet_amd import ops, pages, regions          # noqa: E402
from ordered_paste_time import FEATHER, PAGE_H, PAGE_W, ROWS, SCALE, timed          # noqa: E402


def arc(cx, cy, r_in, r_out, deg0, deg1, K):
    a = [math.radians(d) for d in np.linspace(deg0, deg1, K)]
    top = [[cx + r_out * math.cos(t), cy - r_out * math.sin(t)] for t in a]
    bot = [[cx + r_in * math.cos(t), cy - r_in * math.sin(t)] for t in a]
    return top + bot[::-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    dev = "cuda"
    H, W = SCALE * PAGE_H, SCALE * PAGE_W
    g = torch.Generator(device="cpu").manual_seed(1)
    background = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    out_w = 3413                                                                  # a 1600 x 60 px line restored at 128 rows
    joined = torch.randint(0, 256, (50, ROWS, out_w, 3), dtype=torch.uint8, generator=g).to(dev)
    lines = [dict(box=[200, 60 + 85 * i, 1800, 120 + 85 * i]) for i in range(40)]
    quads = [dict(quad=[[1900, 2900 + 140 * j], [2400, 2930 + 140 * j], [2396, 2990 + 140 * j], [1896, 2960 + 140 * j]]) for j in range(4)]
    arcs_beside = [dict(polygon=arc(2150.0, 350.0 + 500 * k, 180.0, 250.0, 160.0, 20.0, 7)) for k in range(6)]
    arcs_over = [dict(polygon=arc(1000.0, 350.0 + 500 * k, 180.0, 250.0, 160.0, 20.0, 7)) for k in range(6)]
    tiles_x, tiles_y = ops.page_tiles(H, W)
    res = dict(page=[PAGE_W, PAGE_H], scale=SCALE, feather=FEATHER, reps=a.reps, launches=a.launches, page_tiles=tiles_x * tiles_y)
    up = lambda t: ops.table_to_device(t, dev) if len(t) else None              # noqa: E731

    def tables(regs, overlap):
        recs = regions.normalize_regions(PAGE_H, PAGE_W, regs, [True] * len(regs), None, None, SCALE, FEATHER, overlap, ROWS)
        ws = [out_w if r["kind"] == "line" else min(out_w, -(-ROWS * r["cw"] // r["ch"])) for r in recs]
        return regions.mixed_tables(recs, ws, FEATHER, ROWS)

    def mixed(tabs):
        """→ (the launch, its page, the atlas, the spans, the order's length, bin_items' host times)"""
        host = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            spans, order = regions.bin_items(tabs["entries"], tabs["entry_item"], H, W)
            host.append(1e3 * (time.perf_counter() - t0))
        atlas = None
        if tabs["fg"] is not None:
            atlas = ops.paste_u8(joined, ops.table_to_device(tabs["fg"], dev), torch.zeros(tuple(tabs["atlas_hw"]) + (3,), dtype=torch.uint8, device=dev))
        d = [joined if len(tabs["cells"]) else None, atlas, up(tabs["cells"]), up(tabs["quads"]), up(tabs["curves"]), up(tabs["segs"]),
             ops.table_to_device(tabs["items"], dev), ops.table_to_device(spans, dev), torch.from_numpy(order).to(dev)]
        page = background.clone()
        return (lambda: ops.paste_mixed_u8(*d, page)), page, atlas, spans, len(order), (float(np.median(host)), float(min(host)), float(max(host)))

    def record(name, tabs, spans, n_order, host, old_ms, new_ms, **more):
        res[name] = dict(items=len(tabs["items"]), cells=len(tabs["cells"]), quads=len(tabs["quads"]), curves=len(tabs["curves"]), segments=len(tabs["segs"]),
                         workgroups=tiles_x * tiles_y, workgroups_with_work=int(np.count_nonzero(spans["count"])), order_entries=n_order,
                         deepest_tile=int(spans["count"].max()), bin_items_ms=host, old_ms=old_ms, mixed_ms=new_ms, **more)

    def ordered_launch(cells, page):
        spans, order = pages.bin_tiles(cells, H, W)
        d = [ops.table_to_device(cells, dev), ops.table_to_device(spans, dev), torch.from_numpy(order).to(dev)]
        return lambda: ops.paste_ordered_u8(joined, *d, page)

    # (a) 40 disjoint lines: the mixed kernel and the ordered kernel on the same cells
    tabs = tables(lines, "refuse")
    new, new_page, _, spans, n_order, host = mixed(tabs)
    old_page = background.clone()
    old = ordered_launch(tabs["cells"], old_page)
    old(), new()
    assert torch.equal(old_page, new_page) and not torch.equal(new_page, background)
    record("lines_40", tabs, spans, n_order, host, *timed([old, new], a.reps, a.launches))
    del old_page, new_page

    # (b) the lines, 6 arcs and 4 quadrilaterals, disjoint: one launch against the three kernels' sum
    tabs = tables(lines + arcs_beside + quads, "refuse")
    new, new_page, atlas, spans, n_order, host = mixed(tabs)
    old_page = background.clone()
    old_cells = ordered_launch(tabs["cells"], old_page)
    quads_d, curves_d, segs_d = up(tabs["quads"]), up(tabs["curves"]), up(tabs["segs"])
    qmax, cmax = (int(tabs["quads"]["bw"].max()), int(tabs["quads"]["bh"].max())), (int(tabs["curves"]["bw"].max()), int(tabs["curves"]["bh"].max()))

    def old():
        old_cells()
        ops.quad_paste_u8(atlas, quads_d, qmax[0], qmax[1], old_page)
        ops.curve_paste_u8(atlas, curves_d, segs_d, cmax[0], cmax[1], old_page)

    old(), new()
    assert torch.equal(old_page, new_page) and not torch.equal(new_page, background)
    parts = timed([old_cells, lambda: ops.quad_paste_u8(atlas, quads_d, qmax[0], qmax[1], old_page),
                   lambda: ops.curve_paste_u8(atlas, curves_d, segs_d, cmax[0], cmax[1], old_page)], a.reps, a.launches)
    record("lines_40_arcs_6_quads_4", tabs, spans, n_order, host, *timed([old, new], a.reps, a.launches), old_parts_ms=dict(zip(("ordered", "quad", "curve"), parts)))
    del old_page, new_page

    # (c) every arc laid over the lines: the mixed kernel alone
    tabs = tables(lines + arcs_over + quads, "order")
    new, new_page, _, spans, n_order, host = mixed(tabs)
    new()
    assert not torch.equal(new_page, background) and int(spans["count"].max()) >= 2
    record("lines_40_arcs_6_over_them_quads_4", tabs, spans, n_order, host, None, timed([new], a.reps, a.launches)[0])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
