#!/usr/bin/env python
"""Times the ordered page compositor (mnet_paste_ordered_u8: workgroups own page tiles) with device events, beside the per-descriptor paste kernels
(mnet_column_paste_u8, mnet_paste_u8) on the same tables in the same run: DESIGN.md §3's numbers.

    python tools/ordered_paste_time.py [--reps 7] [--launches 20]

The page is an A4 page at 300 dpi (2480 x 3508), scale 4, feather 8, lines of 128 rows.  Scene (a): 40 columns of 30 characters (50 x 110 px cells),
disjoint — both kernels on one cell table.  Scene (b): 40 disjoint lines of 2080 x 60 px — both kernels on the same regions.  Scene (c): 60 lines of
2080 x 58 px at a pitch of 56 rows, each overlapping its neighbour by two page rows — the ordered kernel alone: nothing else can paste it.  Before
anything is timed the two kernels' pages are compared byte for byte.  Each figure is (median, min, max) in ms over ``reps`` repetitions of the time
of ``launches`` back-to-back launches between two events, divided by ``launches``, after a warm-up of as many launches; within a repetition the two
kernels alternate.  ``bin_tiles_ms`` is the host time of pages.bin_tiles (a host clock).  The workgroup counts follow from the shapes.  One JSON
line on stdout.
Scene (a) as one mnet_column_paste_u8 launch is 1200 x 135 935 workgroups of 256 threads, more than 2^32 threads: the launch runs only the
workgroups that remain after the thread count wraps (about 89 cells' worth) and leaves the other cells unpasted.  So the per-descriptor kernel is
run there as 10 launches of 4 columns each, which together paste the whole scene and are what is compared and timed (``old_ms``); the single,
incomplete launch is timed beside them (``old_single_launch_ms``, with the share of the scene's pixels it pastes)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from marconet_amd import columns, ops, pages          # noqa: E402

PAGE_W, PAGE_H, SCALE, FEATHER, ROWS = 2480, 3508, 4, 8, 128


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


def timed(fns, reps, launches):
    """the launches of ``fns`` alternating within every repetition → per function (median, min, max) in ms"""
    for fn in fns:
        for _ in range(launches):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            out[k].append(window(fn, launches))
    return [(float(np.median(o)), float(min(o)), float(max(o))) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    dev = "cuda"
    H, W = SCALE * PAGE_H, SCALE * PAGE_W
    g = torch.Generator(device="cpu").manual_seed(1)
    background = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    tiles_x, tiles_y = ops.page_tiles(H, W)
    res = dict(page=[PAGE_W, PAGE_H], scale=SCALE, feather=FEATHER, reps=a.reps, launches=a.launches, page_tiles=tiles_x * tiles_y)

    def ordered(lines, cells):
        """→ (the launch, its page, the spans, the order's length)"""
        spans, order = pages.bin_tiles(cells, H, W)
        cells_d, spans_d, order_d = ops.table_to_device(cells, dev), ops.table_to_device(spans, dev), torch.from_numpy(order).to(dev)
        page = background.clone()
        return (lambda: ops.paste_ordered_u8(lines, cells_d, spans_d, order_d, page)), page, spans, len(order)

    def record(name, n, spans, n_order, old_ms, new_ms):
        res[name] = dict(descriptors=n, old_workgroups=None if old_ms is None else n * tiles_x * tiles_y, ordered_workgroups=tiles_x * tiles_y,
                         ordered_workgroups_with_work=int(np.count_nonzero(spans["count"])), order_entries=n_order, old_ms=old_ms, ordered_ms=new_ms)

    # (a) 40 columns of 30 characters
    cols = []
    for c in range(40):
        box = [20 + 60 * c, 100, 70 + 60 * c, 100 + 30 * 110]
        cuts = columns.cell_cuts(box, 30)
        cols.append((box, cuts, columns.cell_widths(box, cuts), None))
    rects = [(SCALE * b[0], SCALE * b[1], SCALE * (b[2] - b[0]), SCALE * (b[3] - b[1])) for b, _, _, _ in cols]
    line_w = (ROWS // columns.LQ_H) * max(sum(c[2]) for c in cols)
    col_lines = torch.randint(0, 256, (40, ROWS, line_w, 3), dtype=torch.uint8, generator=g).to(dev)
    cells = columns.paste_table(cols, list(range(40)), rects, FEATHER, ROWS)
    cells_d = ops.table_to_device(cells, dev)
    per_launch = ((2 ** 32 - 1) // 256 // (tiles_x * tiles_y)) // 30 * 30          # whole columns whose workgroups' threads stay under 2^32
    assert per_launch >= 30
    old_page, single_page = background.clone(), background.clone()

    def old():
        for c0 in range(0, len(cells), per_launch):
            ops.column_paste_u8(col_lines, cells_d[c0:c0 + per_launch], old_page)

    single = lambda: ops.column_paste_u8(col_lines, cells_d, single_page)         # noqa: E731
    new, new_page, spans, n_order = ordered(col_lines, cells)
    old(), new(), single()
    assert torch.equal(old_page, new_page) and not torch.equal(new_page, background)
    pasted = lambda page: int((page != background).any(dim=2).sum().item())       # noqa: E731
    single_share = pasted(single_page) / pasted(new_page)
    host = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        pages.bin_tiles(cells, H, W)
        host.append(1e3 * (time.perf_counter() - t0))
    old_ms, new_ms, single_ms = timed([old, new, single], a.reps, a.launches)
    record("columns_40x30", len(cells), spans, n_order, old_ms, new_ms)
    res["columns_40x30"].update(old_launches=-(-len(cells) // per_launch), old_single_launch_ms=single_ms, old_single_launch_pixel_share=single_share)
    res["columns_40x30"]["bin_tiles_ms"] = (float(np.median(host)), float(min(host)), float(max(host)))
    del col_lines, old_page, new_page, single_page

    # (b) 40 disjoint lines, (c) 60 lines that overlap their neighbours by two page rows
    out_w = 4437                                                                  # a 2080 x 60 px line restored at 128 rows
    lines = torch.randint(0, 256, (40, ROWS, out_w, 3), dtype=torch.uint8, generator=g).to(dev)
    boxes_b = [[200, 60 + 85 * i, 2280, 120 + 85 * i] for i in range(40)]
    boxes_c = [[200, 60 + 56 * i, 2280, 118 + 56 * i] for i in range(60)]
    rects_b = pages.region_rects(PAGE_H, PAGE_W, boxes_b, [True] * 40, SCALE, FEATHER, ROWS)
    rects_c = pages.region_rects(PAGE_H, PAGE_W, boxes_c, [True] * 60, SCALE, FEATHER, ROWS, overlap="order")
    reg = pages.build_table(rects_b, [out_w] * 40, FEATHER, ROWS)
    reg_d = ops.table_to_device(reg, dev)
    old_page = background.clone()
    old = lambda: ops.paste_u8(lines, reg_d, old_page)                            # noqa: E731
    new, new_page, spans, n_order = ordered(lines, pages.as_cell(reg))
    old(), new()
    assert torch.equal(old_page, new_page) and not torch.equal(new_page, background)
    record("lines_40", len(reg), spans, n_order, *timed([old, new], a.reps, a.launches))
    del old_page, new_page
    cells_c = pages.as_cell(pages.build_table(rects_c, [out_w] * 60, FEATHER, ROWS, [i % 40 for i in range(60)]))
    new, new_page, spans, n_order = ordered(lines, cells_c)
    new()
    assert not torch.equal(new_page, background) and int(spans["count"].max()) == 2
    record("lines_60_overlapping", len(cells_c), spans, n_order, None, timed([new], a.reps, a.launches)[0])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
