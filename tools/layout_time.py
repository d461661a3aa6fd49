#!/usr/bin/env python
"""Times the finding of a page's text lines (marconet_amd/layout.py, MarconetPipeline.find_lines): DESIGN.md §3's numbers.

    python tools/layout_time.py [--reps 5] [--precision fp32]

The page is an A4 page at 300 dpi (2480 x 3508): two columns of 30 and 25 lines 35 px high at pitches 50 and 60 (their blank rows coincide here
and there, so the cut meets bands of one or two lines as well as blocks), a gutter of at least 140 px, one wide line below, paper noise of
amplitude 5 (under the floor of 24); a glyph is a block of random two-level texture.  The cut runs with its defaults (text_h = 35).
Timed with device events, each as (median, min, max) in ms over ``reps`` repetitions after one warm-up:
    pass_launch    per pass of the cut: the table's copy and the ONE mnet_box_ink_u8 launch over all current boxes as views of the page
    profiles_copy  per pass: the one device→host copy of the profiles
beside, on a host clock, per pass ``layout.xy_cut``'s own work (the cuts, on the profiles the device returned), numpy ``box_ink`` over the same
boxes in the same run (the host's only way to the profiles), the whole ``find_lines`` call (the page's upload included) and the whole
``find_lines_host``.  The device's result is compared with the host's (==) before anything is timed.
One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from marconet_amd import _lib, checkpoints, layout, ops                                          # noqa: E402
from marconet_amd.pipeline import MarconetPipeline                                               # noqa: E402

PAGE_W, PAGE_H, TEXT_H = 2480, 3508, 35


def a4_scene(seed=1):
    """→ (page uint8 [3508, 2480, 3], the 56 drawn lines [x1, y1, x2, y2] in reading order)"""
    rng = np.random.default_rng(seed)
    page = (230 + rng.integers(-5, 6, (PAGE_H, PAGE_W, 1))).astype(np.uint8).repeat(3, axis=2)

    def draw(x1, y1, x2):
        x = x1
        while True:
            gw = int(rng.integers(14, 28))
            if x + gw > x2:
                return [x1, y1, x - 8, y1 + TEXT_H]
            tex = rng.integers(0, 2, (TEXT_H, gw))
            tex[:, 0] = tex[:, -1] = 1
            page[y1:y1 + TEXT_H, x:x + gw] = np.where(tex, 30, 110).astype(np.uint8)[..., None]
            x += gw + 8
    lines = [draw(200, 200 + 50 * k, 1170 - int(rng.integers(0, 200))) for k in range(30)]
    lines += [draw(1310, 215 + 60 * k, 2280 - int(rng.integers(0, 200))) for k in range(25)]
    lines.append(draw(200, 3200, 2280))
    return page, lines


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
    page, lines = a4_scene()
    params = layout.line_params(PAGE_H)
    host = layout.find_lines_host(page)
    found = pipe.find_lines(page)
    assert found == host, "the device's lines are the host's"
    assert sorted(found["tight"]) == sorted([b[0] - 1, b[1], b[2] + 1, b[3]] for b in lines), "and the drawn ones, every one"
    page_d = torch.from_numpy(page).to(dev)
    flat = page_d.reshape(-1)

    # the boxes of every pass, recorded from one run of the cut on the host's profiles
    per_pass = []

    def recording(boxes, axis):
        per_pass.append(([list(b) for b in boxes], axis))
        return [layout.box_ink(page, b, params["floor"])[axis] for b in boxes]
    layout.xy_cut(recording, PAGE_H, PAGE_W, params["text_h"])
    res = dict(page=[PAGE_W, PAGE_H], lines=len(found["boxes"]), passes=found["passes"], text_h=params["text_h"], floor=params["floor"], reps=a.reps, per_pass=[])
    state = {}
    for boxes, axis in per_pass:
        tab, starts, total = layout.ink_table(boxes, PAGE_W, np.dtype(_lib.BoxInkBox))

        def launch():
            state["ink"] = ops.box_ink_u8(flat, ops.table_to_device(tab, dev), int(tab["h"].max()), int(tab["w"].max()), params["floor"], dst_len=total)

        def copy():
            state["host"] = state["ink"].cpu().numpy()

        def host_ink():
            state["numpy"] = [layout.box_ink(page, b, params["floor"]) for b in boxes]

        def cuts():
            for (s_r, s_c), b in zip(starts, boxes):
                h, w = b[3] - b[1], b[2] - b[0]
                prof = state["host"][s_r:s_r + h] if axis == layout.AXIS_Y else layout.pixel_profile(state["host"][s_c:s_c + w])
                layout.cut(prof, max(1, params["text_h"] // 8) if axis == layout.AXIS_Y else 2 * params["text_h"])
        row = dict(axis="Y" if axis == layout.AXIS_Y else "X", boxes=len(boxes), profile_ints=int(total),
                   box_bytes=int(sum(3 * (b[2] - b[0]) * (b[3] - b[1]) for b in boxes)))
        row["pass_launch_ms"] = timed_events(launch, a.reps)
        row["profiles_copy_ms"] = timed_events(copy, a.reps)
        row["host_box_ink_ms"] = timed_host(host_ink, a.reps)
        want = np.concatenate([np.concatenate(rc) for rc in state["numpy"]])
        assert np.array_equal(state["host"], want)
        row["host_cuts_ms"] = timed_host(cuts, a.reps)
        res["per_pass"].append(row)
    for key in ("pass_launch_ms", "profiles_copy_ms", "host_box_ink_ms", "host_cuts_ms"):
        res["sum_" + key] = float(sum(r[key][0] for r in res["per_pass"]))
    res["find_lines_ms"] = timed_host(lambda: pipe.find_lines(page), a.reps)
    res["find_lines_on_device_page_ms"] = timed_host(lambda: pipe._find_lines(page_d, params), a.reps)
    res["find_lines_host_ms"] = timed_host(lambda: layout.find_lines_host(page), max(1, a.reps // 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
