#!/usr/bin/env python
"""Times the skew estimate and the finding of a skewed page's text lines (marconet_amd/skew.py, MarconetPipeline.estimate_skew /
find_lines_skewed): DESIGN.md §3's numbers.

    python tools/skew_time.py [--reps 5] [--precision fp32]

The page is tools/layout_time.py's A4 page at 300 dpi (2480 x 3508, 56 lines 35 px high in two columns and one wide line) rotated by 1.5 degrees,
nearest neighbour, onto fresh paper (tests/skew_scene.py::rotate_nearest).  Everything runs with its defaults (text_h = 35, floor 24, max_slope 6144).
Timed with device events, each as (median, min, max) in ms over ``reps`` repetitions after one warm-up:
    estimate_launch   per stage of the estimate: the table's copy and the ONE mnet_skew_ink_u8 launch — the page's frame box at every candidate
                      slope, rows only
    estimate_copy     per stage: the one device→host copy of the profiles
    pass_launch       per pass of the cut: the table's copy and the ONE mnet_skew_ink_u8 launch over all current frame boxes
    pass_copy         per pass: the one device→host copy of the profiles
beside, on a host clock: the scoring of a stage (Python integers), the whole ``estimate_skew`` and ``find_lines_skewed`` calls (the page's upload
included) and the same on a page that is on the device, ``find_lines`` on the page before it was rotated (what the finding costs without skew),
and — ONE run each, they take seconds — the host definitions ``skew.estimate_host`` and ``skew.find_lines_host``.  The device's results are compared
with the host's (==) before anything is timed.
One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from layout_time import PAGE_H, PAGE_W, a4_scene, timed_events, timed_host               # noqa: E402
from marconet_amd import _lib, checkpoints, ink, layout, ops, skew                               # noqa: E402
from marconet_amd.pipeline import MarconetPipeline                                               # noqa: E402
from tests.skew_scene import rotate_nearest                                                      # noqa: E402

DEGREES = 1.5


def once_host(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="fp32")
    a = ap.parse_args()
    dev = "cuda"
    sde, sdg, sds, _ = checkpoints.load_state_dicts(path="", regime="trained")
    pipe = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, dev), precision=a.precision)
    upright, lines = a4_scene()
    page = rotate_nearest(upright, DEGREES)
    params, eparams = layout.line_params(PAGE_H), skew.estimate_params()
    host_est, host_est_ms = once_host(lambda: skew.estimate_host(page))
    host_found, host_found_ms = once_host(lambda: skew.find_lines_host(page, slope=host_est["slope"]))
    est, found = pipe.estimate_skew(page), pipe.find_lines_skewed(page)
    assert est == host_est, "the device's estimate is the host's"
    assert found == dict(host_found, scores=host_est["scores"]), "and its lines are the host's"
    true = float(np.tan(np.radians(DEGREES)) * 65536)
    res = dict(page=[PAGE_W, PAGE_H], degrees=DEGREES, true_slope=true, slope=est["slope"], lines_drawn=len(lines), lines=len(found["quads"]),
               skipped=len(found["skipped"]), passes=found["passes"], plain_boxes_on_the_skewed_page=len(pipe.find_lines(page)["boxes"]),
               text_h=params["text_h"], floor=params["floor"], reps=a.reps, estimate=[], per_pass=[])
    page_d = torch.from_numpy(page).to(dev)
    m, state = est["slope"], {}
    dtype = np.dtype(_lib.SkewInkBox)

    def timed_table(records, row):
        tab, starts, total = skew.ink_table(records, PAGE_H, PAGE_W, dtype)
        hs, ws = np.maximum(tab["py2"] - tab["py1"], 1), np.maximum(tab["px2"] - tab["px1"], 1)

        def launch():
            state["ink"] = ops.skew_ink_u8(page_d, ops.table_to_device(tab, dev), int(hs.max()), int(ws.max()), params["floor"], dst_len=total)

        def copy():
            state["host"] = state["ink"].cpu().numpy()
        row.update(records=len(records), profile_ints=int(total), scanned_bytes=int((3 * hs.astype(np.int64) * ws).sum()))
        row["launch_ms"] = timed_events(launch, a.reps)
        row["copy_ms"] = timed_events(copy, a.reps)
        return starts

    # the estimate's two stages, their candidates taken from the estimate itself
    coarse = list(range(-eparams["max_slope"], eparams["max_slope"] + 1, eparams["coarse"]))
    for name, slopes in (("coarse", coarse), ("fine", [s for s, _ in est["scores"][len(coarse):]])):
        row = dict(stage=name)
        starts = timed_table([(skew.frame_box(PAGE_H, PAGE_W, s), s, False) for s in slopes], row)
        sizes = [skew.frame_box(PAGE_H, PAGE_W, s) for s in slopes]
        row["host_scores_ms"] = timed_host(lambda: [skew.score(state["host"][sr:sr + b[3] - b[1]]) for (sr, _), b in zip(starts, sizes)], a.reps)
        res["estimate"].append(row)
    # the boxes of every pass, recorded from one run of the cut on the device's profiles
    per_pass = []

    def recording(boxes, axis):
        per_pass.append(([list(b) for b in boxes], axis))
        return [p[axis] for p in ink.frame_profiles(page_d, [(b, m, axis == layout.AXIS_X) for b in boxes], params["floor"])]
    layout.xy_cut(recording, PAGE_H, PAGE_W, params["text_h"], start=([skew.frame_box(PAGE_H, PAGE_W, m)], [[0, 0, 0, 0]]))
    for boxes, axis in per_pass:
        row = dict(axis="Y" if axis == layout.AXIS_Y else "X")
        timed_table([(b, m, axis == layout.AXIS_X) for b in boxes], row)
        res["per_pass"].append(row)
    for key in ("launch_ms", "copy_ms"):
        res["sum_estimate_" + key] = float(sum(r[key][0] for r in res["estimate"]))
        res["sum_pass_" + key] = float(sum(r[key][0] for r in res["per_pass"]))
    res["sum_host_scores_ms"] = float(sum(r["host_scores_ms"][0] for r in res["estimate"]))
    res["estimate_skew_ms"] = timed_host(lambda: pipe.estimate_skew(page), a.reps)
    res["estimate_skew_on_device_page_ms"] = timed_host(lambda: pipe._estimate_skew(page_d, eparams), a.reps)
    res["find_lines_skewed_ms"] = timed_host(lambda: pipe.find_lines_skewed(page), a.reps)
    res["find_lines_skewed_on_device_page_ms"] = timed_host(lambda: pipe._find_lines_skewed(page_d, params, None), a.reps)
    res["find_lines_skewed_given_slope_on_device_page_ms"] = timed_host(lambda: pipe._find_lines_skewed(page_d, params, m), a.reps)
    res["find_lines_upright_ms"] = timed_host(lambda: pipe.find_lines(upright), a.reps)
    upright_d = torch.from_numpy(upright).to(dev)
    res["find_lines_upright_on_device_page_ms"] = timed_host(lambda: pipe._find_lines(upright_d, params), a.reps)
    res["estimate_host_ms"], res["find_lines_host_given_slope_ms"] = host_est_ms, host_found_ms
    print(json.dumps(res))


if __name__ == "__main__":
    main()
