#!/usr/bin/env python
"""A bare scanned page in, the enlarged page with every text line found, read and restored in place out (MarconetPipeline.restore_page_auto).

    python examples/restore_scan.py -i page.png -o out.png [--text-h N] [--floor N] [--deskew | --slope N] [--regions-out found.json] [--scale 4]
                                    [--feather 8] [--precision fp16x2]

Nobody supplies boxes or texts.  The lines are found by a recursive XY-cut over ink profiles (marconet_amd/layout.py states the rules): horizontal
lines in one or more columns on plain paper.  ``--text-h``: the expected height of a line in pixels (default max(8, page height // 100)); every
other size of the cut derives from it.  ``--floor``: the noise floor, 0..255 — a luma difference between two neighbouring pixels below it counts
as nothing (default 24).  ``--regions-out``: the found boxes as a JSON list of ``{"box": [x1, y1, x2, y2]}`` in reading order — the format
``examples/restore_page.py -r`` reads: add the texts you know, move a box, and restore again with that script.
``--deskew``: for a page that was scanned skewed — its slope is estimated from the ink profiles of sheared frames (marconet_amd/skew.py states the
rule), the lines are cut in the frame of that slope and restored as rotated rectangles; ``--slope N`` gives the slope instead (Q16: tan = N / 65536,
|N| <= 8192, positive: the lines run down to the right).  ``--regions-out`` then writes ``{"quad": [[x, y] x 4]}`` regions, which restore_page.py -r
reads as well.
Not covered: vertical columns, rotated or curved text, tables with vertical rules, text on textured backgrounds; without ``--deskew`` any skew, with
it skew beyond about 5 degrees (``--slope``: 7), 90 / 180 degree orientation, perspective and per-block skew (one slope per page) — and the quality
of the finding and of the skew estimate on real scans: the defaults are design choices, not measurements.  A box taller than 4 text heights (a figure, or lines the cut could not
part) and a box too low to paste at this scale are reported and keep the page's pixels.

Weights: ``$MARCONET_CKPT_DIR`` as in examples/restore_strips.py; without them the seeded synthetic weights run and the page shows the plumbing, not a
restoration.  Needs the GPU (there is no CPU path in this package)."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--image", type=str, required=True)
    ap.add_argument("-o", "--output", type=str, required=True)
    ap.add_argument("--text-h", type=int, default=None, help="expected height of a text line in pixels (default: max(8, page height // 100))")
    ap.add_argument("--floor", type=int, default=24, help="noise floor 0..255: a luma difference below it counts as nothing")
    ap.add_argument("--deskew", action="store_true", help="the page was scanned skewed: estimate its slope, find and restore the lines in that frame")
    ap.add_argument("--slope", type=int, default=None, help="the page's slope instead of an estimate, Q16: tan = N / 65536, -8192..8192")
    ap.add_argument("--regions-out", type=str, default=None, help="write the found boxes here, in the format restore_page.py -r reads")
    ap.add_argument("--scale", type=int, default=4, help="integer enlargement of the page, 1..8")
    ap.add_argument("--feather", type=int, default=8, help="width in output pixels of the blend at a region's edge, 0..1024 (0: none)")
    ap.add_argument("--precision", default="fp16x2", choices=["fp16x2", "fp16x3", "fp16", "fp32"])
    a = ap.parse_args(argv)
    if a.text_h is not None and a.text_h < 1:
        ap.error("--text-h must be >= 1")
    if not 0 <= a.floor <= 255:
        ap.error("--floor must lie in 0..255")
    if a.slope is not None and not -8192 <= a.slope <= 8192:
        ap.error("--slope must lie in -8192..8192")
    if a.slope is not None and a.deskew:
        ap.error("--slope gives the slope that --deskew would estimate: one of the two")
    return a


def regions_json(boxes, key="box"):
    """the found boxes — ``key`` "quad": quadrilaterals, four corners each — → the list restore_page.py's ``load_regions`` reads: no "text", so that
    script has the encoder read every region"""
    if key == "quad":
        return [dict(quad=[[float(x), float(y)] for x, y in q]) for q in boxes]
    return [dict(box=[int(v) for v in b]) for b in boxes]


def write_regions(path, boxes, key="box"):
    with open(path, "w", encoding="utf8") as f:
        json.dump(regions_json(boxes, key), f)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from marconet_amd import checkpoints, lq_io, quads
    from marconet_amd.pipeline import MarconetPipeline
    if not torch.cuda.is_available():
        raise SystemExit("restore_scan.py: no GPU visible — this package has no CPU path")
    from PIL import Image
    sde, sdg, sds, source = checkpoints.load_state_dicts()
    print("%28s : %s" % ("Weights", source))
    pipe = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, "cuda"), precision=a.precision)
    image = lq_io.load_png(a.image)
    if a.slope is not None:                                                                           # the caller's slope: find, then restore the found quadrilaterals
        found = pipe.find_lines_skewed(image, slope=a.slope, text_h=a.text_h, floor=a.floor)
        keep = [i for i, q in enumerate(found["quads"]) if a.scale * quads.crop_size(q)[1] * 16 >= 128]          # restore_page_auto's own rule
        found["skipped"] = found["skipped"] + [dict(box=b, reason="too low to paste at scale %d" % a.scale) for i, b in enumerate(found["frame_boxes"]) if i not in keep]
        found["quads"] = [found["quads"][i] for i in keep]
        page, regions = pipe.restore_page_quads(image, found["quads"], texts=None, scale=a.scale, feather=a.feather, details=True)
        found["text"] = [None if r is None else r["text"] for r in regions]
    else:
        page, found = pipe.restore_page_auto(image, scale=a.scale, feather=a.feather, details=True, text_h=a.text_h, floor=a.floor, deskew=a.deskew)
    skewed = a.deskew or a.slope is not None
    if skewed:
        print("Slope %d (Q16): %.2f degrees" % (found["slope"], math.degrees(math.atan(found["slope"] / 65536.0))))
        found["boxes"] = found["quads"]
    print("%d line(s) found in %d pass(es), %d box(es) skipped" % (len(found["boxes"]), found["passes"], len(found["skipped"])))
    for i, (box, text) in enumerate(zip(found["boxes"], found["text"])):
        print("Line %d %s: %s" % (i, box, "keeps the page's pixels (nothing read, or a character outside the alphabet)" if text is None else text))
    for s in found["skipped"]:
        print("Skipped %s: %s" % (s["box"], s["reason"]))
    if a.regions_out:
        write_regions(a.regions_out, found["boxes"], "quad" if skewed else "box")
        print("%s: %d region(s)" % (a.regions_out, len(found["boxes"])))
    Image.fromarray(page).save(a.output)
    print("%s: %d x %d" % (a.output, page.shape[1], page.shape[0]))


if __name__ == "__main__":
    main()
