#!/usr/bin/env python
"""A page and text regions of ANY mix of kinds in, the enlarged page with every region restored in place out (MarconetPipeline.restore_page_regions).

    python examples/restore_regions.py -i page.png -r regions.json -o out.png [--scale 4] [--feather 8] [--overlap refuse] [--blind-columns] [--precision fp16x2]

``regions.json`` is the file examples/restore_page.py reads: a list of objects with ``"text"`` and exactly one of ``"box": [x1, y1, x2, y2]`` (a text
line; with ``"vertical": true`` a column of upright characters), ``"quad": [[x, y] x 4]`` (a rotated or perspective line, corners in reading order)
and ``"polygon": [[x, y], ...]`` (the 2K points of a curved line), optionally with ``"char_boxes"`` in page pixels.  Any mix is accepted and the page
is restored in ONE call: a line, a column, a slanted stamp and a seal over the line.  A region WITHOUT ``"text"`` is read by the encoder itself
(marconet_amd/blind.py; a ``"vertical"`` region only with ``--blind-columns``, which measures its cells from its ink profile —
marconet_amd/blind_columns.py —; without the flag it is refused by name, its cells being cut from its text).
Two regions whose interiors intersect, of whatever kinds, are refused by default; ``--overlap order`` pastes them in the file's order (painter's
order: a later region is blended, under its own feather ramp, over the earlier ones).
Not covered: a blend other than painter's order, vertical columns that are rotated or curved, the quality of a blind column's segmentation and
reading (columns whose cells are far from square), detection, several pages per call.

Weights: ``$MARCONET_CKPT_DIR`` as in examples/restore_strips.py; without them the seeded synthetic weights run and the page shows the plumbing, not a
restoration.  Needs the GPU (there is no CPU path in this package)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from marconet_amd import checkpoints, lq_io, regions as rg                        # noqa: E402
from marconet_amd.pipeline import MarconetPipeline                               # noqa: E402


def load_regions(path):
    """→ (the region dicts, their texts, their character boxes or None)"""
    with open(path, encoding="utf8") as f:
        regions = json.load(f)
    if not isinstance(regions, list) or not all(isinstance(r, dict) and isinstance(r.get("text", ""), str) for r in regions):
        raise SystemExit('restore_regions.py: %s must hold a list of objects with one of "box", "quad" and "polygon" and a "text" (a region without '
                         '"text" is read by the encoder)' % path)
    try:
        for i, r in enumerate(regions):
            rg.region_kind(r, i)
    except ValueError as e:
        raise SystemExit("restore_regions.py: %s: %s" % (path, e))
    char_boxes = [r.get("char_boxes") for r in regions]
    return regions, [r.get("text") for r in regions], char_boxes if any(c is not None for c in char_boxes) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--image", type=str, required=True)
    ap.add_argument("-r", "--regions", type=str, required=True)
    ap.add_argument("-o", "--output", type=str, required=True)
    ap.add_argument("--scale", type=int, default=4, help="integer enlargement of the page, 1..8")
    ap.add_argument("--feather", type=int, default=8, help="width in output pixels of the blend at a region's edge, 0..1024 (0: none)")
    ap.add_argument("--overlap", default="refuse", choices=["refuse", "order"],
                    help="order: overlapping regions of any kind are pasted in the file's order (a later one over the earlier ones); refuse: they are an error")
    ap.add_argument("--blind-columns", action="store_true",
                    help='read a "vertical" region that has no "text": its cells are measured from its ink profile (marconet_amd/blind_columns.py)')
    ap.add_argument("--precision", default="fp16x2", choices=["fp16x2", "fp16x3", "fp16", "fp32"])
    a = ap.parse_args()
    regions, texts, char_boxes = load_regions(a.regions)
    if not torch.cuda.is_available():
        raise SystemExit("restore_regions.py: no GPU visible — this package has no CPU path")
    from PIL import Image
    sde, sdg, sds, source = checkpoints.load_state_dicts()
    print("%28s : %s" % ("Weights", source))
    pipe = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, "cuda"), precision=a.precision)
    page, info = pipe.restore_page_regions(lq_io.load_png(a.image), regions, texts, char_boxes=char_boxes, scale=a.scale, feather=a.feather, details=True,
                                           overlap=a.overlap, blind_columns=a.blind_columns)
    for i, (r, text) in enumerate(zip(info, texts)):
        if text is None and r is not None:
            text = "%s (read%s)" % (r["text"], ", a probe window held more than 16 characters" if r["overflow"] else "")
        if r is None:
            print("Region %d keeps the page's pixels (no character, or a character outside the alphabet): %r" % (i, text))
        else:
            where = "rectangle %s" % (r["rect"],) if "rect" in r else "%d x %d along %d points" % (r["size"] + (len(r.get("quad", r.get("polygon"))),))
            print("Region %d: a %s, %d window(s), restored line %d px wide -> %s: %s" % (i, r["kind"], len(r["plan"]), r["out_w"], where, text))
    Image.fromarray(page).save(a.output)
    print("%s: %d x %d" % (a.output, page.shape[1], page.shape[0]))


if __name__ == "__main__":
    main()
