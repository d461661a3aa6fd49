#!/usr/bin/env python
"""A page and its text-line boxes in, the enlarged page with every text line restored in place out (MarconetPipeline.restore_page).

    python examples/restore_page.py -i page.png -r regions.json -o out.png [--scale 4] [--feather 8] [--overlap refuse] [--blind-columns] [--precision fp16x2]

``regions.json`` is a list of ``{"box": [x1, y1, x2, y2], "text": "...", "char_boxes": [[x1, y1, x2, y2], ...]}``: a text line's box in page pixels
(axis-aligned; numbers that are not integers are rounded outward), its characters, and — optionally — its character boxes in page pixels (evenly
spaced ones otherwise).  The detector that produces the boxes is the caller's (SURVEY.md §8f NEXT-4); so is the recogniser, but a region WITHOUT
``"text"`` is read by the encoder itself (marconet_amd/blind.py: overlapping probe windows give its text and character boxes; a ``"vertical"``
region only with ``--blind-columns``: its cells are then measured from its ink profile, marconet_amd/blind_columns.py — without the flag it is refused,
its cells being cut from its text).  A region with no character or
with a character outside the alphabet keeps the enlarged page's own pixels, as the script skips such a strip (test_sr.py:168-170, :181-190).
A region may carry ``"quad": [[x, y], [x, y], [x, y], [x, y]]`` instead of ``"box"``: the four corners of a rotated or perspective line in its own
reading order (top-left, top-right, bottom-right, bottom-left as the line is read).  If any region does, all regions go through
``MarconetPipeline.restore_page_quads``, each box as its four corners — the same bytes for an integer box; a file with only boxes takes ``restore_page``.
A region with a ``"box"`` may carry ``"vertical": true``: a column of upright characters stacked top to bottom (a shop sign, a couplet, a book
spine), its ``"char_boxes"`` listed top to bottom.  If any region does, all regions go through ``MarconetPipeline.restore_page_columns``, the others as
horizontal lines — ``restore_page``'s bytes for them.  A file that holds both a ``"vertical"`` region and a ``"quad"`` is refused: no entry point takes both.
A region may carry ``"polygon": [[x, y], ...]`` instead: the 2K points (4 to 66) of a curved line — the top side left to right in reading order, then the
bottom side right to left, what a detector of curved text emits.  If any region does, all regions go through ``MarconetPipeline.restore_page_curves``,
each box or quadrilateral as its four points — the same bytes for an integer box.  A file that holds both a ``"vertical"`` region and a ``"polygon"`` is
refused, as with ``"quad"``.
Two regions that share a pixel are refused by default.  ``--overlap order`` pastes overlapping regions in the file's order instead (painter's order: a later
region is blended, under its own feather ramp, over the earlier ones) — stacked lines whose outward-rounded boxes share a row, a sign's column over the
line next to it.  It applies to ``"box"`` regions, ``"vertical"`` ones included; a file with a ``"quad"`` or a ``"polygon"`` is refused with it: those kinds
still refuse overlaps.
Not covered: overlapping quadrilateral and curved regions, vertical columns that are rotated, in perspective or curved, the quality of a blind
column's segmentation and reading (columns whose cells are far from square), several pages per call.

All regions are restored as one batch; the page is enlarged (cv2's INTER_CUBIC arithmetic) and every line resized, pasted and feathered on the GPU —
only the PNG decode and encode run on the host.  Weights: ``$MARCONET_CKPT_DIR`` as in examples/restore_strips.py; without them the seeded
synthetic weights run and the page shows the plumbing, not a restoration.  Needs the GPU (there is no CPU path in this package)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from marconet_amd import checkpoints, lq_io                                      # noqa: E402
from marconet_amd.pipeline import MarconetPipeline                               # noqa: E402


def load_regions(path, blind_columns=False):
    """→ (boxes, texts, char_boxes or None, quads or None, vertical or None, polygons or None): ``quads`` where any region carries "quad" — then every
    region's four corners, a box turned into its own; ``blind_columns``: a "vertical" region may come without "text" (``--blind-columns`` reads it); ``vertical`` where any region carries "vertical": true — then one flag per region; ``polygons``
    where any region carries "polygon" — then every region's points, a box or a quadrilateral turned into its four"""
    with open(path, encoding="utf8") as f:
        regions = json.load(f)
    def well_formed(r):
        if not isinstance(r, dict) or not isinstance(r.get("text", ""), str) or ("box" in r) + ("quad" in r) + ("polygon" in r) != 1:
            return False
        if not isinstance(r.get("vertical", False), bool) or ("vertical" in r and "box" not in r):
            return False
        if r.get("vertical", False) and "text" not in r and not blind_columns:      # a column's cells are cut from its text: read only on request
            return False
        if "box" in r:
            return isinstance(r["box"], list) and len(r["box"]) == 4 and all(isinstance(v, (int, float)) for v in r["box"])
        pts = r["quad"] if "quad" in r else r["polygon"]
        return isinstance(pts, list) and (len(pts) == 4 if "quad" in r else len(pts) >= 4) and all(
            isinstance(p, list) and len(p) == 2 and all(isinstance(v, (int, float)) for v in p) for p in pts)

    if not isinstance(regions, list) or not all(well_formed(r) for r in regions):
        raise SystemExit('restore_page.py: %s must hold a list of {"box": [x1, y1, x2, y2], "text": "..."} or {"quad": [[x, y], [x, y], [x, y], [x, y]], '
                         '"text": "..."} or {"polygon": [[x, y], ...], "text": "..."} objects (numbers; one of "box", "quad" and "polygon" per region; '
                         '"vertical": true or false beside a "box" only; "text" may be left out — the region is then read by the encoder — except for a '
                         '"vertical" region without --blind-columns)' % path)
    vertical = [bool(r.get("vertical", False)) for r in regions] if any(r.get("vertical", False) for r in regions) else None
    if vertical is not None and any("quad" in r for r in regions):
        raise SystemExit('restore_page.py: %s holds a "vertical" region (%d) and a "quad" region (%d): vertical columns go through restore_page_columns, '
                         'which takes axis-aligned boxes only, and restore_page_quads has no vertical columns — give the quadrilateral as a "box", or restore '
                         'the two kinds in two calls' % (path, vertical.index(True), next(i for i, r in enumerate(regions) if "quad" in r)))
    if vertical is not None and any("polygon" in r for r in regions):
        raise SystemExit('restore_page.py: %s holds a "vertical" region (%d) and a "polygon" region (%d): vertical columns go through restore_page_columns, '
                         'which takes axis-aligned boxes only, and restore_page_curves has no vertical columns — restore the two kinds in two calls'
                         % (path, vertical.index(True), next(i for i, r in enumerate(regions) if "polygon" in r)))
    char_boxes = [r.get("char_boxes") for r in regions]
    quads = None
    if any("quad" in r or "polygon" in r for r in regions):
        quads = [r["quad"] if "quad" in r else None if "polygon" in r else [[r["box"][0], r["box"][1]], [r["box"][2], r["box"][1]], [r["box"][2], r["box"][3]],
                                                                     [r["box"][0], r["box"][3]]] for r in regions]
    polygons = None
    if any("polygon" in r for r in regions):
        polygons = [r["polygon"] if "polygon" in r else q for r, q in zip(regions, quads)]
    return ([r.get("box") for r in regions], [r.get("text") for r in regions], char_boxes if any(c is not None for c in char_boxes) else None, quads, vertical,
            polygons)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--image", type=str, required=True)
    ap.add_argument("-r", "--regions", type=str, required=True)
    ap.add_argument("-o", "--output", type=str, required=True)
    ap.add_argument("--scale", type=int, default=4, help="integer enlargement of the page, 1..8")
    ap.add_argument("--feather", type=int, default=8, help="width in output pixels of the blend at a region's edge, 0..1024 (0: none)")
    ap.add_argument("--overlap", default="refuse", choices=["refuse", "order"],
                    help="order: overlapping box regions are pasted in the file's order (a later one over the earlier ones); refuse: they are an error")
    ap.add_argument("--blind-columns", action="store_true",
                    help='read a "vertical" region that has no "text": its cells are measured from its ink profile (marconet_amd/blind_columns.py)')
    ap.add_argument("--precision", default="fp16x2", choices=["fp16x2", "fp16x3", "fp16", "fp32"])
    a = ap.parse_args()
    boxes, texts, char_boxes, quads, vertical, polygons = load_regions(a.regions, a.blind_columns)
    if a.overlap == "order" and (quads is not None or polygons is not None):
        raise SystemExit('restore_page.py: --overlap order applies to "box" regions ("vertical" ones included); %s holds a "quad" or a "polygon", and '
                         'quadrilateral and curved regions still refuse overlaps' % a.regions)
    if not torch.cuda.is_available():
        raise SystemExit("restore_page.py: no GPU visible — this package has no CPU path")
    from PIL import Image
    sde, sdg, sds, source = checkpoints.load_state_dicts()
    print("%28s : %s" % ("Weights", source))
    pipe = MarconetPipeline(*checkpoints.build_networks(sde, sdg, sds, "cuda"), precision=a.precision)
    if vertical is not None:
        page, regions = pipe.restore_page_columns(lq_io.load_png(a.image), boxes, texts, vertical=vertical, char_boxes=char_boxes, scale=a.scale, feather=a.feather,
                                                  details=True, overlap=a.overlap, blind_columns=a.blind_columns)
    elif polygons is not None:
        page, regions = pipe.restore_page_curves(lq_io.load_png(a.image), polygons, texts, char_boxes=char_boxes, scale=a.scale, feather=a.feather, details=True)
    elif quads is not None:
        page, regions = pipe.restore_page_quads(lq_io.load_png(a.image), quads, texts, char_boxes=char_boxes, scale=a.scale, feather=a.feather, details=True)
    else:
        page, regions = pipe.restore_page(lq_io.load_png(a.image), boxes, texts, char_boxes=char_boxes, scale=a.scale, feather=a.feather, details=True,
                                          overlap=a.overlap)
    for i, (r, text) in enumerate(zip(regions, texts)):
        if text is None and r is not None:
            text = "%s (read%s)" % (r["text"], ", a probe window held more than 16 characters" if r["overflow"] else "")
        if r is None:
            print("Region %d keeps the page's pixels (no character, or a character outside the alphabet): %r" % (i, text))
        elif "cuts" in r:
            print("Region %d: a column of %d cell(s) in %d window(s), restored line %d px wide -> rectangle %s: %s"
                  % (i, len(r["widths"]), len(r["plan"]), r["out_w"], r["rect"], text))
        elif polygons is not None:
            print("Region %d: %d window(s), restored line %d px wide -> %d x %d along the %d-point polygon %s: %s"
                  % (i, len(r["plan"]), r["out_w"], r["size"][0], r["size"][1], len(r["polygon"]), [list(p) for p in r["polygon"]], text))
        elif quads is not None:
            print("Region %d: %d window(s), restored line %d px wide -> %d x %d in quadrilateral %s: %s"
                  % (i, len(r["plan"]), r["out_w"], r["size"][0], r["size"][1], [list(p) for p in r["quad"]], text))
        else:
            print("Region %d: %d window(s), restored line %d px wide -> rectangle %s: %s" % (i, len(r["plan"]), r["out_w"], r["rect"], text))
    Image.fromarray(page).save(a.output)
    print("%s: %d x %d" % (a.output, page.shape[1], page.shape[0]))


if __name__ == "__main__":
    main()
