"""A page that was scanned skewed: its skew and its text lines from ink profiles taken in a sheared frame.  ``layout``'s XY-cut needs blank page
rows between lines; a skew of 1 degree moves a line of 2000 px up by 35 rows and no page row is blank any more.  This module keeps every rule of
``layout`` and changes only the coordinates its profiles are taken in.  It is the pure-host definition, numpy and integers only;
``MarconetPipeline.estimate_skew`` / ``find_lines_skewed`` are the device path — every pass ONE ``mnet_skew_ink_u8`` launch — and return exactly
this (tests/test_skew_gpu.py compares them with ``==``).  It never raises on any uint8 RGB page.

The rules:

    sh                with an integer slope m (Q16: t = m / 65536, |m| <= MAX_SLOPE = 8192, tan = 0.125, about 7.1 degrees)
                      sh(v) = floor((v m + 32768) / 65536).
    frame             page pixel (x, r) has the FRAME COORDINATES r' = r − sh(x), c' = x + sh(r).  The linear part of this map,
                      (x, r) → (x + t r, r − t x), is a rotation by atan t times a uniform scale of sqrt(1 + t²): the blank rows and gutters
                      of a page skewed by atan t are blank again in the frame, an axis-aligned box of the frame is a true rotated rectangle of the
                      page, and disjoint frame boxes give disjoint page quadrilaterals.
    frame_ink         ``ink.frame_ink``, with Y, d and e as ``ink``'s head defines them.  For a frame box [c1, r1, c2, r2), whose coordinates may be
                      negative, every pair (x, r) with 0 <= x <= W − 2, 0 <= r < H, r1 <= r' < r2 and c1 <= c', c' + 1 < c2 adds e(x, r) to rows[r' − r1] and to
                      cols[c' − c1]: both pixels of a pair lie in the box and the pair is filed under its LEFT pixel, so cols[−1] = 0 and at
                      m = 0, for a box inside the page, this is ``layout.box_ink`` with ==.  Exact integers: ``mnet_skew_ink_u8`` returns both with ==.
    frame_box         the smallest frame box that holds every page pixel.
    scan_rect         a page rectangle, clipped to the page, that holds every pixel whose frame coordinates can lie in a box: what the
                      kernel's workgroups walk.  Any superset gives the same profiles.
    estimate_host     Postl's criterion: with P_m the frame's row profile of the whole page, S(m) = Σ_i (P_m[i + 1] − P_m[i])², in Python
                      integers; the slope with the largest score wins, ties go to the smaller |m|, then to the positive one.  Two stages: the
                      candidates range(−max_slope, max_slope + 1, coarse), then range(best − coarse, best + coarse + 1, fine) clipped to
                      ±MAX_SLOPE.  (The plainer score Σ P² was tried on a two-column page whose columns have different pitches and was off by
                      up to 1400 units; it is not used.)
    find_lines_host   ``layout.line_params`` unchanged; ``layout.xy_cut`` from the page's frame box with the profiles of ``frame_ink``;
                      ``layout.lines_from_profiles``' min_h / min_w / max_h rules on the frame boxes; every side grows by min(pad, max(allowance − 1,
                      0)) — one pixel less than ``layout``: two neighbours that a blank run of two or more parted keep two frame pixels between
                      them (a run of one is left as it is), so that the float rounding of the rotated corners cannot make
                      ``quads.check_quads`` see an overlap.  A quad is the four corners (top-left,
                      top-right, bottom-right, bottom-left: ``restore_page_quads``' order) of the padded frame box under the inverse linear map
                      x = (c − t r') / (1 + t²), y = (r' + t c) / (1 + t²), in float64.

Limits, stated and not solved here: max_slope = 6144 (about 5.4 degrees), coarse = 256 and fine = 32 are design choices, not measurements, as
``layout``'s defaults are; no claim of the estimate's QUALITY on real scans is made.  Out of scope: skew beyond about ±7 degrees and 90 / 180 degree
orientation, perspective, per-block skew (ONE slope is found per page), and everything ``layout`` leaves out."""
import numpy as np

from . import layout, pages
from .ink import frame_ink, frame_table as ink_table, luma, pair_ink, profiles_of, scan_rect, sh      # noqa: F401  (the profiles: ``ink``'s)

MAX_SLOPE = 8192
Q = 65536


def check_slope(m):
    """``m`` as an int; ValueError for a slope that is no integer or beyond ±MAX_SLOPE — the one refusal this module adds to ``layout.line_params``'"""
    if int(m) != m or abs(int(m)) > MAX_SLOPE:
        raise ValueError("slope must be an integer in [-%d, %d] (Q16: tan = slope / 65536), got %r" % (MAX_SLOPE, MAX_SLOPE, m))
    return int(m)


# --------------------------------------------------------------------------------------------------------------------------- the profiles
def frame_box(H, W, m):
    """the smallest frame box [c1, r1, c2, r2) that holds every pixel of an H x W page (sh is monotone: its extremes lie at the page's sides)"""
    sx, sr = (sh(0, m), sh(int(W) - 1, m)), (sh(0, m), sh(int(H) - 1, m))
    return [min(sr), -max(sx), int(W) + max(sr), int(H) - min(sx)]


# ------------------------------------------------------------------------------------------------------------------------------ the skew
def score(rows):
    """Σ_i (P[i + 1] − P[i])² of a row profile, a Python integer"""
    d = np.diff(np.asarray(rows).astype(np.int64)).tolist()
    return sum(v * v for v in d)


def best_slope(scores):
    """the winner of [(m, S)]: the largest score, ties to the smaller |m|, then to the positive one"""
    return max(scores, key=lambda ms: (ms[1], -abs(ms[0]), ms[0] > 0))[0]


def estimate_params(floor=layout.DEFAULT_FLOOR, max_slope=6144, coarse=256, fine=32):
    """the arguments of ``estimate_host`` checked → dict; ValueError for a ``floor`` outside 0..255, a ``max_slope`` outside 0..MAX_SLOPE and a
    ``coarse`` or ``fine`` under 1, raised before any pixel is read"""
    if int(floor) != floor or not 0 <= floor <= 255:
        raise ValueError("floor must be an integer in [0, 255], got %r" % (floor,))
    if int(max_slope) != max_slope or not 0 <= max_slope <= MAX_SLOPE:
        raise ValueError("max_slope must be an integer in [0, %d], got %r" % (MAX_SLOPE, max_slope))
    for name, v in (("coarse", coarse), ("fine", fine)):
        if int(v) != v or v < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (name, v))
    return dict(floor=int(floor), max_slope=int(max_slope), coarse=int(coarse), fine=int(fine))


def estimate(rows_at, params):
    """``estimate_host`` on the profiles of ``rows_at(slopes)`` — per slope the row profile of the page's frame box, the one thing the host and
    the device paths do not share; it is called once per stage.  ``params``: ``estimate_params``' dict"""
    stage = list(range(-params["max_slope"], params["max_slope"] + 1, params["coarse"]))
    scores = [(m, score(p)) for m, p in zip(stage, rows_at(stage))]
    best = best_slope(scores)
    stage = [m for m in range(best - params["coarse"], best + params["coarse"] + 1, params["fine"]) if abs(m) <= MAX_SLOPE]
    scores += [(m, score(p)) for m, p in zip(stage, rows_at(stage))]
    return dict(slope=best_slope(scores), scores=scores)


def estimate_host(page, floor=layout.DEFAULT_FLOOR, max_slope=6144, coarse=256, fine=32):
    """the skew of ``page`` (uint8 RGB [H, W, 3]) → dict(slope: Q16, the page's text runs along (1, slope / 65536) — positive: down to the right
    —; scores: [(m, S(m))] for every candidate of both stages) — the definition of ``MarconetPipeline.estimate_skew`` (the module's head states
    the rule; the defaults are design choices, not measurements)"""
    page = pages._page_array(page)
    params = estimate_params(floor, max_slope, coarse, fine)
    e, (H, W) = pair_ink(page, params["floor"]), page.shape[:2]
    return estimate(lambda slopes: [profiles_of(e, frame_box(H, W, m), m)[0] for m in slopes], params)


# ------------------------------------------------------------------------------------------------------------------------------ the lines
def frame_quad(box, m):
    """the four page corners, in ``restore_page_quads``' order, of the frame box ``box`` under the inverse linear map (the module's head), float64"""
    t = int(m) / float(Q)
    den = 1.0 + t * t
    c1, r1, c2, r2 = (float(v) for v in box)
    return [[(c - t * r) / den, (r + t * c) / den] for c, r in ((c1, r1), (c2, r1), (c2, r2), (c1, r2))]


def lines_from_frame_profiles(profiles, H, W, m, params, scores):
    """``find_lines_host`` from the cut on: what the host and the device paths share.  ``profiles(boxes, axis)`` as ``layout.xy_cut`` takes it,
    for frame boxes at slope ``m``"""
    found = layout.lines_from_profiles(profiles, H, W, params, frame=frame_box(H, W, m))
    return dict(slope=int(m), frame_boxes=found["boxes"], tight=found["tight"], quads=[frame_quad(b, m) for b in found["boxes"]],
                skipped=found["skipped"], passes=found["passes"], scores=scores)


def find_lines_host(page, slope=None, text_h=None, floor=layout.DEFAULT_FLOOR, pad=None, min_h=None, min_w=None, max_h=None):
    """the text lines of a skewed ``page`` (uint8 RGB [H, W, 3]) → dict(slope; frame_boxes: integer [c1, r1, c2, r2) in FRAME coordinates, in
    reading order, each grown by min(pad, allowance − 1) a side; tight: the same boxes as cut; quads: per frame box its four page corners, what
    ``restore_page_quads`` takes; skipped: [dict(box, reason)], frame boxes taller than ``max_h``; passes; scores: ``estimate_host``'s, [] for a
    given ``slope``) — the definition of ``MarconetPipeline.find_lines_skewed`` (the module's head states the rules).  ``slope=None``:
    ``estimate_host`` runs first, with its defaults and this ``floor``"""
    page = pages._page_array(page)
    params = layout.line_params(page.shape[0], text_h, floor, pad, min_h, min_w, max_h)
    H, W = int(page.shape[0]), int(page.shape[1])
    e = pair_ink(page, params["floor"])
    if slope is None:
        est = estimate(lambda slopes: [profiles_of(e, frame_box(H, W, m), m)[0] for m in slopes], estimate_params(params["floor"]))
        m, scores = est["slope"], est["scores"]
    else:
        m, scores = check_slope(slope), []
    return lines_from_frame_profiles(lambda boxes, axis: [profiles_of(e, b, m)[axis] for b in boxes], H, W, m, params, scores)
