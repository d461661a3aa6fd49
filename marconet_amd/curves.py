"""Text regions that are curved strips of a page: seals and round stamps, arched shop signs, logos, text on bottles and banners — what a text
detector emits as a polygon of 2K points (CTW1500, Total-Text and ArT style).  ``quads`` pastes restored lines into convex quadrilaterals; this
module states, in integers and separately rounded fp64, what "the crop of a polygon strip" and "the line pasted along a polygon strip" mean, and
returns the same bytes from the device:

    strip_sizes, segment_coeffs          the geometry, host scalars only: the rectified strip's size and, per segment, the eight doubles of its
                                         bilinear patch with the segment's size folded in, computed once per region
    curve_pos, curve_inv                 the per-pixel arithmetic in numpy — csrc/curve_map.h states the same for the host and the device
    warp_crop_host, warp_paste_host      the numpy statement of the two kernels (``mnet_curve_crop_u8``, ``mnet_curve_paste_u8``)
    check_curves                         the refusals
    compose_curves_host                  the pure-host definition of a page
    crop_table, paste_table, crop_curves,   the same bytes on the device: one launch rectifies every window of every region, one
    paste_curves, compose_page_curves       ``mnet_paste_u8`` launch makes the regions' upright foregrounds, one launch pastes them all

A region is 2K points [[x, y]] in page pixels (pixel i covers [i, i + 1)), 2 <= K <= 33: the K top points left to right in reading order, then the K
bottom points right to left — clockwise with y down, the detectors' order; for K = 2 exactly the corner order of ``quads``.  With T_k the k-th top
point and B_k the bottom point facing it, the region is a chain of K - 1 segments, segment k the quadrilateral T_k, T_k+1, B_k+1, B_k.
The sizes: ch = rint(mean of the K rung lengths |T_k B_k|), at least 1; w_k = max(1, rint((|T_k T_k+1| + |B_k B_k+1|) / 2)); cw = sum w_k;
u0_k = sum of the w_m before k.  For K = 2 this is ``quads.crop_size``.
The map is piecewise BILINEAR, the ruled surface between the two polylines, not projective: two projective maps of neighbouring segments agree on
their shared rung at its end points only, bilinear patches agree along all of it, so a line of text stays continuous across every seam.  With 1 / w
and 1 / h folded in, a segment is A = T_k, E = (T_k+1 - T_k) / w, F = (B_k - T_k) / h, G = (T_k - T_k+1 + B_k+1 - B_k) / (w h); a point (u, v) of the
segment's w x h rectangle lies at A + E u + F v + G u v.  For a parallelogram G is exactly 0 and the forward map is bit for bit ``quads.quad_pos``
of ``quads.quad_map``: for 4-point polygons that are parallelograms, integer boxes included, everything here is ``quads``' bytes.
``MarconetPipeline.restore_page_curves`` ties it to the networks.  Out of scope: overlapping regions and pages that hold other kinds of region as
well (both are ``regions``': ``MarconetPipeline.restore_page_regions``), curved vertical columns, detection and recognition, several pages per launch.
"""
import math

import numpy as np

from . import _lib, lq_io, ops, pages, quads

ROW_H = pages.ROW_H
MAX_COORD = quads.MAX_COORD   # a point beyond +-32768 page pixels is refused
MIN_SIDE, MAX_SIDE = 2, 33    # points per side: 1 .. 32 segments (MNET_CURVE_MAX_SEGS)

quad_fix, quad_bilinear = quads.quad_fix, quads.quad_bilinear
_separated = quads._separated
enlarge = pages.enlarge


# ------------------------------------------------------------------------------------------------------------------------- the geometry
def _sides(poly):
    """2K points → (the K top points left to right, the K bottom points facing them), as tuples of Python floats"""
    pts = [(float(p[0]), float(p[1])) for p in poly]
    K = len(pts) // 2
    return pts[:K], pts[:K - 1:-1]


def segment_quads(poly):
    """the chain's K - 1 quadrilaterals T_k, T_k+1, B_k+1, B_k, each in ``quads``' corner order"""
    top, bot = _sides(poly)
    return [[top[k], top[k + 1], bot[k + 1], bot[k]] for k in range(len(top) - 1)]


def strip_sizes(poly):
    """the rectified strip's size → (the segments' widths [w_k], ch): see the module's head.  For an integer axis-aligned box split at integer
    abscissae exactly (the pieces' widths, y2 − y1); for K = 2 ``quads.crop_size``."""
    top, bot = _sides(poly)
    K = len(top)
    rungs = 0.0
    for t, b in zip(top, bot):
        rungs += math.hypot(b[0] - t[0], b[1] - t[1])
    ch = max(1, int(np.rint(rungs / K)))
    ws = [max(1, int(np.rint(0.5 * (math.hypot(top[k + 1][0] - top[k][0], top[k + 1][1] - top[k][1]) +
                                    math.hypot(bot[k + 1][0] - bot[k][0], bot[k + 1][1] - bot[k][1]))))) for k in range(K - 1)]
    return ws, ch


def segment_coeffs(poly, ws, h, boxes=None):
    """→ per segment a dict: ``c`` (eight Python floats: Ax, Ex, Fx, Gx, Ay, Ey, Fy, Gy — the bilinear patch that takes (0, 0), (w_k, 0),
    (w_k, h), (0, h) to T_k, T_k+1, B_k+1, B_k), ``u0``, ``w`` and ``box`` (bx0, by0, bw, bh: ``boxes[k]``, or zeros — a crop needs none).  G's
    numerator is summed in ``quads.quad_map``'s order, so it is exactly 0 wherever that map is affine."""
    out, u0, h = [], 0, float(h)
    for k, ((x0, y0), (x1, y1), (x2, y2), (x3, y3)) in enumerate(segment_quads(poly)):
        w = float(ws[k])
        c = [x0, (x1 - x0) / w, (x3 - x0) / h, (x0 - x1 + x2 - x3) / (w * h), y0, (y1 - y0) / w, (y3 - y0) / h, (y0 - y1 + y2 - y3) / (w * h)]
        out.append(dict(c=c, u0=u0, w=int(ws[k]), box=(0, 0, 0, 0) if boxes is None else tuple(int(v) for v in boxes[k])))
        u0 += int(ws[k])
    return out


# --------------------------------------------------------------------------------------------------------- the per-pixel arithmetic
def curve_pos(c, u, v):
    """csrc/curve_map.h's curve_pos for arrays of positions in a segment's rectangle → (X, Y, valid): X = ((Ex u + Fx v) + (Gx u) v) + Ax and Y
    likewise, every operation rounded separately (numpy's element-wise operations are); valid where both are finite, 0 elsewhere"""
    c = [np.float64(t) for t in c]
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        X = ((c[1] * u + c[2] * v) + (c[3] * u) * v) + c[0]
        Y = ((c[5] * u + c[6] * v) + (c[7] * u) * v) + c[4]
        valid = np.isfinite(X) & np.isfinite(Y)
    return np.where(valid, X, 0.0), np.where(valid, Y, 0.0), valid


def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def curve_inv(c, x, y):
    """csrc/curve_map.h's curve_inv for arrays of page points → (u, v, valid): the position in the segment's rectangle whose image is (x, y).
    With q = p − A: a2 = cross(F, G), a1 = cross(F, E) − cross(q, G), a0 = −cross(q, E), disc = a1 a1 − (4 a2) a0, r = sqrt(disc) (IEEE); the
    wanted root is always (−a1 − r) / (2 a2), taken without cancellation as v = a0 / (0.5 (r − a1)) where a1 <= 0 and (−0.5 (a1 + r)) / a2 where
    a1 > 0 (a1 changes sign inside strongly tapered segments: choosing the root by a1's sign alone leaves part of them unpasted); d = E + v G and
    u = (qx − v Fx) / dx where |dx| >= |dy|, else (qy − v Fy) / dy.  Valid iff disc >= 0 and u, v are finite; u and v are 0 elsewhere."""
    Ax, Ex, Fx, Gx, Ay, Ey, Fy, Gy = (np.float64(t) for t in c)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        qx, qy = x - Ax, y - Ay
        a2 = _cross(Fx, Fy, Gx, Gy)
        a1 = _cross(Fx, Fy, Ex, Ey) - _cross(qx, qy, Gx, Gy)
        a0 = -_cross(qx, qy, Ex, Ey)
        disc = a1 * a1 - (4.0 * a2) * a0
        r = np.sqrt(disc)
        v = np.where(a1 <= 0.0, a0 / (0.5 * (r - a1)), (-0.5 * (a1 + r)) / a2)
        dx, dy = Ex + v * Gx, Ey + v * Gy
        u = np.where(np.abs(dx) >= np.abs(dy), (qx - v * Fx) / dx, (qy - v * Fy) / dy)
        valid = (disc >= 0.0) & np.isfinite(u) & np.isfinite(v)
    return np.where(valid, u, 0.0), np.where(valid, v, 0.0), valid


def _check_chain(segs, who):
    u0 = 0
    for s in segs:
        if int(s["u0"]) != u0 or int(s["w"]) < 1:
            raise ValueError("%s: the segments' columns must chain from 0 (u0 %d, w %d where u0 %d was due)" % (who, s["u0"], s["w"], u0))
        u0 += int(s["w"])
    if not 1 <= len(segs) <= MAX_SIDE - 1:
        raise ValueError("%s: 1 to %d segments expected, got %d" % (who, MAX_SIDE - 1, len(segs)))
    return u0


def warp_crop_host(page, segs, w, h, c0=0):
    """the numpy statement of ``mnet_curve_crop_u8`` for one descriptor: column i of the uint8 [h, w, 3] result is column c0 + i of the region's
    strip and lies in the segment k with u0_k <= c0 + i < u0_k + w_k; pixel (i, j) is ``quad_bilinear`` of the page at ``curve_pos(c_k,
    (c0 + i − u0_k) + 0.5, j + 0.5)``, 0 where that position is invalid"""
    page, w, h, c0 = pages._page_array(page), int(w), int(h), int(c0)
    if w < 1 or h < 1 or c0 < 0 or c0 + w > _check_chain(segs, "warp_crop_host"):
        raise ValueError("warp_crop_host: the window [%d, %d) x %d lies outside the strip" % (c0, c0 + w, h))
    out = np.zeros((h, w, 3), np.uint8)
    v = np.arange(h, dtype=np.float64)[:, None] + 0.5
    for s in segs:
        i0, i1 = max(s["u0"] - c0, 0), min(s["u0"] + s["w"] - c0, w)
        if i0 >= i1:
            continue
        u = (c0 + np.arange(i0, i1, dtype=np.int64) - s["u0"]).astype(np.float64)[None, :] + 0.5
        X, Y, valid = curve_pos(s["c"], u, v)
        part = quad_bilinear(page, quad_fix(X), quad_fix(Y))
        part[~valid] = 0
        out[:, i0:i1] = part
    return out


def warp_paste_host(page_up, fg_rgb, segs, rw, rh, feather):
    """the numpy statement of ``mnet_curve_paste_u8`` for one region: ``page_up`` (uint8 RGB [PH, PW, 3]) is changed IN PLACE and returned.  Per page
    pixel (X, Y) the segments are tried in order; segment k claims the pixel iff it lies in the segment's ``box`` and (u, v) = ``curve_inv(c_k,
    X + 0.5, Y + 0.5)`` is valid with 0 <= u < w_k and 0 <= v < rh; the first claim wins and a pixel none claims keeps the background.  fg =
    ``quad_bilinear`` of ``fg_rgb`` (uint8 RGB [rh, rw, 3], the upright foreground) at (``quad_fix(u)`` + 64 u0_k, ``quad_fix(v)``) — the taps
    clamped into the whole foreground, so the interpolation runs across seams; the byte is fg for feather 0, else ``pages.feather_blend``'s
    arithmetic with the weights of foreground pixel (u0_k + floor u, floor v) in rw x rh, so the ramp follows the curved outline."""
    fg_rgb, rw, rh, F = np.asarray(fg_rgb), int(rw), int(rh), int(feather)
    if page_up.dtype != np.uint8 or page_up.ndim != 3 or page_up.shape[2] != 3:
        raise TypeError("warp_paste_host: uint8 RGB HxWx3 page expected")
    if fg_rgb.dtype != np.uint8 or fg_rgb.shape != (rh, rw, 3) or rw < 1 or rh < 1:
        raise ValueError("warp_paste_host: a uint8 [%d, %d, 3] foreground expected, got %s %s" % (rh, rw, fg_rgb.dtype, fg_rgb.shape))
    if not 0 <= F <= pages.MAX_FEATHER:
        raise ValueError("warp_paste_host: feather %d outside [0, %d]" % (F, pages.MAX_FEATHER))
    if _check_chain(segs, "warp_paste_host") != rw:
        raise ValueError("warp_paste_host: the segments' widths must sum to rw = %d" % rw)
    PH, PW = page_up.shape[:2]
    claimed = np.zeros((PH, PW), bool)
    for s in segs:
        bx0, by0, bw, bh = s["box"]
        if bw < 1 or bh < 1:
            continue
        if bx0 < 0 or by0 < 0 or bx0 + bw > PW or by0 + bh > PH:
            raise ValueError("warp_paste_host: segment box %s outside the %d x %d page" % (s["box"], PW, PH))
        x = np.arange(bx0, bx0 + bw, dtype=np.float64)[None, :] + 0.5
        y = np.arange(by0, by0 + bh, dtype=np.float64)[:, None] + 0.5
        u, v, valid = curve_inv(s["c"], x, y)
        claim = valid & (u >= 0.0) & (u < float(s["w"])) & (v >= 0.0) & (v < float(rh)) & ~claimed[by0:by0 + bh, bx0:bx0 + bw]
        claimed[by0:by0 + bh, bx0:bx0 + bw] |= claim
        u, v = u[claim], v[claim]
        fg = quad_bilinear(fg_rgb, quad_fix(u) + 64 * int(s["u0"]), quad_fix(v)).astype(np.int64)
        view = page_up[by0:by0 + bh, bx0:bx0 + bw]
        if F:
            iu, iv = int(s["u0"]) + np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
            m = (pages.feather_axis(rw, F)[iu] * pages.feather_axis(rh, F)[iv])[:, None]
            D = 4 * F * F
            fg = (view[claim].astype(np.int64) * (D - m) + fg * m + D // 2) // D
        view[claim] = fg.astype(np.uint8)
    return page_up


# ------------------------------------------------------------------------------------------------------------------------- the refusals
def _outward_box(pts, s, page_h, page_w):
    """the box of the points ``pts`` scaled by ``s``, rounded outward and clipped to the s-fold page → (x0, y0, x1, y1), empty where x1 <= x0 or y1 <= y0"""
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    return (max(0, math.floor(s * min(xs))), max(0, math.floor(s * min(ys))), min(s * page_w, math.ceil(s * max(xs))), min(s * page_h, math.ceil(s * max(ys))))


def check_curves(page_h, page_w, polygons, restored, scale, feather, rows=ROW_H):
    """the refusals, all ValueError naming the region, and per region a dict: ``polygon`` (the points as floats), ``ws``, ``cw``, ``ch``
    (``strip_sizes``), ``segs`` (``segment_coeffs`` of the polygon: the crop's), ``out_polygon`` (the points in the enlarged page, s·polygon),
    ``rw``, ``rh`` (s·cw, s·ch: the upright foreground's size), ``bbox`` (bx0, by0, bw, bh: ``out_polygon``'s bounding box rounded outward and
    clipped to the enlarged page) and ``out_segs`` (``segment_coeffs`` of ``out_polygon`` with the widths s·w_k and the height s·ch, each with
    its own box: the outward-rounded box of its scaled corners clipped to the enlarged page, (bx0, by0, 0, 0) of the region where that is
    empty — the boxes are part of the definition: a segment claims a pixel only inside its box).  ``restored[i]``: region i has a line to
    paste (the others keep the background: only their points are checked).  Refused: ``scale`` outside [1, 8] or ``feather`` outside
    [0, 1024] (integers); a point count that is odd, under 4 or over 66; points that are not finite or lie beyond ±32768; a segment that is not
    strictly convex in clockwise order with y down (a mirrored, counter-clockwise chain is named as such); two segments of one region whose
    interiors intersect (a chain that folds over itself); a bounding box that misses the page; a restored region's foreground under rows / 16
    rows; two restored regions with intersecting segments.  A region partly outside the page is allowed: the crop replicates the page's border
    and the paste is clipped."""
    pages.check_request(scale, feather, len(polygons), len(restored), "polygon", "polygons")
    s, page_h, page_w, out = int(scale), int(page_h), int(page_w), []
    for i, poly in enumerate(polygons):
        try:
            pts = np.asarray(poly, dtype=np.float64)
        except (TypeError, ValueError):
            pts = np.zeros((0,))
        if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] % 2 or not 2 * MIN_SIDE <= pts.shape[0] <= 2 * MAX_SIDE:
            raise ValueError("region %d: an even number of points [[x, y], ...] from %d to %d expected (the top side left to right, then the bottom "
                             "side right to left), got %r" % (i, 2 * MIN_SIDE, 2 * MAX_SIDE, poly))
        if not np.isfinite(pts).all():
            raise ValueError("region %d: its points must be finite, got %r" % (i, poly))
        if np.abs(pts).max() > MAX_COORD:
            raise ValueError("region %d: a point's coordinate lies beyond +-%d" % (i, int(MAX_COORD)))
        polygon = [(float(x), float(y)) for x, y in pts]
        sq = segment_quads(polygon)
        for k, q in enumerate(sq):
            cross = []
            for n in range(4):
                (ax, ay), (bx, by), (cx, cy) = q[n], q[(n + 1) % 4], q[(n + 2) % 4]
                cross.append((bx - ax) * (cy - by) - (by - ay) * (cx - bx))
            if all(c < 0.0 for c in cross):
                raise ValueError("region %d: segment %d runs counter-clockwise (a mirrored chain): the top side left to right, then the bottom side "
                                 "right to left, of the line as it is read expected" % (i, k))
            if not all(c > 0.0 for c in cross):
                raise ValueError("region %d: segment %d, %s, is not strictly convex (top points left to right, then the bottom points facing them "
                                 "right to left expected)" % (i, k, q))
        for k in range(len(sq)):                                  # (neighbours need no test: each lies strictly on its own side of the rung they share, being convex and clockwise)
            for m in range(k - 1):
                if not _separated(sq[k], sq[m]):
                    raise ValueError("region %d: segments %d and %d intersect: the chain folds over itself" % (i, m, k))
        x0, y0, x1, y1 = _outward_box(polygon, 1, page_h, page_w)
        if x0 >= x1 or y0 >= y1:
            xs, ys = [p[0] for p in polygon], [p[1] for p in polygon]
            raise ValueError("region %d: its bounding box [%g, %g] x [%g, %g] misses the %d x %d page" % (i, min(xs), max(xs), min(ys), max(ys), page_w, page_h))
        ws, ch = strip_sizes(polygon)
        bx0, by0, bx1, by1 = _outward_box(polygon, s, page_h, page_w)
        boxes = []
        for q in sq:
            a0, b0, a1, b1 = _outward_box(q, s, page_h, page_w)
            boxes.append((bx0, by0, 0, 0) if a0 >= a1 or b0 >= b1 else (a0, b0, a1 - a0, b1 - b0))
        out_polygon = [(s * x, s * y) for x, y in polygon]
        rec = dict(polygon=polygon, ws=ws, cw=sum(ws), ch=ch, segs=segment_coeffs(polygon, ws, ch), out_polygon=out_polygon, rw=s * sum(ws), rh=s * ch,
                   bbox=(int(bx0), int(by0), int(bx1 - bx0), int(by1 - by0)), out_segs=segment_coeffs(out_polygon, [s * w for w in ws], s * ch, boxes),
                   quads=sq)
        if not all(math.isfinite(v) for sg in rec["segs"] + rec["out_segs"] for v in sg["c"]):
            raise ValueError("region %d: no finite map for the points %s" % (i, polygon))
        out.append(rec)
        if restored[i] and s * ch * pages.MIN_RECT_H_DIV < rows:
            raise ValueError("region %d: its line is %d rows high at scale %d, under the %d a %d-row line can be reduced to"
                             % (i, s * ch, s, rows // pages.MIN_RECT_H_DIV, rows))
    live = [i for i in range(len(polygons)) if restored[i]]
    for n, i in enumerate(live):
        for j in live[:n]:
            if not _boxes_apart(out[i]["polygon"], out[j]["polygon"]) and any(not _separated(p, q) for p in out[i]["quads"] for q in out[j]["quads"]):
                raise ValueError("regions %d and %d overlap: the paste blends in place, so an overlap has no defined order" % (j, i))
    return out


def _boxes_apart(a, b):
    """the (unclipped) bounding boxes of two point lists do not intersect"""
    ax, ay, bx, by = [p[0] for p in a], [p[1] for p in a], [p[0] for p in b], [p[1] for p in b]
    return max(ax) <= min(bx) or max(bx) <= min(ax) or max(ay) <= min(by) or max(by) <= min(ay)


def box_polygon(box, cuts=()):
    """an axis-aligned box [x1, y1, x2, y2] → its polygon, the two sides split at the abscissae ``cuts`` (ascending, inside the box)"""
    x1, y1, x2, y2 = box
    xs = [x1] + list(cuts) + [x2]
    return [[x, y1] for x in xs] + [[x, y2] for x in reversed(xs)]


# ------------------------------------------------------------------------------------------------------------------- the definition
def compose_curves_host(page, lines, polygons, scale=4, feather=8):
    """the definition of a page: ``page`` uint8 RGB [H, W, 3]; ``lines[i]``: region i's restored line, uint8 BGR [rows, src_w, 3]
    (``MarconetPipeline.restore_lines`` of the crop ``warp_crop_host(page, r["segs"], cw, ch)``), or None for a region that keeps the
    background; ``polygons[i]`` its points → uint8 RGB [s·H, s·W, 3]: ``lq_io.resize_cubic(page, s, s)`` with, for every line, its upright
    foreground ``pages.line_to_rect(line, s·cw, s·ch)`` pasted by ``warp_paste_host`` along ``check_curves``' ``out_segs``."""
    page = pages._page_array(page)
    rows = next((int(np.shape(l)[0]) for l in lines if l is not None), ROW_H)
    regions = check_curves(page.shape[0], page.shape[1], polygons, [l is not None for l in lines], scale, feather, rows)
    out = lq_io.resize_cubic(page, int(scale), int(scale))
    for line, r in zip(lines, regions):
        if line is not None:
            warp_paste_host(out, pages.line_to_rect(line, r["rw"], r["rh"]), r["out_segs"], r["rw"], r["rh"], int(feather))
    return out


# ------------------------------------------------------------------------------------------------------------------- the device path
def _seg_records(seg_lists):
    """→ (numpy record array of ``mnet_curve_seg``: the lists' segments one after the other, the first index of every list)"""
    tab = np.zeros((sum(len(l) for l in seg_lists),), dtype=np.dtype(_lib.CurveSeg))
    first, n = [], 0
    for segs in seg_lists:
        first.append(n)
        for s in segs:
            tab[n] = ([float(v) for v in s["c"]], int(s["u0"]), int(s["w"])) + tuple(int(v) for v in s["box"])
            n += 1
    return tab, first


def crop_table(seg_lists, sizes, c0s=None, base=0):
    """→ (numpy record array of ``mnet_curve_crop``, that of ``mnet_curve_seg``, the flat buffer's size in bytes): crop k is ``sizes[k]`` = (w, h)
    along the segments ``seg_lists[k]`` from column ``c0s[k]`` (default 0) of its region's strip; the crops are packed tightly in order from byte
    ``base``.  A list that serves several windows (the same object) is stored once."""
    uniq, index = [], {}
    for segs in seg_lists:
        if id(segs) not in index:
            index[id(segs)] = len(uniq)
            uniq.append(segs)
    seg_tab, first = _seg_records(uniq)
    tab = np.zeros((len(seg_lists),), dtype=np.dtype(_lib.CurveCrop))
    off = int(base)
    for k, (segs, (w, h)) in enumerate(zip(seg_lists, sizes)):
        tab[k] = (off, int(w), int(h), 0 if c0s is None else int(c0s[k]), first[index[id(segs)]], len(segs), 0)
        off += 3 * int(w) * int(h)
    return tab, seg_tab, off


def paste_table(regions, feather, atlas_xy):
    """→ (numpy record array of ``mnet_curve_region``, that of ``mnet_curve_seg``): ``regions[l]`` (a ``check_curves`` record) has its upright
    foreground at ``atlas_xy[l]``"""
    seg_tab, first = _seg_records([r["out_segs"] for r in regions])
    tab = np.zeros((len(regions),), dtype=np.dtype(_lib.CurveRegion))
    for l, (r, (ax0, ay0)) in enumerate(zip(regions, atlas_xy)):
        tab[l] = (int(ax0), int(ay0), r["rw"], r["rh"]) + tuple(r["bbox"]) + (int(feather), first[l], len(r["out_segs"]), 0)
    return tab, seg_tab


def crop_curves(page_d, seg_lists, sizes, c0s=None, base=0, dst=None):
    """``page_d`` uint8 RGB [H, W, 3] on the device → (uint8 [bytes] on the device: ``warp_crop_host`` of every crop, packed tightly in order from
    byte ``base``, the offsets of the crops): one copy of each table, one launch.  ``dst``: an existing flat buffer that holds the crops' bytes
    (the packed batch several sources share), written inside the crops only; None: a new one, the first ``base`` bytes left to the caller"""
    tab, seg_tab, nbytes = crop_table(seg_lists, sizes, c0s, base)
    dst = pages.crop_buffer("crop_curves", dst, nbytes, page_d.device)
    with ops.on_device(page_d):
        ops.curve_crop_u8(page_d, ops.table_to_device(tab, page_d.device), ops.table_to_device(seg_tab, page_d.device),
                          max(int(w) for w, _ in sizes), max(int(h) for _, h in sizes), dst)
    return dst, [int(o) for o in tab["offset"]]


def paste_curves(out, joined, out_ws, regions, feather, rows=ROW_H):
    """``out``: the enlarged page on the device, changed IN PLACE; ``joined`` / ``out_ws`` as ``pages.compose_page`` takes them; ``regions``:
    ``check_curves``' records.  One ``mnet_paste_u8`` launch (feather 0) makes every line's upright foreground in a zeroed atlas [Σ rh, max rw, 3],
    the regions stacked vertically — ``pages.line_to_rect``'s bytes, by ``pages.build_table`` —, and one ``mnet_curve_paste_u8`` launch pastes them."""
    live = [i for i, w in enumerate(out_ws) if w is not None]
    if not live:
        return out
    rects, atlas_hw = pages.atlas_layout([None if w is None else (r["rw"], r["rh"]) for w, r in zip(out_ws, regions)])
    tab, seg_tab = paste_table([regions[i] for i in live], feather, [rects[i][:2] for i in live])
    atlas = pages.fill_atlas(joined, pages.build_table(rects, out_ws, 0, rows), atlas_hw)
    with ops.on_device(out):
        return ops.curve_paste_u8(atlas, ops.table_to_device(tab, out.device), ops.table_to_device(seg_tab, out.device),
                                  max(regions[i]["bbox"][2] for i in live), max(regions[i]["bbox"][3] for i in live), out)


def compose_page_curves(page, joined, out_ws, polygons, scale=4, feather=8, device=None):
    """the device path of ``compose_curves_host``; the arguments are ``pages.compose_page``'s, with ``polygons[i]`` in the place of the boxes.
    → uint8 RGB [s·H, s·W, 3] on the device.  Every refusal of ``compose_curves_host`` is raised before anything is copied or launched; then one
    copy of the page and one of each small table, one launch for the background, one for the foregrounds and one for all regions."""
    def check(H, W, rows):
        regions = check_curves(H, W, polygons, [w is not None for w in out_ws], scale, feather, rows)
        return regions, [r["rh"] for r in regions]
    page, rows, regions = pages.page_to_device("compose_page_curves", page, joined, out_ws, device, check)
    return paste_curves(enlarge(page, int(scale)), joined, out_ws, regions, int(feather), rows)


def char_boxes_in_crop(boxes, segs, cw, ch):
    """character boxes in PAGE pixels — [x1, y1, x2, y2] or four corners [[x, y]] x 4 each — → boxes in the rectified strip of the region whose
    crop segments are ``segs``: every corner takes the strip column u0_k + u of the first segment whose inverse is valid with 0 <= u <= w_k (v is
    not restricted: a character may stand above or below the strip); a corner no segment accepts goes to the nearer end of the strip (by its
    distance to the middle of the first and of the last rung), 0 or cw; the interval [min, max] clamped to [0, cw] becomes the box
    [u1, 0, u2, ch].  For an integer box region this is ``quads.char_boxes_in_crop``."""
    def rung_mid(c, u):
        x, y, _ = curve_pos(c, u, 0.5 * ch)
        return float(x), float(y)
    first, last, out = rung_mid(segs[0]["c"], 0.0), rung_mid(segs[-1]["c"], float(segs[-1]["w"])), []
    for b in boxes:
        pts = np.asarray(b, dtype=np.float64)
        pts = np.asarray(quads.box_quad(pts), dtype=np.float64) if pts.shape == (4,) else pts
        if pts.shape != (4, 2):
            raise ValueError("a character box [x1, y1, x2, y2] or four corners expected, got %r" % (b,))
        us = []
        for x, y in pts:
            for s in segs:
                u, _, valid = curve_inv(s["c"], float(x), float(y))
                if valid and 0.0 <= float(u) <= float(s["w"]):
                    us.append(float(s["u0"]) + float(u))
                    break
            else:
                us.append(0.0 if math.hypot(x - first[0], y - first[1]) <= math.hypot(x - last[0], y - last[1]) else float(cw))
        out.append([min(max(min(us), 0.0), float(cw)), 0, min(max(max(us), 0.0), float(cw)), int(ch)])
    return out
