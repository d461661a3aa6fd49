"""Text regions that are convex quadrilaterals of a page: what a text detector emits for a sign photographed at an angle, a slanted scan or a
line of rotated characters.  ``pages`` pastes restored lines into axis-aligned integer boxes; this module states, in integers and separately rounded
fp64, what "the crop of a quadrilateral" and "the line pasted into a quadrilateral" mean, and returns the same bytes from the device:

    crop_size, quad_map, inverse_map     the geometry, host scalars only: the rectified crop's size and the 3x3 projective maps (Heckbert's
                                         square-to-quad map with the crop's size folded in), nine doubles each, computed once per region
    quad_pos, quad_fix, quad_bilinear    the per-pixel arithmetic in numpy — csrc/quad_map.h states the same for the host and the device
    warp_crop_host, warp_paste_host      the numpy statement of the two kernels (``mnet_quad_crop_u8``, ``mnet_quad_paste_u8``)
    check_quads                          the refusals
    compose_quads_host                   the pure-host definition of a page
    crop_table, paste_table,             the same bytes on the device: one launch rectifies every window of every region, one
    compose_page_quads                   ``mnet_paste_u8`` launch makes the regions' upright foregrounds, one launch pastes them all

A region is four corners [[x, y]] x 4 in page pixels (pixel i covers [i, i + 1)), in the text's own reading order: top-left, top-right,
bottom-right, bottom-left of the line as it is read — a line rotated by 90 degrees is a quadrilateral whose first corner is elsewhere.  For an
integer axis-aligned box all of this is ``pages``' own bytes; for its right-angle rotations it is ``np.rot90`` of them.  ``MarconetPipeline.
restore_page_quads`` ties it to the networks.  Out of scope: overlapping regions and pages that hold other kinds of region as well (both are
``regions``': ``MarconetPipeline.restore_page_regions``), vertical columns that are rotated or in perspective (upright ones: ``columns``), curved vertical columns (curved text: ``curves``), detection and
recognition, several pages per launch.
"""
import math

import numpy as np

from . import _lib, lq_io, ops, pages

ROW_H = pages.ROW_H
MAX_COORD = 32768.0           # a corner beyond +-32768 page pixels is refused
FIX_LIMIT = float(1 << 30)    # csrc/quad_map.h's QUAD_FIX_LIMIT


# ------------------------------------------------------------------------------------------------------------------------- the geometry
def _corners(q):
    return [(float(p[0]), float(p[1])) for p in q]


def crop_size(q):
    """the rectified crop's size (cw, ch): the means of the two opposite sides' lengths, rounded half to even, at least 1.  For an integer
    axis-aligned box exactly (x2 − x1, y2 − y1)."""
    p0, p1, p2, p3 = _corners(q)
    cw = max(1, int(np.rint(0.5 * (math.hypot(p1[0] - p0[0], p1[1] - p0[1]) + math.hypot(p2[0] - p3[0], p2[1] - p3[1])))))
    ch = max(1, int(np.rint(0.5 * (math.hypot(p3[0] - p0[0], p3[1] - p0[1]) + math.hypot(p2[0] - p1[0], p2[1] - p1[1])))))
    return cw, ch


def quad_map(q, w, h):
    """the projective map that takes (0, 0), (w, 0), (w, h), (0, h) to the corners of ``q`` → nine Python floats, row-major: Heckbert's
    square-to-quad map with 1 / w and 1 / h folded into the columns.  A parallelogram gives an affine map (last row 0, 0, 1); an integer
    axis-aligned box of size w x h gives exactly [1, 0, x1, 0, 1, y1, 0, 0, 1]."""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = _corners(q)
    w, h = float(w), float(h)
    sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
    dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
    if sx == 0.0 and sy == 0.0:
        g = h_ = 0.0
    else:
        den = dx1 * dy2 - dx2 * dy1
        g, h_ = (sx * dy2 - dx2 * sy) / den, (dx1 * sy - sx * dy1) / den
    a, b, c = x1 - x0 + g * x1, x3 - x0 + h_ * x3, x0
    d, e, f = y1 - y0 + g * y1, y3 - y0 + h_ * y3, y0
    return [a / w, b / h, c, d / w, e / h, f, g / w, h_ / h, 1.0]


def inverse_map(M):
    """the inverse of ``M``: its adjugate divided by its determinant → nine Python floats.  The scale of a projective map is free for the point it
    gives but not for the sign of its denominator, which ``quad_pos`` reads as validity: with the true inverse the denominator of N at M(p) is
    1 / (the denominator of M at p), so it is positive wherever M's is — over the whole quadrilateral, wherever its vanishing line runs (the
    adjugate over its own last element would fix the denominator at the page's origin instead, and turn a region behind that line invalid).
    The determinant is 1 for an integer box and its right-angle rotations: their entries stay exact integers.  ValueError for a map whose
    determinant is not positive and finite (no strictly convex clockwise quadrilateral gives one)."""
    a, b, c, d, e, f, g, h, i = (float(v) for v in M)
    adj = (e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d)
    det = a * adj[0] + b * adj[3] + c * adj[6]
    if not (det > 0.0 and math.isfinite(det)) or not all(math.isfinite(v / det) for v in adj):
        raise ValueError("the map has determinant %r: not invertible as an orientation-preserving map" % det)
    return [v / det for v in adj]


def map_point(M, x, y):
    """(x, y) under ``M`` in Python floats (the host's use: corners and character boxes, never pixels)"""
    D = M[6] * x + M[7] * y + M[8]
    return (M[0] * x + M[1] * y + M[2]) / D, (M[3] * x + M[4] * y + M[5]) / D


# --------------------------------------------------------------------------------------------------------- the per-pixel arithmetic
def quad_pos(M, x, y):
    """csrc/quad_map.h's quad_pos for arrays of pixel centres → (u, v, valid): every operation rounded separately (numpy's element-wise
    operations are), u and v 0 where the position is invalid"""
    M = [np.float64(v) for v in M]
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        X = (M[0] * x + M[1] * y) + M[2]
        Y = (M[3] * x + M[4] * y) + M[5]
        D = (M[6] * x + M[7] * y) + M[8]
        valid = (D > 0.0) & np.isfinite(X) & np.isfinite(Y) & np.isfinite(D)
        Ds = np.where(valid, D, 1.0)
        u, v = np.where(valid, X / Ds, 0.0), np.where(valid, Y / Ds, 0.0)
    return u, v, valid


def quad_fix(t):
    """csrc/quad_map.h's quad_fix: coordinates (no NaN) → sample positions in 1/64 pixel, int64 within ±2³⁰"""
    with np.errstate(all="ignore"):
        q = np.floor((np.asarray(t, dtype=np.float64) - 0.5) * 64.0 + 0.5)
    return np.clip(q, -FIX_LIMIT, FIX_LIMIT).astype(np.int64)


def quad_bilinear(src, qx, qy):
    """csrc/quad_map.h's quad_bilinear: ``src`` uint8 [h, w, c]; qx, qy: ``quad_fix`` of the positions (arrays of one shape S) → uint8 S + [c]"""
    src = np.asarray(src)
    h, w = src.shape[:2]
    qx, qy = np.asarray(qx, dtype=np.int64), np.asarray(qy, dtype=np.int64)
    ix, iy, ax, ay = qx >> 6, qy >> 6, (qx & 63)[..., None], (qy & 63)[..., None]
    x0, x1, y0, y1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1), np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    s = src.astype(np.int64)
    top = s[y0, x0] * (64 - ax) + s[y0, x1] * ax
    bot = s[y1, x0] * (64 - ax) + s[y1, x1] * ax
    return ((top * (64 - ay) + bot * ay + 2048) >> 12).astype(np.uint8)


def warp_crop_host(page, M, w, h, c0=0):
    """the numpy statement of ``mnet_quad_crop_u8`` for one descriptor: pixel (i, j) of the uint8 [h, w, 3] result is ``quad_bilinear`` of the
    page at ``quad_pos(M, (c0 + i) + 0.5, j + 0.5)``, 0 where that position is invalid"""
    page = pages._page_array(page)
    x = (int(c0) + np.arange(int(w), dtype=np.int64)).astype(np.float64)[None, :] + 0.5
    y = np.arange(int(h), dtype=np.float64)[:, None] + 0.5
    u, v, valid = quad_pos(M, x, y)
    out = quad_bilinear(page, quad_fix(u), quad_fix(v))
    out[~valid] = 0
    return out


def warp_paste_host(page_up, fg_rgb, N, rw, rh, feather):
    """the numpy statement of ``mnet_quad_paste_u8`` for one region: ``page_up`` (uint8 RGB [PH, PW, 3]) is changed IN PLACE and returned.  Page
    pixel (X, Y) is written iff (u, v) = ``quad_pos(N, X + 0.5, Y + 0.5)`` is valid and 0 ≤ u < rw, 0 ≤ v < rh; fg = ``quad_bilinear`` of
    ``fg_rgb`` (uint8 RGB [rh, rw, 3], the upright foreground) there; the byte is fg for feather 0, else ``pages.feather_blend``'s arithmetic
    with the weights of foreground pixel (floor u, floor v).  (Every pixel of the page is tried: a pixel outside the quadrilateral's bounding box,
    which is all the kernel visits, lies at least half a pixel outside the quadrilateral.)"""
    fg_rgb, rw, rh, F = np.asarray(fg_rgb), int(rw), int(rh), int(feather)
    if page_up.dtype != np.uint8 or page_up.ndim != 3 or page_up.shape[2] != 3:
        raise TypeError("warp_paste_host: uint8 RGB HxWx3 page expected")
    if fg_rgb.dtype != np.uint8 or fg_rgb.shape != (rh, rw, 3) or rw < 1 or rh < 1:
        raise ValueError("warp_paste_host: a uint8 [%d, %d, 3] foreground expected, got %s %s" % (rh, rw, fg_rgb.dtype, fg_rgb.shape))
    if not 0 <= F <= pages.MAX_FEATHER:
        raise ValueError("warp_paste_host: feather %d outside [0, %d]" % (F, pages.MAX_FEATHER))
    x = np.arange(page_up.shape[1], dtype=np.float64)[None, :] + 0.5
    y = np.arange(page_up.shape[0], dtype=np.float64)[:, None] + 0.5
    u, v, valid = quad_pos(N, x, y)
    inside = valid & (u >= 0.0) & (u < float(rw)) & (v >= 0.0) & (v < float(rh))
    u, v = u[inside], v[inside]
    fg = quad_bilinear(fg_rgb, quad_fix(u), quad_fix(v)).astype(np.int64)
    if F:
        iu, iv = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        m = (pages.feather_axis(rw, F)[iu] * pages.feather_axis(rh, F)[iv])[:, None]
        D = 4 * F * F
        fg = (page_up[inside].astype(np.int64) * (D - m) + fg * m + D // 2) // D
    page_up[inside] = fg.astype(np.uint8)
    return page_up


# ------------------------------------------------------------------------------------------------------------------------- the refusals
def _separated(a, b):
    """True where an edge of convex polygon ``a`` or ``b`` separates their interiors (polygons that only touch are separated)"""
    for poly in (a, b):
        for k in range(len(poly)):
            nx, ny = poly[(k + 1) % len(poly)][1] - poly[k][1], poly[k][0] - poly[(k + 1) % len(poly)][0]
            pa, pb = [nx * x + ny * y for x, y in a], [nx * x + ny * y for x, y in b]
            if max(pa) <= min(pb) or max(pb) <= min(pa):
                return True
    return False


def check_quads(page_h, page_w, quads, restored, scale, feather, rows=ROW_H):
    """the refusals, all ValueError naming the region, and per region a dict: ``quad`` (the corners as floats), ``cw``, ``ch`` (``crop_size``),
    ``out_quad`` (the corners in the enlarged page, s·quad), ``rw``, ``rh`` (s·cw, s·ch: the upright foreground's size) and ``bbox`` (bx0, by0,
    bw, bh: ``out_quad``'s bounding box rounded outward and clipped to the enlarged page).  ``restored[i]``: region i has a line to paste (the
    others keep the background: only their corners are checked).  Refused: ``scale`` outside [1, 8] or ``feather`` outside [0, 1024] (integers); a
    region that is not four finite points; a coordinate beyond ±32768; corners that are not strictly convex in clockwise order with y down (every
    cross product of successive edges > 0; a mirrored, counter-clockwise quadrilateral is named as such); a bounding box that misses the page; a
    restored region's foreground under rows / 16 rows; two restored regions whose interiors intersect.  A quadrilateral partly outside the page
    is allowed: the crop replicates the page's border and the paste is clipped."""
    pages.check_request(scale, feather, len(quads), len(restored), "quadrilateral", "quadrilaterals")
    s, page_h, page_w, out = int(scale), int(page_h), int(page_w), []
    for i, q in enumerate(quads):
        try:
            pts = np.asarray(q, dtype=np.float64)
        except (TypeError, ValueError):
            pts = np.zeros((0,))
        if pts.shape != (4, 2) or not np.isfinite(pts).all():
            raise ValueError("region %d: four finite corners [[x, y], [x, y], [x, y], [x, y]] expected, got %r" % (i, q))
        if np.abs(pts).max() > MAX_COORD:
            raise ValueError("region %d: a corner coordinate lies beyond +-%d" % (i, int(MAX_COORD)))
        quad = [(float(x), float(y)) for x, y in pts]
        cross = []
        for k in range(4):
            (ax, ay), (bx, by), (cx, cy) = quad[k], quad[(k + 1) % 4], quad[(k + 2) % 4]
            cross.append((bx - ax) * (cy - by) - (by - ay) * (cx - bx))
        if all(c < 0.0 for c in cross):
            raise ValueError("region %d: the corners run counter-clockwise (a mirrored quadrilateral): top-left, top-right, bottom-right, bottom-left "
                             "of the line as it is read expected" % i)
        if not all(c > 0.0 for c in cross):
            raise ValueError("region %d: the corners %s are not strictly convex (top-left, top-right, bottom-right, bottom-left expected)" % (i, quad))
        xs, ys = [p[0] for p in quad], [p[1] for p in quad]
        if max(0, math.floor(min(xs))) >= min(page_w, math.ceil(max(xs))) or max(0, math.floor(min(ys))) >= min(page_h, math.ceil(max(ys))):
            raise ValueError("region %d: its bounding box [%g, %g] x [%g, %g] misses the %d x %d page" % (i, min(xs), max(xs), min(ys), max(ys), page_w, page_h))
        cw, ch = crop_size(quad)
        out_quad = [(s * x, s * y) for x, y in quad]
        bx0, by0 = max(0, math.floor(s * min(xs))), max(0, math.floor(s * min(ys)))
        bx1, by1 = min(s * page_w, math.ceil(s * max(xs))), min(s * page_h, math.ceil(s * max(ys)))
        try:                                                                                  # both maps and their inverses exist (they do for every such quadrilateral short of overflow)
            inverse_map(quad_map(quad, cw, ch))
            inverse_map(quad_map(out_quad, s * cw, s * ch))
        except (ValueError, ZeroDivisionError, OverflowError) as e:
            raise ValueError("region %d: no projective map for the corners %s (%s)" % (i, quad, e)) from None
        out.append(dict(quad=quad, cw=cw, ch=ch, out_quad=out_quad, rw=s * cw, rh=s * ch, bbox=(int(bx0), int(by0), int(bx1 - bx0), int(by1 - by0))))
        if restored[i] and s * ch * pages.MIN_RECT_H_DIV < rows:
            raise ValueError("region %d: its line is %d rows high at scale %d, under the %d a %d-row line can be reduced to"
                             % (i, s * ch, s, rows // pages.MIN_RECT_H_DIV, rows))
    live = [i for i in range(len(quads)) if restored[i]]
    for n, i in enumerate(live):
        for j in live[:n]:
            if not _separated(out[i]["quad"], out[j]["quad"]):
                raise ValueError("regions %d and %d overlap: the paste blends in place, so an overlap has no defined order" % (j, i))
    return out


def box_quad(box):
    """an axis-aligned box [x1, y1, x2, y2] → its four corners in reading order"""
    x1, y1, x2, y2 = box
    return [[x1, y1], [x2, y1], [x2, y2], [x1, y2]]


# ------------------------------------------------------------------------------------------------------------------- the definition
def compose_quads_host(page, lines, quads, scale=4, feather=8):
    """the definition of a page: ``page`` uint8 RGB [H, W, 3]; ``lines[i]``: region i's restored line, uint8 BGR [rows, src_w, 3]
    (``MarconetPipeline.restore_lines`` of the crop ``warp_crop_host(page, quad_map(q, cw, ch), cw, ch)``), or None for a region that keeps the
    background; ``quads[i]`` its corners → uint8 RGB [s·H, s·W, 3]: ``lq_io.resize_cubic(page, s, s)`` with, for every line, its upright
    foreground ``pages.line_to_rect(line, s·cw, s·ch)`` pasted by ``warp_paste_host`` under N = ``inverse_map(quad_map(s·q, s·cw, s·ch))``."""
    page = pages._page_array(page)
    rows = next((int(np.shape(l)[0]) for l in lines if l is not None), ROW_H)
    regions = check_quads(page.shape[0], page.shape[1], quads, [l is not None for l in lines], scale, feather, rows)
    out = lq_io.resize_cubic(page, int(scale), int(scale))
    for line, r in zip(lines, regions):
        if line is not None:
            N = inverse_map(quad_map(r["out_quad"], r["rw"], r["rh"]))
            warp_paste_host(out, pages.line_to_rect(line, r["rw"], r["rh"]), N, r["rw"], r["rh"], int(feather))
    return out


# ------------------------------------------------------------------------------------------------------------------- the device path
def crop_table(maps, sizes, c0s=None, base=0):
    """→ (numpy record array of ``mnet_quad_crop``, the flat buffer's size in bytes): crop k is ``sizes[k]`` = (w, h) under ``maps[k]`` from column
    ``c0s[k]`` (default 0) of its region's rectified crop; the crops are packed tightly in order from byte ``base``"""
    tab = np.zeros((len(maps),), dtype=np.dtype(_lib.QuadCrop))
    off = int(base)
    for k, (M, (w, h)) in enumerate(zip(maps, sizes)):
        tab[k] = (off, int(w), int(h), 0 if c0s is None else int(c0s[k]), 0, [float(v) for v in M])
        off += 3 * int(w) * int(h)
    return tab, off


def paste_table(regions, feather, atlas_xy):
    """→ numpy record array of ``mnet_quad_region``: ``regions[l]`` (a ``check_quads`` record) has its upright foreground at ``atlas_xy[l]``"""
    tab = np.zeros((len(regions),), dtype=np.dtype(_lib.QuadRegion))
    for l, (r, (ax0, ay0)) in enumerate(zip(regions, atlas_xy)):
        N = inverse_map(quad_map(r["out_quad"], r["rw"], r["rh"]))
        tab[l] = (int(ax0), int(ay0), r["rw"], r["rh"]) + tuple(r["bbox"]) + (int(feather), 0, [float(v) for v in N])
    return tab


def crop_quads(page_d, maps, sizes, c0s=None, base=0, dst=None):
    """``page_d`` uint8 RGB [H, W, 3] on the device → (uint8 [bytes] on the device: ``warp_crop_host`` of every crop, packed tightly in order from
    byte ``base``, the offsets of the crops): one copy of the table, one launch.  ``dst``: an existing flat buffer that holds the crops' bytes
    (the packed batch several sources share), written inside the crops only; None: a new one, the first ``base`` bytes left to the caller"""
    tab, nbytes = crop_table(maps, sizes, c0s, base)
    dst = pages.crop_buffer("crop_quads", dst, nbytes, page_d.device)
    with ops.on_device(page_d):
        ops.quad_crop_u8(page_d, ops.table_to_device(tab, page_d.device), max(int(w) for w, _ in sizes), max(int(h) for _, h in sizes), dst)
    return dst, [int(o) for o in tab["offset"]]


def paste_quads(out, joined, out_ws, regions, feather, rows=ROW_H):
    """``out``: the enlarged page on the device, changed IN PLACE; ``joined`` / ``out_ws`` as ``pages.compose_page`` takes them; ``regions``:
    ``check_quads``' records.  One ``mnet_paste_u8`` launch (feather 0) makes every line's upright foreground in a zeroed atlas [Σ rh, max rw, 3],
    the regions stacked vertically — ``pages.line_to_rect``'s bytes, by ``pages.build_table`` —, and one ``mnet_quad_paste_u8`` launch pastes them."""
    live = [i for i, w in enumerate(out_ws) if w is not None]
    if not live:
        return out
    rects, atlas_hw = pages.atlas_layout([None if w is None else (r["rw"], r["rh"]) for w, r in zip(out_ws, regions)])
    quad_d = ops.table_to_device(paste_table([regions[i] for i in live], feather, [rects[i][:2] for i in live]), out.device)
    atlas = pages.fill_atlas(joined, pages.build_table(rects, out_ws, 0, rows), atlas_hw)
    with ops.on_device(out):
        return ops.quad_paste_u8(atlas, quad_d, max(regions[i]["bbox"][2] for i in live), max(regions[i]["bbox"][3] for i in live), out)


def compose_page_quads(page, joined, out_ws, quads, scale=4, feather=8, device=None):
    """the device path of ``compose_quads_host``; the arguments are ``pages.compose_page``'s, with ``quads[i]`` in the place of the boxes.
    → uint8 RGB [s·H, s·W, 3] on the device.  Every refusal of ``compose_quads_host`` is raised before anything is copied or launched; then one
    copy of the page and one of each small table, one launch for the background, one for the foregrounds and one for all regions."""
    def check(H, W, rows):
        regions = check_quads(H, W, quads, [w is not None for w in out_ws], scale, feather, rows)
        return regions, [r["rh"] for r in regions]
    page, rows, regions = pages.page_to_device("compose_page_quads", page, joined, out_ws, device, check)
    return paste_quads(enlarge(page, int(scale)), joined, out_ws, regions, int(feather), rows)


enlarge = pages.enlarge       # the background step is ``pages``'; the name stays here for its callers


def char_boxes_in_crop(boxes, M, cw, ch):
    """character boxes in PAGE pixels — [x1, y1, x2, y2] or four corners [[x, y]] x 4 each — → boxes in the rectified crop of the region whose crop
    map is ``M``: the corners go through ``inverse_map(M)``, and the interval [min u, max u] clamped to [0, cw] becomes the box [u1, 0, u2, ch]"""
    N, out = inverse_map(M), []
    for b in boxes:
        pts = np.asarray(b, dtype=np.float64)
        pts = np.asarray(box_quad(pts), dtype=np.float64) if pts.shape == (4,) else pts
        if pts.shape != (4, 2):
            raise ValueError("a character box [x1, y1, x2, y2] or four corners expected, got %r" % (b,))
        us = [map_point(N, float(x), float(y))[0] for x, y in pts]
        out.append([min(max(min(us), 0.0), float(cw)), 0, min(max(max(us), 0.0), float(cw)), int(ch)])
    return out
