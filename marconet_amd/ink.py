"""Ink: the one measure a page's layout is found from — ``blind_columns``' cells, ``layout``'s lines, ``skew``'s slope and lines.  The pure-host
definition, numpy and integers only, and the one driver of the three kernels (csrc/ink_kernels.hip) that return it with ``==``: sums of exact integers.

    luma        Y = (77 R + 150 G + 29 B + 128) >> 8, the integer luma of an RGB pixel.
    pair_ink    d(x, r) = |Y(x + 1, r) − Y(x, r)|; e(x, r) = d if d >= floor, else 0 (the noise floor: paper grain and JPEG ripple are differences of
                a few levels, a stroke's edge is tens; 0 and 1 are the same floor).  Filed under the LEFT pixel; blind to polarity; 0 on a flat row.
    row_ink     ink[r] = Σ_x d(x, r) over a box's row r: ``box_ink``'s ``rows`` at floor <= 1.  ``mnet_row_ink_u8``.
    box_ink     rows[r] = Σ_{x = 0 .. w − 2} e(x, r);  cols[x] = Σ_{r = 0 .. h − 1} e(x, r) for x <= w − 2, cols[w − 1] = 0.  ``mnet_box_ink_u8``.
    frame_ink   the same sums filed under the frame coordinates r' = r − sh(x), c' = x + sh(r) of a slope m, sh(v) = floor((v m + 32768) / 65536)
                (``skew``'s head states the frame and its box): at m = 0, for a box inside the page, ``box_ink``.  ``mnet_skew_ink_u8``."""
import numpy as np
import torch

from . import _lib, ops, pages


# -------------------------------------------------------------------------------------------------------------------------- the definition
def luma(rgb):
    """Y = (77 R + 150 G + 29 B + 128) >> 8 of a uint8 RGB array [..., 3] → int32 [...]"""
    rgb = np.asarray(rgb).astype(np.int32)
    return (77 * rgb[..., 0] + 150 * rgb[..., 1] + 29 * rgb[..., 2] + 128) >> 8


def pair_ink(rgb, floor=0):
    """e(x, r) of a uint8 RGB array [h, w, 3] the caller has checked — a page, or a crop of one — → int32 [h, max(w − 1, 0)] (the module's head)"""
    y = luma(rgb)
    d = np.abs(y[:, 1:] - y[:, :-1])
    return np.where(d >= int(floor), d, 0).astype(np.int32)


def row_ink(page, box):
    """the ink profile of ``page[y1:y2, x1:x2]``, int32 [y2 − y1] (the module's head states it): the numpy definition of ``mnet_row_ink_u8``"""
    x1, y1, x2, y2 = (int(v) for v in box)
    return pair_ink(pages._page_array(page)[y1:y2, x1:x2]).sum(axis=1).astype(np.int32)


def box_ink(page, box, floor):
    """both ink profiles of ``page[y1:y2, x1:x2]`` above ``floor`` → (rows int32 [y2 − y1], cols int32 [x2 − x1]) (the module's head states them):
    the numpy definition of ``mnet_box_ink_u8``"""
    x1, y1, x2, y2 = (int(v) for v in box)
    crop = pages._page_array(page)[y1:y2, x1:x2]
    e = pair_ink(crop, floor)
    cols = np.zeros((crop.shape[1],), np.int32)
    cols[:e.shape[1]] = e.sum(axis=0)
    return e.sum(axis=1).astype(np.int32), cols


def sh(v, m):
    """floor((v m + 32768) / 65536) for an integer or an integer array ``v``"""
    if isinstance(v, np.ndarray):
        return (v.astype(np.int64) * int(m) + 32768) >> 16
    return (int(v) * int(m) + 32768) >> 16


def scan_rect(box, m, H, W):
    """a page rectangle [px1, py1, px2, py2), inside the page, that holds every pixel (x, r) whose frame coordinates can lie in ``box`` — empty
    (px2 <= px1 or py2 <= py1, still inside the page) where there is none: what the sheared kernel's workgroups walk; any superset gives the same
    profiles.  x = c' − sh(r) and r = r' + sh(x): each range is bounded by the other's, three times in turn."""
    c1, r1, c2, r2 = (int(v) for v in box)
    H, W = int(H), int(W)
    x_lo, x_hi, y_lo, y_hi = 0, W - 1, 0, H - 1                                                     # inclusive
    for _ in range(3):
        if x_lo > x_hi or y_lo > y_hi:
            break
        s = (sh(y_lo, m), sh(y_hi, m))
        x_lo, x_hi = max(x_lo, c1 - max(s)), min(x_hi, c2 - 1 - min(s))
        if x_lo > x_hi:
            break
        s = (sh(x_lo, m), sh(x_hi, m))
        y_lo, y_hi = max(y_lo, r1 + min(s)), min(y_hi, r2 - 1 + max(s))
    if x_lo > x_hi or y_lo > y_hi:
        return [0, 0, 0, 0]
    return [x_lo, y_lo, x_hi + 1, y_hi + 1]


def profiles_of(e, box, m, rect=None):
    """``frame_ink`` of the page whose pair ink is ``e`` (``pair_ink``); ``rect``: the page rectangle to scan, ``scan_rect``'s unless given"""
    c1, r1, c2, r2 = (int(v) for v in box)
    H, W = int(e.shape[0]), int(e.shape[1]) + 1
    h, w = max(r2 - r1, 0), max(c2 - c1, 0)
    px1, py1, px2, py2 = scan_rect(box, m, H, W) if rect is None else (int(v) for v in rect)
    px2 = min(px2, W - 1)                                                                           # a pair is filed under its left pixel
    if h == 0 or w == 0 or px2 <= px1 or py2 <= py1:
        return np.zeros((h,), np.int32), np.zeros((w,), np.int32)
    x, r, sub = np.arange(px1, px2, dtype=np.int64), np.arange(py1, py2, dtype=np.int64), e[py1:py2, px1:px2]
    rp, cp = r[:, None] - sh(x, m)[None, :] - r1, x[None, :] + sh(r, m)[:, None] - c1
    keep = (rp >= 0) & (rp < h) & (cp >= 0) & (cp + 1 < w) & (sub != 0)
    ink = sub[keep].astype(np.float64)                                                              # sums under 2^25: exact
    return (np.bincount(rp[keep], weights=ink, minlength=h).astype(np.int32), np.bincount(cp[keep], weights=ink, minlength=w).astype(np.int32))


def frame_ink(page, box, m, floor):
    """both ink profiles of the frame box ``box`` = [c1, r1, c2, r2) of ``page`` at slope ``m`` above ``floor`` → (rows int32 [r2 − r1], cols int32
    [c2 − c1]) (the module's head states them): the numpy definition of ``mnet_skew_ink_u8``"""
    return profiles_of(pair_ink(pages._page_array(page), floor), box, m)


# ------------------------------------------------------------------------------------------------------------------- the kernels' tables
ROW_DTYPE, BOX_DTYPE, FRAME_DTYPE = (np.dtype(t) for t in (_lib.RowInkBox, _lib.BoxInkBox, _lib.SkewInkBox))      # once: numpy takes 10 us to read a ctypes structure


def row_table(boxes, page_w):
    """the integer ``boxes`` as views of a page ``page_w`` px wide → (numpy record array of ``mnet_ink_box`` — byte offset, pitch, h, w and the box's
    first row in the one profile buffer —, those first rows, the buffer's length): ``mnet_row_ink_u8``'s table, the profiles one behind the other"""
    tab, starts, total = np.zeros((len(boxes),), dtype=ROW_DTYPE), [], 0
    for k, (x1, y1, x2, y2) in enumerate(boxes):
        tab[k] = ((y1 * page_w + x1) * 3, 3 * page_w, y2 - y1, x2 - x1, total)
        starts.append(total)
        total += y2 - y1
    return tab, starts, total


def box_table(boxes, page_w, dtype):
    """the integer ``boxes`` as views of a page ``page_w`` px wide → (numpy record array of ``mnet_ink_box2`` (``dtype``: ``np.dtype(_lib.BoxInkBox)``) —
    byte offset, pitch, h, w and the first index of each profile in the one buffer —, per box (first index of rows, of cols), the buffer's
    length): ``mnet_box_ink_u8``'s table, a box's two profiles one behind the other"""
    tab, starts, total = np.zeros((len(boxes),), dtype=dtype), [], 0
    for k, (x1, y1, x2, y2) in enumerate(boxes):
        h, w = y2 - y1, x2 - x1
        tab[k] = ((y1 * page_w + x1) * 3, 3 * page_w, h, w, total, total + h, 0)
        starts.append((total, total + h))
        total += h + w
    return tab, starts, total


def frame_table(records, H, W, dtype):
    """``records``: (frame box, slope, columns wanted) each, of an H x W page → (numpy record array of ``mnet_skew_box`` (``dtype``:
    ``np.dtype(_lib.SkewInkBox)``), per record (first index of rows, of cols — None where not wanted), the buffer's length):
    ``mnet_skew_ink_u8``'s table with ``scan_rect``'s rectangles, a record's profiles one behind the other"""
    tab, starts, total = np.zeros((len(records),), dtype=dtype), [], 0
    for k, (box, m, want_cols) in enumerate(records):
        h, w = box[3] - box[1], box[2] - box[0]
        tab[k] = tuple(box) + (m, total, total + h if want_cols else -1) + tuple(scan_rect(box, m, H, W)) + (0,)
        starts.append((total, total + h if want_cols else None))
        total += h + (w if want_cols else 0)
    return tab, starts, total


# ------------------------------------------------------------------------------------------------------------------------ on the device
MAX_LAUNCH_BOXES, MAX_LAUNCH_TILES = 65535, 2 ** 24 - 1          # a tiled ink kernel's grid: its third axis, and 2^32 − 1 threads in workgroups of 256


def launch_chunks(hs, ws, tile_h, tile_w):
    """the records of a table (their grid extents: heights ``hs`` and widths ``ws``, in pixels) → [(k0, k1)]: consecutive runs that one launch of
    ``mnet_box_ink_u8`` or ``mnet_skew_ink_u8`` takes — at most 65535 records and (tiles of the run's largest record) x (records) <= 2^24 − 1
    workgroups.  One run, unless a page breaks into many thousands of boxes beside a large one."""
    out, k0, mh, mw = [], 0, 0, 0
    for k, (h, w) in enumerate(zip(hs, ws)):
        nh, nw = max(mh, -(-int(h) // tile_h)), max(mw, -(-int(w) // tile_w))
        if k > k0 and (k - k0 + 1 > MAX_LAUNCH_BOXES or nh * nw * (k - k0 + 1) > MAX_LAUNCH_TILES):
            out.append((k0, k))
            k0, nh, nw = k, -(-int(h) // tile_h), -(-int(w) // tile_w)
        mh, mw = nh, nw
    return out + [(k0, len(hs))] if len(hs) else out


def device_profiles(src_d, tab, total, hs, ws, launch, tile=None):
    """The one driver of the three ink kernels: the table ``tab`` (a numpy record array) of the page ``src_d`` on the device → its ``total`` profile
    integers, numpy int32: ONE upload of the table, the launches, ONE device→host copy.  ``launch(table, max_h, max_w, dst)``: one launch over a run
    of the table on the device, given the largest of the run's grid extents ``hs`` / ``ws``.  ``tile``: (tile_h, tile_w) of a kernel that ADDS —
    zeros, a launch per ``launch_chunks`` run; None: the row kernel, which writes every entry — no fill, ONE launch over the whole table."""
    tab_d = ops.table_to_device(tab, src_d.device)
    dst = (torch.empty if tile is None else torch.zeros)((total,), dtype=torch.int32, device=src_d.device)
    with ops.on_device(src_d):
        for k0, k1 in [(0, len(tab))] if tile is None else launch_chunks(hs, ws, *tile):
            launch(tab_d[k0:k1], int(hs[k0:k1].max()), int(ws[k0:k1].max()), dst)
    return dst.cpu().numpy()


def row_profiles(flat, page_w, boxes):
    """``row_ink`` of every box of ``boxes`` (integer, inside the page) of the page on the device — ``flat``: its uint8 [bytes], rows ``page_w`` px
    wide — → per box its profile: ONE ``mnet_row_ink_u8`` launch over all boxes as views of the page and one device→host copy"""
    tab, starts, total = row_table(boxes, page_w)
    ink = device_profiles(flat, tab, total, tab["h"], tab["w"], lambda t, max_h, _, dst: ops.row_ink_u8(flat, t, max_h, dst))
    return [ink[s:s + b[3] - b[1]] for s, b in zip(starts, boxes)]


def box_profiles(flat, page_w, boxes, floor, axis):
    """``box_ink`` of every box of ``boxes`` of the page on the device (``flat``, ``page_w``: as ``row_profiles`` takes them) → per box its rows
    (``axis`` 0) or its cols (``axis`` 1), what ``layout.xy_cut`` asks for: ONE ``mnet_box_ink_u8`` launch and one device→host copy"""
    tab, starts, total = box_table(boxes, page_w, BOX_DTYPE)
    ink = device_profiles(flat, tab, total, tab["h"], tab["w"], lambda t, max_h, max_w, dst: ops.box_ink_u8(flat, t, max_h, max_w, floor, dst=dst),
                          tile=(_lib.BOXINK_TILE_H, _lib.BOXINK_TILE_W))
    return [ink[s[axis]:s[axis] + b[3 - axis] - b[1 - axis]] for s, b in zip(starts, boxes)]


def frame_profiles(page_d, records, floor):
    """``frame_ink`` of every record of ``records`` — (frame box, slope, columns wanted) each — of the page on the device, uint8 RGB [H, W, 3] → per
    record (rows, cols or None): ONE ``mnet_skew_ink_u8`` launch over the records' scan rectangles and one device→host copy"""
    tab, starts, total = frame_table(records, page_d.shape[0], page_d.shape[1], FRAME_DTYPE)
    hs, ws = np.maximum(tab["py2"] - tab["py1"], 1), np.maximum(tab["px2"] - tab["px1"], 1)
    ink = device_profiles(page_d, tab, total, hs, ws, lambda t, max_h, max_w, dst: ops.skew_ink_u8(page_d, t, max_h, max_w, floor, dst=dst),
                          tile=(_lib.SKEWINK_TILE_H, _lib.SKEWINK_TILE_W))
    return [(ink[sr:sr + b[3] - b[1]], None if sc is None else ink[sc:sc + b[2] - b[0]]) for (sr, sc), (b, _, _) in zip(starts, records)]
