"""The skewed pages tests/test_skew.py and tests/test_skew_gpu.py find lines on (marconet_amd/skew.py), shared not copied.

``upright``: ``layout_scene.two_columns``' page with more air — a 400 x 600 page, text_h = 12: a left column of 12 lines at pitch 18 and a right one
of 11 lines at pitch 19 that starts 2 rows lower (6 and 7 blank rows between two lines; the columns' pitches differ, so no single period fits
the page's row profile), a gutter of 30 blank pixels, one wide line below: 24 lines.  ``skewed``: that page rotated about its centre by nearest
neighbour onto fresh paper, positive angles turning the lines down to the right — the direction of a positive slope of ``skew``."""
import math

import numpy as np

from tests.layout_scene import TEXT_H, draw_line, paper

H, W = 600, 400
ANGLES = (0.0, 0.5, 1.0, 2.5, -3.0, 5.0, -7.0)


def upright(seed=7, gutter=30):
    """→ (page uint8 [600, 400, 3], the 24 drawn lines [x1, y1, x2, y2] in reading order)"""
    rng = np.random.default_rng(seed)
    page, lines, right_x = paper(rng, H, W), [], None
    for left, y0, pitch, count in ((True, 40, 18, 12), (False, 42, 19, 11)):
        xa = 30 if left else right_x
        col = []
        for k in range(count):
            y = y0 + k * pitch
            col.append([xa, y, draw_line(rng, page, xa, y, xa + 150 - int(rng.integers(0, 30)), y + TEXT_H), y + TEXT_H])
        lines += col
        right_x = max(b[2] for b in col) + 2 + int(gutter)
    lines.append([30, 290, draw_line(rng, page, 30, 290, max(b[2] for b in lines[12:]), 290 + TEXT_H), 290 + TEXT_H])
    return page, lines


def rotate_point(x, y, deg):
    """the point (x, y) of the upright page → where it lies on the page rotated by ``deg``"""
    a, cx, cy = math.radians(deg), W / 2.0, H / 2.0
    return cx + (x - cx) * math.cos(a) - (y - cy) * math.sin(a), cy + (x - cx) * math.sin(a) + (y - cy) * math.cos(a)


def rotate_nearest(page, deg, seed=99):
    """``page`` rotated about its centre by ``deg`` degrees, nearest neighbour; what comes from outside the page is fresh paper"""
    h, w = page.shape[:2]
    a, cx, cy = math.radians(deg), w / 2.0, h / 2.0
    y, x = np.mgrid[0:h, 0:w]
    dx, dy = x + 0.5 - cx, y + 0.5 - cy
    sx = np.floor(cx + dx * math.cos(a) + dy * math.sin(a)).astype(np.int64)                        # the inverse rotation of the pixel's centre
    sy = np.floor(cy - dx * math.sin(a) + dy * math.cos(a)).astype(np.int64)
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    out = paper(np.random.default_rng(seed), h, w)
    out[inside] = page[sy[inside], sx[inside]]
    return out


def skewed(deg, seed=7):
    """→ (the upright page rotated by ``deg``, the rotated centres [(x, y)] of its 24 drawn lines, tan(deg) in Q16)"""
    page, lines = upright(seed)
    centres = [rotate_point(0.5 * (b[0] + b[2]), 0.5 * (b[1] + b[3]), deg) for b in lines]
    return (page if deg == 0 else rotate_nearest(page, deg)), centres, math.tan(math.radians(deg)) * 65536.0
