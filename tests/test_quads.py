"""not-gpu: the host side of the quadrilateral page path (marconet_amd/quads.py, mnet_quad_crop_u8, mnet_quad_paste_u8) — csrc/quad_map.h compiled
for the CPU against the numpy statement, the exactness of the geometry at right angles, one general quadrilateral, the refusals, the C layout of the
two descriptors, the entry points' argument checks (the library loads without a GPU) and the build script's lines.  Every comparison of pixels is
np.array_equal."""
import ctypes
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from marconet_amd import _lib, lq_io, pages, quads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marconet_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
GENERAL = [(20.25, 8.5), (120.0, 14.75), (118.5, 40.0), (17.0, 30.5)]      # fractional corners, visibly non-parallel sides


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise RuntimeError("no C++ compiler found")


def _orientations(x1, y1, x2, y2):
    """the four right-angle orientations of a box: k → its corners in the reading order of a line whose crop is np.rot90(page[y1:y2, x1:x2], k)"""
    tl, tr, br, bl = (x1, y1), (x2, y1), (x2, y2), (x1, y2)
    return {0: [tl, tr, br, bl], 1: [tr, br, bl, tl], 2: [br, bl, tl, tr], -1: [bl, tl, tr, br]}


# ------------------------------------------------------------------------------------------------------------------------- quad_map.h
_MAP_MAIN = r'''
#include <stdio.h>
#include <string.h>
#include "quad_map.h"
/* stdin: commands -> stdout: one line of integers each.  The source of 'b' is src[y][x][c] = (7 x + 13 y + 101 c + x y) & 255. */
static unsigned long long bits(double d) { unsigned long long u; memcpy(&u, &d, 8); return u; }
int main(void) {
    char what;
    static uint8_t src[32 * 32 * 3];
    while (scanf(" %c", &what) == 1) {
        if (what == 'p') {                 /* p m0 .. m8 x y: valid, the bits of u and v, quad_fix of both (0 where invalid) */
            double m[9], x, y;
            for (int k = 0; k < 9; ++k) if (scanf("%la", &m[k]) != 1) return 2;
            if (scanf("%la %la", &x, &y) != 2) return 2;
            const QuadPos p = quad_pos(m, x, y);
            printf("%d %llu %llu %d %d\n", p.valid, p.valid ? bits(p.u) : 0ull, p.valid ? bits(p.v) : 0ull, p.valid ? quad_fix(p.u) : 0, p.valid ? quad_fix(p.v) : 0);
        } else if (what == 'f') {          /* f t: quad_fix */
            double t;
            if (scanf("%la", &t) != 1) return 2;
            printf("%d\n", quad_fix(t));
        } else if (what == 'b') {          /* b w h qx qy: the three channels of quad_bilinear */
            int w, h, qx, qy;
            if (scanf("%d %d %d %d", &w, &h, &qx, &qy) != 4 || w < 1 || h < 1 || w > 32 || h > 32) return 2;
            for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) for (int c = 0; c < 3; ++c) src[(y * w + x) * 3 + c] = (uint8_t)((7 * x + 13 * y + 101 * c + x * y) & 255);
            printf("%d %d %d\n", quad_bilinear(src, (size_t)w * 3, 3, w, h, qx, qy), quad_bilinear(src + 1, (size_t)w * 3, 3, w, h, qx, qy),
                   quad_bilinear(src + 2, (size_t)w * 3, 3, w, h, qx, qy));
        } else return 4;
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def map_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("quad_map")
    src, exe = str(d / "quad_map_main.cpp"), str(d / "quad_map_main")
    with open(src, "w") as f:
        f.write(_MAP_MAIN)
    subprocess.check_call([_cxx(), "-O2", "-ffp-contract=off", "-I", CSRC, src, "-o", exe])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
    return [[int(v) for v in l.split()] for l in out if l]


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def test_position_header_matches_numpy(map_exe):
    """quad_pos and quad_fix on a few thousand random positions of the general quadrilateral's two maps, on pixel centres, outside the source on
    all four sides, at D <= 0 and under a NaN or infinite coefficient: the same validity, the same bits, the same 1/64 positions"""
    rng = np.random.default_rng(11)
    cw, ch = quads.crop_size(GENERAL)
    M = quads.quad_map(GENERAL, cw, ch)
    N = quads.inverse_map(M)
    ident = [1.0, 0.0, 5.0, 0.0, 1.0, 7.0, 0.0, 0.0, 1.0]
    cases = []
    for m, (xs, ys) in ((M, (cw, ch)), (N, (140, 50)), (ident, (20, 20))):
        pts = rng.uniform([-30.0, -30.0], [xs + 30.0, ys + 30.0], (1500, 2))
        centres = np.stack(np.meshgrid(np.arange(-3, 6) + 0.5, np.arange(-3, 6) + 0.5), -1).reshape(-1, 2)       # pixel centres, also outside on every side
        far = np.float64([[-1e6, 3.5], [1e6, 3.5], [3.5, -1e6], [3.5, 1e6], [1e300, 1e300], [-1e300, 2.0]])
        cases += [(m, x, y) for x, y in np.concatenate([pts, centres, far])]
    neg = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.01, 0.0, 1.0]                                                    # D = 1 - x / 100: 0 at x = 100, negative beyond
    cases += [(neg, x, 2.5) for x in (99.5, 100.0, 100.5, 1000.5)]
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(9):
            m = list(M)
            m[k] = bad
            cases.append((m, 10.5, 4.5))
    got = _run(map_exe, ["p " + " ".join(float(v).hex() for v in list(m) + [x, y]) for m, x, y in cases])
    assert len(got) == len(cases)
    n_valid = 0
    for (m, x, y), g in zip(cases, got):
        u, v, valid = quads.quad_pos(m, x, y)
        if not valid:
            assert g == [0, 0, 0, 0, 0], (m, x, y)
            continue
        n_valid += 1
        assert g == [1, _bits(u), _bits(v), int(quads.quad_fix(u)), int(quads.quad_fix(v))], (m, x, y)
    assert n_valid > 4000 and len(cases) - n_valid >= 2 + 3 * 4                                              # both kinds were seen
    assert [g[0] for g in got[-27 - 4:-27]] == [1, 0, 0, 0]                                                  # D > 0, D = 0, D < 0
    u, v, valid = quads.quad_pos(ident, 3.5, 4.5)                                                            # a pixel centre stays one: weights 0
    assert valid and (u, v) == (8.5, 11.5) and int(quads.quad_fix(u)) == 8 * 64 and int(quads.quad_fix(v)) == 11 * 64


def test_fix_header_matches_numpy(map_exe):
    rng = np.random.default_rng(12)
    ts = list(rng.uniform(-100.0, 100.0, 2000)) + list(np.arange(-8, 9) / 64.0 + 0.5) + list(np.arange(-8, 9) / 128.0) + \
        [1e300, -1e300, float("inf"), -float("inf"), 2.0 ** 24, -2.0 ** 24, 2.0 ** 24 + 0.5, 16777215.9921875, 0.5 - 1.0 / 128, 0.5 - 1.0 / 128 - 1e-12]
    got = [g[0] for g in _run(map_exe, ["f " + float(t).hex() for t in ts])]
    assert got == [int(v) for v in quads.quad_fix(np.float64(ts))]
    assert quads.quad_fix(np.float64([1e300, -1e300])).tolist() == [1 << 30, -(1 << 30)]
    assert quads.quad_fix(np.float64([0.5, 1.5, 0.5 + 1 / 64, 0.5 - 1 / 128, 0.0])).tolist() == [0, 64, 1, 0, -32]


def test_bilinear_header_matches_numpy(map_exe):
    rng = np.random.default_rng(13)
    cases = []
    for w, h in ((1, 1), (2, 1), (1, 3), (7, 5), (32, 32)):
        qs = rng.integers(-3 * 64, (max(w, h) + 3) * 64, (400, 2))
        edge = [(-64, -64), (-1, -1), (0, 0), (63, 63), (64, 64), ((w - 1) * 64, (h - 1) * 64), ((w - 1) * 64 + 1, (h - 1) * 64 + 63), (w * 64, h * 64),
                (1 << 30, 1 << 30), (-(1 << 30), -(1 << 30)), (1 << 30, -(1 << 30)), (-(1 << 30), 1 << 30)]
        cases += [(w, h, int(qx), int(qy)) for qx, qy in list(qs) + edge]
    got = _run(map_exe, ["b %d %d %d %d" % c for c in cases])
    for (w, h, qx, qy), g in zip(cases, got):
        y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
        src = ((7 * x + 13 * y + 101 * c + x * y) & 255).astype(np.uint8)
        assert g == quads.quad_bilinear(src, np.int64([qx]), np.int64([qy]))[0].tolist(), (w, h, qx, qy)
        if qx % 64 == 0 and qy % 64 == 0:                                                                    # on a pixel centre: that pixel, clamped
            assert g == src[min(max(qy // 64, 0), h - 1), min(max(qx // 64, 0), w - 1)].tolist()


# ---------------------------------------------------------------------------------------------------------------- right-angle exactness
def test_right_angle_maps_are_exact_integers():
    x1, y1, x2, y2 = 13, 7, 60, 29
    W, H = x2 - x1, y2 - y1
    want = {0: ([1, 0, x1, 0, 1, y1, 0, 0, 1], (W, H)), 1: ([0, -1, x2, 1, 0, y1, 0, 0, 1], (H, W)),
            2: ([-1, 0, x2, 0, -1, y2, 0, 0, 1], (W, H)), -1: ([0, 1, x1, -1, 0, y2, 0, 0, 1], (H, W))}
    for k, q in _orientations(x1, y1, x2, y2).items():
        assert quads.crop_size(q) == want[k][1], k
        M = quads.quad_map(q, *quads.crop_size(q))
        assert [float(v) for v in M] == [float(v) for v in want[k][0]], k
        N = quads.inverse_map(M)
        assert all(float(v) == int(v) and abs(v) <= max(x2, y2) for v in N), (k, N)
        P = np.float64(M).reshape(3, 3) @ np.float64(N).reshape(3, 3)
        assert np.array_equal(P, np.eye(3)), k
    assert quads.inverse_map([1, 0, x1, 0, 1, y1, 0, 0, 1]) == [1, 0, -x1, 0, 1, -y1, 0, 0, 1]
    assert quads.inverse_map([2, 0, 0, 0, 4, 0, 0, 0, 1]) == [0.5, 0, 0, 0, 0.25, 0, 0, 0, 1]                  # the true inverse: adjugate / determinant
    for bad in ([1, 0, 0, 0, -1, 0, 0, 0, 1], [1, 2, 0, 2, 4, 0, 0, 0, 1], [float("nan"), 0, 0, 0, 1, 0, 0, 0, 1]):
        with pytest.raises(ValueError, match="determinant"):                                                 # mirrored, singular, not a number
            quads.inverse_map(bad)


def test_right_angle_crops_are_slices_and_rotations():
    rng = np.random.default_rng(14)
    page = rng.integers(0, 256, (40, 90, 3), dtype=np.uint8)
    for box in ((13, 7, 60, 29), (0, 0, 90, 40), (89, 39, 90, 40)):
        x1, y1, x2, y2 = box
        for k, q in _orientations(*box).items():
            cw, ch = quads.crop_size(q)
            crop = quads.warp_crop_host(page, quads.quad_map(q, cw, ch), cw, ch)
            assert np.array_equal(crop, np.rot90(page[y1:y2, x1:x2], k)), (box, k)
    q = _orientations(13, 7, 60, 29)[0]
    M = quads.quad_map(q, 47, 22)
    assert np.array_equal(quads.warp_crop_host(page, M, 10, 22, c0=30), page[7:29, 43:53])                 # a window of the crop


@pytest.mark.parametrize("scale", (1, 4))
@pytest.mark.parametrize("feather", (0, 8))
def test_right_angle_pastes_are_feather_blends(scale, feather):
    rng = np.random.default_rng(15)
    s = scale
    bg = rng.integers(0, 256, (40 * s, 90 * s, 3), dtype=np.uint8)
    x1, y1, x2, y2 = (s * v for v in (13, 7, 60, 29))
    for k, q in _orientations(x1, y1, x2, y2).items():
        rw, rh = quads.crop_size(q)
        fg = rng.integers(0, 256, (rh, rw, 3), dtype=np.uint8)
        N = quads.inverse_map(quads.quad_map(q, rw, rh))
        got = quads.warp_paste_host(bg.copy(), fg, N, rw, rh, feather)
        want = bg.copy()
        want[y1:y2, x1:x2] = pages.feather_blend(bg[y1:y2, x1:x2], np.rot90(fg, -k), feather)
        assert np.array_equal(got, want), k


@pytest.mark.parametrize("scale", (1, 4))
def test_compose_quads_host_with_boxes_is_compose_host(scale):
    rng = np.random.default_rng(16)
    page = rng.integers(0, 256, (40, 90, 3), dtype=np.uint8)
    lines = [rng.integers(0, 256, (128, 333, 3), dtype=np.uint8), None, rng.integers(0, 256, (128, 64, 3), dtype=np.uint8)]
    boxes = [[2, 3, 60, 20], [0, 0, 90, 40], [70, 25, 90, 40]]
    got = quads.compose_quads_host(page, lines, [quads.box_quad(b) for b in boxes], scale, 8)
    assert np.array_equal(got, pages.compose_host(page, lines, boxes, scale, 8))
    assert np.array_equal(quads.compose_quads_host(page, [], [], scale, 0), lq_io.resize_cubic(page, scale, scale))


# -------------------------------------------------------------------------------------------------------------------- one general quad
def _area_perimeter(q):
    n = len(q)
    area = 0.5 * abs(sum(q[k][0] * q[(k + 1) % n][1] - q[(k + 1) % n][0] * q[k][1] for k in range(n)))
    return area, sum(math.hypot(q[(k + 1) % n][0] - q[k][0], q[(k + 1) % n][1] - q[k][1]) for k in range(n))


def test_general_quadrilateral():
    s = 4
    cw, ch = quads.crop_size(GENERAL)
    assert (cw, ch) == (101, 24)
    M = quads.quad_map(GENERAL, cw, ch)
    assert M[6] != 0.0 and M[7] != 0.0                                                                       # a true perspective map
    N = quads.inverse_map(M)
    for (x, y), (cx, cy) in zip(GENERAL, ((0, 0), (cw, 0), (cw, ch), (0, ch))):
        px, py = quads.map_point(M, cx, cy)
        assert abs(px - x) <= 1e-9 and abs(py - y) <= 1e-9
        bx, by = quads.map_point(N, x, y)
        assert abs(bx - cx) <= 1e-9 and abs(by - cy) <= 1e-9
    # the bilinear path is exercised: at least half of the crop's samples have a fractional weight (a condition on the input)
    x = np.arange(cw, dtype=np.float64)[None, :] + 0.5
    y = np.arange(ch, dtype=np.float64)[:, None] + 0.5
    u, v, valid = quads.quad_pos(M, x, y)
    assert valid.all()
    frac = ((quads.quad_fix(u) & 63) != 0) | ((quads.quad_fix(v) & 63) != 0)
    assert 2 * int(frac.sum()) >= frac.size
    rng = np.random.default_rng(17)
    page = rng.integers(0, 256, (50, 140, 3), dtype=np.uint8)
    crop = quads.warp_crop_host(page, M, cw, ch)
    assert crop.shape == (ch, cw, 3) and crop.dtype == np.uint8
    flat = quads.warp_crop_host(np.full_like(page, 77), M, cw, ch)
    assert (flat == 77).all()                                                                                # the weights sum to one
    # the paste: the number of pasted pixels is the polygon's area, up to its perimeter; nothing else changes
    out_quad = [(s * px, s * py) for px, py in GENERAL]
    rw, rh = s * cw, s * ch
    No = quads.inverse_map(quads.quad_map(out_quad, rw, rh))
    bg = np.zeros((s * 50, s * 140, 3), np.uint8)
    got = quads.warp_paste_host(bg.copy(), np.full((rh, rw, 3), 200, np.uint8), No, rw, rh, 0)
    area, perimeter = _area_perimeter(out_quad)
    pasted = int((got[:, :, 0] == 200).sum())
    print("pasted pixels %d, polygon area %.1f, perimeter %.1f" % (pasted, area, perimeter))
    assert abs(pasted - area) <= perimeter
    assert ((got == 200) | (got == 0)).all() and np.array_equal(got[:, :, 0], got[:, :, 2])
    r = quads.check_quads(50, 140, [GENERAL], [True], s, 8)[0]
    bx0, by0, bw, bh = r["bbox"]
    mask = np.ones(bg.shape[:2], bool)
    mask[by0:by0 + bh, bx0:bx0 + bw] = False
    assert (got[mask] == 0).all() and (r["rw"], r["rh"]) == (rw, rh)                                         # the bounding box holds every pasted pixel
    soft = quads.warp_paste_host(bg.copy(), np.full((rh, rw, 3), 200, np.uint8), No, rw, rh, 8)
    assert np.array_equal(soft != 0, got != 0) and soft.max() == 200 and 0 < soft[soft != 0].min() < 200      # the feather: a ramp inside the same pixels


# a strong trapezoid (parallel sides 2 : 1, so its vanishing line is one width to the left of it) at three places of the page: the line between
# the page's origin and the region, the line THROUGH the origin, and the origin on the region's side of the line
TRAPEZOIDS = {"line between origin and region": [(200, 40), (300, 30), (300, 70), (200, 60)],
              "line through the origin": [(100, 40), (200, 30), (200, 70), (100, 60)],
              "origin on the region's side": [(60, 40), (160, 30), (160, 70), (60, 60)]}


@pytest.mark.parametrize("where", list(TRAPEZOIDS))
def test_strong_perspective_is_pasted_wherever_its_vanishing_line_runs(where):
    """whether a region is restored must not depend on where it lies relative to page pixel (0, 0): the inverse map's denominator is positive over
    the whole quadrilateral, so the paste covers the polygon (its area, up to its perimeter) and the page definition changes those pixels"""
    q = TRAPEZOIDS[where]
    x0 = q[0][0]
    rw, rh = quads.crop_size(q)
    M = quads.quad_map(q, rw, rh)
    N = quads.inverse_map(M)
    centre = N[6] * (x0 + 50) + N[7] * 50 + N[8]
    assert abs(N[6] * (x0 - 100) + N[8]) <= 1e-9 * centre and abs(N[7]) * 80 <= 1e-9 * centre                # the vanishing line: x = x0 - 100
    for (x, y), (cx, cy) in zip(q, ((0, 0), (rw, 0), (rw, rh), (0, rh))):
        bx, by = quads.map_point(N, x, y)
        assert abs(bx - cx) <= 1e-9 and abs(by - cy) <= 1e-9
    probes = list(q) + [(x0 + 50, 50), (x0 + 0.5, 50.5), (x0 + 99.5, 30.5)]
    assert all(N[6] * x + N[7] * y + N[8] > 0.0 for x, y in probes)                                          # valid over the region, corners included
    assert all(abs((N[6] * x + N[7] * y + N[8]) * (M[6] * u + M[7] * v + M[8]) - 1.0) <= 1e-12               # D_N = 1 / D_M: the true inverse
               for (x, y), (u, v) in zip(q, ((0, 0), (rw, 0), (rw, rh), (0, rh))))
    bg = np.zeros((80, 320, 3), np.uint8)
    got = quads.warp_paste_host(bg.copy(), np.full((rh, rw, 3), 200, np.uint8), N, rw, rh, 0)
    area, perimeter = _area_perimeter(q)
    pasted = int((got[:, :, 0] == 200).sum())
    print("%s: pasted pixels %d, polygon area %.1f, perimeter %.1f" % (where, pasted, area, perimeter))
    assert area == 3000.0 and abs(pasted - area) <= perimeter
    assert got[50, x0 + 50, 0] == 200 and got[50, x0 - 2, 0] == 0 and got[32, x0 + 5, 0] == 0 and got[32, x0 + 95, 0] == 200
    rng = np.random.default_rng(18)
    page = rng.integers(0, 256, (80, 320, 3), dtype=np.uint8)
    line = rng.integers(0, 256, (128, 300, 3), dtype=np.uint8)
    out = quads.compose_quads_host(page, [line], [q], 1, 0)
    changed = int((out != page).any(axis=2).sum())
    assert abs(changed - area) <= perimeter
    boxes = quads.char_boxes_in_crop([[x0, 30, x0 + 50, 70], [x0 + 50, 30, x0 + 100, 70]], M, rw, rh)       # the crop map's inverse serves here too
    assert abs(boxes[0][0]) <= 1e-9 and abs(boxes[1][2] - rw) <= 1e-9 and abs(boxes[0][2] - boxes[1][0]) <= 1e-9 and 0.5 * rw < boxes[0][2] < rw


# ------------------------------------------------------------------------------------------------------------- refusals and layouts
def test_check_quads_refusals_name_the_region():
    ok = [quads.box_quad([2, 3, 60, 20]), [(70.0, 25.5), (88.0, 24.0), (89.5, 38.0), (71.0, 39.0)]]

    def refused(match, quads_=ok, restored=(True, True), scale=2, feather=3):
        with pytest.raises(ValueError, match=match):
            quads.check_quads(40, 90, quads_, list(restored), scale, feather)

    recs = quads.check_quads(40, 90, ok, [True, True], 2, 3)
    assert recs[0]["bbox"] == (4, 6, 116, 34) and (recs[0]["rw"], recs[0]["rh"]) == (116, 34) and recs[0]["out_quad"][2] == (120, 40)
    refused("region 1: four finite corners", [ok[0], [(1, 2), (3, 4), (5, 6)]])
    refused("region 1: four finite corners", [ok[0], [(1, 2), (3, 4), (5, 6), (7, float("nan"))]])
    refused("region 1: four finite corners", [ok[0], [1, 2, 3, 4]])
    refused("region 0: a corner coordinate lies beyond", [[(0, 0), (40000, 0), (40000, 10), (0, 10)], ok[1]])
    refused("region 1: .*counter-clockwise", [ok[0], ok[1][::-1]])
    refused("region 1: .*not strictly convex", [ok[0], [(70, 25), (88, 25), (79, 27), (71, 39)]])             # a reflex corner
    refused("region 1: .*not strictly convex", [ok[0], [(70, 25), (80, 25), (90, 25), (71, 39)]])             # three corners on one line
    refused("region 1: .*not strictly convex", [ok[0], [(70, 25), (88, 39), (88, 25), (70, 39)]])             # self-intersecting
    refused("region 1: .*misses the 90 x 40 page", [ok[0], [(95, 5), (120, 5), (120, 20), (95, 20)]])
    refused("region 1: .*misses the 90 x 40 page", [ok[0], [(10, -30), (60, -30), (60, -2), (10, -2)]], restored=(True, False))
    refused("region 1: .*6 rows", [ok[0], quads.box_quad([70, 25, 90, 28])])
    quads.check_quads(40, 90, [ok[0], quads.box_quad([70, 25, 90, 28])], [True, False], 2, 3)               # not restored: only its corners are checked
    quads.check_quads(40, 90, [ok[0], quads.box_quad([70, 25, 90, 29])], [True, True], 2, 3)                # 8 rows: accepted
    refused("regions 0 and 1 overlap", [ok[0], [(55, 10), (80, 5), (82, 18), (57, 25)]])
    quads.check_quads(40, 90, [ok[0], [(55, 10), (80, 5), (82, 18), (57, 25)]], [True, False], 2, 3)        # a region without a line may cover another
    quads.check_quads(40, 90, [ok[0], quads.box_quad([60, 3, 90, 20])], [True, True], 2, 3)                 # touching quadrilaterals do not overlap
    quads.check_quads(40, 90, [ok[0], [(80, 20), (100, 25), (98, 45), (78, 38)]], [True, True], 2, 3)       # partly outside the page: allowed
    for scale in (0, 9, 1.5, -1):
        refused("scale", scale=scale)
    for feather in (-1, 1025, 0.5):
        refused("feather", feather=feather)
    refused("one line", restored=(True,))


def test_entry_point_refuses_before_anything_runs():
    """the host checks of restore_page_quads need neither weights on a device nor a launch"""
    from marconet_amd import networks
    from marconet_amd.pipeline import MarconetPipeline
    pipe = MarconetPipeline(networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet())
    page = np.zeros((60, 200, 3), np.uint8)
    a = lq_io.alphabet()[10]
    q = quads.box_quad([0, 0, 100, 30])
    with pytest.raises(ValueError, match="needs texts"):
        pipe.restore_page_quads(page, [q], None)
    with pytest.raises(ValueError, match="one text"):
        pipe.restore_page_quads(page, [q], [a, a])
    with pytest.raises(ValueError, match="restore_page_quads: regions 0 and 1 overlap"):
        pipe.restore_page_quads(page, [q, [(90, 10), (150, 5), (152, 40), (92, 45)]], [a, a])
    with pytest.raises(ValueError, match="restore_page_quads: region 1: .*counter-clockwise"):
        pipe.restore_page_quads(page, [q, q[::-1]], [a, a])
    with pytest.raises(ValueError, match="restore_page_quads: region 0: .*4 rows"):
        pipe.restore_page_quads(page, [quads.box_quad([0, 0, 100, 4])], [a], scale=1)
    with pytest.raises(ValueError, match="restore_page_quads: region 0: a character box"):
        pipe.restore_page_quads(page, [q], [a], char_boxes=[[[1, 2, 3]]])
    with pytest.raises(ValueError, match="scale"):
        pipe.restore_page_quads(page, [q], [a], scale=9)
    with pytest.raises(TypeError):
        pipe.restore_page_quads(page.astype(np.float32), [q], [a])


def test_char_boxes_in_crop():
    q = _orientations(10, 20, 70, 40)[1]                                                                     # read top to bottom: cw = 20, ch = 60
    M = quads.quad_map(q, 20, 60)
    got = quads.char_boxes_in_crop([[10, 20, 70, 25], [[10, 25], [70, 25], [70, 31.5], [10, 31.5]], [0, 38, 100, 50]], M, 20, 60)
    assert got == [[0.0, 0, 5.0, 60], [5.0, 0, 11.5, 60], [18.0, 0, 20.0, 60]]                               # the last one clamped into the crop
    with pytest.raises(ValueError):
        quads.char_boxes_in_crop([[1, 2, 3]], M, 20, 60)


CROP_FIELDS = ("offset", "w", "h", "c0", "reserved", "m")
REGION_FIELDS = ("ax0", "ay0", "rw", "rh", "bx0", "by0", "bw", "bh", "feather", "reserved", "n")


def test_descriptor_layouts_match_c(tmp_path):
    """sizeof / offsetof of the two descriptors from a C program compiled against the header == the ctypes mirrors and the tables' records"""
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "marconet_hip_quad.h"\nint main(void){\n'
    for name, fields in (("mnet_quad_crop", CROP_FIELDS), ("mnet_quad_region", REGION_FIELDS)):
        code += 'printf("%%zu %%zu", sizeof(%s), _Alignof(%s));\n' % (name, name)
        code += "".join('printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f in fields) + 'printf("\\n");\n'
    code += "return 0; }\n"
    cpath, exe = str(tmp_path / "quad_probe.c"), str(tmp_path / "quad_probe")
    with open(cpath, "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-std=c11", "-I", INCLUDE, cpath, "-o", exe])
    got = [[int(v) for v in l.split()] for l in subprocess.check_output([exe]).decode().strip().split("\n")]
    for row, S, fields in ((got[0], _lib.QuadCrop, CROP_FIELDS), (got[1], _lib.QuadRegion, REGION_FIELDS)):
        assert row == [ctypes.sizeof(S), ctypes.alignment(S)] + [getattr(S, f).offset for f in fields]
        assert np.dtype(S).itemsize == row[0]
    assert got[0] == [96, 8, 0, 8, 12, 16, 20, 24] and got[1] == [112, 8, 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40]
    tab, nbytes = quads.crop_table([list(range(9)), list(range(9, 18))], [(5, 3), (7, 2)], [0, 4])
    assert nbytes == 45 + 42 and tab["offset"].tolist() == [0, 45] and tab["c0"].tolist() == [0, 4] and tab["m"][1].tolist() == list(range(9, 18))
    assert (tab["w"].tolist(), tab["h"].tolist()) == ([5, 7], [3, 2])
    recs = quads.check_quads(40, 90, [quads.box_quad([2, 3, 60, 20])], [True], 2, 3)
    reg = quads.paste_table(recs, 3, [(0, 11)])
    assert tuple(reg[0])[:10] == (0, 11, 116, 34, 4, 6, 116, 34, 3, 0) and reg["n"][0].tolist() == [1, 0, -4, 0, 1, -6, 0, 0, 1]


def test_quad_header_compiles_as_c99(tmp_path):
    cpath = str(tmp_path / "probe.c")
    with open(cpath, "w") as f:
        f.write('#include "marconet_hip_quad.h"\nint main(void) {\n'
                'int (*c)(const uint8_t*, int32_t, int32_t, const mnet_quad_crop*, int32_t, int32_t, int32_t, uint8_t*, int64_t, void*) = mnet_quad_crop_u8;\n'
                'int (*p)(const uint8_t*, int32_t, int32_t, const mnet_quad_region*, int32_t, int32_t, int32_t, uint8_t*, int32_t, int32_t, void*) = mnet_quad_paste_u8;\n'
                '(void)c; (void)p; return MNET_ABI_VERSION == 4 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, cpath])
    assert set(_lib.QUAD_SYMBOLS) == {"mnet_quad_crop_u8", "mnet_quad_paste_u8"} and not set(_lib.QUAD_SYMBOLS) & set(_lib.SYMBOLS)
    assert _lib.ABI_VERSION == 4


def test_entry_points_validate_arguments_without_device():
    lib = _lib.load()
    ok = dict(page=16, page_h=70, page_w=150, crops=16, n=3, max_w=100, max_h=40, dst=16, dst_bytes=1 << 20)

    def crop(**kw):
        a = dict(ok, **kw)
        return lib.mnet_quad_crop_u8(a["page"], a["page_h"], a["page_w"], a["crops"], a["n"], a["max_w"], a["max_h"], a["dst"], a["dst_bytes"], None)

    for bad in ("page", "crops", "dst"):
        assert crop(**{bad: None}) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(page_h=0), dict(page_w=-3), dict(n=0), dict(n=-1), dict(max_w=0), dict(max_h=0), dict(max_h=-2), dict(dst_bytes=0), dict(dst_bytes=-5)):
        assert crop(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    assert crop(n=1 << 20, max_w=1 << 20, max_h=1 << 20) == -1 and b"too large" in lib.mnet_last_error()
    assert crop(n=1, max_w=(1 << 31) - 1, max_h=(1 << 31) - 1) == -1 and b"too large" in lib.mnet_last_error()
    for bad in (dict(crops=20), dict(crops=17), dict(crops=2)):
        assert crop(**bad) == -2 and b"aligned" in lib.mnet_last_error()

    okp = dict(atlas=16, atlas_h=64, atlas_w=300, regions=16, n=2, max_bw=200, max_bh=90, page=16, page_h=280, page_w=600)

    def paste(**kw):
        a = dict(okp, **kw)
        return lib.mnet_quad_paste_u8(a["atlas"], a["atlas_h"], a["atlas_w"], a["regions"], a["n"], a["max_bw"], a["max_bh"], a["page"], a["page_h"], a["page_w"], None)

    for bad in ("atlas", "regions", "page"):
        assert paste(**{bad: None}) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(atlas_h=0), dict(atlas_w=-1), dict(n=0), dict(n=-4), dict(max_bw=0), dict(max_bh=-1), dict(page_h=0), dict(page_w=0)):
        assert paste(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    assert paste(n=1 << 20, max_bw=1 << 20, max_bh=1 << 20) == -1 and b"too large" in lib.mnet_last_error()
    for bad in (dict(regions=20), dict(regions=17)):
        assert paste(**bad) == -2 and b"aligned" in lib.mnet_last_error()


def test_ops_and_drivers_refuse_cpu_tensors_and_bad_tables():
    from marconet_amd import lq_device, ops
    page = torch.zeros((80, 180, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.quad_crop_u8(page, torch.zeros((1, 96), dtype=torch.uint8), 10, 10, torch.zeros((300,), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.quad_paste_u8(page, torch.zeros((1, 112), dtype=torch.uint8), 10, 10, page.clone())
    lines = torch.zeros((2, 128, 300, 3), dtype=torch.uint8)
    qs = [quads.box_quad([0, 0, 90, 40]), quads.box_quad([80, 30, 100, 50])]
    with pytest.raises(ValueError, match="regions 0 and 1 overlap"):                          # found before any copy or launch
        quads.compose_page_quads(page.numpy(), lines, [300, 200], qs, 1, 3)
    with pytest.raises(ValueError, match="one joined line per region"):
        quads.compose_page_quads(page, lines, [300], qs[:1], 2, 3)
    with pytest.raises(ValueError, match="line width 301"):
        quads.compose_page_quads(page.numpy(), lines, [301, 200], [qs[0], quads.box_quad([90, 40, 100, 50])], 1, 3)
    with pytest.raises(ValueError, match="lies outside"):
        lq_device.prepare_packed(torch.zeros((100,), dtype=torch.uint8), [(4, 9)], [0])
    with pytest.raises(lq_io.StripTooWide):
        lq_device.prepare_packed(torch.zeros((3 * 8 * 200,), dtype=torch.uint8), [(8, 200)], [0])
    with pytest.raises(TypeError):
        lq_device.prepare_packed(np.zeros((100,), np.uint8), [(4, 8)], [0])


# ----------------------------------------------------------------------------------------------------------------------- the build
def test_build_script_compiles_and_stamps_the_kernels():
    sh = open(os.path.join(CSRC, "build.sh")).read()
    assert re.search(r'^SRCS="[^"]*\bquad_kernels\b[^"]*"', sh, flags=re.M)
    assert 'quad_kernels) echo "-ffp-contract=off" ;;' in sh
    assert ('[ "$1" = quad_kernels ] && cat "$HERE/quad_map.h" "$HERE/lq_taps.h" "$HERE/page_blend.h" "$HERE/page_tile.h" '
            '"$HERE/../../include/marconet_hip_quad.h"') in sh
    src = open(os.path.join(CSRC, "quad_kernels.hip")).read()
    assert '#include "quad_map.h"' in src and '#include "page_blend.h"' in src and '#include "page_tile.h"' in src and "marconet_hip_quad.h" in src
    assert '#include "lq_taps.h"' in open(os.path.join(CSRC, "quad_map.h")).read()
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in _lib.QUAD_SYMBOLS)
