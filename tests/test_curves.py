"""not-gpu: the host side of the curved page path (marconet_amd/curves.py, mnet_curve_crop_u8, mnet_curve_paste_u8) — csrc/curve_map.h compiled for
the CPU against the numpy statement, the identities with ``pages`` and ``quads``, the coverage of the polygon, the continuity across seams, the
refusals, the C layout of the three records, the entry points' argument checks (the library loads without a GPU) and the build script's lines.
Every comparison of pixels is np.array_equal."""
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

from marconet_amd import _lib, curves, lq_io, pages, quads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marconet_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
TAPERED = [(187.0, 95.5), (198.7, 96.7), (204.5, 144.0), (177.0, 156.0)]          # a1 of the inverse changes sign inside this segment
PARALLELOGRAM = [(20.25, 8.5), (100.5, 14.75), (97.25, 40.0), (17.0, 33.75)]      # fractional corners, G exactly 0


def arc(cx, cy, r_in, r_out, deg0, deg1, K):
    """K points a side on two concentric circles; the angles (degrees, counter-clockwise as seen with y down: 90 is above the centre) run from
    deg0 to deg1; the first side is the circle of radius r_out"""
    a = [math.radians(d) for d in np.linspace(deg0, deg1, K)]
    top = [(cx + r_out * math.cos(t), cy - r_out * math.sin(t)) for t in a]
    bot = [(cx + r_in * math.cos(t), cy - r_in * math.sin(t)) for t in a]
    return top + bot[::-1]


def s_curve(x0, y0, n, step, amp, height):
    top = [(x0 + step * k, y0 + amp * math.sin(2.0 * math.pi * k / (n - 1))) for k in range(n)]
    return top + [(x, y + height) for x, y in reversed(top)]


SHAPES = {
    "arc": arc(110.0, 130.0, 70.0, 92.0, 150.0, 30.0, 6),                       # text over the top of a seal: 5 segments
    "inverted arc": arc(110.0, 20.0, 92.0, 70.0, 210.0, 330.0, 7),              # text along the bottom of a seal, read left to right
    "S-curve": s_curve(12.5, 60.25, 9, 24.0, 14.0, 21.5),
    "sideways arc": arc(40.0, 100.0, 60.0, 85.0, 60.0, -60.0, 8),               # read top to bottom around the right of a centre
    "tight arc": arc(110.0, 110.0, 6.0, 30.0, 170.0, 10.0, 9),                  # inner radius a quarter of the line's height
    "tapered chain": TAPERED[:2] + [(215.0, 100.0), (235.0, 140.0)] + TAPERED[2:],
}
PAGE_H, PAGE_W = 200, 260


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise RuntimeError("no C++ compiler found")


def _region(poly, scale=1, feather=0, page=(PAGE_H, PAGE_W)):
    return curves.check_curves(page[0], page[1], [poly], [True], scale, feather)[0]


# ------------------------------------------------------------------------------------------------------------------------ curve_map.h
_MAP_MAIN = r'''
#include <stdio.h>
#include <string.h>
#include "curve_map.h"
/* stdin: commands -> stdout: one line of integers each */
static unsigned long long bits(double d) { unsigned long long u; memcpy(&u, &d, 8); return u; }
int main(void) {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'p' || what == 'i') {          /* p c0 .. c7 u v: curve_pos;  i c0 .. c7 x y: curve_inv — valid, the bits of both results (0 where invalid) */
            double c[8], a, b;
            for (int k = 0; k < 8; ++k) if (scanf("%la", &c[k]) != 1) return 2;
            if (scanf("%la %la", &a, &b) != 2) return 2;
            if (what == 'p') {
                const CurvePos p = curve_pos(c, a, b);
                printf("%d %llu %llu\n", p.valid, p.valid ? bits(p.x) : 0ull, p.valid ? bits(p.y) : 0ull);
            } else {
                const CurveInv p = curve_inv(c, curve_prep(c), a, b);
                printf("%d %llu %llu\n", p.valid, p.valid ? bits(p.u) : 0ull, p.valid ? bits(p.v) : 0ull);
            }
        } else if (what == 't') {                  /* t qu u0 rw: curve_taps_x */
            int qu, u0, rw, x0, x1, ax;
            if (scanf("%d %d %d", &qu, &u0, &rw) != 3) return 2;
            curve_taps_x(qu, u0, rw, &x0, &x1, &ax);
            printf("%d %d %d\n", x0, x1, ax);
        } else return 4;
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def map_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("curve_map")
    src, exe = str(d / "curve_map_main.cpp"), str(d / "curve_map_main")
    with open(src, "w") as f:
        f.write(_MAP_MAIN)
    subprocess.check_call([_cxx(), "-O2", "-ffp-contract=off", "-I", CSRC, src, "-o", exe])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
    return [[int(v) for v in l.split()] for l in out if l]


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _cmd(what, c, a, b):
    return what + " " + " ".join(float(v).hex() for v in list(c) + [a, b])


def _header_segments():
    """(coefficients, a box of page points around the segment) of: every segment of the arc at scale 1 and 4, the tapered segment, a parallelogram"""
    out = []
    for poly, s in ((SHAPES["arc"], 1), (SHAPES["arc"], 4), (TAPERED, 1), (SHAPES["tight arc"], 2), (PARALLELOGRAM, 1)):
        r = _region(poly, s)
        for sg, q in zip(r["out_segs"], r["quads"]):
            xs, ys = [s * p[0] for p in q], [s * p[1] for p in q]
            out.append((sg, (min(xs) - 6.0, max(xs) + 6.0, min(ys) - 6.0, max(ys) + 6.0), r["rh"]))
    return out


def test_forward_header_matches_numpy(map_exe):
    """curve_pos on random positions of every kind of segment, on pixel centres of the strip, outside it, and under NaN or infinite coefficients:
    the same validity and the same bits"""
    rng = np.random.default_rng(21)
    cases = []
    for sg, _, rh in _header_segments():
        uv = rng.uniform([-3.0, -3.0], [sg["w"] + 3.0, rh + 3.0], (150, 2))
        centres = np.stack(np.meshgrid(np.arange(-1, 4) + 0.5, np.arange(-1, 4) + 0.5), -1).reshape(-1, 2)
        cases += [(sg["c"], u, v) for u, v in np.concatenate([uv, centres, np.float64([[1e300, 1e300], [-1e200, 2.5]])])]
    par = _region(PARALLELOGRAM)["segs"][0]["c"]
    assert par[3] == 0.0 and par[7] == 0.0                                                                  # G = 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(8):
            cases.append((par[:k] + [bad] + par[k + 1:], 10.5, 4.5))
    got = _run(map_exe, [_cmd("p", *case) for case in cases])
    assert len(got) == len(cases) > 3000
    n_valid = 0
    for (c, u, v), g in zip(cases, got):
        X, Y, valid = curves.curve_pos(c, u, v)
        n_valid += bool(valid)
        assert g == ([1, _bits(X), _bits(Y)] if valid else [0, 0, 0]), (c, u, v)
    assert n_valid > 3000 and len(cases) - n_valid >= 20
    M = quads.quad_map(PARALLELOGRAM, *quads.crop_size(PARALLELOGRAM))                                       # G = 0: quad_pos of the affine map, bit for bit
    u, v = rng.uniform(-5.0, 90.0, 500), rng.uniform(-5.0, 30.0, 500)
    X, Y, valid = curves.curve_pos(par, u, v)
    qu, qv, qvalid = quads.quad_pos(M, u, v)
    assert valid.all() and qvalid.all() and np.array_equal(X, qu) and np.array_equal(Y, qv)


def test_inverse_header_matches_numpy(map_exe):
    """curve_inv (u, v, valid) on a few thousand page points: random ones around every kind of segment, the pixel centres ON the seams of a chain
    whose rungs lie at half-integer abscissae, the whole tapered segment (a1 changes sign inside it), G = 0, points with disc < 0, NaN and
    infinite coefficients — the same validity and the same bits"""
    rng = np.random.default_rng(22)
    cases = []
    for sg, (xa, xb, ya, yb), _ in _header_segments():
        cases += [(sg["c"], x, y) for x, y in rng.uniform([xa, ya], [xb, yb], (120, 2))]
    seam = curves.box_polygon([10.5, 20.0, 70.5, 41.0], (30.5, 31.5, 50.5))                                  # rungs through pixel centres
    for sg in _region(seam)["out_segs"]:
        cases += [(sg["c"], x + 0.5, y + 0.5) for x in (10, 30, 31, 50, 70) for y in (19, 20, 30, 40, 41)]
    tap = _region(TAPERED)["out_segs"][0]
    xs, ys = np.meshgrid(np.arange(170, 212) + 0.5, np.arange(90, 160) + 0.5)
    tapered = [(tap["c"], x, y) for x, y in zip(xs.reshape(-1)[::3], ys.reshape(-1)[::3])]
    far = [(tap["c"], x, y) for x, y in rng.uniform([-400.0, -400.0], [800.0, 800.0], (600, 2))]
    cases += tapered + far
    par = _region(PARALLELOGRAM)["out_segs"][0]["c"]
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(8):
            cases.append((par[:k] + [bad] + par[k + 1:], 40.5, 20.5))
    got = _run(map_exe, [_cmd("i", *case) for case in cases])
    assert len(got) == len(cases) > 3000
    n_valid = 0
    for (c, x, y), g in zip(cases, got):
        u, v, valid = curves.curve_inv(c, x, y)
        n_valid += bool(valid)
        assert g == ([1, _bits(u), _bits(v)] if valid else [0, 0, 0]), (c, x, y)
    assert n_valid > 2500 and len(cases) - n_valid > 50

    def a1_disc(c, x, y):
        Ax, Ex, Fx, Gx, Ay, Ey, Fy, Gy = c
        qx, qy = x - Ax, y - Ay
        a1 = (Fx * Ey - Fy * Ex) - (qx * Gy - qy * Gx)
        return a1, a1 * a1 - 4.0 * (Fx * Gy - Fy * Gx) * -(qx * Ey - qy * Ex)
    inside = [(x, y) for c, x, y in tapered if _inside(TAPERED, x, y) > 0.01]
    signs = {a1_disc(tap["c"], x, y)[0] > 0.0 for x, y in inside}
    assert signs == {True, False} and len(inside) > 300                                                    # both branches of the root are taken INSIDE the segment
    assert sum(a1_disc(c, x, y)[1] < 0.0 for c, x, y in far) > 20                                            # disc < 0 was seen
    for x, y in inside:                                                                                      # and forward(inverse(p)) = p
        u, v, valid = curves.curve_inv(tap["c"], x, y)
        X, Y, _ = curves.curve_pos(tap["c"], u, v)
        assert valid and 0.0 <= u <= tap["w"] and 0.0 <= v <= 54.0 and abs(X - x) <= 1e-11 and abs(Y - y) <= 1e-11


def test_taps_header_matches_numpy(map_exe):
    """curve_taps_x is quad_taps' x half at quad_fix(u) + 64 u0, clamped into the whole foreground"""
    rng = np.random.default_rng(23)
    cases = [(int(q), int(u0), int(rw)) for q, u0, rw in zip(rng.integers(-64, 40 * 64, 500), rng.integers(0, 300, 500), rng.integers(1, 340, 500))]
    cases += [(-32, 0, 5), (-1, 0, 5), (0, 0, 1), (63, 4, 5), (64, 4, 5), (1 << 30, (1 << 31) - 1, (1 << 31) - 1), (-(1 << 30), 0, 7)]
    got = _run(map_exe, ["t %d %d %d" % c for c in cases])
    for (q, u0, rw), g in zip(cases, got):
        ix = (q + 64 * u0) >> 6
        assert g == [min(max(ix, 0), rw - 1), min(max(ix + 1, 0), rw - 1), q & 63], (q, u0, rw)


# ------------------------------------------------------------------------------------------------------------------------ identities
CUTS = ((), (40,), (20, 31, 32, 70))             # 1, 2 and 5 segments, one of them 1 pixel wide


@pytest.mark.parametrize("cuts", CUTS, ids=["1 segment", "2 segments", "5 segments"])
def test_integer_box_crops_are_slices(cuts):
    page = np.random.default_rng(24).integers(0, 256, (60, 120, 3), dtype=np.uint8)
    box = [13, 7, 90, 29]
    r = _region(curves.box_polygon(box, cuts), page=(60, 120))
    assert (r["cw"], r["ch"], len(r["segs"])) == (77, 22, len(cuts) + 1) and r["ws"] == list(np.diff([13] + list(cuts) + [90]))
    for sg, x in zip(r["segs"], [13] + list(cuts)):
        assert sg["c"] == [x, 1.0, 0.0, 0.0, 7.0, 0.0, 1.0, 0.0]
    assert np.array_equal(curves.warp_crop_host(page, r["segs"], 77, 22), page[7:29, 13:90])
    assert np.array_equal(curves.warp_crop_host(page, r["segs"], 30, 22, c0=15), page[7:29, 28:58])          # a window that starts and ends mid-segment
    for bad in (dict(w=78), dict(c0=48, w=30), dict(w=0), dict(c0=-1, w=5)):
        with pytest.raises(ValueError):
            curves.warp_crop_host(page, r["segs"], bad.get("w"), 22, bad.get("c0", 0))


@pytest.mark.parametrize("scale", (1, 4))
@pytest.mark.parametrize("feather", (0, 8))
def test_integer_box_pages_are_compose_host(scale, feather):
    rng = np.random.default_rng(25)
    page = rng.integers(0, 256, (40, 90, 3), dtype=np.uint8)
    lines = [rng.integers(0, 256, (128, 333, 3), dtype=np.uint8), None, rng.integers(0, 256, (128, 64, 3), dtype=np.uint8)]
    boxes = [[2, 3, 60, 20], [0, 0, 90, 40], [70, 25, 90, 40]]
    want = pages.compose_host(page, lines, boxes, scale, feather)
    for cuts in ([(), (), ()], [(30,), (45,), (80,)], [(5, 6, 30, 59), (10, 20, 30, 40), (71, 75, 76, 89)]):
        polys = [curves.box_polygon(b, c) for b, c in zip(boxes, cuts)]
        assert np.array_equal(curves.compose_curves_host(page, lines, polys, scale, feather), want), cuts
    assert np.array_equal(curves.compose_curves_host(page, [], [], scale, 0), lq_io.resize_cubic(page, scale, scale))


def test_parallelogram_is_quads():
    """a 4-point parallelogram with fractional corners: the strip's size, the crop and the paste are ``quads``' (the forward map bit for bit)"""
    rng = np.random.default_rng(26)
    page = rng.integers(0, 256, (60, 120, 3), dtype=np.uint8)
    q = PARALLELOGRAM
    assert q[0][0] - q[1][0] + q[2][0] - q[3][0] == 0.0 and q[0][1] - q[1][1] + q[2][1] - q[3][1] == 0.0
    cw, ch = quads.crop_size(q)
    r = _region(q, 4, 8, page=(60, 120))
    rq = quads.check_quads(60, 120, [q], [True], 4, 8)[0]
    assert (r["cw"], r["ch"], r["rw"], r["rh"], r["bbox"]) == (cw, ch, rq["rw"], rq["rh"], rq["bbox"]) and r["out_segs"][0]["box"] == rq["bbox"]
    assert np.array_equal(curves.warp_crop_host(page, r["segs"], cw, ch), quads.warp_crop_host(page, quads.quad_map(q, cw, ch), cw, ch))
    bg = rng.integers(0, 256, (240, 480, 3), dtype=np.uint8)
    fg = rng.integers(0, 256, (r["rh"], r["rw"], 3), dtype=np.uint8)
    N = quads.inverse_map(quads.quad_map(rq["out_quad"], rq["rw"], rq["rh"]))
    for F in (0, 8):
        want = quads.warp_paste_host(bg.copy(), fg, N, r["rw"], r["rh"], F)
        assert np.array_equal(curves.warp_paste_host(bg.copy(), fg, r["out_segs"], r["rw"], r["rh"], F), want), F
        assert (want != bg).any(axis=2).sum() > 8000
    line = rng.integers(0, 256, (128, 300, 3), dtype=np.uint8)
    assert np.array_equal(curves.compose_curves_host(page, [line], [q], 4, 8), quads.compose_quads_host(page, [line], [q], 4, 8))


# -------------------------------------------------------------------------------------------------------------------------- coverage
def _inside(poly, x, y):
    """an independent fp64 test: + the distance to the polygon's outline for a point inside it (even-odd rule), − that distance outside"""
    n, odd, best = len(poly), False, float("inf")
    for k in range(n):
        (x0, y0), (x1, y1) = poly[k], poly[(k + 1) % n]
        if (y0 > y) != (y1 > y) and x < x0 + (y - y0) * (x1 - x0) / (y1 - y0):
            odd = not odd
        dx, dy = x1 - x0, y1 - y0
        t = min(1.0, max(0.0, ((x - x0) * dx + (y - y0) * dy) / (dx * dx + dy * dy)))
        best = min(best, math.hypot(x - (x0 + t * dx), y - (y0 + t * dy)))
    return best if odd else -best


@pytest.mark.parametrize("scale", (1, 2))
@pytest.mark.parametrize("name", list(SHAPES))
def test_paste_covers_the_polygon_and_nothing_else(name, scale):
    """every page pixel whose centre lies more than 0.01 px inside the polygon is written — by one segment or another, no gap along a seam — and no
    pixel more than 0.01 px outside it is: no miss is allowed"""
    poly, s = SHAPES[name], scale
    r = _region(poly, s)
    fg = np.full((r["rh"], r["rw"], 3), 200, np.uint8)
    got = curves.warp_paste_host(np.zeros((s * PAGE_H, s * PAGE_W, 3), np.uint8), fg, r["out_segs"], r["rw"], r["rh"], 0)
    assert ((got == 0) | (got == 200)).all()
    written = got[:, :, 0] == 200
    bx0, by0, bw, bh = r["bbox"]
    assert not written[:by0].any() and not written[by0 + bh:].any() and not written[:, :bx0].any() and not written[:, bx0 + bw:].any()
    out_poly, missed, spilled, n_in = r["out_polygon"], 0, 0, 0
    for Y in range(by0, by0 + bh):
        for X in range(bx0, bx0 + bw):
            d = _inside(out_poly, X + 0.5, Y + 0.5)
            n_in += d > 0.01
            missed += d > 0.01 and not written[Y, X]
            spilled += d < -0.01 and bool(written[Y, X])
    print("%s at scale %d: %d pixel centres inside, %d written, %d missed, %d spilled" % (name, s, n_in, int(written.sum()), missed, spilled))
    assert n_in > 500 and missed == 0 and spilled == 0
    soft = curves.warp_paste_host(np.zeros_like(got), fg, r["out_segs"], r["rw"], r["rh"], 6)                # the feather: a ramp inside the same pixels
    assert np.array_equal(soft[:, :, 0] != 0, written) and soft.max() == 200 and 0 < soft[written].min() < 200


def test_textbook_root_rule_would_miss_the_tapered_segment():
    """the condition on the input that makes the tapered segment a test: choosing the root by a1's sign alone — a0 / z with z = −(a1 + copysign(r, a1))
    / 2 — leaves a good part of it unclaimed, the rule of curve_inv none"""
    sg = _region(TAPERED)["out_segs"][0]
    Ax, Ex, Fx, Gx, Ay, Ey, Fy, Gy = sg["c"]
    pts = [(X + 0.5, Y + 0.5) for Y in range(90, 160) for X in range(170, 212) if _inside(TAPERED, X + 0.5, Y + 0.5) > 0.01]
    lost = 0
    for x, y in pts:
        qx, qy = x - Ax, y - Ay
        a2, a1, a0 = Fx * Gy - Fy * Gx, (Fx * Ey - Fy * Ex) - (qx * Gy - qy * Gx), -(qx * Ey - qy * Ex)
        v = a0 / (-0.5 * (a1 + math.copysign(math.sqrt(a1 * a1 - 4.0 * a2 * a0), a1)))
        lost += not 0.0 <= v < 54.0
        u, v, valid = curves.curve_inv(sg["c"], x, y)
        assert valid and 0.0 <= u < sg["w"] and 0.0 <= v < 54.0
    assert len(pts) > 900 and lost > len(pts) // 10


# ------------------------------------------------------------------------------------------------------------------- seam continuity
def test_a_gradient_stays_continuous_across_seams():
    """a foreground that is a horizontal ramp, pasted along the arc: page neighbours that lie in different segments differ by no more than
    neighbours inside one segment do — the bound is taken from the same image's interior"""
    r = _region(SHAPES["arc"], 2)
    rw, rh = r["rw"], r["rh"]
    ramp = np.broadcast_to((np.arange(rw) * 255 // (rw - 1)).astype(np.uint8)[None, :, None], (rh, rw, 3))
    ids = np.zeros((rh, rw, 3), np.uint8)
    for k, sg in enumerate(r["out_segs"]):
        ids[:, sg["u0"]:sg["u0"] + sg["w"]] = 40 * (k + 1)
    shape = (2 * PAGE_H, 2 * PAGE_W, 3)
    img = curves.warp_paste_host(np.zeros(shape, np.uint8), np.ascontiguousarray(ramp), r["out_segs"], rw, rh, 0)[:, :, 0].astype(np.int64)
    seg = curves.warp_paste_host(np.zeros(shape, np.uint8), ids, r["out_segs"], rw, rh, 0)[:, :, 0].astype(np.int64)
    worst = {}
    for axis in (0, 1):
        a, b = (seg[:-1], seg[1:]) if axis == 0 else (seg[:, :-1], seg[:, 1:])
        d = np.abs(np.diff(img, axis=axis))
        both = (a > 0) & (b > 0)
        inner = both & (a == b) & (a % 40 == 0)                                                   # both in the plain interior of ONE segment
        across = both & (np.abs(a - b) >= 20)                                                     # the seam runs between the two pixels
        assert inner.sum() > 5000 and across.sum() > 20
        worst[axis] = (int(d[across].max()), int(d[inner].max()))
    print("largest step across a seam / inside a segment: rows %s, columns %s" % (worst[0], worst[1]))
    assert all(a <= i for a, i in worst.values())


# ------------------------------------------------------------------------------------------------------------- refusals and layouts
def test_strip_sizes_and_coefficients():
    ws, ch = curves.strip_sizes(PARALLELOGRAM)
    assert ([sum(ws)], ch) == ([quads.crop_size(PARALLELOGRAM)[0]], quads.crop_size(PARALLELOGRAM)[1])
    r = _region(SHAPES["arc"], 4)
    assert r["ws"] == [34] * 5 and r["ch"] == 22 and (r["cw"], r["rw"], r["rh"]) == (170, 680, 88)
    assert [sg["u0"] for sg in r["out_segs"]] == [0, 136, 272, 408, 544] and all(sg["w"] == 136 for sg in r["out_segs"])
    for sg, q in zip(r["out_segs"], r["quads"]):                                                             # the patch takes the rectangle's corners to the segment's
        for (u, v), (x, y) in zip(((0, 0), (136, 0), (136, 88), (0, 88)), q):
            X, Y, valid = curves.curve_pos(sg["c"], u, v)
            assert valid and abs(X - 4 * x) <= 1e-9 and abs(Y - 4 * y) <= 1e-9
        bx0, by0, bw, bh = sg["box"]
        assert bx0 == math.floor(4 * min(p[0] for p in q)) and bx0 + bw == math.ceil(4 * max(p[0] for p in q))
        assert by0 == math.floor(4 * min(p[1] for p in q)) and by0 + bh == math.ceil(4 * max(p[1] for p in q))
        RX, RY, RW, RH = r["bbox"]
        assert RX <= bx0 and bx0 + bw <= RX + RW and RY <= by0 and by0 + bh <= RY + RH
    out = _region(arc(250.0, 100.0, 30.0, 50.0, 150.0, 30.0, 4))                                             # its last segment lies beyond the page's right edge
    assert out["out_segs"][2]["box"] == out["bbox"][:2] + (0, 0) and out["out_segs"][0]["box"][2] > 0


def test_check_curves_refusals_name_the_region():
    ok = [curves.box_polygon([2, 3, 60, 20], (30,)), [(70.0, 25.5), (79.0, 23.0), (88.0, 24.0), (89.5, 38.0), (80.0, 36.5), (71.0, 39.0)]]

    def refused(match, polys=ok, restored=(True, True), scale=2, feather=3):
        with pytest.raises(ValueError, match=match):
            curves.check_curves(40, 90, polys, list(restored), scale, feather)

    recs = curves.check_curves(40, 90, ok, [True, True], 2, 3)
    assert recs[0]["bbox"] == (4, 6, 116, 34) and (recs[0]["rw"], recs[0]["rh"]) == (116, 34) and recs[0]["out_polygon"][3] == (120, 40)
    refused("region 1: an even number of points", [ok[0], ok[1][:5]])
    refused("region 1: an even number of points", [ok[0], [(1, 2), (3, 4)]])
    refused("region 1: an even number of points", [ok[0], curves.box_polygon([2, 21, 80, 38], range(3, 35))])             # 68 points
    refused("region 1: an even number of points", [ok[0], [1, 2, 3, 4]])
    curves.check_curves(40, 90, [curves.box_polygon([2, 21, 80, 38], range(3, 34))], [True], 2, 3)                       # 66 points: 32 segments
    refused("region 1: its points must be finite", [ok[0], ok[1][:5] + [(71.0, float("nan"))]])
    refused("region 0: a point's coordinate lies beyond", [[(0, 0), (40000, 0), (40000, 10), (0, 10)], ok[1]])
    refused("region 1: segment 0 runs counter-clockwise \\(a mirrored chain\\)", [ok[0], ok[1][::-1]])
    refused("region 1: segment 1, .*not strictly convex", [ok[0], [(70, 25), (79, 25), (88, 25), (80, 30), (79, 39), (70, 39)]])   # a reflex corner
    refused("region 1: segment 0, .*not strictly convex", [ok[0], [(70, 25), (88, 39), (88, 25), (70, 39)]])             # self-intersecting
    refused("region 1: segments 0 and 9 intersect: the chain folds over itself", [ok[0], arc(75.0, 20.0, 6.0, 14.0, 200.0, -200.0, 12)])   # 400 degrees
    refused("region 1: .*misses the 90 x 40 page", [ok[0], curves.box_polygon([95, 5, 120, 20], (100,))])
    refused("region 1: .*misses the 90 x 40 page", [ok[0], curves.box_polygon([10, -30, 60, -2])], restored=(True, False))
    refused("region 1: .*6 rows", [ok[0], curves.box_polygon([70, 25, 90, 28], (80,))])
    curves.check_curves(40, 90, [ok[0], curves.box_polygon([70, 25, 90, 28])], [True, False], 2, 3)         # not restored: only its points are checked
    curves.check_curves(40, 90, [ok[0], curves.box_polygon([70, 25, 90, 29])], [True, True], 2, 3)          # 8 rows: accepted
    refused("regions 0 and 1 overlap", [ok[0], [(55, 10), (68, 7), (80, 5), (82, 18), (70, 21), (57, 25)]])
    curves.check_curves(40, 90, [ok[0], [(55, 10), (80, 5), (82, 18), (57, 25)]], [True, False], 2, 3)      # a region without a line may cover another
    curves.check_curves(40, 90, [ok[0], curves.box_polygon([60, 3, 90, 20], (75,))], [True, True], 2, 3)    # touching regions do not overlap
    curves.check_curves(40, 90, [ok[0], [(80, 20), (100, 25), (98, 45), (78, 38)]], [True, True], 2, 3)     # partly outside the page: allowed
    for name, poly in SHAPES.items():
        _region(poly)
    for scale in (0, 9, 1.5, -1):
        refused("scale", scale=scale)
    for feather in (-1, 1025, 0.5):
        refused("feather", feather=feather)
    refused("one line", restored=(True,))


def test_entry_point_refuses_before_anything_runs():
    """the host checks of restore_page_curves need neither weights on a device nor a launch"""
    from marconet_amd import networks
    from marconet_amd.pipeline import MarconetPipeline
    pipe = MarconetPipeline(networks.TextContextEncoderV2(), networks.TSPGAN(), networks.TSPSRNet())
    page = np.zeros((60, 200, 3), np.uint8)
    a = lq_io.alphabet()[10]
    p = curves.box_polygon([0, 0, 100, 30], (40,))
    with pytest.raises(ValueError, match="needs texts"):
        pipe.restore_page_curves(page, [p], None)
    with pytest.raises(ValueError, match="one text"):
        pipe.restore_page_curves(page, [p], [a, a])
    with pytest.raises(ValueError, match="restore_page_curves: regions 0 and 1 overlap"):
        pipe.restore_page_curves(page, [p, [(90, 10), (150, 5), (152, 40), (92, 45)]], [a, a])
    with pytest.raises(ValueError, match="restore_page_curves: region 1: .*mirrored"):
        pipe.restore_page_curves(page, [p, p[::-1]], [a, a])
    with pytest.raises(ValueError, match="restore_page_curves: region 0: an even number of points"):
        pipe.restore_page_curves(page, [p[:5]], [a])
    with pytest.raises(ValueError, match="restore_page_curves: region 0: .*4 rows"):
        pipe.restore_page_curves(page, [curves.box_polygon([0, 0, 100, 4], (50,))], [a], scale=1)
    with pytest.raises(ValueError, match="restore_page_curves: region 0: a character box"):
        pipe.restore_page_curves(page, [p], [a], char_boxes=[[[1, 2, 3]]])
    with pytest.raises(ValueError, match="scale"):
        pipe.restore_page_curves(page, [p], [a], scale=9)
    with pytest.raises(TypeError):
        pipe.restore_page_curves(page.astype(np.float32), [p], [a])


def test_char_boxes_in_crop():
    box = [10, 20, 70, 40]
    boxes = [[10, 20, 25, 40], [[25, 20], [41.5, 20], [41.5, 40], [25, 40]], [38, 0, 100, 50], [-5, 25, 12, 30]]
    want = quads.char_boxes_in_crop(boxes, quads.quad_map(quads.box_quad(box), 60, 20), 60, 20)
    assert want == [[0.0, 0, 15.0, 20], [15.0, 0, 31.5, 20], [28.0, 0, 60.0, 20], [0.0, 0, 2.0, 20]]
    for cuts in ((), (30,), (12, 25, 26, 50)):                                                               # on an integer box: quads', however it is cut
        r = _region(curves.box_polygon(box, cuts))
        assert curves.char_boxes_in_crop(boxes, r["segs"], 60, 20) == want, cuts
    r = _region(SHAPES["arc"])                                                                               # along the arc: a cell between two rungs
    (t1, t2), (b1, b2) = r["polygon"][1:3], r["polygon"][10:8:-1]
    got = curves.char_boxes_in_crop([[t1, t2, b2, b1], [10.0, 118.0, 12.0, 122.0], [208.0, 118.0, 210.0, 122.0]],
                                    r["segs"], r["cw"], r["ch"])
    assert abs(got[0][0] - 34.0) <= 1e-9 and abs(got[0][2] - 68.0) <= 1e-9 and got[0][1::2] == [0, 22]
    assert got[1] == [0.0, 0, 0.0, 22] and got[2] == [170.0, 0, 170.0, 22]                                   # beyond the first and the last rung, where no segment accepts a corner: the nearer end
    with pytest.raises(ValueError):
        curves.char_boxes_in_crop([[1, 2, 3]], r["segs"], 170, 22)


SEG_FIELDS = ("c", "u0", "w", "bx0", "by0", "bw", "bh")
CROP_FIELDS = ("offset", "w", "h", "c0", "seg0", "nseg", "reserved")
REGION_FIELDS = ("ax0", "ay0", "rw", "rh", "bx0", "by0", "bw", "bh", "feather", "seg0", "nseg", "reserved")
LAYOUTS = (("mnet_curve_seg", SEG_FIELDS, "CurveSeg"), ("mnet_curve_crop", CROP_FIELDS, "CurveCrop"), ("mnet_curve_region", REGION_FIELDS, "CurveRegion"))


def test_descriptor_layouts_match_c(tmp_path):
    """sizeof / offsetof of the three records from a C program compiled against the header == the ctypes mirrors and the tables' records"""
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "marconet_hip_curve.h"\nint main(void){\n'
    for name, fields, _ in LAYOUTS:
        code += 'printf("%%zu %%zu", sizeof(%s), _Alignof(%s));\n' % (name, name)
        code += "".join('printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f in fields) + 'printf("\\n");\n'
    code += "return 0; }\n"
    cpath, exe = str(tmp_path / "curve_probe.c"), str(tmp_path / "curve_probe")
    with open(cpath, "w") as f:
        f.write(code)
    subprocess.check_call(["gcc", "-std=c11", "-I", INCLUDE, cpath, "-o", exe])
    got = [[int(v) for v in l.split()] for l in subprocess.check_output([exe]).decode().strip().split("\n")]
    for row, (_, fields, mirror) in zip(got, LAYOUTS):
        S = getattr(_lib, mirror)
        assert row == [ctypes.sizeof(S), ctypes.alignment(S)] + [getattr(S, f).offset for f in fields]
        assert np.dtype(S).itemsize == row[0] and row[0] % 8 == 0
    assert got[0][:2] == [88, 8] and got[1][:2] == [32, 8] and got[2][:2] == [48, 4]
    a, b = _region(SHAPES["arc"], 2, 3), _region(curves.box_polygon([200, 150, 250, 170], (230,)), 2, 3)
    tab, segs, nbytes = curves.crop_table([a["segs"], a["segs"], b["segs"]], [(100, 22), (70, 22), (50, 20)], [0, 100, 0])
    assert nbytes == 3 * (100 * 22 + 70 * 22 + 50 * 20) and tab["offset"].tolist() == [0, 6600, 6600 + 4620] and tab["c0"].tolist() == [0, 100, 0]
    assert (tab["seg0"].tolist(), tab["nseg"].tolist(), len(segs)) == ([0, 0, 5], [5, 5, 2], 7)              # a region's segments are stored once
    assert segs["u0"].tolist() == [0, 34, 68, 102, 136, 0, 30] and segs["c"][5].tolist() == [200, 1, 0, 0, 150, 0, 1, 0] and not segs["bw"].any()
    reg, segs = curves.paste_table([a, b], 3, [(0, 0), (0, 44)])
    assert tuple(reg[1]) == (0, 44, 100, 40, 400, 300, 100, 40, 3, 5, 2, 0) and tuple(reg[0])[:4] == (0, 0, 340, 44) and tuple(reg[0])[8:] == (3, 0, 5, 0)
    assert segs["u0"].tolist() == [0, 68, 136, 204, 272, 0, 60] and tuple(segs[6])[1:] == (60, 40, 460, 300, 40, 40)
    assert segs["c"][6].tolist() == [460, 1, 0, 0, 300, 0, 1, 0]


def test_curve_header_compiles_as_c99(tmp_path):
    cpath = str(tmp_path / "probe.c")
    with open(cpath, "w") as f:
        f.write('#include "marconet_hip_curve.h"\nint main(void) {\n'
                'int (*c)(const uint8_t*, int32_t, int32_t, const mnet_curve_crop*, int32_t, const mnet_curve_seg*, int32_t, int32_t, int32_t, uint8_t*, int64_t, '
                'void*) = mnet_curve_crop_u8;\n'
                'int (*p)(const uint8_t*, int32_t, int32_t, const mnet_curve_region*, int32_t, const mnet_curve_seg*, int32_t, int32_t, int32_t, uint8_t*, int32_t, '
                'int32_t, void*) = mnet_curve_paste_u8;\n'
                '(void)c; (void)p; return MNET_ABI_VERSION == 4 && MNET_CURVE_MAX_SEGS == 32 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, cpath])
    assert set(_lib.CURVE_SYMBOLS) == {"mnet_curve_crop_u8", "mnet_curve_paste_u8"}
    others = set(_lib.SYMBOLS) | set(_lib.UPFOLD_SYMBOLS) | set(_lib.UPFOLD_F32Z_SYMBOLS) | set(_lib.QUAD_SYMBOLS) | set(_lib.COLUMN_SYMBOLS)
    assert not set(_lib.CURVE_SYMBOLS) & others and len(_lib.SYMBOLS) == 45 and _lib.ABI_VERSION == 4


def test_entry_points_validate_arguments_without_device():
    lib = _lib.load()
    ok = dict(page=16, page_h=70, page_w=150, crops=16, n=3, segs=32, n_segs=9, max_w=100, max_h=40, dst=16, dst_bytes=1 << 20)

    def crop(**kw):
        a = dict(ok, **kw)
        return lib.mnet_curve_crop_u8(a["page"], a["page_h"], a["page_w"], a["crops"], a["n"], a["segs"], a["n_segs"], a["max_w"], a["max_h"], a["dst"],
                                      a["dst_bytes"], None)

    for bad in ("page", "crops", "segs", "dst"):
        assert crop(**{bad: None}) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(page_h=0), dict(page_w=-3), dict(n=0), dict(n=-1), dict(n_segs=0), dict(n_segs=-2), dict(max_w=0), dict(max_h=0), dict(max_h=-2),
                dict(dst_bytes=0), dict(dst_bytes=-5)):
        assert crop(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    assert crop(n=1 << 20, max_w=1 << 20, max_h=1 << 20) == -1 and b"too large" in lib.mnet_last_error()
    assert crop(n=1, max_w=(1 << 31) - 1, max_h=(1 << 31) - 1) == -1 and b"too large" in lib.mnet_last_error()
    for bad in (dict(crops=20), dict(crops=17), dict(segs=36), dict(segs=33)):
        assert crop(**bad) == -2 and b"aligned" in lib.mnet_last_error()

    okp = dict(atlas=16, atlas_h=64, atlas_w=300, regions=16, n=2, segs=32, n_segs=9, max_bw=200, max_bh=90, page=16, page_h=280, page_w=600)

    def paste(**kw):
        a = dict(okp, **kw)
        return lib.mnet_curve_paste_u8(a["atlas"], a["atlas_h"], a["atlas_w"], a["regions"], a["n"], a["segs"], a["n_segs"], a["max_bw"], a["max_bh"], a["page"],
                                       a["page_h"], a["page_w"], None)

    for bad in ("atlas", "regions", "segs", "page"):
        assert paste(**{bad: None}) == -1 and b"null" in lib.mnet_last_error()
    for bad in (dict(atlas_h=0), dict(atlas_w=-1), dict(n=0), dict(n=-4), dict(n_segs=0), dict(max_bw=0), dict(max_bh=-1), dict(page_h=0), dict(page_w=0)):
        assert paste(**bad) == -1 and b"bad shape" in lib.mnet_last_error()
    assert paste(n=1 << 20, max_bw=1 << 20, max_bh=1 << 20) == -1 and b"too large" in lib.mnet_last_error()
    for bad in (dict(regions=20), dict(regions=17), dict(segs=36)):
        assert paste(**bad) == -2 and b"aligned" in lib.mnet_last_error()


def test_ops_and_drivers_refuse_cpu_tensors_and_bad_tables():
    from marconet_amd import ops
    page = torch.zeros((80, 180, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.curve_crop_u8(page, torch.zeros((1, 32), dtype=torch.uint8), torch.zeros((1, 88), dtype=torch.uint8), 10, 10, torch.zeros((300,), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.curve_paste_u8(page, torch.zeros((1, 48), dtype=torch.uint8), torch.zeros((1, 88), dtype=torch.uint8), 10, 10, page.clone())
    assert "curve_crop_u8" in ops.__all__ and "curve_paste_u8" in ops.__all__
    lines = torch.zeros((2, 128, 300, 3), dtype=torch.uint8)
    ps = [curves.box_polygon([0, 0, 90, 40], (30,)), curves.box_polygon([80, 30, 100, 50], (90,))]
    with pytest.raises(ValueError, match="regions 0 and 1 overlap"):                          # found before any copy or launch
        curves.compose_page_curves(page.numpy(), lines, [300, 200], ps, 1, 3)
    with pytest.raises(ValueError, match="one joined line per region"):
        curves.compose_page_curves(page, lines, [300], ps[:1], 2, 3)
    with pytest.raises(ValueError, match="line width 301"):
        curves.compose_page_curves(page.numpy(), lines, [301, 200], [ps[0], curves.box_polygon([90, 40, 100, 50])], 1, 3)


# ----------------------------------------------------------------------------------------------------------------------- the build
def test_build_script_compiles_and_stamps_the_kernels():
    sh = open(os.path.join(CSRC, "build.sh")).read()
    assert re.search(r'^SRCS="[^"]*\bcurve_kernels\b[^"]*"', sh, flags=re.M)
    assert 'curve_kernels) echo "-ffp-contract=off" ;;' in sh
    assert ('[ "$1" = curve_kernels ] && cat "$HERE/curve_map.h" "$HERE/quad_map.h" "$HERE/lq_taps.h" "$HERE/page_blend.h" "$HERE/page_tile.h" '
            '"$HERE/../../include/marconet_hip_curve.h"') in sh
    src = open(os.path.join(CSRC, "curve_kernels.hip")).read()
    assert '#include "curve_map.h"' in src and '#include "page_blend.h"' in src and '#include "page_tile.h"' in src and "marconet_hip_curve.h" in src
    assert "asm" not in src
    assert '#include "quad_map.h"' in open(os.path.join(CSRC, "curve_map.h")).read()
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in _lib.CURVE_SYMBOLS)


# ----------------------------------------------------------------------------------------------------------------------- the example
def test_example_script_reads_polygon_regions_and_refuses_them_beside_a_column(tmp_path):
    """examples/restore_page.py's region file: a "polygon" anywhere sends every region through restore_page_curves, boxes and quadrilaterals as their
    four points; beside a "vertical" region, or malformed, the script exits with a message before it looks for a GPU"""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("restore_page_example_curves", os.path.join(ROOT, "examples", "restore_page.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = str(tmp_path / "regions.json")

    def load(regions):
        with open(path, "w", encoding="utf8") as f:
            json.dump(regions, f)
        return mod.load_regions(path)

    line, quad = dict(box=[40, 5, 90, 25], text="cd"), dict(quad=[[40, 40], [90, 42], [89, 60], [39, 58]], text="ef")
    poly = dict(polygon=[[10, 70], [40, 64], [70, 70], [68, 88], [40, 82], [12, 88]], text="gh")
    got = load([line, quad, poly])
    assert len(got) == 6 and got[4] is None
    assert got[5] == [[[40, 5], [90, 5], [90, 25], [40, 25]], quad["quad"], poly["polygon"]]
    assert load([line, quad])[5] is None and load([line])[5] is None and load([line])[3] is None                # no polygon: as before
    with pytest.raises(SystemExit, match='holds a "vertical" region \\(1\\) and a "polygon" region \\(0\\)'):
        load([poly, dict(box=[5, 5, 30, 60], text="ab", vertical=True)])
    for bad in (dict(poly, box=[1, 2, 3, 4]), dict(polygon=[[1, 2], [3, 4], [5, 6]], text="a"), dict(polygon=[[1, 2], [3, 4], [5, 6], [7]], text="a"),
                dict(poly, vertical=True)):
        with pytest.raises(SystemExit, match="must hold a list"):
            load([bad])
