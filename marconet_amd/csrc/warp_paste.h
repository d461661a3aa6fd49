// The paste of ONE page pixel of a quadrilateral region and of a curved region, and the lists a region's descriptor must pass to be followed — on the
// host and on the device, stated once for the per-descriptor kernels (quad_kernels.hip, curve_kernels.hip: the destination is the page's pixel in
// memory) and for the page-tile compositor (mixed_kernels.hip: the destination is the pixel in registers).  A CPU test compiles this header alone
// (tests/test_regions.py).  The arithmetic is quad_map.h's, curve_map.h's and page_blend.h's, unchanged; every translation unit that includes this
// header is compiled with -ffp-contract=off (build.sh).
// Bounds: with a followed region (the lists below) every foreground index is clamped into [0, rw) x [0, rh), which lies inside the atlas, and the
// feather's pixel lies inside that rectangle too; d is the caller's, one pixel of three bytes, read and written by the calling thread only.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/marconet_hip_quad.h"
#include "../../include/marconet_hip_curve.h"
#include "curve_map.h"
#include "page_blend.h"

QUAD_HD inline bool quad_finite9(const double* m) {
    bool ok = true;
    for (int k = 0; k < 9; ++k) ok = ok && isfinite(m[k]);
    return ok;
}

// what mnet_quad_paste_u8 and mnet_curve_paste_u8 ask of the fields the two region records share (include/marconet_hip_quad.h)
QUAD_HD inline bool warp_rects_followed(int ax0, int ay0, int rw, int rh, int bx0, int by0, int bw, int bh, int feather, int atlas_h, int atlas_w,
                                        int page_h, int page_w) {
    return rw >= 1 && rh >= 1 && bw >= 1 && bh >= 1 && ax0 >= 0 && ay0 >= 0 && bx0 >= 0 && by0 >= 0 && (long long)ax0 + rw <= atlas_w &&
           (long long)ay0 + rh <= atlas_h && (long long)bx0 + bw <= page_w && (long long)by0 + bh <= page_h && feather >= 0 &&
           feather <= PAGE_MAX_FEATHER;
}

QUAD_HD inline bool quad_region_followed(const mnet_quad_region& R, int atlas_h, int atlas_w, int page_h, int page_w) {
    return warp_rects_followed(R.ax0, R.ay0, R.rw, R.rh, R.bx0, R.by0, R.bw, R.bh, R.feather, atlas_h, atlas_w, page_h, page_w) && quad_finite9(R.n);
}

// the region's own fields; its segments are checked where they are staged (curve_stage, curve_seg_in_region)
QUAD_HD inline bool curve_region_followed(const mnet_curve_region& R, int atlas_h, int atlas_w, int page_h, int page_w, int n_segs) {
    return warp_rects_followed(R.ax0, R.ay0, R.rw, R.rh, R.bx0, R.by0, R.bw, R.bh, R.feather, atlas_h, atlas_w, page_h, page_w) && R.seg0 >= 0 &&
           R.nseg >= 1 && R.nseg <= CURVE_MAX_SEGS && (long long)R.seg0 + R.nseg <= n_segs;
}

// the sample at (x0 | x1, q.y0 | q.y1) with the weights (ax, q.ay) of the foreground whose first pixel is fg0 → the pixel d, under the feather
// weights of foreground pixel (fu, fv) in rw x rh
QUAD_HD inline void warp_blend(const uint8_t* fg0, size_t row_bytes, int x0, int x1, int ax, const QuadTaps& q, unsigned fu, unsigned fv, int rw, int rh,
                               unsigned F, uint8_t* d) {
    const uint8_t* r0 = fg0 + (size_t)q.y0 * row_bytes;
    const uint8_t* r1 = fg0 + (size_t)q.y1 * row_bytes;
    unsigned fa = 0u, fb = 0u;
    if (F) {
        fa = page_feather_axis(fu, (unsigned)rw, F);
        fb = page_feather_axis(fv, (unsigned)rh, F);
    }
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned fg = (unsigned)quad_mix(r0[(size_t)x0 * 3 + ch], r0[(size_t)x1 * 3 + ch], r1[(size_t)x0 * 3 + ch], r1[(size_t)x1 * 3 + ch], ax, q.ay);
        d[ch] = (uint8_t)(F ? page_feather(d[ch], fg, fa, fb, F) : fg);
    }
}

// The page pixel whose centre is (x, y) under the region's map n (page pixel → foreground coordinates) → whether the region claims it; a claimed
// pixel is blended into d.  fg0: the foreground's first pixel in the atlas, rows row_bytes apart.
QUAD_HD inline bool quad_paste_pixel(const double* n, int rw, int rh, unsigned F, const uint8_t* fg0, size_t row_bytes, double x, double y, uint8_t* d) {
    const QuadPos p = quad_pos(n, x, y);
    if (!(p.valid && p.u >= 0.0 && p.u < (double)rw && p.v >= 0.0 && p.v < (double)rh)) return false;
    const QuadTaps q = quad_taps(quad_fix(p.u), quad_fix(p.v), rw, rh);
    warp_blend(fg0, row_bytes, q.x0, q.x1, q.ax, q, (unsigned)(int)floor(p.u), (unsigned)(int)floor(p.v), rw, rh, F, d);
    return true;
}

struct CurveSegL {           // a segment as the paste and the crop keep it (in LDS on the device)
    double c[8];
    CurvePrep s;
    int u0, w, bx0, by0, bw, bh;
};

// Segment seg0 + t of `segs` → S[t], and whether it can be followed as far as this one record and its predecessor show: finite coefficients,
// w >= 1, and its first column is where its predecessor's ends (0 for the first).  The caller has checked 0 <= seg0, seg0 + nseg <= n_segs, t < nseg.
QUAD_HD inline bool curve_stage(CurveSegL* S, const mnet_curve_seg* segs, int seg0, int t, mnet_curve_seg& g) {
    g = segs[(size_t)seg0 + t];
    long long due = 0;
    if (t > 0) {
        const mnet_curve_seg* p = segs + ((size_t)seg0 + t - 1);
        due = (long long)p->u0 + p->w;
    }
    for (int k = 0; k < 8; ++k) S[t].c[k] = g.c[k];
    S[t].s = curve_prep(g.c);
    S[t].u0 = g.u0; S[t].w = g.w;
    S[t].bx0 = g.bx0; S[t].by0 = g.by0; S[t].bw = g.bw; S[t].bh = g.bh;
    return curve_finite8(g.c) && g.w >= 1 && (long long)g.u0 == due;
}

// a paste segment's box has bw, bh >= 0 and lies inside its region's
QUAD_HD inline bool curve_seg_in_region(const mnet_curve_seg& g, const mnet_curve_region& R) {
    return g.bw >= 0 && g.bh >= 0 && g.bx0 >= R.bx0 && g.by0 >= R.by0 && (long long)g.bx0 + g.bw <= (long long)R.bx0 + R.bw &&
           (long long)g.by0 + g.bh <= (long long)R.by0 + R.bh;
}

// a segment's box shares a pixel with [tx0, tx0 + tw) x [ty0, ty0 + th)
QUAD_HD inline bool curve_seg_hits(const mnet_curve_seg& g, long long tx0, long long ty0, int tw, int th) {
    return g.bw > 0 && g.bh > 0 && g.bx0 < tx0 + tw && (long long)g.bx0 + g.bw > tx0 && g.by0 < ty0 + th && (long long)g.by0 + g.bh > ty0;
}

// Page pixel (X, Y), centre (x, y), against the staged segments S[0 .. nseg) of a region whose foreground is rw x rh: the segments are tried in
// order, by the integer box before any fp64; the first claim wins and is blended into d → whether one claimed it.
QUAD_HD inline bool curve_paste_pixel(const CurveSegL* S, int nseg, int rw, int rh, unsigned F, const uint8_t* fg0, size_t row_bytes, int X, int Y, double x,
                                      double y, uint8_t* d) {
#pragma unroll 1
    for (int k = 0; k < nseg; ++k) {
        const CurveSegL& s = S[k];
        if (X < s.bx0 || X - s.bx0 >= s.bw || Y < s.by0 || Y - s.by0 >= s.bh) continue;      // the integer box, before any fp64
        const CurveInv p = curve_inv(s.c, s.s, x, y);
        if (!(p.valid && p.u >= 0.0 && p.u < (double)s.w && p.v >= 0.0 && p.v < (double)rh)) continue;
        int x0, x1, ax;
        curve_taps_x(quad_fix(p.u), s.u0, rw, &x0, &x1, &ax);
        const QuadTaps q = quad_taps(0, quad_fix(p.v), rw, rh);
        warp_blend(fg0, row_bytes, x0, x1, ax, q, (unsigned)(s.u0 + (int)floor(p.u)), (unsigned)(int)floor(p.v), rw, rh, F, d);
        return true;                                                                          // the first claim wins
    }
    return false;
}
