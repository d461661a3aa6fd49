// The per-pixel arithmetic of the quadrilateral page path, as marconet_amd/quads.py states it (quad_pos, quad_fix, quad_bilinear) — on the host and
// on the device, so that a CPU test can compile this header alone and compare every value with the numpy statement (tests/test_quads.py).
//
// Position: a 3x3 projective map M (nine doubles, row-major, computed ONCE per region on the host: quads.quad_map / quads.inverse_map) takes a
// pixel centre (x, y) to X = (M0 x + M1 y) + M2, Y = (M3 x + M4 y) + M5, D = (M6 x + M7 y) + M8 and (u, v) = (X / D, Y / D).  Every fp64
// operation is rounded separately, and the division is the IEEE-rounded one: the translation unit that includes this header is compiled with
// -ffp-contract=off and without fast-math, for lq_taps.h's reason (its LQ_D* macros are used here).  The position is valid iff D > 0 and X, Y, D
// are finite; an invalid position is never sampled.  So the sign of a map's scale is part of it: quads.quad_map has D = 1 at the crop's origin
// and D > 0 over the crop, quads.inverse_map is the true inverse (adjugate / determinant), whose D is the reciprocal of the forward map's and
// hence positive over the whole quadrilateral, wherever its vanishing line runs.
// Sample: quad_fix turns a coordinate into 1/64 pixel, floor((t - 0.5) 64 + 0.5), clamped in double to +-2^30 before the conversion (so that
// any double converts, and index + 1 cannot overflow); quad_bilinear splits it into the pixel index q >> 6 and the weight q & 63, clamps the
// four neighbours into the source (BORDER_REPLICATE) and mixes them in integers: at most 255 * 64 * 64 + 2048 < 2^21.  A position on a pixel
// centre has both weights 0 and gives that pixel's byte.
#pragma once
#include <math.h>
#include <stdint.h>
#include "lq_taps.h"

#define QUAD_HD LQ_HD
#define QUAD_FIX_LIMIT 1073741824.0      /* 2^30 */

struct QuadPos {
    double u, v;     // X / D, Y / D (unspecified where valid == 0)
    int valid;       // D > 0 and X, Y, D finite
};

struct QuadTaps {
    int x0, x1, y0, y1;      // the four neighbours' indices, clamped into [0, w) x [0, h)
    int ax, ay;              // the weights of x1 and y1 in 1/64
};

QUAD_HD inline QuadPos quad_pos(const double* M, double x, double y) {
    const double X = LQ_DADD(LQ_DADD(LQ_DMUL(M[0], x), LQ_DMUL(M[1], y)), M[2]);
    const double Y = LQ_DADD(LQ_DADD(LQ_DMUL(M[3], x), LQ_DMUL(M[4], y)), M[5]);
    const double D = LQ_DADD(LQ_DADD(LQ_DMUL(M[6], x), LQ_DMUL(M[7], y)), M[8]);
    QuadPos p;
    p.valid = (D > 0.0 && isfinite(X) && isfinite(Y) && isfinite(D)) ? 1 : 0;
    p.u = p.valid ? X / D : 0.0;
    p.v = p.valid ? Y / D : 0.0;
    return p;
}

// a coordinate (pixel i has its centre at i + 0.5) → the sample position in 1/64 pixel, |result| <= 2^30; t must not be a NaN
QUAD_HD inline int quad_fix(double t) {
    const double q = floor(LQ_DADD(LQ_DMUL(LQ_DADD(t, -0.5), 64.0), 0.5));
    return (int)fmin(fmax(q, -QUAD_FIX_LIMIT), QUAD_FIX_LIMIT);
}

QUAD_HD inline int quad_clampi(int i, int n) {
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// qx, qy: quad_fix of the two coordinates; w, h >= 1: the source's size
QUAD_HD inline QuadTaps quad_taps(int qx, int qy, int w, int h) {
    QuadTaps t;
    const int ix = qx >> 6, iy = qy >> 6;        // arithmetic shifts: floor for a negative position
    t.ax = qx & 63;
    t.ay = qy & 63;
    t.x0 = quad_clampi(ix, w);
    t.x1 = quad_clampi(ix + 1, w);
    t.y0 = quad_clampi(iy, h);
    t.y1 = quad_clampi(iy + 1, h);
    return t;
}

// the four neighbours' bytes (p00 at (x0, y0), p01 at (x1, y0), p10 at (x0, y1), p11 at (x1, y1)) → the sample's byte
QUAD_HD inline int quad_mix(int p00, int p01, int p10, int p11, int ax, int ay) {
    return ((p00 * (64 - ax) + p01 * ax) * (64 - ay) + (p10 * (64 - ax) + p11 * ax) * ay + 2048) >> 12;
}

// one channel of a uint8 image of w x h pixels, `row_bytes` from one row to the next and `pix_bytes` from one pixel to the next, at (qx, qy)
QUAD_HD inline int quad_bilinear(const uint8_t* src, size_t row_bytes, size_t pix_bytes, int w, int h, int qx, int qy) {
    const QuadTaps t = quad_taps(qx, qy, w, h);
    const uint8_t* r0 = src + (size_t)t.y0 * row_bytes;
    const uint8_t* r1 = src + (size_t)t.y1 * row_bytes;
    return quad_mix(r0[(size_t)t.x0 * pix_bytes], r0[(size_t)t.x1 * pix_bytes], r1[(size_t)t.x0 * pix_bytes], r1[(size_t)t.x1 * pix_bytes], t.ax, t.ay);
}
