// The per-pixel arithmetic of the curved page path, as marconet_amd/curves.py states it (curve_pos, curve_inv) — on the host and on the device, so
// that a CPU test can compile this header alone and compare every value with the numpy statement (tests/test_curves.py).
//
// A curved region is a chain of segments; a segment is a bilinear patch, eight doubles computed ONCE per region on the host
// (curves.segment_coeffs): c = Ax, Ex, Fx, Gx, Ay, Ey, Fy, Gy, and the point (u, v) of the segment's w x h rectangle lies at A + E u + F v + G u v
// (1 / w and 1 / h are folded into E, F and G).  Bilinear, not projective: neighbouring patches agree along the whole of their shared rung.
// Forward (the crop): X = ((Ex u + Fx v) + (Gx u) v) + Ax, Y likewise; valid iff both are finite.  With G = 0 (a parallelogram) this is bit for
// bit quad_map.h's quad_pos of an affine map.
// Inverse (the paste): with q = p - A and cross(a, b) = ax by - ay bx,
//     a2 = cross(F, G),  a1 = cross(F, E) - cross(q, G),  a0 = -cross(q, E),  disc = a1 a1 - (4 a2) a0,  r = sqrt(disc)
// and the wanted root of a2 v^2 + a1 v + a0 is ALWAYS (-a1 - r) / (2 a2), taken without cancellation: v = a0 / (0.5 (r - a1)) where a1 <= 0, and
// v = (-0.5 (a1 + r)) / a2 where a1 > 0.  (a1 changes sign inside strongly tapered convex segments: the textbook rule that picks the root by a1's
// sign alone leaves up to a third of such a segment unpasted.)  Then d = E + v G and u = (qx - v Fx) / dx where |dx| >= |dy|, else
// (qy - v Fy) / dy.  Valid iff disc >= 0 and u, v are finite.  a2 and cross(F, E) depend on the segment alone: curve_prep computes them, with
// the same operations, wherever the segment is loaded.
// Every fp64 operation is rounded separately (lq_taps.h's LQ_D* macros; the translation unit is compiled with -ffp-contract=off and without
// fast-math); the divisions and the square root are the IEEE correctly rounded ones (curve_sqrt: the one place to correct a library whose
// square root were not).  Sampling is quad_map.h's, unchanged: quad_fix, quad_taps, quad_mix.
#pragma once
#include <math.h>
#include <stdint.h>
#include "quad_map.h"

#define CURVE_MAX_SEGS 32

struct CurvePos {
    double x, y;     // the page position (unspecified where valid == 0)
    int valid;       // both finite
};

struct CurveInv {
    double u, v;     // the position in the segment's rectangle (unspecified where valid == 0)
    int valid;       // disc >= 0 and u, v finite
};

struct CurvePrep {
    double a2, cfe;  // cross(F, G), cross(F, E)
};

#define CURVE_DSUB(a, b) LQ_DADD((a), -(b))

QUAD_HD inline double curve_cross(double ax, double ay, double bx, double by) {
    return CURVE_DSUB(LQ_DMUL(ax, by), LQ_DMUL(ay, bx));
}

QUAD_HD inline double curve_sqrt(double d) {
    return sqrt(d);
}

QUAD_HD inline bool curve_finite8(const double* c) {
    bool ok = true;
    for (int k = 0; k < 8; ++k) ok = ok && isfinite(c[k]);
    return ok;
}

QUAD_HD inline CurvePos curve_pos(const double* c, double u, double v) {
    CurvePos p;
    p.x = LQ_DADD(LQ_DADD(LQ_DADD(LQ_DMUL(c[1], u), LQ_DMUL(c[2], v)), LQ_DMUL(LQ_DMUL(c[3], u), v)), c[0]);
    p.y = LQ_DADD(LQ_DADD(LQ_DADD(LQ_DMUL(c[5], u), LQ_DMUL(c[6], v)), LQ_DMUL(LQ_DMUL(c[7], u), v)), c[4]);
    p.valid = (isfinite(p.x) && isfinite(p.y)) ? 1 : 0;
    return p;
}

QUAD_HD inline CurvePrep curve_prep(const double* c) {
    CurvePrep s;
    s.a2 = curve_cross(c[2], c[6], c[3], c[7]);
    s.cfe = curve_cross(c[2], c[6], c[1], c[5]);
    return s;
}

QUAD_HD inline CurveInv curve_inv(const double* c, CurvePrep s, double x, double y) {
    const double qx = CURVE_DSUB(x, c[0]), qy = CURVE_DSUB(y, c[4]);
    const double a1 = CURVE_DSUB(s.cfe, curve_cross(qx, qy, c[3], c[7]));
    const double a0 = -curve_cross(qx, qy, c[1], c[5]);
    const double disc = CURVE_DSUB(LQ_DMUL(a1, a1), LQ_DMUL(LQ_DMUL(4.0, s.a2), a0));
    const double r = curve_sqrt(disc);
    const double v = a1 <= 0.0 ? a0 / LQ_DMUL(0.5, CURVE_DSUB(r, a1)) : LQ_DMUL(-0.5, LQ_DADD(a1, r)) / s.a2;
    const double dx = LQ_DADD(c[1], LQ_DMUL(v, c[3])), dy = LQ_DADD(c[5], LQ_DMUL(v, c[7]));
    const double u = fabs(dx) >= fabs(dy) ? CURVE_DSUB(qx, LQ_DMUL(v, c[2])) / dx : CURVE_DSUB(qy, LQ_DMUL(v, c[6])) / dy;
    CurveInv p;
    p.valid = (disc >= 0.0 && isfinite(u) && isfinite(v)) ? 1 : 0;
    p.u = u;
    p.v = v;
    return p;
}

// The horizontal taps of the paste: the segment-local position qu = quad_fix(u) moved by the segment's first column u0 of a foreground rw wide —
// quad_taps' x half at qu + 64 u0, without forming that sum (which need not fit 32 bits); the neighbours are clamped into the WHOLE foreground,
// so the interpolation runs across seams.
QUAD_HD inline void curve_taps_x(int qu, int u0, int rw, int* x0, int* x1, int* ax) {
    const long long ix = (long long)(qu >> 6) + u0;
    *ax = qu & 63;
    *x0 = (int)(ix < 0 ? 0 : (ix > rw - 1 ? rw - 1 : ix));
    *x1 = (int)(ix + 1 < 0 ? 0 : (ix + 1 > rw - 1 ? rw - 1 : ix + 1));
}
