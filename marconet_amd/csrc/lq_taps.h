// One axis of the 8-bit INTER_CUBIC resize as marconet_amd/lq_io.py::_cubic_taps states it (OpenCV's table for an 8-bit image: A = -0.75,
// centre-aligned sampling, 11-bit fixed-point taps, BORDER_REPLICATE) — for ONE destination coordinate, on the host and on the device, so that
// a CPU test can compile this header alone and compare every tap with the numpy statement (tests/test_lq_device.py).
//
// Every fp32 / fp64 operation is rounded separately: a fused multiply-add changes taps (for sample positions whose products are not exact; at
// dst_h = 32 / 128 they happen to be exact).  The _rn intrinsics do NOT guarantee that — in this ROCm's headers they are plain `x * y` / `x + y`,
// which hipcc's default -ffp-contract=fast fuses, and a `#pragma clang fp contract(off)` in this function's body did not stop it (seen in the
// ISA) — so every translation unit that includes this header is compiled with -ffp-contract=off: build.sh does it for lq_kernels.hip, and
// tests/test_lq_device.py checks the gfx950 ISA of that build for fused operations and builds its own host program the same way.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LQ_HD __host__ __device__
#else
#define LQ_HD
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define LQ_FMUL(a, b) __fmul_rn((a), (b))
#define LQ_FADD(a, b) __fadd_rn((a), (b))
#define LQ_FSUB(a, b) __fsub_rn((a), (b))
#define LQ_DMUL(a, b) __dmul_rn((a), (b))
#define LQ_DADD(a, b) __dadd_rn((a), (b))
#else
#define LQ_FMUL(a, b) ((float)(a) * (float)(b))
#define LQ_FADD(a, b) ((float)(a) + (float)(b))
#define LQ_FSUB(a, b) ((float)(a) - (float)(b))
#define LQ_DMUL(a, b) ((double)(a) * (double)(b))
#define LQ_DADD(a, b) ((double)(a) + (double)(b))
#endif

struct LqTaps {
    int idx[4];      // source indices of the 4 taps, clamped into [0, n_src)
    int tap[4];      // the taps: rint(weight * 2048) saturated to int16; their sum of magnitudes is at most 2816 (x = 0.5)
};

// destination coordinate d of an axis with n_src source samples; scale = 1.0 / (n_dst / n_src) as the caller's double
LQ_HD inline LqTaps lq_cubic_taps(int d, int n_src, double scale) {
    const double f = LQ_DADD(LQ_DMUL(LQ_DADD((double)d, 0.5), scale), -0.5);
    const double fl = floor(f);
    const float x = (float)LQ_DADD(f, -fl);                        // f - floor(f) is exact in fp64; ONE rounding, to fp32
    const float A = -0.75f, x1 = LQ_FADD(x, 1.0f), u = LQ_FSUB(1.0f, x);
    // c0 = ((A (x+1) - 5A) (x+1) + 8A) (x+1) - 4A ; c1 = ((A+2) x - (A+3)) x x + 1 ; c2 = c1 at 1 - x ; c3 = 1 - c0 - c1 - c2, left to right
    const float c0 = LQ_FSUB(LQ_FMUL(LQ_FADD(LQ_FMUL(LQ_FSUB(LQ_FMUL(A, x1), -3.75f), x1), -6.0f), x1), -3.0f);
    const float c1 = LQ_FADD(LQ_FMUL(LQ_FMUL(LQ_FSUB(LQ_FMUL(1.25f, x), 2.25f), x), x), 1.0f);
    const float c2 = LQ_FADD(LQ_FMUL(LQ_FMUL(LQ_FSUB(LQ_FMUL(1.25f, u), 2.25f), u), u), 1.0f);
    const float c3 = LQ_FSUB(LQ_FSUB(LQ_FSUB(1.0f, c0), c1), c2);
    const float c[4] = {c0, c1, c2, c3};
    // floor(f) lies in [-1, n_src) for every destination coordinate of the axis; the clamp only keeps the conversion defined for a
    // coordinate beyond it (the padding columns of a tile) or a scale that is not a number
    const int s = (int)fmin(fmax(fl, -4.0), (double)n_src + 4.0);
    LqTaps t;
    for (int k = 0; k < 4; ++k) {
        const float r = rintf(LQ_FMUL(c[k], 2048.0f));              // half to even
        t.tap[k] = (int)fminf(fmaxf(r, -32768.0f), 32767.0f);       // saturate_cast<short>
        const int i = s - 1 + k;
        t.idx[k] = i < 0 ? 0 : (i > n_src - 1 ? n_src - 1 : i);     // BORDER_REPLICATE
    }
    return t;
}
