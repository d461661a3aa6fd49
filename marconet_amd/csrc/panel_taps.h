// One destination column of the two-tap INTER_LINEAR resize as marconet_amd/lq_io.py::resize_linear states it (its inner `taps`: centre-aligned
// sampling in fp64, the fraction rounded once to fp32, positions outside the row clamped to the border sample with a zero fraction) — on the host
// and on the device, so that a CPU test can compile this header alone and compare every tap with the numpy statement (tests/test_panel_device.py).
//
// Every operation is rounded separately, as numpy rounds it.  As for lq_taps.h, the _rn intrinsics do not guarantee that (they are plain operators
// that -ffp-contract=fast fuses), so every translation unit that includes this header is compiled with -ffp-contract=off: build.sh does it for
// panel_kernels.hip, and tests/test_panel_device.py checks the gfx950 ISA of that build and builds its own host program the same way.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PANEL_HD __host__ __device__
#else
#define PANEL_HD
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define PANEL_DMUL(a, b) __dmul_rn((a), (b))
#define PANEL_DADD(a, b) __dadd_rn((a), (b))
#else
#define PANEL_DMUL(a, b) ((double)(a) * (double)(b))
#define PANEL_DADD(a, b) ((double)(a) + (double)(b))
#endif

struct PanelTap {
    int i0, i1;      // the two source columns, both in [0, n_src)
    float t;         // weight of i1; i0 weighs 1 - t (the caller's one fp32 subtraction)
};

// destination column x of a row with n_src >= 1 source samples; step = n_src / n_dst as the caller's double
PANEL_HD inline PanelTap panel_linear_tap(int x, int n_src, double step) {
    const double f = PANEL_DADD(PANEL_DMUL(PANEL_DADD((double)x, 0.5), step), -0.5);
    const double fl = floor(f);
    PanelTap p;
    p.t = (float)PANEL_DADD(f, -fl);                               // f - floor(f) is exact in fp64; ONE rounding, to fp32
    // floor(f) lies in [-1, n_src) for every column of the row; the clamp only keeps the conversion defined for a column beyond it (the padding
    // columns of a tile) or a step that is not a number
    int i0 = (int)fmin(fmax(fl, -4.0), (double)n_src + 4.0);
    if (i0 < 0) { p.t = 0.0f; i0 = 0; }
    if (i0 >= n_src - 1) { p.t = 0.0f; i0 = n_src - 1; }
    p.i0 = i0;
    p.i1 = i0 + 1 < n_src - 1 ? i0 + 1 : n_src - 1;
    return p;
}
