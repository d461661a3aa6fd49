// The cross-fade of two restored windows of one long text line where they overlap, as marconet_amd/long_lines.py::stitch_host states it — on the
// host and on the device, so that a CPU test can compile this header alone and compare every byte with the Python statement
// (tests/test_long_lines.py).
//
// The overlap [A, B) of windows k and k + 1 has D = B - A >= 1 output columns; column A + t (0 <= t < D) samples the ramp at its centre
// (t + 1/2) / D:  a (1 - (2 t + 1) / (2 D)) + b (2 t + 1) / (2 D), rounded half up — all in integers.  The weights are positive and sum to 2 D, so
// the result lies in [min(a, b), max(a, b)], and (a, b, t) -> (b, a, D - 1 - t) gives the same byte: it does not matter which window is called the
// left one.  Unsigned 32-bit arithmetic: the numerator is at most 511 D, which fits for D <= STITCH_MAX_D (the entry point bounds sr_w by it).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define STITCH_HD __host__ __device__
#else
#define STITCH_HD
#endif

#define STITCH_MAX_D (1 << 22)

// a: the byte of window k, b: the byte of window k + 1, 0 <= t < D <= STITCH_MAX_D
STITCH_HD inline uint32_t stitch_blend(uint32_t a, uint32_t b, uint32_t t, uint32_t D) {
    return (a * (2u * D - 2u * t - 1u) + b * (2u * t + 1u) + D) / (2u * D);
}
