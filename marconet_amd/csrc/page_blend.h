// The two integer steps around the cubic of the page paste, as marconet_amd/pages.py states them (box_reduce, feather_blend) — on the host and on
// the device, so that a CPU test can compile this header alone and compare every byte with the Python statement (tests/test_pages.py).
//
// Box average: cnt = k x c source bytes (k in {1, 2, 4, 8}, 1 <= c <= k: cnt <= 64) → their mean rounded half up, (2 sum + cnt) / (2 cnt); the
// numerator is at most 2 * 64 * 255 + 64.  cnt = 1 gives the byte itself.
// Feather: at local (u, v) of an RW x RH rectangle the weight of the restored line is (a / 2F) (b / 2F) with a = min(2 min(u, RW - 1 - u) + 1, 2F)
// and b the same on (v, RH): a ramp sampled at pixel centres, <= 1 / (2F) at the edge and exactly 1 from F pixels inside, symmetric on both axes.
// out = (bg (D - m) + fg m + D / 2) / D with m = a b <= D = 4 F^2, rounded half up; the weights are non-negative and sum to D, so the result lies in
// [min(bg, fg), max(bg, fg)].  Unsigned 32-bit arithmetic: the numerator is at most 255 D + D / 2 < 2^31 at F = PAGE_MAX_FEATHER (D = 2^22).  F = 0: no
// feather, the pixel is the line's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PAGE_HD __host__ __device__
#else
#define PAGE_HD
#endif

#define PAGE_MAX_FEATHER 1024
#define PAGE_MAX_K 8

// sum of cnt bytes, 1 <= cnt <= PAGE_MAX_K * PAGE_MAX_K
PAGE_HD inline uint32_t page_box_avg(uint32_t sum, uint32_t cnt) {
    return (2u * sum + cnt) / (2u * cnt);
}

// one axis of the weight: coordinate 0 <= u < n, 1 <= F <= PAGE_MAX_FEATHER → 1 .. 2F
PAGE_HD inline uint32_t page_feather_axis(uint32_t u, uint32_t n, uint32_t F) {
    const uint32_t e = u < n - 1u - u ? u : n - 1u - u, a = 2u * e + 1u;
    return a < 2u * F ? a : 2u * F;
}

// bg, fg: bytes; a, b: page_feather_axis of the two axes; 1 <= F <= PAGE_MAX_FEATHER
PAGE_HD inline uint32_t page_feather(uint32_t bg, uint32_t fg, uint32_t a, uint32_t b, uint32_t F) {
    const uint32_t D = 4u * F * F, m = a * b;
    return (bg * (D - m) + fg * m + D / 2u) / D;
}
