// What the three ink-profile kernels (ink_kernels.hip) state once: the integer luma Y, the row step of the two tiled kernels, the 64-bit check of
// a box that is a view of the page, and the host-side check of an entry point's arguments.  The definition of Y, d and e is marconet_amd/ink.py's.
#pragma once
#include "common.h"

// Y = (77 R + 150 G + 29 B + 128) >> 8 of the pixel at p
__device__ __forceinline__ int ink_luma(const unsigned char* p) { return (77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8; }

// One row of a tile whose threads own consecutive columns, thread by thread: e of the pair whose LEFT pixel is this thread's, at p.  The luma of
// the own pixel (`own`: it may be read), the right neighbour's from the next lane — or, where `loads_right` (the last lane of a wave, the last
// column of a rectangle), loaded by this lane itself —, d = |difference|, e = d where d >= floor, else 0; 0 without a pair.  p is dereferenced only
// where own, p + 3 only where loads_right && has_pair.  EVERY lane of the wave must call this: the neighbour's luma comes by a shuffle.
__device__ __forceinline__ int ink_pair_e(const unsigned char* p, bool own, bool has_pair, bool loads_right, int floor) {
    const int y0 = own ? ink_luma(p) : 0;
    int y1 = __shfl_down(y0, 1, 64);
    if (loads_right) y1 = has_pair ? ink_luma(p + 3) : 0;
    int e = 0;
    if (has_pair) {
        const int d = abs(y1 - y0);
        e = d >= floor ? d : 0;
    }
    return e;
}

// A box record b (mnet_ink_box, mnet_ink_box2): h x w pixels, rows `pitch` bytes apart, first byte at `offset`, lies inside [0, src_bytes) — its last
// byte, offset + (h - 1) pitch + 3 w, in 64 bits.  w < 2^23 (a row's sum stays below 2^31); BOUND_H: h too, for a kernel that sums along columns.
// (The record goes in whole: with its four fields as arguments hipcc arranged the box kernel's prologue otherwise, at 0.5 us a launch.)
template <bool BOUND_H, typename Box>
__device__ __forceinline__ bool ink_view_ok(const Box& b, long long src_bytes) {
    if (b.h < 1 || b.w < 1 || (BOUND_H && b.h >= (1 << 23)) || b.w >= (1 << 23) || b.offset < 0 || (long long)b.pitch < 3ll * b.w) return false;
    // offset <= src_bytes first: the sum below then stays far inside 64 bits (pitch, h < 2^31), as window_ok (window_kernels.hip) has it
    return b.offset <= src_bytes && (long long)(b.h - 1) * b.pitch + 3ll * b.w <= src_bytes - b.offset;
}

// Host: what the three entry points ask alike, after their own shape checks (so that gx, gy are small enough for the product below) → MNET_OK, or the
// code mnet_fail filed under `who`.  `unit`: a table entry's name; `floor`: 0 from a kernel without one; the launch is gx x gy x n workgroups of 256.
static inline int ink_check_launch(const char* who, const char* unit, const void* src, const void* table, const void* dst, int n, long long dst_len, int floor,
                                   long long gx, long long gy) {
    MNET_CHECK_ARG(src && table && dst, "%s: null pointer", who);
    MNET_CHECK_ARG(n >= 1 && dst_len >= 1, "%s: bad shape (n=%d, dst_len=%lld)", who, n, dst_len);
    MNET_CHECK_ARG(n <= 65535, "%s: %d %ss (the grid's last axis holds 65535)", who, n, unit);
    MNET_CHECK_ARG(floor >= 0 && floor <= 255, "%s: floor %d outside 0..255", who, floor);
    MNET_CHECK_ALIGN(reinterpret_cast<uintptr_t>(table) % 8 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0,
                     "%s: the %s table must be 8-byte aligned and dst 4-byte aligned", who, unit);
    MNET_CHECK_ARG(gy <= 65535 && gx * gy * n * 256 <= 4294967295ll, "%s: batch too large (%lld x %lld x %d workgroups of 256 threads)", who, gx, gy, n);
    return MNET_OK;
}
