// What the page-path kernels share (lq_kernels.hip, page_kernels.hip, column_kernels.hip, quad_kernels.hip and, through cell_paste.h,
// mixed_kernels.hip): the tile, its place in the grid, the cubic taps of a tile in LDS and the integer cubic itself — stated once, so that a fix
// reaches every kernel.
//
// The tile: 256 threads take 64 columns x 16 rows of ONE descriptor's output, counted from that output's own corner; thread t has column t % 64 and
// the rows t / 64 + 4 i, i < 4 (x fastest: stores coalesce).  The launcher does not see the device table, so the grid is n descriptors x the tiles of
// the largest output the caller names (pt_grid); a workgroup whose tile lies outside its descriptor's output returns, or writes fill, before it
// loads anything — each kernel states its own condition.
// The taps: the tile's 64 column taps and 16 row taps are computed once (fp64 sample positions: 80 lanes, not 1024 pixels) by lq_taps.h's
// lq_cubic_taps, whose arithmetic is not restated here, and kept as 16-byte records; every translation unit that includes this header is compiled
// with -ffp-contract=off (build.sh), as lq_taps.h requires.
// The cubic: four rows x four columns of byte loads per channel (3-byte pixels at any offset), both passes in integers, one rounding shift by 22
// bits and a clip.  With sum |taps| <= 2816 per axis, |v| <= 255 * 2816^2 and v + 2^21 <= 2 024 210 432 < 2^31: int32 holds every sum
// (tests/test_lq_device.py asserts the tap bound), and integer sums are exact in any order.
#pragma once
#include "lq_taps.h"

constexpr int PT_TX = 64, PT_TY = 16;      // tile: 64 columns x 16 rows, 256 threads x 4 rows each
constexpr long long PT_MAX_BLOCKS = 0x7fffffffll;

struct alignas(16) PtI4 { int v[4]; };
struct PtTaps { PtI4 ci[PT_TX], ct[PT_TX], ri[PT_TY], rt[PT_TY]; };      // a tile's taps in LDS: source indices and weights, columns and rows

struct PtTile { int x0, y0, desc; };       // the tile's first column and row in its descriptor's output; the descriptor's index

__device__ __forceinline__ PtTile pt_tile(int tiles_x, int tiles_y) {
    const int bid = (int)blockIdx.x;
    return {(bid % tiles_x) * PT_TX, ((bid / tiles_x) % tiles_y) * PT_TY, bid / (tiles_x * tiles_y)};
}

// The taps of tile T on a source of nx columns x ny rows at the steps (step_x, step_y), by the first 80 threads, then a barrier: every thread of the
// workgroup must call it.  A column index is stored as (col0 + idx) * col_mul and a row index as row0 + idx (a source origin; 3 for a byte offset).
__device__ __forceinline__ void pt_stage_taps(PtTaps& s, PtTile T, int nx, double step_x, int ny, double step_y, int col0, int col_mul, int row0) {
    const int t = (int)threadIdx.x;
    if (t < PT_TX) {
        const LqTaps c = lq_cubic_taps(T.x0 + t, nx, step_x);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s.ci[t].v[j] = (col0 + c.idx[j]) * col_mul; s.ct[t].v[j] = c.tap[j]; }
    } else if (t < PT_TX + PT_TY) {
        const int r = t - PT_TX;
        const LqTaps c = lq_cubic_taps(T.y0 + r, ny, step_y);
#pragma unroll
        for (int j = 0; j < 4; ++j) { s.ri[r].v[j] = row0 + c.idx[j]; s.rt[r].v[j] = c.tap[j]; }
    }
    __syncthreads();
}

// a sum of the two passes → the byte: their one rounding, and the clip
__device__ __forceinline__ int pt_round_clip(int acc) { return min(max((acc + (1 << 21)) >> 22, 0), 255); }

// One pixel of three interleaved channels: rows ri of `src` (row_bytes apart), byte offsets ci within a row → the sums acc[0..2], which the caller
// turns into bytes with pt_round_clip where it stores them (clipped here, column_gather_u8_kernel took 7 more registers and lost a wave)
__device__ __forceinline__ void pt_cubic_rgb(const unsigned char* src, size_t row_bytes, const PtI4& ci, const PtI4& ct, const PtI4& ri, const PtI4& rt,
                                             int acc[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned char* row = src + (size_t)ri.v[j] * row_bytes;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int hor = (int)row[(size_t)ci.v[0] + c] * ct.v[0] + (int)row[(size_t)ci.v[1] + c] * ct.v[1] + (int)row[(size_t)ci.v[2] + c] * ct.v[2] +
                            (int)row[(size_t)ci.v[3] + c] * ct.v[3];
            acc[c] += hor * rt.v[j];
        }
    }
}

// The launcher's half: the tiles of a width x height output and the grid of n descriptors.  blocks > PT_MAX_BLOCKS: the launcher refuses, in its
// own words (a count beyond 2^31 - 1 tiles per descriptor is returned as that count: n x it may not fit 64 bits).
struct PtGrid { long long tiles_x, tiles_y, blocks; };

inline PtGrid pt_grid(int n, int width, int height) {
    const long long tiles_x = ((long long)width + PT_TX - 1) / PT_TX, tiles_y = ((long long)height + PT_TY - 1) / PT_TY, per = tiles_x * tiles_y;
    return {tiles_x, tiles_y, per <= PT_MAX_BLOCKS ? (long long)n * per : per};
}
