// Both ink profiles of boxes of a sheared frame of a page on the device (include/marconet_hip_skewink.h): boxink_kernels.hip's sums, filed under the
// frame coordinates r' = r - sh(x), c' = x + sh(r) of a pair's left pixel, sh(v) = floor((v slope + 32768) / 65536).  The definition is
// marconet_amd/skew.py::frame_ink; the sums are exact integers (a bin holds at most one pair per column or per row of a page under 2^17 a side: below
// 2^25), so the order of the additions — across lanes, waves, workgroups — does not matter and the result equals the host's with ==.
//
// Launch shape: grid (ceil(max_w / 256), ceil(max_h / 32), n), 256 threads = 4 waves; workgroup (bx, by, b) covers the tile of columns
// [px1 + 256 bx, + 256) and rows [py1 + 32 by, + 32) of record b's scan rectangle.  Thread t owns column x of the tile and walks its rows, as
// box_ink_u8_kernel does: its own pixel's luma, the right neighbour's from the next lane (the last lane of a wave and the last column of the
// rectangle load it themselves), membership of the box tested per pair.  |slope| <= 8192, so over a tile sh(x) takes at most 33 values and sh(r) at
// most 5: the tile's pairs fall into at most 64 row bins and 260 column bins, kept as two LDS histograms.
//   row bins:    sh(x) is monotone along a wave, so the lanes of one row bin are a run; a segmented scan over the wave (6 shuffles, the runs known
//                before the rows are walked) leaves a run's sum in its last lane, which adds it to the LDS bin where it is not 0: at most 9 LDS
//                atomics per wave and row, all to different bins.
//   column bins: sh(r) is uniform over the workgroup; a thread sums its column in a register while sh(r) stays and adds it to the LDS bin when it
//                changes (at most 5 times a tile).  A record with out_cols = -1 — the skew search — skips this.
// After the rows every bin that is not 0 is added to dst by one global atomicAdd.  The kernel only ADDS: the caller zeroes dst.
// Bounds: a record's box, slope, scan rectangle (inside the page) and wanted output ranges (inside [0, dst_len), in 64 bits) are checked before
// anything is read; every load is at a column < px2 (or its right neighbour, < W) and a row < py2 of a rectangle that passed; every add at
// out_rows + (r' - r1) with r1 <= r' < r2 or out_cols + (c' - c1) with c1 <= c' < c2 of ranges that passed (tested again at the flush); every LDS
// index is tested against its histogram's size.  A record that fails marks the in-range ones of its wanted profiles -1 by plain stores, the
// workgroups of the record sharing the entries out between them, one writer per entry.
#include "common.h"
#include "../../include/marconet_hip_skewink.h"

namespace {

constexpr int SKEWINK_TILE_W = 256, SKEWINK_TILE_H = 32, SKEWINK_MAX_SLOPE = 8192, SKEWINK_MAX_SIDE = 1 << 17;
constexpr int SKEWINK_ROW_BINS = SKEWINK_TILE_H + SKEWINK_TILE_W / 8 + 1;              // 65
constexpr int SKEWINK_COL_BINS = SKEWINK_TILE_W + SKEWINK_TILE_H / 8 + 1;              // 261

static_assert(sizeof(mnet_skew_box) == 48, "mnet_skew_box is 48 bytes");

__device__ __forceinline__ int skew_sh(int v, int m) { return (v * m + 32768) >> 16; }          // v < 2^17 + 256, |m| <= 2^13: inside 32 bits; >> floors

__device__ __forceinline__ int skew_luma(const unsigned char* p) { return (77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8; }

__global__ void __launch_bounds__(SKEWINK_TILE_W) skew_ink_u8_kernel(const unsigned char* __restrict__ page, int H, int W,
                                                                     const mnet_skew_box* __restrict__ boxes, int floor, int* __restrict__ dst,
                                                                     long long dst_len) {
    __shared__ int hrow[SKEWINK_ROW_BINS];
    __shared__ int hcol[SKEWINK_COL_BINS];
    const mnet_skew_box b = boxes[blockIdx.z];
    const int t = (int)threadIdx.x, lane = t & 63;
    const long long bh = (long long)b.r2 - b.r1, bw = (long long)b.c2 - b.c1;
    const bool want_r = b.out_rows != -1, want_c = b.out_cols != -1;
    if (bh < 1 || bw < 1 || (!want_r && !want_c)) return;                               // uniform over the workgroup, as every test up to the rows
    const bool in_r = want_r && b.out_rows >= 0 && (long long)b.out_rows + bh <= dst_len;
    const bool in_c = want_c && b.out_cols >= 0 && (long long)b.out_cols + bw <= dst_len;
    const bool ok = b.slope >= -SKEWINK_MAX_SLOPE && b.slope <= SKEWINK_MAX_SLOPE && b.px1 >= 0 && b.px1 <= b.px2 && b.px2 <= W && b.py1 >= 0 &&
                    b.py1 <= b.py2 && b.py2 <= H && in_r == want_r && in_c == want_c;
    if (!ok) {                                                                          // one writer per entry: the record's workgroups stride over them
        const long long first = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * SKEWINK_TILE_W + t;
        const long long step = (long long)gridDim.x * gridDim.y * SKEWINK_TILE_W;
        if (in_r) for (long long i = first; i < bh; i += step) dst[(long long)b.out_rows + i] = -1;
        if (in_c) for (long long i = first; i < bw; i += step) dst[(long long)b.out_cols + i] = -1;
        return;
    }
    const int X0 = b.px1 + (int)blockIdx.x * SKEWINK_TILE_W, R0 = b.py1 + (int)blockIdx.y * SKEWINK_TILE_H;      // max_w, max_h < 2^17: no overflow
    if (X0 >= b.px2 || R0 >= b.py2) return;
    for (int i = t; i < SKEWINK_ROW_BINS; i += SKEWINK_TILE_W) hrow[i] = 0;
    for (int i = t; i < SKEWINK_COL_BINS; i += SKEWINK_TILE_W) hcol[i] = 0;
    __syncthreads();
    const int rows = min(SKEWINK_TILE_H, b.py2 - R0), m = b.slope;
    const int x = X0 + t;
    const bool own = x < b.px2, has_pair = own && x + 1 < W, loads_right = lane == 63 || x + 1 >= b.px2;
    // sh is monotone: over the tile's columns and rows its extremes lie at their ends (X0 < px2 <= W, so every argument is below 2^17)
    const int sx = skew_sh(min(x, W - 1), m);
    const int sx_max = max(skew_sh(X0, m), skew_sh(min(X0 + SKEWINK_TILE_W - 1, W - 1), m));
    const int sr_min = min(skew_sh(R0, m), skew_sh(R0 + rows - 1, m));
    const int rbin0 = sx_max - sx;                                                      // row r0 + rr of column x: bin rr + rbin0 = r' - (R0 - sx_max)
    unsigned same = 0;                                                                  // bit k: lane - 2^k lies in this lane's run of equal sh(x)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int other = __shfl_up(sx, 1u << k, 64);
        if (lane >= (1 << k) && other == sx) same |= 1u << k;
    }
    const int next = __shfl_down(sx, 1, 64);
    const bool run_end = lane == 63 || next != sx;
    const unsigned char* p = page + ((long long)R0 * W + x) * 3;                        // dereferenced only where own / has_pair
    int col = 0, cur = skew_sh(R0, m);
    for (int rr = 0; rr < rows; ++rr, p += 3ll * W) {                                   // `rows` is uniform: every lane takes part in the shuffles
        const int r = R0 + rr, sr = skew_sh(r, m);
        if (want_c && sr != cur) {                                                      // uniform
            const int i = t + cur - sr_min;
            if (col != 0 && (unsigned)i < (unsigned)SKEWINK_COL_BINS) atomicAdd(&hcol[i], col);
            col = 0;
            cur = sr;
        }
        const int y0 = own ? skew_luma(p) : 0;
        int y1 = __shfl_down(y0, 1, 64);
        if (loads_right) y1 = has_pair ? skew_luma(p + 3) : 0;
        int e = 0;
        if (has_pair) {
            const int d = abs(y1 - y0);
            e = d >= floor ? d : 0;
        }
        const int rp = r - sx, cp = x + sr;
        if (rp < b.r1 || rp >= b.r2 || cp < b.c1 || cp + 1 >= b.c2) e = 0;
        col += e;
        if (want_r) {
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int v = __shfl_up(e, 1u << k, 64);
                if (same & (1u << k)) e += v;
            }
            const int i = rr + rbin0;
            if (run_end && e != 0 && (unsigned)i < (unsigned)SKEWINK_ROW_BINS) atomicAdd(&hrow[i], e);
        }
    }
    if (want_c) {
        const int i = t + cur - sr_min;
        if (col != 0 && (unsigned)i < (unsigned)SKEWINK_COL_BINS) atomicAdd(&hcol[i], col);
    }
    __syncthreads();
    if (want_r && t < SKEWINK_ROW_BINS) {
        const int v = hrow[t];
        const long long i = (long long)(R0 - sx_max + t) - b.r1;
        if (v != 0 && i >= 0 && i < bh) atomicAdd(dst + ((long long)b.out_rows + i), v);
    }
    if (want_c) {
        for (int k = t; k < SKEWINK_COL_BINS; k += SKEWINK_TILE_W) {
            const int v = hcol[k];
            const long long i = (long long)(X0 + sr_min + k) - b.c1;
            if (v != 0 && i >= 0 && i < bw) atomicAdd(dst + ((long long)b.out_cols + i), v);
        }
    }
}

}  // namespace

extern "C" int mnet_skew_ink_u8(const uint8_t* page, int32_t H, int32_t W, const mnet_skew_box* boxes, int32_t n, int32_t max_h, int32_t max_w, int32_t floor,
                                int32_t* dst, int64_t dst_len, void* stream) {
    MNET_CHECK_ARG(page && boxes && dst, "skew_ink_u8: null pointer");
    MNET_CHECK_ARG(H >= 1 && W >= 1 && H < SKEWINK_MAX_SIDE && W < SKEWINK_MAX_SIDE, "skew_ink_u8: page %d x %d outside [1, 2^17) a side", W, H);
    MNET_CHECK_ARG(n >= 1 && dst_len >= 1 && max_h >= 1 && max_w >= 1 && max_h < SKEWINK_MAX_SIDE && max_w < SKEWINK_MAX_SIDE,
                   "skew_ink_u8: bad shape (n=%d, max_h=%d, max_w=%d, dst_len=%lld)", n, max_h, max_w, (long long)dst_len);
    MNET_CHECK_ARG(n <= 65535, "skew_ink_u8: %d records (the grid's third axis holds 65535)", n);
    MNET_CHECK_ARG(floor >= 0 && floor <= 255, "skew_ink_u8: floor %d outside 0..255", floor);
    MNET_CHECK_ALIGN(reinterpret_cast<uintptr_t>(boxes) % 8 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0,
                     "skew_ink_u8: the record table must be 8-byte aligned and dst 4-byte aligned");
    const long long gx = ((long long)max_w + SKEWINK_TILE_W - 1) / SKEWINK_TILE_W, gy = ((long long)max_h + SKEWINK_TILE_H - 1) / SKEWINK_TILE_H;
    MNET_CHECK_ARG(gy <= 65535 && gx * gy * n * SKEWINK_TILE_W <= 4294967295ll, "skew_ink_u8: batch too large (%lld x %lld x %d workgroups of 256 threads)",
                   gx, gy, n);
    hipLaunchKernelGGL(skew_ink_u8_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)n), dim3(SKEWINK_TILE_W), 0, reinterpret_cast<hipStream_t>(stream),
                       page, (int)H, (int)W, boxes, (int)floor, reinterpret_cast<int*>(dst), (long long)dst_len);
    MNET_LAUNCH_CHECK("skew_ink_u8");
    return MNET_OK;
}
