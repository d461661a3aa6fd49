// The ink profiles of boxes of a page on the device: three kernels over one definition (marconet_amd/ink.py; the shared pieces are ink.h's).  With
// Y the integer luma (77 R + 150 G + 29 B + 128) >> 8, d = |Y(x + 1, r) - Y(x, r)| and e = d where d >= floor, else 0, a pair (x, x + 1) belongs to
// the thread of its LEFT pixel, so one that straddles two lanes' strides, two waves or two tiles is counted once.  Every sum is an exact integer
// below 2^31, so the order of the additions — across lanes, waves, workgroups — does not matter and the results equal the host's with ==.
//
// row_ink_u8_kernel (include/marconet_hip_rowink.h; ink.py::row_ink): per row of a box the sum over x of d (w < 2^23 pairs of at most 255).
// Launch shape: grid (ceil(max_h / 4), n), 256 threads = 4 waves; wave v of workgroup (bx, b) owns row 4 bx + v of box b.  Lane l takes the pairs
// (x, x + 1) for x = l, l + 64, ... < w - 1.  The row is contiguous; the 64 lanes read 192 consecutive bytes (and the 3 behind them) per step.  A
// butterfly over the 64 lanes, lane 0 stores: the kernel WRITES every row of a box it follows and never adds.
// Bounds: the box's last byte, offset + (h - 1) pitch + 3 w, is checked against src_bytes in 64 bits and [out, out + h) against [0, dst_len); every
// load is at a row < h and a pixel < w of a box that passed, every store at out + r with r < h of a range that passed.  A box that fails its source
// check is marked -1, a row by lane 0 of its wave; a box whose rows have no place in dst writes nothing.
//
// box_ink_u8_kernel (include/marconet_hip_boxink.h; ink.py::box_ink): per row r of a box the sum over x of e, per column x the sum over r of e
// (h, w < 2^23 terms of at most 255).
// Launch shape: grid (ceil(max_w / 256), ceil(max_h / 32), n), 256 threads = 4 waves; workgroup (bx, by, b) covers the tile of columns
// [256 bx, 256 bx + 256) and rows [32 by, 32 by + 32) of box b.  Thread t owns column x = 256 bx + t and walks the tile's rows: the 256 threads
// read 768 consecutive bytes of a row per step.  A thread computes the luma of its own pixel and takes its right neighbour's from the next lane;
// lane 63 of a wave loads that neighbour itself (three more bytes): ink.h's row step.
//   column sum: one register per thread, one int atomicAdd per thread per tile where it is not 0 (a wave's adds are 256 contiguous bytes);
//   row sums:   a butterfly over the 64 lanes, lane 0 of each wave into LDS [4][32]; after the rows the first 32 threads add the 4 waves' parts and
//               issue one int atomicAdd per row per tile where it is not 0.
// The kernel only ADDS: the caller zeroes dst (the header says so; ops.box_ink_u8 allocates zeros).  A sum of 0 is not added: a blank tile — most
// of a page — issues no atomic at all.
// Bounds: the box's last byte is checked as the row kernel's, and [out_rows, out_rows + h) and [out_cols, out_cols + w) against [0, dst_len); every
// load is at a row < h and a pixel < w of a box that passed, every store or add at out_rows + r with r < h or at out_cols + x with x < w of ranges
// that passed.  A box that fails its source check is marked -1 by plain stores: the row profile by the tiles of bx = 0, the column profile by the
// tiles of by = 0, one writer per element.
//
// skew_ink_u8_kernel (include/marconet_hip_skewink.h; ink.py::frame_ink): the box kernel's sums, filed under the frame coordinates r' = r - sh(x),
// c' = x + sh(r) of a pair's left pixel, sh(v) = floor((v slope + 32768) / 65536) (a bin holds at most one pair per column or row of a page under
// 2^17 a side: below 2^25).  Launch shape: the box kernel's, over the tiles of columns [px1 + 256 bx, + 256) and rows [py1 + 32 by, + 32) of record
// b's scan rectangle, with the same row step (the last lane of a wave and the last column of the rectangle load the right neighbour themselves)
// and membership of the box tested per pair.  |slope| <= 8192, so over a tile sh(x) takes at most 33 values and sh(r) at most 5: the tile's pairs
// fall into at most 64 row bins and 260 column bins, kept as two LDS histograms.
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
#include "ink.h"
#include "../../include/marconet_hip_rowink.h"
#include "../../include/marconet_hip_boxink.h"
#include "../../include/marconet_hip_skewink.h"

namespace {

constexpr int BOXINK_TILE_W = 256, BOXINK_TILE_H = 32;
constexpr int SKEWINK_TILE_W = 256, SKEWINK_TILE_H = 32, SKEWINK_MAX_SLOPE = 8192, SKEWINK_MAX_SIDE = 1 << 17;
constexpr int SKEWINK_ROW_BINS = SKEWINK_TILE_H + SKEWINK_TILE_W / 8 + 1;              // 65
constexpr int SKEWINK_COL_BINS = SKEWINK_TILE_W + SKEWINK_TILE_H / 8 + 1;              // 261

static_assert(sizeof(mnet_ink_box) == 24, "mnet_ink_box is 24 bytes");
static_assert(sizeof(mnet_ink_box2) == 32, "mnet_ink_box2 is 32 bytes");
static_assert(sizeof(mnet_skew_box) == 48, "mnet_skew_box is 48 bytes");

__global__ void __launch_bounds__(256) row_ink_u8_kernel(const unsigned char* __restrict__ src, long long src_bytes, const mnet_ink_box* __restrict__ boxes,
                                                         int* __restrict__ dst, long long dst_len) {
    const mnet_ink_box b = boxes[blockIdx.y];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const long long r = 4ll * blockIdx.x + wave;
    if (b.h < 1 || r >= b.h) return;                                                   // uniform over the wave
    if (b.out < 0 || (long long)b.out + b.h > dst_len) return;                         // the rows have no place in dst: nothing is written
    int* d = dst + ((long long)b.out + r);
    if (!ink_view_ok<false>(b, src_bytes)) {
        if (lane == 0) *d = -1;
        return;
    }
    const unsigned char* row = src + b.offset + r * (long long)b.pitch;
    int acc = 0;
    for (int x = lane; x < b.w - 1; x += 64) {
        const unsigned char* p = row + 3ll * x;
        acc += abs(ink_luma(p + 3) - ink_luma(p));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) *d = acc;
}

__global__ void __launch_bounds__(BOXINK_TILE_W) box_ink_u8_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                                   const mnet_ink_box2* __restrict__ boxes, int floor, int* __restrict__ dst,
                                                                   long long dst_len) {
    __shared__ int part[4][BOXINK_TILE_H];
    const mnet_ink_box2 b = boxes[blockIdx.z];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int x0 = (int)blockIdx.x * BOXINK_TILE_W, r0 = (int)blockIdx.y * BOXINK_TILE_H;       // max_w, max_h < 2^23: no overflow
    if (b.h < 1 || b.w < 1 || x0 >= b.w || r0 >= b.h) return;                           // uniform over the workgroup
    if (b.out_rows < 0 || (long long)b.out_rows + b.h > dst_len || b.out_cols < 0 || (long long)b.out_cols + b.w > dst_len) return;
    const int x = x0 + t;
    int* drows = dst + ((long long)b.out_rows + r0);
    int* dcols = dst + (long long)b.out_cols;
    if (!ink_view_ok<true>(b, src_bytes)) {                                              // uniform too: one writer per element
        if (blockIdx.x == 0 && t < BOXINK_TILE_H && r0 + t < b.h) drows[t] = -1;
        if (blockIdx.y == 0 && x < b.w) dcols[x] = -1;
        return;
    }
    const int rows = min(BOXINK_TILE_H, b.h - r0);
    const bool has_px = x < b.w, has_pair = x + 1 < b.w;
    const unsigned char* p = src + b.offset + (long long)r0 * b.pitch + 3ll * x;       // dereferenced only where has_px / has_pair
    int col = 0;
    for (int rr = 0; rr < rows; ++rr, p += b.pitch) {                                  // `rows` is uniform: every lane takes part in the shuffles
        int e = ink_pair_e(p, has_px, has_pair, lane == 63, floor);
        col += e;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
        if (lane == 0) part[wave][rr] = e;
    }
    if (has_pair && col != 0) atomicAdd(dcols + x, col);
    __syncthreads();
    if (t < rows) {
        const int s = part[0][t] + part[1][t] + part[2][t] + part[3][t];
        if (s != 0) atomicAdd(drows + t, s);
    }
}

__device__ __forceinline__ int skew_sh(int v, int m) { return (v * m + 32768) >> 16; }          // v < 2^17 + 256, |m| <= 2^13: inside 32 bits; >> floors

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
        int e = ink_pair_e(p, own, has_pair, loads_right, floor);
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

extern "C" int mnet_row_ink_u8(const uint8_t* src, int64_t src_bytes, const mnet_ink_box* boxes, int32_t n, int32_t max_h, int32_t* dst, int64_t dst_len,
                               void* stream) {
    MNET_CHECK_ARG(max_h >= 1 && src_bytes >= 1, "row_ink_u8: bad shape (max_h=%d, src_bytes=%lld)", max_h, (long long)src_bytes);
    const long long gx = ((long long)max_h + 3) / 4;
    if (const int err = ink_check_launch("row_ink_u8", "box", src, boxes, dst, n, dst_len, 0, gx, 1)) return err;
    hipLaunchKernelGGL(row_ink_u8_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, (long long)src_bytes,
                       boxes, reinterpret_cast<int*>(dst), (long long)dst_len);
    MNET_LAUNCH_CHECK("row_ink_u8");
    return MNET_OK;
}

extern "C" int mnet_box_ink_u8(const uint8_t* src, int64_t src_bytes, const mnet_ink_box2* boxes, int32_t n, int32_t max_h, int32_t max_w, int32_t floor,
                               int32_t* dst, int64_t dst_len, void* stream) {
    MNET_CHECK_ARG(src_bytes >= 1 && max_h >= 1 && max_w >= 1 && max_h < (1 << 23) && max_w < (1 << 23),
                   "box_ink_u8: bad shape (max_h=%d, max_w=%d, src_bytes=%lld)", max_h, max_w, (long long)src_bytes);
    const long long gx = ((long long)max_w + BOXINK_TILE_W - 1) / BOXINK_TILE_W, gy = ((long long)max_h + BOXINK_TILE_H - 1) / BOXINK_TILE_H;
    if (const int err = ink_check_launch("box_ink_u8", "box", src, boxes, dst, n, dst_len, floor, gx, gy)) return err;
    hipLaunchKernelGGL(box_ink_u8_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)n), dim3(BOXINK_TILE_W), 0, reinterpret_cast<hipStream_t>(stream), src,
                       (long long)src_bytes, boxes, (int)floor, reinterpret_cast<int*>(dst), (long long)dst_len);
    MNET_LAUNCH_CHECK("box_ink_u8");
    return MNET_OK;
}

extern "C" int mnet_skew_ink_u8(const uint8_t* page, int32_t H, int32_t W, const mnet_skew_box* boxes, int32_t n, int32_t max_h, int32_t max_w, int32_t floor,
                                int32_t* dst, int64_t dst_len, void* stream) {
    MNET_CHECK_ARG(H >= 1 && W >= 1 && H < SKEWINK_MAX_SIDE && W < SKEWINK_MAX_SIDE, "skew_ink_u8: page %d x %d outside [1, 2^17) a side", W, H);
    MNET_CHECK_ARG(max_h >= 1 && max_w >= 1 && max_h < SKEWINK_MAX_SIDE && max_w < SKEWINK_MAX_SIDE, "skew_ink_u8: bad shape (%d x %d)", max_w, max_h);
    const long long gx = ((long long)max_w + SKEWINK_TILE_W - 1) / SKEWINK_TILE_W, gy = ((long long)max_h + SKEWINK_TILE_H - 1) / SKEWINK_TILE_H;
    if (const int err = ink_check_launch("skew_ink_u8", "record", page, boxes, dst, n, dst_len, floor, gx, gy)) return err;
    hipLaunchKernelGGL(skew_ink_u8_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)n), dim3(SKEWINK_TILE_W), 0, reinterpret_cast<hipStream_t>(stream),
                       page, (int)H, (int)W, boxes, (int)floor, reinterpret_cast<int*>(dst), (long long)dst_len);
    MNET_LAUNCH_CHECK("skew_ink_u8");
    return MNET_OK;
}
