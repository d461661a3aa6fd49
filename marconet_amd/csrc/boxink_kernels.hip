// Both ink profiles of boxes of a page on the device (include/marconet_hip_boxink.h): with Y the integer luma (77 R + 150 G + 29 B + 128) >> 8,
// d = |Y(x + 1, r) - Y(x, r)| and e = d where d >= floor, else 0: per row r of a box the sum over x of e, per column x the sum over r of e.  The
// definition is marconet_amd/layout.py::box_ink; the sums are exact integers (h, w < 2^23 terms of at most 255: below 2^31), so the order of the
// additions — across lanes, waves, workgroups — does not matter and the result equals the host's with ==.
//
// Launch shape: grid (ceil(max_w / 256), ceil(max_h / 32), n), 256 threads = 4 waves; workgroup (bx, by, b) covers the tile of columns
// [256 bx, 256 bx + 256) and rows [32 by, 32 by + 32) of box b.  Thread t owns column x = 256 bx + t and walks the tile's rows: the 256 threads
// read 768 consecutive bytes of a row per step.  A pair (x, x + 1) belongs to the thread of its LEFT pixel, so one that straddles two waves or two
// tiles is counted once.  A thread computes the luma of its own pixel and takes its right neighbour's from the next lane; lane 63 of a wave loads
// that neighbour itself (three more bytes).
//   column sum: one register per thread, one int atomicAdd per thread per tile where it is not 0 (a wave's adds are 256 contiguous bytes);
//   row sums:   a butterfly over the 64 lanes, lane 0 of each wave into LDS [4][32]; after the rows the first 32 threads add the 4 waves' parts and
//               issue one int atomicAdd per row per tile where it is not 0.
// The kernel only ADDS: the caller zeroes dst (the header says so; ops.box_ink_u8 allocates zeros).  A sum of 0 is not added: a blank tile — most
// of a page — issues no atomic at all.
// Bounds: the box's last byte, offset + (h - 1) pitch + 3 w, is checked against src_bytes in 64 bits, and [out_rows, out_rows + h) and
// [out_cols, out_cols + w) against [0, dst_len); every load is at a row < h and a pixel < w of a box that passed, every store or add at
// out_rows + r with r < h or at out_cols + x with x < w of ranges that passed.  A box that fails its source check is marked -1 by plain stores:
// the row profile by the tiles of bx = 0, the column profile by the tiles of by = 0, one writer per element.
#include "common.h"
#include "../../include/marconet_hip_boxink.h"

namespace {

constexpr int BOXINK_TILE_W = 256, BOXINK_TILE_H = 32;

static_assert(sizeof(mnet_ink_box2) == 32, "mnet_ink_box2 is 32 bytes");

__device__ __forceinline__ bool ink_box2_ok(const mnet_ink_box2& b, long long src_bytes) {
    if (b.h < 1 || b.w < 1 || b.h >= (1 << 23) || b.w >= (1 << 23) || b.offset < 0 || (long long)b.pitch < 3ll * b.w) return false;
    // offset <= src_bytes first: the sum below then stays far inside 64 bits (pitch, h < 2^31), as ink_box_ok (rowink_kernels.hip) has it
    return b.offset <= src_bytes && (long long)(b.h - 1) * b.pitch + 3ll * b.w <= src_bytes - b.offset;
}

__device__ __forceinline__ int ink2_luma(const unsigned char* p) { return (77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8; }

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
    if (!ink_box2_ok(b, src_bytes)) {                                                  // uniform too: one writer per element
        if (blockIdx.x == 0 && t < BOXINK_TILE_H && r0 + t < b.h) drows[t] = -1;
        if (blockIdx.y == 0 && x < b.w) dcols[x] = -1;
        return;
    }
    const int rows = min(BOXINK_TILE_H, b.h - r0);
    const bool has_px = x < b.w, has_pair = x + 1 < b.w;
    const unsigned char* p = src + b.offset + (long long)r0 * b.pitch + 3ll * x;       // dereferenced only where has_px / has_pair
    int col = 0;
    for (int rr = 0; rr < rows; ++rr, p += b.pitch) {                                  // `rows` is uniform: every lane takes part in the shuffles
        const int y0 = has_px ? ink2_luma(p) : 0;
        int y1 = __shfl_down(y0, 1, 64);
        if (lane == 63) y1 = has_pair ? ink2_luma(p + 3) : 0;
        int e = 0;
        if (has_pair) {
            const int d = abs(y1 - y0);
            e = d >= floor ? d : 0;
        }
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

}  // namespace

extern "C" int mnet_box_ink_u8(const uint8_t* src, int64_t src_bytes, const mnet_ink_box2* boxes, int32_t n, int32_t max_h, int32_t max_w, int32_t floor,
                               int32_t* dst, int64_t dst_len, void* stream) {
    MNET_CHECK_ARG(src && boxes && dst, "box_ink_u8: null pointer");
    MNET_CHECK_ARG(n >= 1 && src_bytes >= 1 && dst_len >= 1 && max_h >= 1 && max_w >= 1 && max_h < (1 << 23) && max_w < (1 << 23),
                   "box_ink_u8: bad shape (n=%d, max_h=%d, max_w=%d, src_bytes=%lld, dst_len=%lld)", n, max_h, max_w, (long long)src_bytes,
                   (long long)dst_len);
    MNET_CHECK_ARG(n <= 65535, "box_ink_u8: %d boxes (the grid's third axis holds 65535)", n);
    MNET_CHECK_ARG(floor >= 0 && floor <= 255, "box_ink_u8: floor %d outside 0..255", floor);
    MNET_CHECK_ALIGN(reinterpret_cast<uintptr_t>(boxes) % 8 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0,
                     "box_ink_u8: the box table must be 8-byte aligned and dst 4-byte aligned");
    const long long gx = ((long long)max_w + BOXINK_TILE_W - 1) / BOXINK_TILE_W, gy = ((long long)max_h + BOXINK_TILE_H - 1) / BOXINK_TILE_H;
    MNET_CHECK_ARG(gy <= 65535 && gx * gy * n * BOXINK_TILE_W <= 4294967295ll, "box_ink_u8: batch too large (%lld x %lld x %d workgroups of 256 threads)",
                   gx, gy, n);
    hipLaunchKernelGGL(box_ink_u8_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)n), dim3(BOXINK_TILE_W), 0, reinterpret_cast<hipStream_t>(stream), src,
                       (long long)src_bytes, boxes, (int)floor, reinterpret_cast<int*>(dst), (long long)dst_len);
    MNET_LAUNCH_CHECK("box_ink_u8");
    return MNET_OK;
}
