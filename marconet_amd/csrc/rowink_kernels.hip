// The ink profile of boxes of a page on the device (include/marconet_hip_rowink.h): per row of a box the sum over x of |Y(x + 1) - Y(x)|, Y the
// integer luma (77 R + 150 G + 29 B + 128) >> 8.  The definition is marconet_amd/blind_columns.py::row_ink; the sum is an exact integer (w < 2^23
// pairs of at most 255: below 2^31), so the order of the reduction does not matter and the result equals the host's with ==.
//
// Launch shape: grid (ceil(max_h / 4), n), 256 threads = 4 waves; wave v of workgroup (bx, b) owns row 4 bx + v of box b.  Lane l takes the pairs
// (x, x + 1) for x = l, l + 64, ... < w - 1: a pair belongs to the lane of its LEFT pixel, so one that straddles two lanes' strides is counted once.
// The row is contiguous; the 64 lanes read 192 consecutive bytes (and the 3 behind them) per step.  A butterfly over the 64 lanes, lane 0 stores.
// Bounds: the box's last byte, offset + (h - 1) pitch + 3 w, is checked against src_bytes in 64 bits and [out, out + h) against [0, dst_len); every
// load is at a row < h and a pixel < w of a box that passed, every store at out + r with r < h of a range that passed.
#include "common.h"
#include "../../include/marconet_hip_rowink.h"

namespace {

static_assert(sizeof(mnet_ink_box) == 24, "mnet_ink_box is 24 bytes");

__device__ __forceinline__ bool ink_box_ok(const mnet_ink_box& b, long long src_bytes) {
    if (b.h < 1 || b.w < 1 || b.w >= (1 << 23) || b.offset < 0 || (long long)b.pitch < 3ll * b.w) return false;
    // offset <= src_bytes first: the sum below then stays far inside 64 bits (pitch, h < 2^31), as window_ok (window_kernels.hip) has it
    return b.offset <= src_bytes && (long long)(b.h - 1) * b.pitch + 3ll * b.w <= src_bytes - b.offset;
}

__device__ __forceinline__ int ink_luma(const unsigned char* p) { return (77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8; }

__global__ void __launch_bounds__(256) row_ink_u8_kernel(const unsigned char* __restrict__ src, long long src_bytes, const mnet_ink_box* __restrict__ boxes,
                                                         int* __restrict__ dst, long long dst_len) {
    const mnet_ink_box b = boxes[blockIdx.y];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const long long r = 4ll * blockIdx.x + wave;
    if (b.h < 1 || r >= b.h) return;                                                   // uniform over the wave
    if (b.out < 0 || (long long)b.out + b.h > dst_len) return;                         // the rows have no place in dst: nothing is written
    int* d = dst + ((long long)b.out + r);
    if (!ink_box_ok(b, src_bytes)) {
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

}  // namespace

extern "C" int mnet_row_ink_u8(const uint8_t* src, int64_t src_bytes, const mnet_ink_box* boxes, int32_t n, int32_t max_h, int32_t* dst, int64_t dst_len,
                               void* stream) {
    MNET_CHECK_ARG(src && boxes && dst, "row_ink_u8: null pointer");
    MNET_CHECK_ARG(n >= 1 && max_h >= 1 && src_bytes >= 1 && dst_len >= 1, "row_ink_u8: bad shape (n=%d, max_h=%d, src_bytes=%lld, dst_len=%lld)", n, max_h,
                   (long long)src_bytes, (long long)dst_len);
    MNET_CHECK_ARG(n <= 65535, "row_ink_u8: %d boxes (the grid's second axis holds 65535)", n);
    MNET_CHECK_ALIGN(reinterpret_cast<uintptr_t>(boxes) % 8 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0,
                     "row_ink_u8: the box table must be 8-byte aligned and dst 4-byte aligned");
    const long long gx = ((long long)max_h + 3) / 4;
    MNET_CHECK_ARG(gx * n * 256 <= 4294967295ll, "row_ink_u8: batch too large (%lld workgroups of 256 threads)", gx * n);
    hipLaunchKernelGGL(row_ink_u8_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, (long long)src_bytes,
                       boxes, reinterpret_cast<int*>(dst), (long long)dst_len);
    MNET_LAUNCH_CHECK("row_ink_u8");
    return MNET_OK;
}
