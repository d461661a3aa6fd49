// HBM-bound and small kernels around the implicit-GEMM conv: layout changes, bilinear x2, GroupNorm
// statistics, the per-glyph AdaIN/crop and ordered scatter of TSPSRNet, SelectText gather, PixelNorm,
// demodulation.  All move 16-byte chunks per lane along the channel-minor (NHWC) axis, so a wave
// touches 1 KiB of contiguous memory per instruction; reductions use fp64 partial sums and
// wave64 butterflies, no atomics (results are bit-reproducible run to run).
#include <cstdlib>
#include "common.h"

// ============================================================================ layout: NCHW fp32 <-> NHWC T
template <typename T>
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ dst,
                                                           int C, int HW, int Cld) {
    // tile: 32 channels x 32 pixels through LDS (transpose), block (32, 8)
    __shared__ float tile[32][33];
    const int n = blockIdx.z, c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const float* s = src + (size_t)n * C * HW;
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, p = p0 + tx;
        tile[j][tx] = (c < C && p < HW) ? s[(size_t)c * HW + p] : 0.f;
    }
    __syncthreads();
    T* d = dst + (size_t)n * HW * Cld;
    for (int j = ty; j < 32; j += 8) {
        const int p = p0 + j, c = c0 + tx;
        if constexpr (__is_same(T, hm)) {
            if (p < HW) st_block32_hm(d + (size_t)p * Cld, c, tile[tx][j]);      // Cld % 32 == 0: the 32 lanes tx are one block
        } else {
            if (p < HW && c < Cld) st_elem<T>(d + (size_t)p * Cld, c, tile[tx][j]);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const T* __restrict__ src, float* __restrict__ dst,
                                                           int C, int HW, int Cld) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z, c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const T* s = src + (size_t)n * HW * Cld;
    for (int j = ty; j < 32; j += 8) {
        const int p = p0 + j, c = c0 + tx;
        tile[j][tx] = (p < HW && c < C) ? ld_elem<T>(s + (size_t)p * Cld, c) : 0.f;
    }
    __syncthreads();
    float* d = dst + (size_t)n * C * HW;
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, p = p0 + tx;
        if (c < C && p < HW) d[(size_t)c * HW + p] = tile[tx][j];
    }
}

extern "C" int mnet_nchw_to_nhwc(const float* src, void* dst, int32_t dst_dtype, int32_t n, int32_t c, int32_t h,
                                 int32_t w, int32_t c_ld, void* stream) {
    MNET_CHECK_ARG(src && dst && n > 0 && c > 0 && h > 0 && w > 0 && c_ld >= c, "nchw_to_nhwc: bad args");
    MNET_CHECK_ARG(n <= 65535 && (c_ld + 31) / 32 <= 65535, "nchw_to_nhwc: grid too large");
    MNET_CHECK_ARG(is_storage(dst_dtype), "nchw_to_nhwc: bad dtype");
    MNET_CHECK_ALIGN(!is_split4(dst_dtype) || (c_ld % 32 == 0 && aligned128(dst)), "nchw_to_nhwc: split-half output needs c_ld %% 32 == 0 and a 128-byte aligned base");
    const int HW = h * w;
    dim3 grid((HW + 31) / 32, (c_ld + 31) / 32, n), block(32, 8);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_storage(dst_dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, grid, block, 0, st, src, (T*)dst, c, HW, c_ld);
    });
    MNET_LAUNCH_CHECK("nchw_to_nhwc");
    return MNET_OK;
}

extern "C" int mnet_nhwc_to_nchw(const void* src, int32_t src_dtype, float* dst, int32_t n, int32_t c, int32_t h,
                                 int32_t w, int32_t c_ld, void* stream) {
    MNET_CHECK_ARG(src && dst && n > 0 && c > 0 && h > 0 && w > 0 && c_ld >= c, "nhwc_to_nchw: bad args");
    MNET_CHECK_ARG(n <= 65535 && (c + 31) / 32 <= 65535, "nhwc_to_nchw: grid too large");
    MNET_CHECK_ARG(is_storage(src_dtype), "nhwc_to_nchw: bad dtype");
    MNET_CHECK_ALIGN(!is_split4(src_dtype) || (c_ld % 32 == 0 && aligned128(src)), "nhwc_to_nchw: split-half input needs c_ld %% 32 == 0 and a 128-byte aligned base");
    const int HW = h * w;
    dim3 grid((HW + 31) / 32, (c + 31) / 32, n), block(32, 8);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_storage(src_dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, grid, block, 0, st, (const T*)src, dst, c, HW, c_ld);
    });
    MNET_LAUNCH_CHECK("nhwc_to_nchw");
    return MNET_OK;
}

// ============================================================================ bilinear x2 (align_corners=False)
// out row 2j   = 1/4 * in[j-1] + 3/4 * in[j]     (j-1 clamped to 0)
// out row 2j+1 = 3/4 * in[j]   + 1/4 * in[j+1]   (j+1 clamped to H-1)        same along W
// One thread = one 16-byte channel chunk of one INPUT pixel: it reads the 3x3 neighbourhood (9 loads, mostly L1/L2 hits)
// and writes the 2x2 output quad (2.25 loads per output chunk instead of 4; the kernel is bound by its 4x write stream).
// Per output the arithmetic is wy0*(wx0*a + wx1*b) + wy1*(wx0*c + wx1*d), horizontal first — ATen's order.
// TD != T (round 5): the output in another storage type — the batched driver's image-only generator level reads the fp16+8 / split-half 64-px prior
// and writes plain f16, which removes the separate mnet_convert pass over that map.  Both types carry 8 channels per chunk.
// Round 6: a thread walks UPS_RUN consecutive input rows of its column and carries the horizontally interpolated rows y-1 and y in registers: 3 chunk loads (+ decodes)
// per input pixel instead of 9 — the kernel was bound by its own instruction stream, not by the 4x write stream (4.0 TB/s where a one-trip copy of this storage's
// access pattern does 5.97, tools/microbench/stream_variants.hip).  Same operands, same operation order per output: same bits.
#ifndef MNET_UPS_RUN
#define MNET_UPS_RUN 4
#endif
#ifndef MNET_UPS_XCD
#define MNET_UPS_XCD 1
#endif
#ifndef MNET_UPS_ZIGZAG
#define MNET_UPS_ZIGZAG 1
#endif
template <typename T, typename TD = T>
__global__ void __launch_bounds__(256) upsample2x_kernel(const T* __restrict__ src, TD* __restrict__ dst,
                                                         int H, int W, int C, const float* __restrict__ scale,
                                                         unsigned items_per_image) {
    // grid: x strides over the (chunk, column, row run) items of ONE input image (32-bit index math only), y = image
    constexpr int N = Vec<T>::N;
    constexpr int R = MNET_UPS_RUN;
    static_assert(Vec<TD>::N == N, "source and destination chunks hold the same number of channels");
    const unsigned cpp = (unsigned)C / N;
    // XCD-aware order (round 6): workgroups go to the 8 XCDs round-robin, each with its own L2 — in dispatch order the neighbours of a workgroup (which read its halo
    // columns / rows again) sit on other XCDs and every re-read came from HBM / the Infinity Cache: 2.25x the input (the kernel ran at the rate of its writes + 2.25 reads).
    // Virtual order: XCD k takes the k-th eighth of the (image, workgroup) sequence — whole images, neighbours in one L2.
    unsigned bx = blockIdx.x, by = blockIdx.y;
    {
        const unsigned NWG = gridDim.x * gridDim.y, L = by * gridDim.x + bx;
        if ((NWG & 7u) == 0u && MNET_UPS_XCD) { const unsigned V = (L & 7u) * (NWG >> 3) + (L >> 3); by = V / gridDim.x; bx = V - by * gridDim.x; }
    }
    const int n = (int)by;
    const T* sbase = src + (size_t)n * H * W * C;
    TD* dbase = dst + (size_t)n * 4 * H * W * C;
    for (unsigned id = bx * 256u + threadIdx.x; id < items_per_image; id += gridDim.x * 256u) {
        const unsigned ch = id % cpp, col = id / cpp;
        const int x = (int)(col % (unsigned)W), y0 = (int)(col / (unsigned)W) * R, y1 = min(y0 + R, H);
        const int xm = max(x - 1, 0), xp = min(x + 1, W - 1);
        const T* base = sbase + (size_t)ch * N;
        // horizontally interpolated left / right output column of one input row
        auto hrow = [&](int r, float (&hl)[N], float (&hr)[N]) __attribute__((always_inline)) {
            float a[N], b[N], c[N];
            const T* rp = base + (size_t)r * W * C;
            unpackr<T>(ldraw<T>(rp + (size_t)xm * C), a);
            unpackr<T>(ldraw<T>(rp + (size_t)x * C), b);
            unpackr<T>(ldraw<T>(rp + (size_t)xp * C), c);
#pragma unroll
            for (int j = 0; j < N; ++j) { hl[j] = 0.25f * a[j] + 0.75f * b[j]; hr[j] = 0.75f * b[j] + 0.25f * c[j]; }
        };
        float sc[N];
#pragma unroll
        for (int j = 0; j < N; ++j) sc[j] = 1.f;
        if (scale) {
            const float* sp = scale + (size_t)n * C + (size_t)ch * N;
#pragma unroll
            for (int j = 0; j < N; j += 4) {
                const f32x4 s4 = *reinterpret_cast<const f32x4*>(sp + j);
                sc[j] = s4[0]; sc[j + 1] = s4[1]; sc[j + 2] = s4[2]; sc[j + 3] = s4[3];
            }
        }
        float al[N], ar[N], bl[N], br[N], cl[N], cr[N];          // rows y-1 (clamped), y, y+1 (clamped)
        const size_t orow = (size_t)2 * W * C;
        auto emit = [&](int y) __attribute__((always_inline)) {
            float o[N];
            TD* q = dbase + ((size_t)(2 * y) * (2 * W) + 2 * x) * C + (size_t)ch * N;      // output pixel (2y, 2x)
#pragma unroll
            for (int j = 0; j < N; ++j) o[j] = (0.25f * al[j] + 0.75f * bl[j]) * sc[j];
            straw<TD>(q, packr<TD>(o));
#pragma unroll
            for (int j = 0; j < N; ++j) o[j] = (0.25f * ar[j] + 0.75f * br[j]) * sc[j];
            straw<TD>(q + C, packr<TD>(o));
#pragma unroll
            for (int j = 0; j < N; ++j) o[j] = (0.75f * bl[j] + 0.25f * cl[j]) * sc[j];
            straw<TD>(q + orow, packr<TD>(o));
#pragma unroll
            for (int j = 0; j < N; ++j) o[j] = (0.75f * br[j] + 0.25f * cr[j]) * sc[j];
            straw<TD>(q + orow + C, packr<TD>(o));
        };
        // Odd runs walk UP: a run and its lower neighbour then meet at their common border at the same time (both at the end, or both at the start, of their walks) — the
        // two border rows each of them reads were fetched from HBM twice, the second reader finding them flushed from the L2 by the 4x write stream (FETCH_SIZE: 1.5x the input)
        if (!MNET_UPS_ZIGZAG || ((y0 / R) & 1) == 0) {
            hrow(max(y0 - 1, 0), al, ar);
            hrow(y0, bl, br);
            for (int y = y0; y < y1; ++y) {
                if (y + 1 < H) hrow(y + 1, cl, cr);
                else {
#pragma unroll
                    for (int j = 0; j < N; ++j) { cl[j] = bl[j]; cr[j] = br[j]; }
                }
                emit(y);
#pragma unroll
                for (int j = 0; j < N; ++j) { al[j] = bl[j]; ar[j] = br[j]; bl[j] = cl[j]; br[j] = cr[j]; }
            }
        } else {
            hrow(min(y1, H - 1), cl, cr);
            hrow(y1 - 1, bl, br);
            for (int y = y1 - 1; y >= y0; --y) {
                if (y > 0) hrow(y - 1, al, ar);
                else {
#pragma unroll
                    for (int j = 0; j < N; ++j) { al[j] = bl[j]; ar[j] = br[j]; }
                }
                emit(y);
#pragma unroll
                for (int j = 0; j < N; ++j) { cl[j] = bl[j]; cr[j] = br[j]; bl[j] = al[j]; br[j] = ar[j]; }
            }
        }
    }
}

extern "C" int mnet_upsample2x_convert_nhwc(const void* src, int32_t dtype, void* dst, int32_t dst_dtype, int32_t n, int32_t h, int32_t w,
                                            int32_t c, const float* scale, void* stream) {
    MNET_CHECK_ARG(src && dst && n > 0 && h > 0 && w > 0 && c > 0 && n <= 65535, "upsample2x: bad args");
    MNET_CHECK_ARG(is_storage(dtype), "upsample2x: bad dtype");
    MNET_CHECK_ARG(dst_dtype == dtype || (dst_dtype == MNET_F16 && is_split4(dtype)), "upsample2x: the output is the input's storage type, or MNET_F16 for a split-half / fp16+8 input");
    const int N = chunk_n(dtype);
    MNET_CHECK_ARG((long long)h * w * (c / N) * 4 < (1ll << 31), "upsample2x: image too large");
    MNET_CHECK_ALIGN(c % N == 0 && aligned16(src) && aligned16(dst) && aligned16(scale), "upsample2x: c %% %d != 0 or unaligned", N);
    MNET_CHECK_ALIGN(!is_split4(dtype) || (c % 32 == 0 && aligned128(src)), "upsample2x: split-half needs c %% 32 == 0, 128-byte aligned");
    MNET_CHECK_ALIGN(!is_split4(dst_dtype) || aligned128(dst), "upsample2x: split-half output must be 128-byte aligned");
    const long long per = (long long)((h + MNET_UPS_RUN - 1) / MNET_UPS_RUN) * w * (c / N);      // one thread per (chunk, column, run of MNET_UPS_RUN input rows)
    const int gx = (int)((per + 255) / 256 < 2048 ? (per + 255) / 256 : 2048);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_storage(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        auto launch = [&](auto dtag) {
            using TD = typename decltype(dtag)::type;
            hipLaunchKernelGGL((upsample2x_kernel<T, TD>), dim3(gx, n), dim3(256), 0, st, (const T*)src, (TD*)dst, h, w, c, scale, (unsigned)per);
        };
        if constexpr (is_split4_type<T>) { if (dst_dtype != dtype) return launch(TypeTag<f16>{}); }      // the one other output: plain f16 from a blocked storage
        launch(tag);
    });
    MNET_LAUNCH_CHECK("upsample2x");
    return MNET_OK;
}

extern "C" int mnet_upsample2x_scale_nhwc(const void* src, void* dst, int32_t dtype, int32_t n, int32_t h, int32_t w,
                                          int32_t c, const float* scale, void* stream) {
    return mnet_upsample2x_convert_nhwc(src, dtype, dst, dtype, n, h, w, c, scale, stream);
}

extern "C" int mnet_upsample2x_nhwc(const void* src, void* dst, int32_t dtype, int32_t n, int32_t h, int32_t w,
                                    int32_t c, void* stream) {
    return mnet_upsample2x_scale_nhwc(src, dst, dtype, n, h, w, c, nullptr, stream);
}

// ============================================================================ GroupNorm statistics -> affine
// stage 1: grid (slices, n). thread t owns chunk column (t % cpp) and pixel lane (t / cpp); it walks the
// pixels of its slice accumulating sum / sum of squares in fp64 (masked by valid_w); an LDS pass folds
// the threads of one group; partial[n][slice][group][2].
template <typename T>
__global__ void __launch_bounds__(256) gn_partial_kernel(const T* __restrict__ x, int H, int W, int C,
                                                         const int* __restrict__ valid_w,
                                                         double* __restrict__ partial, int slices) {
    constexpr int N = Vec<T>::N;
    __shared__ double red[256][2];
    const int n = blockIdx.y, sl = blockIdx.x, t = threadIdx.x;
    const int cpp = C / N, plane = 256 / cpp;     // cpp divides 256 (checked on host)
    const int ch = t % cpp, pl = t / cpp;
    const int vw = valid_w ? min(valid_w[n], W) : W;
    const int HW = H * W;
    const int per = (HW + slices - 1) / slices;
    const int p_begin = sl * per, p_end = min(HW, p_begin + per);
    double s = 0.0, ss = 0.0;
    const T* base = x + (size_t)n * HW * C + (size_t)ch * N;
    for (int p = p_begin + pl; p < p_end; p += plane) {
        if ((p % W) >= vw) continue;
        float v[N];
        unpackr<T>(ldraw<T>(base + (size_t)p * C), v);
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) { a += v[j]; b += v[j] * v[j]; }
        s += (double)a; ss += (double)b;
    }
    red[t][0] = s; red[t][1] = ss;
    __syncthreads();
    const int G = C / 32, cpg = 32 / N;           // chunks per group
    if (t < G) {
        double S = 0.0, SS = 0.0;
        for (int pl2 = 0; pl2 < plane; ++pl2)
            for (int k = 0; k < cpg; ++k) { const int u = pl2 * cpp + t * cpg + k; S += red[u][0]; SS += red[u][1]; }
        double* o = partial + (((size_t)n * slices + sl) * G + t) * 2;
        o[0] = S; o[1] = SS;
    }
}

// (fp64 sum, sum of squares, count, eps) of a group -> its mean (fp64: each caller rounds it where it always did) and 1/sqrt(var + eps); the variance
// is clamped at 0.  GroupNorm's one finalize: gn_finalize_kernel, gn_finalize_frag_kernel and the AdaIN kernels' group affine.
struct MeanRstd { double mean; float rstd; };
__device__ __forceinline__ MeanRstd gn_mean_rstd(double S, double SS, double cnt, float eps) {
    const double mean = S / cnt;
    double var = SS / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    return {mean, (float)(1.0 / sqrt(var + (double)eps))};
}

// stage 2: one thread per (n, channel)
__global__ void gn_finalize_kernel(const double* __restrict__ partial, int slices, int n_img, int H, int W, int C,
                                   const int* __restrict__ valid_w, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float eps, float* __restrict__ scale,
                                   float* __restrict__ shift) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_img * C) return;
    const int n = id / C, c = id - n * C, G = C / 32, g = c / 32;
    double S = 0.0, SS = 0.0;
    for (int sl = 0; sl < slices; ++sl) {
        const double* o = partial + (((size_t)n * slices + sl) * G + g) * 2;
        S += o[0]; SS += o[1];
    }
    const int vw = valid_w ? min(valid_w[n], W) : W;
    const MeanRstd m = gn_mean_rstd(S, SS, (double)H * vw * 32.0, eps);
    const float ga = gamma[c] * m.rstd;
    scale[id] = ga;
    shift[id] = beta[c] - (float)m.mean * ga;
}

extern "C" int mnet_groupnorm_affine(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c,
                                     const int32_t* valid_w, const float* gamma, const float* beta, float eps,
                                     double* partial, int32_t slices, float* scale, float* shift, void* stream) {
    MNET_CHECK_ARG(x && gamma && beta && partial && scale && shift, "groupnorm: null pointer");
    MNET_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0 && slices > 0 && n <= 65535, "groupnorm: bad geometry");
    MNET_CHECK_ARG(is_storage(dtype), "groupnorm: bad dtype");
    const int N = chunk_n(dtype);
    MNET_CHECK_ALIGN(c % 32 == 0 && 256 % (c / N) == 0 && aligned16(x), "groupnorm: c=%d unsupported", c);
    MNET_CHECK_ALIGN(!is_split4(dtype) || aligned128(x), "groupnorm: split-half tensors must be 128-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_storage(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(gn_partial_kernel<T>, dim3(slices, n), dim3(256), 0, st, (const T*)x, h, w, c, valid_w, partial, slices);
    });
    MNET_LAUNCH_CHECK("gn_partial");
    const int tot = n * c;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, partial, slices, n, h, w, c,
                       valid_w, gamma, beta, eps, scale, shift);
    MNET_LAUNCH_CHECK("gn_finalize");
    return MNET_OK;
}

// ---------------------------------------------------------------------------- the same affine from epilogue partial sums (round 5)
// partial[(n * frags + f) * G + g] = (sum, sum of squares) of fragment f (32 consecutive pixels) x group g, written by the producing convolution's
// epilogue (mnet_conv_desc.gn_partial).  One wave per (group, image): lane l folds fragments l, l + 64, ... in fp64, then a fixed butterfly.
// `ring` (or nullptr): fp64 [n][G][2] sums the fragments leave out — the hi-res ring of a polyphase convolution's output, summed by polyphase_ring_kernel.
__global__ void __launch_bounds__(64) gn_finalize_frag_kernel(const float* __restrict__ partial, const double* __restrict__ ring, int frags, int H, int W, int C,
                                                              const int* __restrict__ valid_w, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, float* __restrict__ scale,
                                                              float* __restrict__ shift) {
    const int g = blockIdx.x, n = blockIdx.y, lane = threadIdx.x, G = C / 32;
    const f32x2* pp = reinterpret_cast<const f32x2*>(partial) + (size_t)n * frags * G + g;
    double S = 0.0, SS = 0.0;
    for (int f = lane; f < frags; f += 64) { const f32x2 v = pp[(size_t)f * G]; S += (double)v[0]; SS += (double)v[1]; }
    S = wave_sum_d(S); SS = wave_sum_d(SS);
    if (ring) { S += ring[((size_t)n * G + g) * 2]; SS += ring[((size_t)n * G + g) * 2 + 1]; }
    const int vw = valid_w ? min(valid_w[n], W) : W;
    const MeanRstd m = gn_mean_rstd(S, SS, (double)H * vw * 32.0, eps);
    if (lane < 32) {
        const int c = g * 32 + lane;
        const float ga = gamma[c] * m.rstd;
        scale[(size_t)n * C + c] = ga;
        shift[(size_t)n * C + c] = beta[c] - (float)m.mean * ga;
    }
}

extern "C" int mnet_groupnorm_affine_from_partial(const float* partial, int32_t n, int32_t h, int32_t w, int32_t c, const int32_t* valid_w,
                                                  const float* gamma, const float* beta, float eps, float* scale, float* shift, void* stream) {
    MNET_CHECK_ARG(partial && gamma && beta && scale && shift, "groupnorm_from_partial: null pointer");
    MNET_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && c > 0 && c % 32 == 0 && (h * w) % 32 == 0, "groupnorm_from_partial: bad geometry (c %% 32, h*w %% 32)");
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(partial) & 7u) == 0, "groupnorm_from_partial: partial must be 8-byte aligned");
    hipLaunchKernelGGL(gn_finalize_frag_kernel, dim3(c / 32, n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), partial, (const double*)nullptr, h * w / 32, h, w, c,
                       valid_w, gamma, beta, eps, scale, shift);
    MNET_LAUNCH_CHECK("gn_finalize_frag");
    return MNET_OK;
}

// ---------------------------------------------------------------------------- ring fix-up of a polyphase conv3x3(bilinear x2) (MNET_CONV_ALGO_FLAG_SHUFFLE2)
// The polyphase form zero-pads at LOW resolution where conv(up(x)) clamps the up-sample and zero-pads at hi resolution: hi-res rows and columns {0, 1, last two} of y
// differ.  The caller runs the two-launch form on four thin strips (low-res rows 0..1 / H-2..H-1, columns 0..1 / W-2..W-1) and this kernel copies their ring parts over y:
//     top    [n,4,W2,c]: rows 0..1            → y rows 0..1           bottom [n,4,W2,c]: rows 2..3    → y rows H2-2..H2-1     (all columns: the corners)
//     left   [n,H2,4,c]: columns 0..1         → y columns 0..1        right  [n,H2,4,c]: columns 2..3 → y columns W2-2..W2-1  (rows 2..H2-3)
// and sums what it stores, in fp64, per (image, 32-channel group): sums[n][c/32][2], the part of the GroupNorm statistics the main launch's epilogue leaves out.
// Grid (c/32, n); thread t takes ring pixels t, t + 256, ... of its group's 128-byte block; a fixed fold (butterfly per wave, then the four waves in order).
__global__ void __launch_bounds__(256) polyphase_ring_kernel(const unsigned char* __restrict__ top, const unsigned char* __restrict__ bottom,
                                                             const unsigned char* __restrict__ left, const unsigned char* __restrict__ right,
                                                             unsigned char* __restrict__ y, int H2, int W2, int C, double* __restrict__ sums) {
    __shared__ double red[4][2];
    const int g = blockIdx.x, n = blockIdx.y, G = C / 32, t = threadIdx.x;
    const size_t px = (size_t)C * 4;                                    // bytes per pixel (fp16+8: 128 per 32-channel block)
    const int nrow = 4 * W2, R = nrow + 4 * (H2 - 4);
    double S = 0.0, SS = 0.0;
    for (int r = t; r < R; r += 256) {
        const unsigned char* src;
        int row, col;
        if (r < nrow) {
            const int bot = r >= 2 * W2, q = r - bot * 2 * W2, sr = q / W2;
            col = q - sr * W2;
            row = bot ? H2 - 2 + sr : sr;
            src = (bot ? bottom : top) + (((size_t)n * 4 + (bot ? 2 + sr : sr)) * W2 + col) * px;
        } else {
            const int q = r - nrow, ci = q & 3;
            row = 2 + (q >> 2);
            col = ci < 2 ? ci : W2 - 4 + ci;
            src = (ci < 2 ? left : right) + (((size_t)n * H2 + row) * 4 + ci) * px;
        }
        src += (size_t)g * 128;
        unsigned char* dst = y + (((size_t)n * H2 + row) * W2 + col) * px + (size_t)g * 128;
        u32x4 b[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) b[k] = ldg16(src + k * 16);
#pragma unroll
        for (int k = 0; k < 8; ++k) stg16(dst + k * 16, b[k]);
        const float sl = hm_lo_scale((int)(b[6][0] & 255u));
        float a = 0.f, q2 = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                   // lo bytes of chunk c: 8-byte slot hm_lo_slot(c) of the block's bytes 64..95
            const int slot = hm_lo_slot(c);
            float v[8];
            hm_decode8(b[c], u32x2{b[4 + (slot >> 1)][2 * (slot & 1)], b[4 + (slot >> 1)][2 * (slot & 1) + 1]}, sl, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) { a += v[j]; q2 = fmaf(v[j], v[j], q2); }
        }
        S += (double)a; SS += (double)q2;
    }
    S = wave_sum_d(S); SS = wave_sum_d(SS);
    if ((t & 63) == 0) { red[t >> 6][0] = S; red[t >> 6][1] = SS; }
    __syncthreads();
    if (t == 0) {
        double* o = sums + ((size_t)n * G + g) * 2;
        o[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        o[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
}

extern "C" int mnet_polyphase_ring_fix(const void* top, const void* bottom, const void* left, const void* right, void* y, int32_t dtype,
                                       int32_t n, int32_t h2, int32_t w2, int32_t c, double* sums, void* stream) {
    MNET_CHECK_ARG(top && bottom && left && right && y && sums, "polyphase_ring_fix: null pointer");
    MNET_CHECK_ARG(dtype == MNET_F16M, "polyphase_ring_fix: MNET_F16M tensors only");
    MNET_CHECK_ARG(n > 0 && n <= 65535 && h2 >= 8 && w2 >= 8 && h2 % 2 == 0 && w2 % 2 == 0 && c > 0 && c % 32 == 0, "polyphase_ring_fix: bad geometry (hi-res h, w even and >= 8, c %% 32)");
    MNET_CHECK_ARG(4ll * w2 + 4ll * h2 < (1ll << 30), "polyphase_ring_fix: map too large");
    MNET_CHECK_ALIGN(aligned128(top) && aligned128(bottom) && aligned128(left) && aligned128(right) && aligned128(y) && (reinterpret_cast<uintptr_t>(sums) & 7u) == 0,
                     "polyphase_ring_fix: tensors must be 128-byte aligned, sums 8-byte aligned");
    hipLaunchKernelGGL(polyphase_ring_kernel, dim3(c / 32, n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (const unsigned char*)top, (const unsigned char*)bottom,
                       (const unsigned char*)left, (const unsigned char*)right, (unsigned char*)y, h2, w2, c, sums);
    MNET_LAUNCH_CHECK("polyphase_ring");
    return MNET_OK;
}

// mnet_groupnorm_affine_from_partial of a polyphase convolution's output [n,h,w,c] (hi-res): the epilogue's partial sums (ring left out) + the ring's fp64 sums
extern "C" int mnet_groupnorm_affine_from_partial_ring(const float* partial, const double* ring_sums, int32_t n, int32_t h, int32_t w, int32_t c,
                                                       const float* gamma, const float* beta, float eps, float* scale, float* shift, void* stream) {
    MNET_CHECK_ARG(partial && ring_sums && gamma && beta && scale && shift, "groupnorm_from_partial_ring: null pointer");
    MNET_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && c > 0 && c % 32 == 0 && (h * w) % 128 == 0, "groupnorm_from_partial_ring: bad geometry (c %% 32, h*w %% 128)");
    MNET_CHECK_ALIGN((reinterpret_cast<uintptr_t>(partial) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ring_sums) & 7u) == 0, "groupnorm_from_partial_ring: buffers must be 8-byte aligned");
    hipLaunchKernelGGL(gn_finalize_frag_kernel, dim3(c / 32, n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), partial, ring_sums, h * w / 32, h, w, c,
                       (const int*)nullptr, gamma, beta, eps, scale, shift);
    MNET_LAUNCH_CHECK("gn_finalize_frag");
    return MNET_OK;
}

// ============================================================================ AdaIN + crop + concat (per glyph)
// Two forms of one computation, both compositions of the pieces below.  Fused (adain_crop_kernel): one workgroup per glyph; pass 1: fp64 sums of the
// prior crop and the feature crop per channel; pass 2: write [S,S,2C] (zeros beyond the glyph's width).  In three launches for few glyphs: further down.
// The statistics [4][C] (pm, ps, fm, fs) sit behind a pointer: LDS in the fused kernel, `stat_g` in the three-launch form.

// what a thread knows of its glyph: the window, and its own chunk column ch and pixel lane pl among the 256 threads
template <typename T>
struct AdainWin {
    const T* pbase; const T* fbase;                 // row 0 of the glyph's prior [G,S,S,C] and of its image's feature map [B,S,FW,C], at this thread's chunk
    int S, C, FW, x1, y1, gw, cpp, plane, ch, pl, t;
    __device__ __forceinline__ AdainWin(const T* prior, const T* feat, int S_, int C_, int FW_, const int* g_img, const int* g_x1, const int* g_y1,
                                        const int* g_w, int g, int t_) {
        constexpr int N = Vec<T>::N;
        S = S_; C = C_; FW = FW_; t = t_;
        cpp = C / N; plane = 256 / cpp; ch = t % cpp; pl = t / cpp;
        const int img = g_img[g];
        x1 = g_x1[g]; y1 = g_y1[g]; gw = g_w[g];
        pbase = prior + (size_t)g * S * S * C + (size_t)ch * N;
        fbase = feat + (size_t)img * S * FW * C + (size_t)ch * N;
    }
};

// accumulate: this thread's fp64 sums over its lane's pixels of slice sl (of `slices`) of the window -> red[256][N][4] (sum, sum of squares of the prior, of the feature).
// The sums are taken of (value - pivot), the pivot being the channel's value at the window's first pixel: a channel whose mean is 1e4 times its spread
// loses 8 digits in sum(x^2) - n mean^2 otherwise, and the fused and the three-launch form (other association) then differ by ulps of fp32 in the std.
// own_piv: this thread hands the pivots on in stat[c] / stat[2C + c] (stat [4][C]), the slots adain_channel_stats overwrites with the means — before the
// loop, so that only their fp64 forms stay in registers across it.
template <typename T>
__device__ __forceinline__ void adain_accumulate(const AdainWin<T>& w, int sl, int slices, double* red, float* stat, bool own_piv) {
    constexpr int N = Vec<T>::N;
    const int C = w.C;
    const T *pbase = w.pbase, *fbase = w.fbase;
    const int npx = w.S * w.gw, per = (npx + slices - 1) / slices;
    const int p_end = min(npx, (sl + 1) * per);
    float pk[N], fk[N];
    unpackr<T>(ldraw<T>(pbase + (size_t)w.y1 * C), pk);
    unpackr<T>(ldraw<T>(fbase + (size_t)w.x1 * C), fk);
    if (own_piv) {
#pragma unroll
        for (int j = 0; j < N; ++j) { stat[w.ch * N + j] = pk[j]; stat[2 * C + w.ch * N + j] = fk[j]; }
    }
    // (vectors, not double[N]: what the compiler made of the arrays while this loop stood in the kernels; as arrays in a function of its own they become
    //  4 N scalars, which the vectoriser regroups with more registers in flight — adain_stats_kernel<hs> 128 VGPRs against 123)
    typedef double f64xN __attribute__((ext_vector_type(N)));
    f64xN ps_ = 0.0, pss = 0.0, fs_ = 0.0, fss = 0.0;
    for (int p = sl * per + w.pl; p < p_end; p += w.plane) {
        const int y = p / w.gw, x = p - y * w.gw;
        float a[N], b[N];
        unpackr<T>(ldraw<T>(pbase + ((size_t)y * w.S + (w.y1 + x)) * C), a);
        unpackr<T>(ldraw<T>(fbase + ((size_t)y * w.FW + (w.x1 + x)) * C), b);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double da = (double)a[j] - (double)pk[j], db = (double)b[j] - (double)fk[j];     // exact
            ps_[j] += da; pss[j] += da * da;
            fs_[j] += db; fss[j] += db * db;
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double* r = red + ((size_t)w.t * N + j) * 4;
        r[0] = ps_[j]; r[1] = pss[j]; r[2] = fs_[j]; r[3] = fss[j];
    }
}

struct AdainSums { double a0, a1, b0, b1; };         // of one channel: sum, sum of squares of (prior - pivot); the same of the feature

// fold: the sums of channel c over its pixel lanes, in lane order
template <typename T>
__device__ __forceinline__ AdainSums adain_fold(const AdainWin<T>& w, const double* red, int c) {
    constexpr int N = Vec<T>::N;
    const int chn = c / N, j = c % N;
    AdainSums s = {0, 0, 0, 0};
    for (int q = 0; q < w.plane; ++q) {
        const double* r = red + ((size_t)(q * w.cpp + chn) * N + j) * 4;
        s.a0 += r[0]; s.a1 += r[1]; s.b0 += r[2]; s.b1 += r[3];
    }
    return s;
}

// channel statistics: the sums s of (value - pivot) over cnt pixels and the pivots in stat[c] / stat[2C + c] -> stat[c], [C + c], [2C + c], [3C + c] = prior
// mean, prior std, feature mean, feature std; gn: also gsum [2][2C], the sum / sum of squares of the [.., 2C] OUTPUT per channel over the window
__device__ __forceinline__ void adain_channel_stats(AdainSums s, double cnt, float* stat, int C, int c, double* gsum, bool gn) {
    const double pd = s.a0 / cnt, fd = s.b0 / cnt;                      // means of (value - pivot)
    const double pm = (double)stat[c] + pd, fm = (double)stat[2 * C + c] + fd;
    double pdev = s.a1 - cnt * pd * pd, fdev = s.b1 - cnt * fd * fd;    // sums of squared deviations from the mean
    if (pdev < 0) pdev = 0; if (fdev < 0) fdev = 0;
    // unbiased variance (torch .var default, networks.py:522) + eps 1e-5, then sqrt
    const double pv = pdev / (cnt - 1.0), fv = fdev / (cnt - 1.0);
    const float psd = sqrtf((float)pv + 1e-5f), fsd = sqrtf((float)fv + 1e-5f);
    stat[c] = (float)pm; stat[C + c] = psd; stat[2 * C + c] = (float)fm; stat[3 * C + c] = fsd;
    if (gn) {           // in closed form: channel c (restyled prior) = (p - pm)/ps*fs + fm → sum = cnt*fm, sumsq = r^2 * sum (p-pm)^2 + cnt*fm^2
                        // channel C + c (feature crop) = the accumulated sums themselves
        const double r = (double)fsd / (double)psd;
        gsum[c] = cnt * fm;            gsum[2 * C + c] = r * r * pdev + cnt * fm * fm;
        gsum[C + c] = cnt * fm;        gsum[3 * C + c] = fdev + cnt * fm * fm;
    }
}

// group affine: GroupNorm(2C/32 groups) of the concatenated output (networks.py:508: norm1 of conv_*_fuse) from gsum → gn_scale / gn_shift of glyph g.
// gmr [2C/32][2]: group mean, rstd (LDS, like gsum)
__device__ __forceinline__ void adain_group_affine(const double* gsum, float* gmr, int C, int npx, int g, int t, const float* gn_gamma, const float* gn_beta,
                                                   float gn_eps, float* gn_scale, float* gn_shift) {
    const int G2 = 2 * C / 32;
    for (int gq = t; gq < G2; gq += 256) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < 32; ++k) { s1 += gsum[gq * 32 + k]; s2 += gsum[2 * C + gq * 32 + k]; }
        const MeanRstd m = gn_mean_rstd(s1, s2, (double)npx * 32.0, gn_eps);
        gmr[2 * gq] = (float)m.mean; gmr[2 * gq + 1] = m.rstd;
    }
    __syncthreads();
    for (int c = t; c < 2 * C; c += 256) {
        const float ga = gn_gamma[c] * gmr[2 * (c / 32) + 1];
        gn_scale[(size_t)g * 2 * C + c] = ga;
        gn_shift[(size_t)g * 2 * C + c] = gn_beta[c] - gmr[2 * (c / 32)] * ga;
    }
}

// apply: this thread's lane of the pixels of slice sl (of `slices`) of the glyph's S x S x 2C output obase: the restyled prior, then the feature crop; zeros beyond gw
template <typename T>
__device__ __forceinline__ void adain_apply(const AdainWin<T>& w, const float* stat, T* obase, int sl, int slices) {
    constexpr int N = Vec<T>::N;
    const int C = w.C, S = w.S;
    const T *pbase = w.pbase, *fbase = w.fbase;
    const int c0 = w.ch * N;
    const int per = (S * S + slices - 1) / slices, p_end = min(S * S, (sl + 1) * per);
    for (int p = sl * per + w.pl; p < p_end; p += w.plane) {
        const int y = p / w.S, x = p - y * w.S;
        Raw<T> oa = zero_raw<T>(), ob = zero_raw<T>();
        if (x < w.gw) {
            float a[N], o[N];
            unpackr<T>(ldraw<T>(pbase + ((size_t)y * w.S + (w.y1 + x)) * C), a);
            ob = ldraw<T>(fbase + ((size_t)y * w.FW + (w.x1 + x)) * C);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int c = c0 + j;
                o[j] = (a[j] - stat[c]) / stat[C + c] * stat[3 * C + c] + stat[2 * C + c];
            }
            oa = packr<T>(o);
        }
        straw<T>(obase + (size_t)p * 2 * C + c0, oa);
        straw<T>(obase + (size_t)p * 2 * C + C + c0, ob);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) adain_crop_kernel(const T* __restrict__ prior, const T* __restrict__ feat,
                                                         T* __restrict__ out, int S, int C, int FW,
                                                         const int* __restrict__ g_img, const int* __restrict__ g_x1,
                                                         const int* __restrict__ g_y1, const int* __restrict__ g_w,
                                                         const float* __restrict__ gn_gamma, const float* __restrict__ gn_beta,
                                                         float gn_eps, float* __restrict__ gn_scale, float* __restrict__ gn_shift) {
    constexpr int N = Vec<T>::N;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int g = blockIdx.x, t = threadIdx.x;
    const AdainWin<T> w(prior, feat, S, C, FW, g_img, g_x1, g_y1, g_w, g, t);
    double* red = reinterpret_cast<double*>(dyn);                       // [256][N][4]  (only N*4 per thread)
    float* stat = reinterpret_cast<float*>(dyn + (size_t)256 * N * 4 * sizeof(double));   // [4][C]: pm, ps, fm, fs
    double* gsum = reinterpret_cast<double*>(stat + 4 * C);              // [2][2C]: per output channel sum, sum of squares
    float* gmr = reinterpret_cast<float*>(gsum + 4 * C);                 // [2C/32][2]: group mean, rstd
    const int npx = S * w.gw;
    adain_accumulate<T>(w, 0, 1, red, stat, w.pl == 0);
    __syncthreads();
    for (int c = t; c < C; c += 256) {      // thread c (< C) folds the pixel lanes of channel c
        adain_channel_stats(adain_fold<T>(w, red, c), (double)npx, stat, C, c, gsum, gn_scale != nullptr);
    }
    __syncthreads();
    if (gn_scale) adain_group_affine(gsum, gmr, C, npx, g, t, gn_gamma, gn_beta, gn_eps, gn_scale, gn_shift);
    adain_apply<T>(w, stat, out + (size_t)g * S * S * 2 * C, 0, 1);
}

static int adain_launch(const void* prior, const void* feat, void* out, int32_t dtype, int32_t G, int32_t S, int32_t C,
                        int32_t feat_w, const int32_t* g_img, const int32_t* g_x1, const int32_t* g_y1, const int32_t* g_w,
                        const float* gamma, const float* beta, float eps, float* scale, float* shift, void* stream) {
    MNET_CHECK_ARG(prior && feat && out && g_img && g_x1 && g_y1 && g_w, "adain: null pointer");
    MNET_CHECK_ARG(G > 0 && S > 0 && C > 0 && feat_w >= S, "adain: bad geometry");
    MNET_CHECK_ARG(is_storage(dtype), "adain: bad dtype");
    const int N = chunk_n(dtype);
    MNET_CHECK_ALIGN(C % N == 0 && 256 % (C / N) == 0 && C % 32 == 0 && aligned16(prior) && aligned16(feat) && aligned16(out),
                     "adain: C=%d unsupported or unaligned", C);
    MNET_CHECK_ALIGN(!is_split4(dtype) || (aligned128(prior) && aligned128(feat) && aligned128(out)), "adain: split-half tensors must be 128-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // (round 5: a form of this kernel with four pixels in flight per thread and a 16 KiB fold — three workgroups per CU instead of two, bit-identical —
    //  measured 24.2-24.9 ms per step against 23.2: the kernel is not latency-bound.  It reads the prior and the feature windows TWICE (statistics, then
    //  apply): 102 GB of real traffic per step in 18.8 ms = 5.4 TB/s, the copy ceiling of this chip; `roofline.hbm_tail` books the algorithmic 69 GB.)
    const size_t lds = (size_t)256 * N * 4 * sizeof(double) + (size_t)4 * C * sizeof(float) + (size_t)4 * C * sizeof(double) +
                       (size_t)(2 * C / 32) * 2 * sizeof(float);
    // a workgroup can have 160 KiB of LDS: C = 2048 in an 8-wide storage asks for 164,864 bytes — refused here, before any HIP call, like adain_split's lds2
    MNET_CHECK_ARG(lds <= 160 * 1024, "adain: C=%d too large (%zu bytes of LDS per workgroup, 163840 at most)", C, lds);
    dispatch_storage(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        // per instantiation, per thread, per device: the attribute is raised when a larger size is asked for, never lowered (and not during graph capture replays)
        static thread_local size_t lds_set[256] = {};
        size_t& have = lds_set[DeviceOnce::dev()];
        if (lds > have) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(adain_crop_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); have = lds; }
        hipLaunchKernelGGL(adain_crop_kernel<T>, dim3(G), dim3(256), lds, st, (const T*)prior, (const T*)feat, (T*)out, S, C, feat_w,
                           g_img, g_x1, g_y1, g_w, gamma, beta, eps, scale, shift);
    });
    MNET_LAUNCH_CHECK("adain_crop");
    return MNET_OK;
}

extern "C" int mnet_adain_crop_concat(const void* prior, const void* feat, void* out, int32_t dtype, int32_t G,
                                      int32_t S, int32_t C, int32_t feat_w, const int32_t* g_img,
                                      const int32_t* g_x1, const int32_t* g_y1, const int32_t* g_w, void* stream) {
    return adain_launch(prior, feat, out, dtype, G, S, C, feat_w, g_img, g_x1, g_y1, g_w, nullptr, nullptr, 0.f, nullptr, nullptr, stream);
}

extern "C" int mnet_adain_crop_concat_gn(const void* prior, const void* feat, void* out, int32_t dtype, int32_t G,
                                         int32_t S, int32_t C, int32_t feat_w, const int32_t* g_img,
                                         const int32_t* g_x1, const int32_t* g_y1, const int32_t* g_w,
                                         const float* gamma, const float* beta, float eps, float* scale, float* shift,
                                         void* stream) {
    MNET_CHECK_ARG(gamma && beta && scale && shift, "adain_gn: null pointer");
    return adain_launch(prior, feat, out, dtype, G, S, C, feat_w, g_img, g_x1, g_y1, g_w, gamma, beta, eps, scale, shift, stream);
}

// ---------------------------------------------------------------------------- the same in three launches for FEW glyphs
// One workgroup per glyph walks its window as a chain of exposed load latencies (≈380 us for a 64x64x256 window): fine when a
// thousand glyphs share the chip (batch 64: the kernel is HBM-bound), but a single strip has 16.  Here `slices` workgroups share
// a glyph: (1) per-slice fp64 partial sums, (2) one workgroup per glyph folds them in slice order into the AdaIN statistics and
// the GroupNorm affine, (3) `slices` workgroups write the output.  The arithmetic per element is the fused kernel's — the same functions; only the
// association of the fp64 sums differs (slice-major instead of lane-major), i.e. results agree to fp64 rounding of the sums.
template <typename T>
__global__ void __launch_bounds__(256) adain_stats_kernel(const T* __restrict__ prior, const T* __restrict__ feat, int S, int C, int FW,
                                                          const int* __restrict__ g_img, const int* __restrict__ g_x1,
                                                          const int* __restrict__ g_y1, const int* __restrict__ g_w,
                                                          double* __restrict__ partial, float* __restrict__ stat_g, int slices) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    double* red = reinterpret_cast<double*>(dyn);                       // [256][N][4]
    const int g = blockIdx.y, sl = blockIdx.x, t = threadIdx.x;
    const AdainWin<T> w(prior, feat, S, C, FW, g_img, g_x1, g_y1, g_w, g, t);
    // the pivots are the same for every slice of the glyph: slice 0 hands them to adain_finalize_kernel
    adain_accumulate<T>(w, sl, slices, red, stat_g + (size_t)g * 4 * C, sl == 0 && w.pl == 0);
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        const AdainSums s = adain_fold<T>(w, red, c);
        double* o = partial + (((size_t)g * slices + sl) * C + c) * 4;
        o[0] = s.a0; o[1] = s.a1; o[2] = s.b0; o[3] = s.b1;
    }
}

// one workgroup per glyph: stat[g][4][C] = (prior mean, prior std, feature mean, feature std) and the GroupNorm affine
__global__ void __launch_bounds__(256) adain_finalize_kernel(const double* __restrict__ partial, int slices, int S, int C,
                                                             const int* __restrict__ g_w, float* __restrict__ stat,
                                                             const float* __restrict__ gn_gamma, const float* __restrict__ gn_beta,
                                                             float gn_eps, float* __restrict__ gn_scale, float* __restrict__ gn_shift) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    double* gsum = reinterpret_cast<double*>(dyn);                       // [2][2C]
    float* gmr = reinterpret_cast<float*>(gsum + 4 * C);                 // [2C/32][2]
    const int g = blockIdx.x, t = threadIdx.x;
    const int npx = S * g_w[g];
    for (int c = t; c < C; c += 256) {
        AdainSums s = {0, 0, 0, 0};
        for (int sl = 0; sl < slices; ++sl) {
            const double* r = partial + (((size_t)g * slices + sl) * C + c) * 4;
            s.a0 += r[0]; s.a1 += r[1]; s.b0 += r[2]; s.b1 += r[3];
        }
        adain_channel_stats(s, (double)npx, stat + (size_t)g * 4 * C, C, c, gsum, gn_scale != nullptr);
    }
    if (!gn_scale) return;
    __syncthreads();
    adain_group_affine(gsum, gmr, C, npx, g, t, gn_gamma, gn_beta, gn_eps, gn_scale, gn_shift);
}

template <typename T>
__global__ void __launch_bounds__(256) adain_apply_kernel(const T* __restrict__ prior, const T* __restrict__ feat, T* __restrict__ out,
                                                          int S, int C, int FW, const int* __restrict__ g_img,
                                                          const int* __restrict__ g_x1, const int* __restrict__ g_y1,
                                                          const int* __restrict__ g_w, const float* __restrict__ stat_g, int slices) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    float* stat = reinterpret_cast<float*>(dyn);                         // [4][C]
    const int g = blockIdx.y, sl = blockIdx.x, t = threadIdx.x;
    const AdainWin<T> w(prior, feat, S, C, FW, g_img, g_x1, g_y1, g_w, g, t);
    for (int i = t; i < 4 * C; i += 256) stat[i] = stat_g[(size_t)g * 4 * C + i];
    __syncthreads();
    adain_apply<T>(w, stat, out + (size_t)g * S * S * 2 * C, sl, slices);
}

extern "C" int mnet_adain_crop_concat_split(const void* prior, const void* feat, void* out, int32_t dtype, int32_t G,
                                            int32_t S, int32_t C, int32_t feat_w, const int32_t* g_img,
                                            const int32_t* g_x1, const int32_t* g_y1, const int32_t* g_w,
                                            const float* gamma, const float* beta, float eps, float* scale, float* shift,
                                            double* partial, float* stat, int32_t slices, void* stream) {
    MNET_CHECK_ARG(prior && feat && out && g_img && g_x1 && g_y1 && g_w && partial && stat, "adain_split: null pointer");
    MNET_CHECK_ARG(G > 0 && G <= 65535 && S > 0 && C > 0 && feat_w >= S && slices > 0 && slices <= 1024, "adain_split: bad geometry");
    MNET_CHECK_ARG(is_storage(dtype), "adain_split: bad dtype");
    MNET_CHECK_ALIGN(!is_split4(dtype) || (aligned128(prior) && aligned128(feat) && aligned128(out)), "adain_split: split-half tensors must be 128-byte aligned");
    MNET_CHECK_ARG((gamma != nullptr) == (beta != nullptr) && (gamma != nullptr) == (scale != nullptr) && (gamma != nullptr) == (shift != nullptr),
                   "adain_split: gamma, beta, scale, shift go together");
    const int N = chunk_n(dtype);
    MNET_CHECK_ALIGN(C % N == 0 && 256 % (C / N) == 0 && C % 32 == 0 && aligned16(prior) && aligned16(feat) && aligned16(out),
                     "adain_split: C=%d unsupported or unaligned", C);
    const size_t lds1 = (size_t)256 * N * 4 * sizeof(double);
    const size_t lds2 = (size_t)4 * C * sizeof(double) + (size_t)(2 * C / 32) * 2 * sizeof(float);
    const size_t lds3 = (size_t)4 * C * sizeof(float);
    MNET_CHECK_ARG(lds2 <= 65536 && lds3 <= 65536, "adain_split: C=%d too large", C);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_storage(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        const T *p = (const T*)prior, *f = (const T*)feat;
        static thread_local DeviceOnce attr_once;      // per instantiation, per thread, per device: lds1 is a constant of T (64 KiB for the 8-wide storages)
        if (!attr_once.done()) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(adain_stats_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1); attr_once.mark(); }
        hipLaunchKernelGGL(adain_stats_kernel<T>, dim3(slices, G), dim3(256), lds1, st, p, f, S, C, feat_w, g_img, g_x1, g_y1, g_w, partial, stat, slices);
        MNET_LAUNCH_CHECK("adain_stats");
        hipLaunchKernelGGL(adain_finalize_kernel, dim3(G), dim3(256), lds2, st, partial, slices, S, C, g_w, stat, gamma, beta, eps, scale, shift);
        MNET_LAUNCH_CHECK("adain_finalize");
        hipLaunchKernelGGL(adain_apply_kernel<T>, dim3(slices, G), dim3(256), lds3, st, p, f, (T*)out, S, C, feat_w, g_img, g_x1, g_y1, g_w, stat, slices);
        MNET_LAUNCH_CHECK("adain_apply");
        return MNET_OK;
    });
}

// ============================================================================ ordered glyph scatter
// grid (x-chunks of one feature row, image): a thread owns one 16-byte channel chunk of one COLUMN; the glyph that owns the
// column (last glyph of the image whose window covers it) is looked up once and reused for all S rows
// fl(fl(a * b) + c): the reference's two PyTorch operations.  `__fadd_rn(__fmul_rn(a, b), c)` does NOT say that: the intrinsics are plain `*` / `+` to the
// compiler and were contracted into one v_fmac_f32 (a single rounding, an ulp away from the reference on ~1 element in 4); the pragma is what holds them apart
__device__ __forceinline__ float mul_add_unfused(float a, float b, float c) {
#pragma clang fp contract(off)
    const float m = a * b;
    return m + c;
}
#ifndef MNET_SCATTER_RUN
#define MNET_SCATTER_RUN 8
#endif
template <typename T>
__global__ void __launch_bounds__(256) glyph_scatter_kernel(const T* __restrict__ feat, const T* __restrict__ scale,
                                                            const T* __restrict__ shift, T* __restrict__ out,
                                                            int S, int C, int FW, const int* __restrict__ g_start,
                                                            const int* __restrict__ g_x1, const int* __restrict__ g_w) {
    constexpr int N = Vec<T>::N;
    const int cpp = C / N;
    const int b = blockIdx.y;
    const int id = blockIdx.x * 256 + threadIdx.x;                 // (x, ch) inside one row
    if (id >= FW * cpp) return;
    const int ch = id % cpp, x = id / cpp;
    int owner = -1, ox = 0;
    for (int gg = g_start[b + 1] - 1; gg >= g_start[b]; --gg) {    // last writer wins
        const int x1 = g_x1[gg];
        if (x >= x1 && x < x1 + g_w[gg]) { owner = gg; ox = x - x1; break; }
    }
    const size_t row = (size_t)FW * C;
    const T* fp = feat + (size_t)b * S * row + (size_t)id * N;
    T* op = out + (size_t)b * S * row + (size_t)id * N;
    // round 6: grid.z = runs of MNET_SCATTER_RUN rows — a thread walked all S rows of its column in a rolled loop (one row's loads in flight per thread, 5.1 TB/s where a
    // one-trip stream of this storage does 5.9); now SCATTER_RUN rows per thread, unrolled, every row's loads requested before the first use
    constexpr int R = MNET_SCATTER_RUN;
    const int y0 = (int)blockIdx.z * R;
    if (owner < 0) {
        Raw<T> raw[R];
#pragma unroll
        for (int k = 0; k < R; ++k) if (y0 + k < S) raw[k] = ldraw<T>(fp + (size_t)(y0 + k) * row);
#pragma unroll
        for (int k = 0; k < R; ++k) if (y0 + k < S) straw<T>(op + (size_t)(y0 + k) * row, raw[k]);
        return;
    }
    const size_t go = ((size_t)owner * S * S + ox) * C + (size_t)ch * N;     // + y*S*C per row
    Raw<T> rf[R], rs[R], rh[R];
#pragma unroll
    for (int k = 0; k < R; ++k)
        if (y0 + k < S) {
            rf[k] = ldraw<T>(fp + (size_t)(y0 + k) * row);
            rs[k] = ldraw<T>(scale + go + (size_t)(y0 + k) * S * C);
            rh[k] = ldraw<T>(shift + go + (size_t)(y0 + k) * S * C);
        }
#pragma unroll
    for (int k = 0; k < R; ++k)
        if (y0 + k < S) {
            float f[N], sc[N], sh[N], o[N];
            unpackr<T>(rf[k], f); unpackr<T>(rs[k], sc); unpackr<T>(rh[k], sh);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float r = mul_add_unfused(f[j], sc[j], sh[j]);         // res = f*scale + shift  (:448)
                o[j] = __fadd_rn(f[j], r);                                    // ori + res             (:449)
            }
            straw<T>(op + (size_t)(y0 + k) * row, packr<T>(o));
        }
}

extern "C" int mnet_glyph_scatter_affine(const void* feat, const void* scale, const void* shift, void* out,
                                         int32_t dtype, int32_t B, int32_t S, int32_t C, int32_t feat_w,
                                         const int32_t* g_start, const int32_t* g_x1, const int32_t* g_w, void* stream) {
    MNET_CHECK_ARG(feat && scale && shift && out && g_start && g_x1 && g_w, "scatter: null pointer");
    MNET_CHECK_ARG(B > 0 && S > 0 && C > 0 && feat_w > 0, "scatter: bad geometry");
    MNET_CHECK_ARG(is_storage(dtype), "scatter: bad dtype");
    const int N = chunk_n(dtype);
    MNET_CHECK_ALIGN(!is_split4(dtype) || (C % 32 == 0 && aligned128(feat) && aligned128(scale) && aligned128(shift) && aligned128(out)),
                     "scatter: split-half needs C %% 32 == 0, 128-byte aligned");
    MNET_CHECK_ALIGN(C % N == 0 && aligned16(feat) && aligned16(scale) && aligned16(shift) && aligned16(out),
                     "scatter: unaligned");
    MNET_CHECK_ARG(B <= 65535, "scatter: too many images");
    const int blocks = (int)(((long long)feat_w * (C / N) + 255) / 256);
    const int runs = (S + MNET_SCATTER_RUN - 1) / MNET_SCATTER_RUN;
    MNET_CHECK_ARG(runs <= 65535, "scatter: S too large");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_storage(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(glyph_scatter_kernel<T>, dim3(blocks, B, runs), dim3(256), 0, st, (const T*)feat, (const T*)scale, (const T*)shift, (T*)out, S, C, feat_w,
                           g_start, g_x1, g_w);
    });
    MNET_LAUNCH_CHECK("glyph_scatter");
    return MNET_OK;
}

// ============================================================================ SelectText gather
template <typename T>
__global__ void __launch_bounds__(256) embed_gather_kernel(const float* __restrict__ emb, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ scale, T* __restrict__ out, int nc, int C,
                                                           long long total_chunks) {
    constexpr int N = Vec<T>::N;
    const int cpp = C / N;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total_chunks;
         id += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(id % cpp);
        long long pix = id / cpp;                 // pixel in [N,4,4*nc]
        const int x = (int)(pix % (4 * nc));
        const int i = (int)(pix / (16 * nc));
        const int64_t lab = labels[(size_t)i * nc + x / 4];
        const float* e = emb + (size_t)lab * C + (size_t)ch * N;
        float v[N];
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = e[j];
        if (scale) {                              // per-(sample, channel) factor: the first StyledConv's modulation, applied before the storage rounding
            const float* sp = scale + (size_t)i * C + (size_t)ch * N;
#pragma unroll
            for (int j = 0; j < N; ++j) v[j] *= sp[j];
        }
        straw<T>(out + (size_t)id * N, packr<T>(v));
    }
}

extern "C" int mnet_embed_gather_scaled(const float* emb, const int64_t* labels, const float* scale, void* out, int32_t dtype, int32_t N_,
                                        int32_t nc, int32_t C, int32_t num_classes, void* stream) {
    MNET_CHECK_ARG(emb && labels && out && N_ > 0 && nc > 0 && C > 0 && num_classes > 0, "embed_gather: bad args");
    MNET_CHECK_ALIGN(aligned16(scale), "embed_gather: unaligned scale");
    MNET_CHECK_ARG(is_storage(dtype), "embed_gather: bad dtype");
    const int N = chunk_n(dtype);
    MNET_CHECK_ALIGN(C % N == 0 && aligned16(out), "embed_gather: unaligned");
    MNET_CHECK_ALIGN(!is_split4(dtype) || (C % 32 == 0 && aligned128(out)), "embed_gather: split-half needs C %% 32 == 0, 128-byte aligned");
    const long long total = (long long)N_ * 16 * nc * (C / N);
    const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_storage(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(embed_gather_kernel<T>, dim3(blocks), dim3(256), 0, st, emb, labels, scale, (T*)out, nc, C, total);
    });
    MNET_LAUNCH_CHECK("embed_gather");
    return MNET_OK;
}

extern "C" int mnet_embed_gather(const float* emb, const int64_t* labels, void* out, int32_t dtype, int32_t N_,
                                 int32_t nc, int32_t C, int32_t num_classes, void* stream) {
    return mnet_embed_gather_scaled(emb, labels, nullptr, out, dtype, N_, nc, C, num_classes, stream);
}

// ============================================================================ PixelNorm (one wave per row)
__global__ void __launch_bounds__(256) pixelnorm_kernel(const float* __restrict__ x, float* __restrict__ y, int N_, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N_) return;
    const float* xr = x + (size_t)row * D;
    float s = 0.f;
    for (int i = lane; i < D; i += 64) s += xr[i] * xr[i];
    s = wave_sum(s);
    const float r = rsqrtf(s / (float)D + 1e-8f);
    for (int i = lane; i < D; i += 64) y[(size_t)row * D + i] = xr[i] * r;
}

extern "C" int mnet_pixelnorm(const float* x, float* y, int32_t N_, int32_t D, void* stream) {
    MNET_CHECK_ARG(x && y && N_ > 0 && D > 0, "pixelnorm: bad args");
    hipLaunchKernelGGL(pixelnorm_kernel, dim3((N_ + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, y, N_, D);
    MNET_LAUNCH_CHECK("pixelnorm");
    return MNET_OK;
}

// ============================================================================ demodulation
// block per sample n: s^2 staged in LDS, thread o walks i with coalesced reads of wsq_t[i][o]
// grid (cout/64, styles): a workgroup owns 64 output channels of one style; its 4 waves each sum one quarter of cin (the loop
// is a chain of exposed load latencies — 16 loads are kept in flight per lane), folded in fixed order through LDS.
__global__ void __launch_bounds__(256) demod_kernel(const float* __restrict__ style, const float* __restrict__ wsq_t,
                                                    float* __restrict__ demod, int cin, int cout, const float* __restrict__ eps_scale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    float* s2 = reinterpret_cast<float*>(dyn);                  // [cin] squared style
    __shared__ float part[4][64];
    const int n = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int o = blockIdx.x * 64 + lane, oc = min(o, cout - 1);
    for (int i = threadIdx.x; i < cin; i += 256) { const float s = style[(size_t)n * cin + i]; s2[i] = s * s; }
    __syncthreads();
    const int per = (cin + 3) >> 2, i0 = q * per, i1 = min(cin, i0 + per);
    const float* wp = wsq_t + oc;
    float acc = 0.f;
    int i = i0;
    for (; i + 16 <= i1; i += 16) {
        float w[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) w[u] = wp[(size_t)(i + u) * cout];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = fmaf(s2[i + u], w[u], acc);
    }
    for (; i < i1; ++i) acc = fmaf(s2[i], wp[(size_t)i * cout], acc);
    part[q][lane] = acc;
    __syncthreads();
    // eps_scale[n] = 4^-e when the style row was normalised by 2^-e (mnet_style_rows): rsqrt(4^-e (S + 1e-8)) = 2^e rsqrt(S + 1e-8), exactly
    const float eps = eps_scale ? 1e-8f * eps_scale[n] : 1e-8f;
    if (q == 0 && o < cout) demod[(size_t)n * cout + o] = rsqrtf(((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) + eps);
}

extern "C" int mnet_demod_scaled(const float* style, const float* wsq_t, float* demod, int32_t N_, int32_t cin,
                                 int32_t cout, const float* eps_scale, void* stream) {
    MNET_CHECK_ARG(style && wsq_t && demod && N_ > 0 && cin > 0 && cout > 0 && N_ <= 65535, "demod: bad args");
    MNET_CHECK_ARG((size_t)cin * sizeof(float) <= 65536, "demod: cin=%d too large (the squared style row is staged in 64 KiB of LDS)", cin);
    hipLaunchKernelGGL(demod_kernel, dim3((cout + 63) / 64, N_), dim3(256), (size_t)cin * sizeof(float), reinterpret_cast<hipStream_t>(stream),
                       style, wsq_t, demod, cin, cout, eps_scale);
    MNET_LAUNCH_CHECK("demod");
    return MNET_OK;
}

extern "C" int mnet_demod(const float* style, const float* wsq_t, float* demod, int32_t N_, int32_t cin,
                          int32_t cout, void* stream) {
    return mnet_demod_scaled(style, wsq_t, demod, N_, cin, cout, nullptr, stream);
}

// ============================================================================ dtype conversion (flat)
// 8 logical elements per thread-iteration (one chunk of f16 / split-half, two chunks of f32).  Split-half tensors are
// channel-minor with C % 32 == 0, so their 32-element blocks tile the flat index space too.
template <typename T> __device__ __forceinline__ void ld8(const T* p, float* v) { unpackr<T>(ldraw<T>(p), v); }
template <> __device__ __forceinline__ void ld8<float>(const float* p, float* v) { Vec<float>::unpack(ldg16(p), v); Vec<float>::unpack(ldg16(p + 4), v + 4); }
template <typename T> __device__ __forceinline__ void st8(T* p, const float* v) { straw<T>(p, packr<T>(v)); }
template <> __device__ __forceinline__ void st8<float>(float* p, const float* v) { stg16(p, Vec<float>::pack(v)); stg16(p + 4, Vec<float>::pack(v + 4)); }

template <typename S, typename D>
__global__ void __launch_bounds__(256) convert_kernel(const S* __restrict__ src, D* __restrict__ dst, long long n8) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
        float v[8];
        ld8<S>(src + i * 8, v);
        st8<D>(dst + i * 8, v);
    }
}

extern "C" int mnet_convert(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t count, void* stream) {
    MNET_CHECK_ARG(src && dst && count > 0 && count % 8 == 0, "convert: bad args (count %% 8 == 0)");
    MNET_CHECK_ARG(is_storage(src_dtype) && is_storage(dst_dtype), "convert: bad dtype");
    MNET_CHECK_ALIGN(aligned16(src) && aligned16(dst), "convert: unaligned pointer");
    MNET_CHECK_ALIGN((!is_split4(src_dtype) || aligned128(src)) && (!is_split4(dst_dtype) || aligned128(dst)) &&
                     ((!is_split4(src_dtype) && !is_split4(dst_dtype)) || count % 32 == 0),
                     "convert: split-half tensors need count %% 32 == 0 and a 128-byte aligned base");
    const long long n8 = count / 8;
    const int blocks = (int)((n8 + 255) / 256 < 16384 ? (n8 + 255) / 256 : 16384);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_storage(src_dtype, [&](auto stag) {
        dispatch_storage(dst_dtype, [&](auto dtag) {
            using S = typename decltype(stag)::type;
            using D = typename decltype(dtag)::type;
            hipLaunchKernelGGL((convert_kernel<S, D>), dim3(blocks), dim3(256), 0, st, (const S*)src, (D*)dst, n8);
        });
    });
    MNET_LAUNCH_CHECK("convert");
    return MNET_OK;
}

// ============================================================================ fused bias + LeakyReLU (standalone op)
// The operator boundary the reference already has: basicsr.ops.fused_act.fused_leaky_relu(input, bias, 0.2, sqrt2)
// on a contiguous fp32 [N,C,inner] tensor (upstream kernel: x += b[(i/inner) % C]; y = x>0?x:alpha*x; out = y*scale).
// On the hot path this math lives in the conv epilogue; this entry point exists so that
// `from basicsr.ops.fused_act import fused_leaky_relu, FusedLeakyReLU` can be served without basicsr.
__global__ void __launch_bounds__(256) fused_bias_act_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                             float* __restrict__ y, long long total, int C, int inner,
                                                             float slope, float scale) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        float v = x[i];
        if (bias) v += bias[(i / inner) % C];
        v = v > 0.f ? v : v * slope;
        y[i] = v * scale;
    }
}

extern "C" int mnet_fused_bias_act(const float* x, const float* bias, float* y, int64_t total, int32_t C, int32_t inner,
                                   float negative_slope, float scale, void* stream) {
    MNET_CHECK_ARG(x && y && total > 0 && C > 0 && inner > 0, "fused_bias_act: bad args");
    const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(fused_bias_act_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, bias, y,
                       (long long)total, C, inner, negative_slope, scale);
    MNET_LAUNCH_CHECK("fused_bias_act");
    return MNET_OK;
}

// ============================================================================ per-(n,c) affine (+ swish), elementwise
// grid: x covers the chunks of ONE image, PPT chunks per thread 256 apart (256 % chunks-per-pixel == 0: a thread always lands on the same channel chunk, its 2x8
// scale / shift values are loaded once); y = image.
// Round 6: ONE trip per thread (the grid was capped at 1024 workgroups per image: 8 trips on the SR-size maps, 5.0-5.4 TB/s; uncapped 5.9 on the same box — the rate of a
// one-trip copy with this storage's half-line pattern, tools/microbench/stream_variants.hip), and PPT = 2 chunks per thread — both loads requested before the first
// use — where a pixel has >= 128 chunks (C = 1024, the fuse blocks' concatenated map): there the 64 bytes of scale / shift per thread are as many bytes again as the chunk
// itself: 4.7 -> 5.3 TB/s; on every smaller C one chunk per thread measured the same or better, 4 per thread worse everywhere (tools/experiments/gn_apply_shapes.py).
template <typename T, int PPT>
__global__ void __launch_bounds__(256) affine_act_kernel(const T* __restrict__ x, T* __restrict__ y, int C,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         int swish, unsigned chunks_per_image) {
    constexpr int N = Vec<T>::N;
    const unsigned cpp = (unsigned)C / N;
    const int n = blockIdx.y;
    const unsigned first = blockIdx.x * (256u * PPT) + threadIdx.x;
    const unsigned ch = first % cpp;
    float sc[N], sh[N];
    const size_t so = (size_t)n * C + (size_t)ch * N;
#pragma unroll
    for (int j = 0; j < N; j += 4) {
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(scale + so + j);
        f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
        if (shift) b4 = *reinterpret_cast<const f32x4*>(shift + so + j);
        sc[j] = a4[0]; sc[j + 1] = a4[1]; sc[j + 2] = a4[2]; sc[j + 3] = a4[3];
        sh[j] = b4[0]; sh[j + 1] = b4[1]; sh[j + 2] = b4[2]; sh[j + 3] = b4[3];
    }
    const T* xb = x + (size_t)n * chunks_per_image * N;
    T* yb = y + (size_t)n * chunks_per_image * N;
    Raw<T> r[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const unsigned id = first + 256u * k;
        r[k] = id < chunks_per_image ? ldraw<T>(xb + (size_t)id * N) : zero_raw<T>();      // (a quad of lanes shares a block: all four in range or none — per % 4 == 0)
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const unsigned id = first + 256u * k;
        float v[N];
        unpackr<T>(r[k], v);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float t = v[j] * sc[j] + sh[j];
            if (swish) t = t * __builtin_amdgcn_rcpf(1.f + __expf(-t));       // v_exp_f32 / v_rcp_f32: ~1 ulp each
            v[j] = t;
        }
        const Raw<T> o = packr<T>(v);
        if (id < chunks_per_image) straw<T>(yb + (size_t)id * N, o);
    }
}

template <typename T>
static void affine_act_launch(const void* x, void* y, int n, int c, long long per, const float* scale, const float* shift, int swish, hipStream_t st) {
    constexpr int N = Vec<T>::N;
    static const int env_ppt = [] { const char* e = getenv("MNET_AFFINE_PPT"); return e ? atoi(e) : 0; }();      // A/B: 1, 2 or 4 for every launch
    const int ppt = env_ppt == 1 || env_ppt == 2 || env_ppt == 4 ? env_ppt : (c / N >= 128 ? 2 : 1);
    const int gx = (int)((per + 256 * ppt - 1) / (256 * ppt));
    if (ppt == 4) hipLaunchKernelGGL((affine_act_kernel<T, 4>), dim3(gx, n), dim3(256), 0, st, (const T*)x, (T*)y, c, scale, shift, swish, (unsigned)per);
    else if (ppt == 2) hipLaunchKernelGGL((affine_act_kernel<T, 2>), dim3(gx, n), dim3(256), 0, st, (const T*)x, (T*)y, c, scale, shift, swish, (unsigned)per);
    else hipLaunchKernelGGL((affine_act_kernel<T, 1>), dim3(gx, n), dim3(256), 0, st, (const T*)x, (T*)y, c, scale, shift, swish, (unsigned)per);
}

extern "C" int mnet_affine_act_nhwc(const void* x, void* y, int32_t dtype, int32_t n, int32_t hw, int32_t c,
                                    const float* scale, const float* shift, int32_t swish, void* stream) {
    MNET_CHECK_ARG(x && y && scale && n > 0 && hw > 0 && c > 0 && n <= 65535, "affine_act: bad args");
    MNET_CHECK_ARG(is_storage(dtype), "affine_act: bad dtype");
    const int N = chunk_n(dtype);
    const long long per = (long long)hw * (c / N);
    MNET_CHECK_ARG(per < (1ll << 31), "affine_act: image too large");
    MNET_CHECK_ALIGN(!is_split4(dtype) || (c % 32 == 0 && aligned128(x) && aligned128(y)), "affine_act: split-half needs c %% 32 == 0, 128-byte aligned");
    MNET_CHECK_ALIGN(c % N == 0 && 256 % (c / N) == 0 && aligned16(x) && aligned16(y) && aligned16(scale) && aligned16(shift),
                     "affine_act: c=%d unsupported or unaligned", c);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_storage(dtype, [&](auto tag) { affine_act_launch<typename decltype(tag)::type>(x, y, n, c, per, scale, shift, swish, st); });
    MNET_LAUNCH_CHECK("affine_act");
    return MNET_OK;
}

// ============================================================================ K19: SR output post-processing (test_sr.py:198-200)
//   sr*0.5 + 0.5 → HWC → RGB→BGR flip → clip(0,1) * 255     as float32 (what the script hands to cv2) or as uint8 with
//   cv2.imwrite's float→uchar conversion (round half to even, saturate).  src NHWC [n, hw, c_ld] (RGB in channels 0..2).
template <typename T, typename O>
__global__ void __launch_bounds__(256) sr_postprocess_kernel(const T* __restrict__ src, O* __restrict__ dst, long long npix, int c_ld) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
        const T* s = src + (size_t)i * c_ld;
        O* d = dst + (size_t)i * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = __fadd_rn(__fmul_rn((float)s[c], 0.5f), 0.5f);
            v = fminf(fmaxf(v, 0.f), 1.f) * 255.0f;
            if constexpr (sizeof(O) == 1) d[2 - c] = (O)__float2int_rn(v);       // 0..255 after the clip
            else d[2 - c] = (O)v;
        }
    }
}

extern "C" int mnet_sr_postprocess(const void* src, int32_t src_dtype, void* dst, int32_t dst_u8, int64_t npix, int32_t c_ld,
                                   void* stream) {
    MNET_CHECK_ARG(src && dst && npix > 0 && c_ld >= 3, "sr_postprocess: bad args");
    MNET_CHECK_ARG(is_f16_f32(src_dtype), "sr_postprocess: bad dtype");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int grid = (int)((npix + 255) / 256 < 65536 ? (npix + 255) / 256 : 65536);
    dispatch_f16_f32(src_dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (dst_u8) hipLaunchKernelGGL((sr_postprocess_kernel<T, unsigned char>), dim3(grid), dim3(256), 0, st, (const T*)src, (unsigned char*)dst, (long long)npix, c_ld);
        else hipLaunchKernelGGL((sr_postprocess_kernel<T, float>), dim3(grid), dim3(256), 0, st, (const T*)src, (float*)dst, (long long)npix, c_ld);
    });
    MNET_LAUNCH_CHECK("sr_postprocess");
    return MNET_OK;
}

// ============================================================================ finiteness flag
// One streaming read (16 bytes per lane and trip): an element is non-finite iff its exponent field is all ones.  No atomics — every
// thread that finds one stores the same 1; the flag was zeroed on the stream just before.
template <typename T>
__global__ void __launch_bounds__(256) nonfinite_flag_kernel(const T* __restrict__ x, long long n, int* __restrict__ flag) {
    constexpr int N = 16 / (int)sizeof(T);
    const long long nv = n / N;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        const u32x4 v = ldg16(x + i * N);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (sizeof(T) == 4) bad |= (v[j] & 0x7f800000u) == 0x7f800000u;
            else bad |= (v[j] & 0x7c00u) == 0x7c00u || (v[j] & 0x7c000000u) == 0x7c000000u;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)                  // the tail (< 16 bytes)
        for (long long i = nv * N; i < n; ++i) { const float f = (float)x[i]; bad |= !(fabsf(f) <= 3.402823466e38f); }      // FLT_MAX: finite values above 3.0e38 are finite
    if (bad) *flag = 1;
}

extern "C" int mnet_nonfinite_flag(const void* x, int32_t dtype, int64_t n, int32_t* flag, void* stream) {
    MNET_CHECK_ARG(x && flag && n > 0, "nonfinite_flag: bad args");
    MNET_CHECK_ARG(is_f16_f32(dtype), "nonfinite_flag: MNET_F32 or MNET_F16 expected");
    MNET_CHECK_ALIGN(aligned16(x), "nonfinite_flag: x must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(flag, 0, sizeof(int32_t), st) != hipSuccess) return mnet_fail(MNET_E_LAUNCH, "nonfinite_flag: hipMemsetAsync failed");
    const long long nv = n / chunk_n(dtype);
    const int grid = (int)((nv + 255) / 256 < 4096 ? (nv + 255) / 256 > 0 ? (nv + 255) / 256 : 1 : 4096);
    dispatch_f16_f32(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(nonfinite_flag_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)x, (long long)n, flag);
    });
    MNET_LAUNCH_CHECK("nonfinite_flag");
    return MNET_OK;
}

// ============================================================================ ToRGB (StyleGAN skip branch)
// ToRGB.forward (models/networks.py:313-321): a MODULATED 1x1 conv to 3 channels without demodulation, + bias, + the bilinearly
// up-sampled RGB of the level below, then tanh.  Through the implicit-GEMM kernel this is a register-staged launch with a style
// prologue that wastes a 32-wide MFMA tile on 3 outputs (2.8 TB/s split-half, 1.5 TB/s fp16+8: 52 ms per step) plus an up-sample
// pass over a 32-channel-padded RGB tensor.  Here: one streaming pass over x — a thread takes 8 channels of a pixel, multiplies
// them by the style and the three weight rows, the C/8 lanes of the pixel fold their partial sums by butterfly shuffles, lane 0
// adds bias and the up-sampled skip (4 taps of the fp32 [N,H/2,W/2,4] image below, horizontal first like ATen) and writes fp32 RGB0.
//   out[n,y,x,o] = tanh( sb[n] * sum_c W[o,c] * (x[n,y,x,c] * s[n,c]) + bias[o] + up2(skip)[n,y,x,o] )
#ifndef MNET_TORGB_DPP
#define MNET_TORGB_DPP 1
#endif
#ifndef MNET_TORGB_U
#define MNET_TORGB_U 4      // pixels per thread and trip (their loads are issued together; their tails run in U lanes at once)
#endif
template <typename T>
__global__ void __launch_bounds__(256) torgb_kernel(const T* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ style,
                                                    const float* __restrict__ sb, const float* __restrict__ bias,
                                                    const float* __restrict__ skip, float* __restrict__ out, int H, int W, int C) {
    const int cpp = C >> 3;                                    // lanes per pixel (16, 32 or 64: a power of two <= 64)
    const int t = threadIdx.x, ch = t & (cpp - 1), pl = t / cpp, ppb = 256 / cpp;
    const int n = blockIdx.y, HW = H * W;
    float s8[8], w0[8], w1[8], w2[8];
    {
        const float* sp = style + (size_t)n * C + ch * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) { s8[j] = sp[j]; w0[j] = wgt[ch * 8 + j]; w1[j] = wgt[C + ch * 8 + j]; w2[j] = wgt[2 * C + ch * 8 + j]; }
    }
    const float osc = sb ? sb[n] : 1.f;
    const T* xb = x + (size_t)n * HW * C + (size_t)ch * 8;
    const int h2 = H >> 1, w2_ = W >> 1;
    const float* kb = skip ? skip + (size_t)n * h2 * w2_ * 4 : nullptr;
    // four pixels per trip: their loads are issued together (one load in flight per lane measured 2.7 TB/s on the 128-px level)
    constexpr int U = MNET_TORGB_U;
    const int step = gridDim.x * ppb;
    for (int pix0 = blockIdx.x * ppb + pl; pix0 < HW; pix0 += U * step) {
        float vv[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int pq = pix0 + u * step;
            ld8<T>(xb + (size_t)(pq < HW ? pq : pix0) * C, vv[u]);
        }
#if MNET_TORGB_DPP
        // the fold over a pixel's C/8 lanes on the VALU (round 6): the butterfly of __shfl_xor is ds_bpermute — 12-18 LDS instructions per pixel, and the ONE LDS pipe of the
        // CU was what bounded this read-only stream (3.1 TB/s).  DPP: quad, half-row and row mirrors leave the sum of each 16-lane row in all its lanes; row_bcast15 / 31 add
        // the rows below into the LAST row of a 32- / 64-lane pixel, whose 16 lanes (8 when C = 64) then all hold the pixel's sums.
        auto fold = [&](float v) __attribute__((always_inline)) -> float {
            auto dpp = [](float q, auto ctrl, auto rmask) __attribute__((always_inline)) {
                return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, q), decltype(ctrl)::value, decltype(rmask)::value, 0xf, false));
            };
            v += dpp(v, std::integral_constant<int, 0xB1>{}, std::integral_constant<int, 0xf>{});       // quad_perm [1,0,3,2]
            v += dpp(v, std::integral_constant<int, 0x4E>{}, std::integral_constant<int, 0xf>{});       // quad_perm [2,3,0,1]
            v += dpp(v, std::integral_constant<int, 0x141>{}, std::integral_constant<int, 0xf>{});      // row_half_mirror
            if (cpp > 8) v += dpp(v, std::integral_constant<int, 0x140>{}, std::integral_constant<int, 0xf>{});      // row_mirror (C = 64: a pixel is 8 lanes, half a row)
            if (cpp > 16) v += dpp(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});      // row_bcast15 into rows 1, 3
            if (cpp > 32) v += dpp(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});      // row_bcast31 into rows 2, 3
            return v;
        };
        // the U pixels' tails (bias, the four skip taps, three tanh, the store: ~150 instructions) run ONCE, in U lanes of the pixel's last row — lane u of that row takes
        // pixel u — instead of U times with one lane active each: the tails were most of this kernel's instruction stream
        float q0[U], q1[U], q2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float* v = vv[u];
            float p0 = 0.f, p1 = 0.f, p2 = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float m = v[j] * s8[j]; p0 = fmaf(m, w0[j], p0); p1 = fmaf(m, w1[j], p1); p2 = fmaf(m, w2[j], p2); }
            q0[u] = fold(p0); q1[u] = fold(p1); q2[u] = fold(p2);
        }
        const int mu = ch - (cpp > 16 ? cpp - 16 : 0);               // lane of the pixel's last row (< 0: an earlier row)
        if (mu < 0 || mu >= U) continue;
        float p0 = q0[0], p1 = q1[0], p2 = q2[0];
#pragma unroll
        for (int u = 1; u < U; ++u) { p0 = mu == u ? q0[u] : p0; p1 = mu == u ? q1[u] : p1; p2 = mu == u ? q2[u] : p2; }
        const int pix = pix0 + mu * step;
        if (pix >= HW) continue;
        {
#else
#pragma unroll
        for (int u = 0; u < U; ++u) {
        const int pix = pix0 + u * step;
        if (pix >= HW) break;                                      // (uniform over the lanes of a pixel: they share pix)
        const float* v = vv[u];
        float p0 = 0.f, p1 = 0.f, p2 = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float m = v[j] * s8[j]; p0 = fmaf(m, w0[j], p0); p1 = fmaf(m, w1[j], p1); p2 = fmaf(m, w2[j], p2); }
        for (int o = 1; o < cpp; o <<= 1) { p0 += __shfl_xor(p0, o, 64); p1 += __shfl_xor(p1, o, 64); p2 += __shfl_xor(p2, o, 64); }
        if (ch != 0) continue;
#endif
        float r0 = p0 * osc + bias[0], r1 = p1 * osc + bias[1], r2 = p2 * osc + bias[2];
        if (kb) {
            const int y = pix / W, xx = pix - y * W;
            const int jy = y >> 1, jx = xx >> 1;
            const int ya = (y & 1) ? jy : max(jy - 1, 0), yb = (y & 1) ? min(jy + 1, h2 - 1) : jy;
            const int xa = (xx & 1) ? jx : max(jx - 1, 0), xb2 = (xx & 1) ? min(jx + 1, w2_ - 1) : jx;
            const float wya = (y & 1) ? 0.75f : 0.25f, wxa = (xx & 1) ? 0.75f : 0.25f;
            const f32x4 aa = *reinterpret_cast<const f32x4*>(kb + ((size_t)ya * w2_ + xa) * 4), ab = *reinterpret_cast<const f32x4*>(kb + ((size_t)ya * w2_ + xb2) * 4);
            const f32x4 ba = *reinterpret_cast<const f32x4*>(kb + ((size_t)yb * w2_ + xa) * 4), bb = *reinterpret_cast<const f32x4*>(kb + ((size_t)yb * w2_ + xb2) * 4);
            const f32x4 top = aa * wxa + ab * (1.f - wxa), bot = ba * wxa + bb * (1.f - wxa);
            const f32x4 up = top * wya + bot * (1.f - wya);
            r0 += up[0]; r1 += up[1]; r2 += up[2];
        }
        *reinterpret_cast<f32x4*>(out + ((size_t)n * HW + pix) * 4) = f32x4{tanhf(r0 - r0 + r0), tanhf(r1 - r1 + r1), tanhf(r2 - r2 + r2), 0.f};
        }
    }
}

extern "C" int mnet_torgb(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, const float* wgt, const float* style,
                          const float* scale_b, const float* bias, const float* skip, float* out, void* stream) {
    MNET_CHECK_ARG(x && wgt && style && bias && out && n > 0 && h > 0 && w > 0 && n <= 65535, "torgb: bad args");
    MNET_CHECK_ARG(is_storage(dtype), "torgb: bad dtype");
    MNET_CHECK_ARG(c >= 64 && c <= 512 && (c & (c - 1)) == 0, "torgb: c=%d (supported: 64, 128, 256, 512)", c);
    MNET_CHECK_ARG(!skip || (h % 2 == 0 && w % 2 == 0), "torgb: a skip image needs even h, w");
    MNET_CHECK_ALIGN(aligned16(x) && aligned16(skip) && aligned16(out) && (!is_split4(dtype) || aligned128(x)), "torgb: unaligned pointer");
    const long long groups = (((long long)h * w + (256 / (c / 8)) - 1) / (256 / (c / 8)) + MNET_TORGB_U - 1) / MNET_TORGB_U;      // MNET_TORGB_U pixels per thread and trip
    // round 5: a workgroup makes (up to) four trips — its prologue (this thread's 8 style values and 3 x 8 weights: 32 loads) was paid once
    // per trip on the 64- and 128-px levels, whose 128 / 256 trips per image had one workgroup each; MNET_TORGB_TRIPS=1 is that form (A/B knob)
    static const int trips = [] { const char* e = getenv("MNET_TORGB_TRIPS"); return e && atoi(e) > 0 ? atoi(e) : 4; }();
    const long long wgs = (groups + trips - 1) / trips;
    const int gx = (int)(wgs < 1024 ? wgs : 1024);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_storage(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(torgb_kernel<T>, dim3(gx, n), dim3(256), 0, st, (const T*)x, wgt, style, scale_b, bias, skip, out, h, w, c);
    });
    MNET_LAUNCH_CHECK("torgb");
    return MNET_OK;
}

// ============================================================================ 3x3 conv to RGB (the last layer of TSPSRNet)
// conv_final.6 + tanh (models/networks.py:374-375): 64 → 3 channels at 128 x 2048.  Through the implicit-GEMM kernel this
// wastes a 16-wide MFMA tile on 3 outputs (1.84 ms per 64 images, 1.1 TB/s) and needs a separate NHWC→NCHW pass for the
// fp32 image the module returns.  Here: one workgroup per 8 x 32 pixel tile, the (8+2) x (32+2) x Cin input patch staged in
// LDS (XOR-swizzled 16-byte chunks, zero halo), one thread per output pixel, 3 fp32 accumulators, weights read through the
// scalar cache (wave-uniform addresses).  f16: v_dot2_f32_f16 (the same exact f16 x f16 products as the MFMA path, fp32
// sums); f32: plain fma.  Output: NHWC [N,H,W,8] in the input dtype and/or fp32 NCHW [N,3,H,W].
template <typename T> struct RgbW;            // weight element as the kernel reads it
template <> struct RgbW<f16> { typedef unsigned int pair_t; };   // two f16 packed
template <> struct RgbW<float> { typedef float pair_t; };

// SPLIT (T = float): the input is a split-half tensor, converted to fp32 while it is staged; weights, arithmetic and both
// outputs are the fp32 ones.
template <typename T, int CIN, bool SPLIT = false, typename ST = hs>
__global__ void __launch_bounds__(256) conv3x3_rgb_kernel(const T* __restrict__ x, const void* __restrict__ wgt_,
                                                          const float* __restrict__ bias, T* __restrict__ y_nhwc,
                                                          float* __restrict__ y_nchw, int H, int W, int act) {
    constexpr int TH = 8, TW = 32, PW = TW + 2, PH = TH + 2;
    constexpr int ROWB = CIN * (int)sizeof(T);                 // bytes per pixel
    constexpr int CH = ROWB / 16;                              // 16-byte chunks per pixel
    constexpr int RPB = ROWB >= 256 ? 1 : 256 / ROWB;          // pixels per 256-byte LDS bank line
    // chunk c of patch pixel q lives at q*ROWB + ((c ^ key(q)) * 16), key(q) = (q / RPB) & (CH-1): the 16 lanes of a
    // ds_read_b128 group (16 consecutive pixels, same logical chunk) then hit 16 distinct 16-byte slots of the bank line(s)
    auto lds_off = [](int q, int c) __attribute__((always_inline)) { return q * ROWB + ((c ^ ((q / RPB) & (CH - 1))) << 4); };
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int t = threadIdx.x;
    const int tiles_x = (W + TW - 1) / TW;
    const int n = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * TH - 1, x0 = tx * TW - 1;              // patch origin (halo included)
    const T* xb = x + (size_t)n * H * W * CIN;
    // stage the patch (zero halo outside the image)
    if constexpr (SPLIT) {
        // split-half input: converted to fp32 while staged, 32 channels (one split block) at a time — a 43.5 KiB patch instead of
        // 87 KiB, so three workgroups share a CU instead of one (the kernel is a chain of LDS / global latencies at 4 waves per CU)
        const ST* xs = reinterpret_cast<const ST*>(x) + (size_t)n * H * W * CIN;
        const float* wp = reinterpret_cast<const float*>(wgt_);              // [3][9][CIN]
        auto off32 = [](int q, int c) __attribute__((always_inline)) { return q * 128 + ((c ^ ((q >> 1) & 7)) << 4); };   // 128-byte rows, 8 chunks
        const int ly_ = t / TW, lx_ = t - ly_ * TW;
        float b0 = 0.f, b1 = 0.f, b2 = 0.f;
        for (int half = 0; half < CIN / 32; ++half) {
            if (half) __syncthreads();
            for (int i = t; i < PH * PW * 4; i += 256) {
                const int c8 = i & 3, q = i >> 2;
                const int py = q / PW, px = q - py * PW;
                const int gy = y0 + py, gx = x0 + px;
                float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) unpackr<ST>(ldraw<ST>(xs + ((size_t)gy * W + gx) * CIN + half * 32 + c8 * 8), v);
                *reinterpret_cast<u32x4*>(dyn + off32(q, 2 * c8)) = Vec<float>::pack(v);
                *reinterpret_cast<u32x4*>(dyn + off32(q, 2 * c8 + 1)) = Vec<float>::pack(v + 4);
            }
            __syncthreads();
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int q = (ly_ + tap / 3) * PW + lx_ + tap % 3;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const f32x4 v = bitcast<f32x4>(*reinterpret_cast<const u32x4*>(dyn + off32(q, c)));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = tap * CIN + half * 32 + c * 4 + j;
                        b0 = fmaf(v[j], wp[k], b0); b1 = fmaf(v[j], wp[9 * CIN + k], b1); b2 = fmaf(v[j], wp[18 * CIN + k], b2);
                    }
                }
            }
        }
        const int oy_ = ty * TH + ly_, ox_ = tx * TW + lx_;
        if (oy_ >= H || ox_ >= W) return;
        float r[8] = {b0 + bias[0], b1 + bias[1], b2 + bias[2], 0.f, 0.f, 0.f, 0.f, 0.f};
        // half-range storage: an overflowed (infinite) pre-activation must not hide behind tanh's saturation — it is written as NaN
        // (tanhf(inf - inf) is NaN already), so that the pipeline's finiteness check of the SR result sees it
        if (act == MNET_ACT_TANH) { r[0] = tanhf(r[0] - r[0] + r[0]); r[1] = tanhf(r[1] - r[1] + r[1]); r[2] = tanhf(r[2] - r[2] + r[2]); }
        if (y_nhwc) {
            T* yp = y_nhwc + (((size_t)n * H + oy_) * W + ox_) * 8;
            stg16(yp, Vec<float>::pack(r)); stg16(yp + 4, Vec<float>::pack(r + 4));
        }
        if (y_nchw) {
            const size_t plane = (size_t)H * W;
            float* op = y_nchw + (size_t)n * 3 * plane + (size_t)oy_ * W + ox_;
#pragma unroll
            for (int o = 0; o < 3; ++o) op[o * plane] = r[o];
        }
        return;
    } else
    for (int i = t; i < PH * PW * CH; i += 256) {
        const int c = i % CH, q = i / CH;
        const int py = q / PW, px = q - py * PW;
        const int gy = y0 + py, gx = x0 + px;
        u32x4 v = {0u, 0u, 0u, 0u};
        if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) v = ldg16(xb + ((size_t)gy * W + gx) * CIN + c * (16 / (int)sizeof(T)));
        *reinterpret_cast<u32x4*>(dyn + lds_off(q, c)) = v;
    }
    __syncthreads();
    const int ly = t / TW, lx = t - ly * TW;
    const int oy = ty * TH + ly, ox = tx * TW + lx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if constexpr (sizeof(T) == 2) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const unsigned* wp = reinterpret_cast<const unsigned*>(wgt_);        // [3][9][CIN/2] packed f16 pairs
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int q = (ly + tap / 3) * PW + lx + tap % 3;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(dyn + lds_off(q, c));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const h2 xv = bitcast<h2>(v[j]);
                    const int k = tap * (CIN / 2) + c * 4 + j;
                    a0 = __builtin_amdgcn_fdot2(xv, bitcast<h2>(wp[k]), a0, false);
                    a1 = __builtin_amdgcn_fdot2(xv, bitcast<h2>(wp[9 * (CIN / 2) + k]), a1, false);
                    a2 = __builtin_amdgcn_fdot2(xv, bitcast<h2>(wp[18 * (CIN / 2) + k]), a2, false);
                }
            }
        }
    } else {
        const float* wp = reinterpret_cast<const float*>(wgt_);              // [3][9][CIN]
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int q = (ly + tap / 3) * PW + lx + tap % 3;
#pragma unroll 4
            for (int c = 0; c < CH; ++c) {
                const f32x4 v = bitcast<f32x4>(*reinterpret_cast<const u32x4*>(dyn + lds_off(q, c)));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = tap * CIN + c * 4 + j;
                    a0 = fmaf(v[j], wp[k], a0); a1 = fmaf(v[j], wp[9 * CIN + k], a1); a2 = fmaf(v[j], wp[18 * CIN + k], a2);
                }
            }
        }
    }
    if (oy >= H || ox >= W) return;
    float r[8] = {a0 + bias[0], a1 + bias[1], a2 + bias[2], 0.f, 0.f, 0.f, 0.f, 0.f};
    if (act == MNET_ACT_TANH) {
        if constexpr (sizeof(T) == 2) {      // f16 storage: see above (an infinite pre-activation becomes NaN, not +-1)
            r[0] = tanhf(r[0] - r[0] + r[0]); r[1] = tanhf(r[1] - r[1] + r[1]); r[2] = tanhf(r[2] - r[2] + r[2]);
        } else { r[0] = tanhf(r[0]); r[1] = tanhf(r[1]); r[2] = tanhf(r[2]); }
    }
    if (y_nhwc) {
        T* yp = y_nhwc + (((size_t)n * H + oy) * W + ox) * 8;
        if constexpr (sizeof(T) == 2) stg16(yp, Vec<f16>::pack(r));
        else { stg16(yp, Vec<float>::pack(r)); stg16(yp + 4, Vec<float>::pack(r + 4)); }
    }
    if (y_nchw) {
        // what the module hands back: fp32 NCHW; in f16 mode the values are the f16-rounded ones the NHWC tensor holds
        const size_t plane = (size_t)H * W;
        float* op = y_nchw + (size_t)n * 3 * plane + (size_t)oy * W + ox;
#pragma unroll
        for (int o = 0; o < 3; ++o) op[o * plane] = sizeof(T) == 2 ? (float)(f16)r[o] : r[o];
    }
}

extern "C" int mnet_conv3x3_rgb(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t cin, const void* wgt,
                                const float* bias, int32_t act, void* y_nhwc, float* y_nchw, void* stream) {
    MNET_CHECK_ARG(x && wgt && bias && (y_nhwc || y_nchw) && n > 0 && h > 0 && w > 0 && n <= 65535, "conv3x3_rgb: bad args");
    MNET_CHECK_ARG(is_storage(dtype), "conv3x3_rgb: bad dtype");
    MNET_CHECK_ARG(cin == 64, "conv3x3_rgb: cin=%d (supported: 64)", cin);
    MNET_CHECK_ALIGN(!is_split4(dtype) || aligned128(x), "conv3x3_rgb: split-half input must be 128-byte aligned");
    MNET_CHECK_ARG(act == MNET_ACT_NONE || act == MNET_ACT_TANH, "conv3x3_rgb: act %d", act);
    MNET_CHECK_ALIGN(aligned16(x) && aligned16(y_nhwc) && aligned16(wgt), "conv3x3_rgb: unaligned pointer");
    const int tiles = ((h + 7) / 8) * ((w + 31) / 32);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dispatch_storage(dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        if constexpr (__is_same(T, f16)) {
            const int lds = 10 * 34 * 64 * 2;
            hipLaunchKernelGGL((conv3x3_rgb_kernel<f16, 64>), dim3(tiles, n), dim3(256), lds, st, (const f16*)x, wgt, bias, (f16*)y_nhwc, y_nchw, h, w, act);
        } else {                        // fp32 arithmetic and outputs; a blocked storage is converted while it is staged, half a patch at a time
            constexpr bool SPLIT = is_split4_type<T>;
            const auto kern = conv3x3_rgb_kernel<float, 64, SPLIT, std::conditional_t<SPLIT, T, hs>>;
            const int lds = 10 * 34 * 64 * 4;
            static thread_local DeviceOnce attr_once;      // per instantiation, per thread, per device
            if (!attr_once.done()) {
                const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
                if (e != hipSuccess) return mnet_fail(MNET_E_LAUNCH, "hipFuncSetAttribute(conv3x3_rgb): %s", hipGetErrorString(e));
                attr_once.mark();
            }
            hipLaunchKernelGGL(kern, dim3(tiles, n), dim3(256), SPLIT ? 10 * 34 * 32 * 4 : lds, st, (const float*)x, wgt, bias, (float*)y_nhwc, y_nchw, h, w, act);
        }
        MNET_LAUNCH_CHECK("conv3x3_rgb");
        return MNET_OK;
    });
}
