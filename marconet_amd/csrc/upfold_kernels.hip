// The "fold" of an up-sampling 3x3 convolution in tap-conv form (mnet_upfold3x3_nhwc).
//
// conv3x3(U x)[o,p] = sum_t (U Z_t)[o, p + t],  Z_t[o,q] = sum_c W[o,c,t] x[c,q]      (U: bilinear x2, align_corners=False, edge clamp; zero where p + t leaves the
// hi-res map): the channel contraction runs on the LOW-res map as one 1x1 convolution with 9 C output channels (a quarter of the MACs of the conv on the up-sampled map,
// which is never written), and this kernel sums the nine up-sampled, shifted tap planes and applies the conv epilogue.  HBM-bound: Z [n,h,w,9C] is read once, y
// [n,2h,2w,C] written once.
//
// Separable, horizontal first.  With up[2j] = 1/4 in[j-1] + 3/4 in[j], up[2j+1] = 3/4 in[j] + 1/4 in[j+1] (indices clamped):
//   H_ky[i][X] = sum_kx (U_x Z_{ky,kx}[i,:])[X + kx - 1]                  (terms whose hi-res column X + kx - 1 is outside [0, 2w) are zero)
//   y[Y][X]    = sum_ky (U_y H_ky[:,X])[Y + ky - 1]                       (terms whose hi-res row    Y + ky - 1 is outside [0, 2h) are zero)
// One thread = one 8-channel chunk of one HI-res column X: it walks UPF_RUN low-res rows.  (Two columns per thread share a third of their loads, but carry twice the
// state: 330 registers, one wave per SIMD, 2.4 TB/s measured; this form fits two waves.)  Row r of H enters three output row pairs —
// as the row ABOVE (P: pair r+1), the row ITSELF (C: pair r) and the row BELOW (N: pair r-1) — so the walk carries two partial pairs instead of three H rows:
//   even row 2i   = [3/4 H0 + 1/4 H1](i-1) + [1/4 H0 + 3/4 H1 + 3/4 H2](i) + [1/4 H2](i+1)
//   odd  row 2i+1 = [1/4 H0](i-1)          + [3/4 H0 + 3/4 H1 + 1/4 H2](i) + [1/4 H1 + 3/4 H2](i+1)
// and at the map's edge the clamp puts row 0 / h-1 in the place of row -1 / h while the zero padding removes the tap that looks outside:
//   i = 0:   P = (1/4 H1(0), 1/4 H0(0)), C's even row loses 1/4 H0          i = h-1:   N = (1/4 H2(h-1), 1/4 H1(h-1)), C's odd row loses 1/4 H2
// Every output is summed as (P + C) + N by the one thread that owns it, in fp32, whatever the batch or the grid: one glyph alone gives the bytes it gives in a batch.
// Storage: the readers / writers of common.h; a quad of lanes holds the four chunks of one 32-channel block of one pixel (cpp % 4 == 0, linear thread -> chunk map).
// upfold_kernel<TZ, TY>: z and y in the same storage (mnet_upfold3x3_nhwc, all four), or z in fp32 under a y in fp16+8 (mnet_upfold3x3_f32z_nhwc): Z is an intermediate
// that only this kernel reads and fp16+8 costs fp32's 4 bytes per element, so the tap conv writes the planes in fp32 (MNET_CONV_ALGO_FLAG_F32_OUT) and a loaded chunk is
// already the decoded value — the same thread map, the same sums in the same order, one rounding (of Z to the storage) less.
#include "common.h"
#include "../../include/marconet_hip_upfold_f32.h"

#ifndef MNET_UPF_RUN
#define MNET_UPF_RUN 8
#endif

// A tap chunk of the thread's N channels as fp32.  Z in y's storage: the storage's reader.  Z in fp32 under a y of 8-channel chunks (upfold_kernel<float, hm>,
// mnet_upfold3x3_f32z_nhwc): the same nominal address — 8 channels are 32 bytes in both — holds the values themselves: two plain 16-byte loads, no decode instruction,
// no quad co-operation and no raw copy of the chunk beside the decoded one.
template <typename TZ, int N>
__device__ __forceinline__ void upf_load(const TZ* p, float (&o)[N]) {
    if constexpr (__is_same(TZ, float) && N == 8) {
        Vec<float>::unpack(ldg16s(p), o);
        Vec<float>::unpack(ldg16s(p + 4), o + 4);
    } else {
        unpackr<TZ>(ldraw<TZ>(p), o);
    }
}

// waves per SIMD the kernel is compiled for.  The fp32-plane form carries no raw chunks, but its walk state (h, the two open pairs, six chunks of a filter row in flight)
// still fills the file: compiled for 2 waves it takes 256 VGPRs with 20 spilled (fp16+8 planes: 256 with 33), for 3 waves 168 with 85 spilled, for 4 waves 128 with 177
// — so it stays at 2 like every same-storage form (MNET_UPF_F32Z_WAVES: the A/B build).  Measured at 2: 3.46 / 3.70 TB/s of Z + y bytes on the 16→32 / 32→64 levels of
// 1024 glyphs against 2.71 / 2.69 with fp16+8 planes (profiles/upfold_f32z_kernel_ab.json).
#ifndef MNET_UPF_F32Z_WAVES
#define MNET_UPF_F32Z_WAVES 2
#endif
template <typename TZ, typename TY> constexpr int upf_waves = __is_same(TZ, TY) ? 2 : MNET_UPF_F32Z_WAVES;

template <typename TZ, typename TY = TZ>
__global__ void __launch_bounds__(256, (upf_waves<TZ, TY>)) upfold_kernel(const TZ* __restrict__ z, TY* __restrict__ y, int H, int W, int C,
                                                        const float* __restrict__ out_scale, const float* __restrict__ bias,
                                                        const float* __restrict__ post_scale, int act, unsigned items_per_image) {
    // grid: x strides over the (chunk, hi-res column, row run) items of ONE image (32-bit index math only), y = image — upsample2x_kernel's launch shape
    using T = TY;                                                           // (the thread's chunk is y's: N channels; z is addressed in the same 4-byte elements)
    constexpr int N = Vec<T>::N;
    static_assert(sizeof(TZ) == sizeof(TY) || __is_same(TZ, TY), "z and y: the same storage, or two storages of 4 bytes per element");
    constexpr int R = MNET_UPF_RUN;
    const unsigned cpp = (unsigned)C / N;
    // XCD-aware order (see upsample2x_kernel): XCD k takes the k-th eighth of the (image, workgroup) sequence, so the neighbours that re-read a workgroup's halo share its L2
    unsigned bx = blockIdx.x, by = blockIdx.y;
    {
        const unsigned NWG = gridDim.x * gridDim.y, L = by * gridDim.x + bx;
        if ((NWG & 7u) == 0u) { const unsigned V = (L & 7u) * (NWG >> 3) + (L >> 3); by = V / gridDim.x; bx = V - by * gridDim.x; }
    }
    const int n = (int)by;
    const size_t zpix = (size_t)9 * C;                                      // elements per low-res pixel of z
    const TZ* zbase = z + (size_t)n * H * W * zpix;
    T* ybase = y + (size_t)n * 4 * H * W * C;
    const int W2 = 2 * W;
    for (unsigned id = bx * 256u + threadIdx.x; id < items_per_image; id += gridDim.x * 256u) {
        const unsigned ch = id % cpp, col = id / cpp;
        const int X = (int)(col % (unsigned)W2), y0 = (int)(col / (unsigned)W2) * R, y1 = min(y0 + R, H);
        // tap kx reads hi-res column X + kx - 1 of the up-sampled plane: two low-res columns and their weights, or nothing outside the map
        unsigned c0[3], c1[3];
        float w0[3], w1[3];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int xu = X + kx - 1, xc = min(max(xu, 0), W2 - 1), m = xc >> 1;
            const bool odd = xc & 1, in = xu >= 0 && xu < W2;
            c0[kx] = (unsigned)(odd ? m : max(m - 1, 0)) * (unsigned)zpix;      // (element offsets inside a row: < 2^31 / 4, checked by the launcher)
            c1[kx] = (unsigned)(odd ? min(m + 1, W - 1) : m) * (unsigned)zpix;
            w0[kx] = in ? (odd ? 0.75f : 0.25f) : 0.f;
            w1[kx] = in ? (odd ? 0.25f : 0.75f) : 0.f;
        }
        const TZ* base = zbase + (size_t)ch * N;
        // H_ky of low-res row r at this hi-res column: six chunks per filter row, summed one at a time in this order
        auto hrow = [&](int r, float (&h)[3][N]) __attribute__((always_inline)) {
            const TZ* rp = base + (size_t)r * W * zpix;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const TZ* tp = rp + (size_t)(3 * ky + kx) * C;
                    float a[N], b[N];
                    upf_load<TZ, N>(tp + c0[kx], a);
                    upf_load<TZ, N>(tp + c1[kx], b);
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        const float t = w0[kx] * a[j] + w1[kx] * b[j];
                        h[ky][j] = kx == 0 ? t : h[ky][j] + t;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);      // one filter row's six chunks in flight at a time: hipcc otherwise hoists all 18 loads (144 registers of raw chunks) and spills
            }
        };
        const float* osp = out_scale ? out_scale + (size_t)n * C + (size_t)ch * N : nullptr;
        const float* bsp = bias ? bias + (size_t)ch * N : nullptr;
        const float* psp = post_scale ? post_scale + (size_t)n * C + (size_t)ch * N : nullptr;
        // the conv epilogue's contract on one chunk: post_scale * act(out_scale * v + bias), rounded to storage once.  (The three vectors are re-read at every store —
        // L1 hits — instead of living in 24 registers through the walk.)
        auto emit1 = [&](T* q, float (&v)[N]) __attribute__((always_inline)) {
            float o[N];
#pragma unroll
            for (int j = 0; j < N; ++j) o[j] = v[j];
            if (osp) {
#pragma unroll
                for (int j = 0; j < N; j += 4) { const f32x4 s4 = *reinterpret_cast<const f32x4*>(osp + j); o[j] *= s4[0]; o[j + 1] *= s4[1]; o[j + 2] *= s4[2]; o[j + 3] *= s4[3]; }
            }
            if (bsp) {
#pragma unroll
                for (int j = 0; j < N; j += 4) { const f32x4 b4 = *reinterpret_cast<const f32x4*>(bsp + j); o[j] += b4[0]; o[j + 1] += b4[1]; o[j + 2] += b4[2]; o[j + 3] += b4[3]; }
            }
            act_apply_vec<N, true>(o, act);
            if (psp) {
#pragma unroll
                for (int j = 0; j < N; j += 4) { const f32x4 p4 = *reinterpret_cast<const f32x4*>(psp + j); o[j] *= p4[0]; o[j + 1] *= p4[1]; o[j + 2] *= p4[2]; o[j + 3] *= p4[3]; }
            }
            straw<T>(q, packr<T>(o));
        };
        float h[3][N];
        float e[N], o[N];          // pair i: even / odd hi-res row (P + C so far)
        float ne[N], no[N];        // pair i + 1 (P so far)
        // P of pair y0: from row y0 - 1, or at the top edge from row 0 itself
        hrow(max(y0 - 1, 0), h);
        {
            const bool in = y0 > 0;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                e[j] = (in ? 0.75f * h[0][j] : 0.f) + 0.25f * h[1][j];
                o[j] = 0.25f * h[0][j];
            }
        }
        // C of pair r into the open pair, P of pair r + 1 into the next one
        auto centre = [&](int r) __attribute__((always_inline)) {
            const bool up = r > 0, dn = r + 1 < H;      // false: the tap ky = 0 of hi-res row 0 / ky = 2 of row 2h - 1 looks outside the map (zero padding)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                e[j] += ((up ? 0.25f * h[0][j] : 0.f) + 0.75f * h[1][j]) + 0.75f * h[2][j];
                o[j] += (0.75f * h[0][j] + 0.75f * h[1][j]) + (dn ? 0.25f * h[2][j] : 0.f);
                ne[j] = 0.75f * h[0][j] + 0.25f * h[1][j];
                no[j] = 0.25f * h[0][j];
            }
        };
        hrow(y0, h);
        centre(y0);
        const size_t orow = (size_t)W2 * C;
#pragma unroll 1
        for (int i = y0; i < y1; ++i) {
            // N of pair i: from row i + 1, or at the bottom edge from row h - 1 itself
            hrow(min(i + 1, H - 1), h);
            const bool in = i + 1 < H;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                e[j] += 0.25f * h[2][j];
                o[j] += 0.25f * h[1][j] + (in ? 0.75f * h[2][j] : 0.f);
            }
            T* q = ybase + ((size_t)(2 * i) * W2 + X) * C + (size_t)ch * N;      // output pixel (2i, X)
            emit1(q, e);
            emit1(q + orow, o);
            if (i + 1 < y1) {
#pragma unroll
                for (int j = 0; j < N; ++j) { e[j] = ne[j]; o[j] = no[j]; }
                centre(i + 1);
            }
        }
    }
}

extern "C" int mnet_upfold3x3_nhwc(const void* z, void* y, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c,
                                   const float* out_scale, const float* bias, int32_t act, const float* post_scale, void* stream) {
    MNET_CHECK_ARG(z && y && z != y, "upfold3x3: null pointer (or y == z: not an in-place kernel)");
    MNET_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && c > 0, "upfold3x3: bad geometry");
    MNET_CHECK_ARG(is_storage(dtype), "upfold3x3: bad dtype");
    MNET_CHECK_ARG(act == MNET_ACT_NONE || act == MNET_ACT_LRELU || act == MNET_ACT_LRELU_SQRT2, "upfold3x3: activation must be NONE, LRELU or LRELU_SQRT2");
    const int N = chunk_n(dtype);
    MNET_CHECK_ALIGN(c % N == 0 && aligned16(z) && aligned16(y) && aligned16(out_scale) && aligned16(bias) && aligned16(post_scale),
                     "upfold3x3: c %% %d != 0 or unaligned", N);
    MNET_CHECK_ALIGN(!is_split4(dtype) || (c % 32 == 0 && aligned128(z) && aligned128(y)), "upfold3x3: blocked storages need c %% 32 == 0, 128-byte aligned");
    MNET_CHECK_ARG((long long)h * w * (c / N) * 4 < (1ll << 31) && (long long)w * 9 * c < (1ll << 29), "upfold3x3: image too large");
    const long long per = (long long)((h + MNET_UPF_RUN - 1) / MNET_UPF_RUN) * 2 * w * (c / N);      // one thread per (chunk, hi-res column, run of MNET_UPF_RUN low-res rows)
    const int gx = (int)((per + 255) / 256 < 2048 ? (per + 255) / 256 : 2048);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    dispatch_storage(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((upfold_kernel<T>), dim3(gx, n), dim3(256), 0, st, (const T*)z, (T*)y, h, w, c, out_scale, bias, post_scale, act, (unsigned)per);
    });
    MNET_LAUNCH_CHECK("upfold3x3");
    return MNET_OK;
}

// z in fp32, y in fp16+8: the checks, the items and the grid of mnet_upfold3x3_nhwc at dtype = MNET_F16M (8-channel chunks, a blocked y; z is 128-byte aligned like y, so
// that the planes are whole lines) — the same launch shape for the same thread map
extern "C" int mnet_upfold3x3_f32z_nhwc(const float* z, void* y, int32_t ydtype, int32_t n, int32_t h, int32_t w, int32_t c,
                                        const float* out_scale, const float* bias, int32_t act, const float* post_scale, void* stream) {
    MNET_CHECK_ARG(ydtype == MNET_F16M, "upfold3x3: fp32 tap planes fold into an MNET_F16M output only (ydtype %d)", ydtype);
    MNET_CHECK_ARG(z && y && (const void*)z != y, "upfold3x3: null pointer (or y == z: not an in-place kernel)");
    MNET_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && c > 0, "upfold3x3: bad geometry");
    MNET_CHECK_ARG(act == MNET_ACT_NONE || act == MNET_ACT_LRELU || act == MNET_ACT_LRELU_SQRT2, "upfold3x3: activation must be NONE, LRELU or LRELU_SQRT2");
    constexpr int N = Vec<hm>::N;
    MNET_CHECK_ALIGN(c % 32 == 0 && aligned128(z) && aligned128(y) && aligned16(out_scale) && aligned16(bias) && aligned16(post_scale),
                     "upfold3x3: fp32 planes under an fp16+8 output need c %% 32 == 0, z and y 128-byte aligned, the vectors 16-byte aligned");
    MNET_CHECK_ARG((long long)h * w * (c / N) * 4 < (1ll << 31) && (long long)w * 9 * c < (1ll << 29), "upfold3x3: image too large");
    const long long per = (long long)((h + MNET_UPF_RUN - 1) / MNET_UPF_RUN) * 2 * w * (c / N);
    const int gx = (int)((per + 255) / 256 < 2048 ? (per + 255) / 256 : 2048);
    hipLaunchKernelGGL((upfold_kernel<float, hm>), dim3(gx, n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), z, (hm*)y, h, w, c, out_scale, bias, post_scale, act,
                       (unsigned)per);
    MNET_LAUNCH_CHECK("upfold3x3");
    return MNET_OK;
}
