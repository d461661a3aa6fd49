/*
 * marconet_hip.h — C-ABI of libmarconet_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * MARCONet test_sr.py / test_w.py inference forward.
 *
 * Boundary rules:
 *   - plain C: raw device pointers, ints, a dtype enum and a hipStream_t (passed as void*); no torch types
 *   - every buffer (inputs, outputs, workspaces) is owned and allocated by the caller
 *   - every call enqueues work on the given stream and returns; no call synchronises or allocates
 *   - return value: 0 = ok, negative = MNET_E_* ; mnet_last_error() returns a thread-local message
 *   - re-entrant, no mutable global state
 *
 * The reference has no native layer of its own: its operator layer is ATen + one third-party CUDA op
 * (basicsr.ops.fused_act, models/networks.py:10).  Each entry point below therefore cites the reference
 * *call sites* (file:line under /root/reference) whose arithmetic it replaces.
 *
 * Tensor layout: activations are NHWC ("pixel-major, channel-minor") in MNET_F32 or MNET_F16; conv
 * weights are [Cout][KH][KW][Cin] in the same dtype.  All statistics, softmax, demodulation and
 * epilogue math are fp32 (fp64 for the GroupNorm / AdaIN sums).
 */
#ifndef MARCONET_HIP_H
#define MARCONET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNET_ABI_VERSION 4

/* MNET_F16X2 ("split half", the storage of the fp16x3 precision mode): every logical element is a pair of halves (hi, lo),
 * value = float(hi) + float(lo), hi = f16(v), lo = f16(v - hi): ~22 significant bits at fp16 MFMA rates (x*w is evaluated as
 * hi*hi + hi*lo + lo*hi, fp32 accumulate) — the throughput mode that meets the 1e-3 parity bar.  NHWC layout [.., C] with
 * C % 32 == 0 and a 128-byte aligned base: per pixel 4*C bytes in blocks of 32 channels, 64 bytes of hi followed by 64 bytes
 * of lo.  Conv weights [cout][kh][kw][cin] use the same blocking along cin and hold hi/lo of 256*W (the conv multiplies its
 * accumulator by 2^-8).  Entry points that accept it say so; sizes/strides are always given in LOGICAL elements. */
/* MNET_F16M ("fp16+8", the storage of the fp16x2 precision mode): the same 4 bytes per logical element and the same blocking
 * (128 bytes per (pixel, 32-channel block), C % 32 == 0, 128-byte aligned base), but only the hi part is a half; the lo part is an
 * OCP e4m3 byte under one E8M0 scale per block, so that x*w = hi*hi on the f16 MFMA + (w_lo8*x_hi8 + w_hi8*x_lo8) as ONE block-scaled
 * fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, twice the f16 rate): 2 MFMA units per product instead of 3, ~16 significant bits.
 *   activations  bytes 0-63 hi = f16(v) of channels 0..31 | 64-95 lo8 = e4m3((v - hi) * 2^11 / s), channel order 0-7,16-23,8-15,24-31 |
 *                byte 96 E: s = 2^(E-127) = 2^(floor(log2 max|hi|) - 7) | bytes 97-127 zero
 *                The whole rule for E (max|hi| over the block's 32 HALVES, not over v: a maximum that rounds up into the next binade takes that binade's scale):
 *                  max|hi| > 0:   E = max(floor(log2 max|hi|) + 120, 105).  The floor 105 (s = 2^-22, max|hi| < 2^-15) is for blocks of fp16 subnormals, whose
 *                                 rounding error stops shrinking with the block: with it (v - hi) * 2^11 / s is at most 2^8, without it it leaves e4m3's range.
 *                                 In a block of normal halves it is at most 2^7: no writer ever saturates, and no finite input gives a NaN byte (0x7f / 0xff).
 *                  max|hi| == 0:  E = 0 — a true all-zero block, and a block of values below 2^-25 alike.  Its lo bytes are e4m3((v - hi) * 0): zero bytes that keep
 *                                 the residual's sign (0x00, or 0x80 where v < 0), exactly as a residual that underflows e4m3 in any other block does; the
 *                                 block decodes to its hi halves (+-0) exactly.
 *                  e4m3 rounds to nearest even.  Decoding is fl32(hi + lo8 * 2^(E - 138)), ONE rounding, with a lo scale of 0 for E < 12.
 *                  Every writer — streaming kernels, layout kernels, every conv epilogue — and the host packer (marconet_amd/mxfmt.py) produce these bytes for
 *                  finite input (tests/storage_codec.py is the rule as code).  The bytes of a block that holds an inf or a NaN are not defined beyond: that element
 *                  decodes non-finite, the other blocks of the pixel are untouched.
 *   conv weights bytes 0-63 hi = f16(256 W) | 64-79 lo8 of channels 0-7,16-23 | 80-95 hi8 = e4m3(hi / s) of the same | 96-111 lo8 of
 *                8-15,24-31 | 112-127 hi8 of the same; s per OUTPUT channel; after the cout*kh*kw*cin elements one byte per output
 *                channel (E8M0 of s * 2^-11), i.e. a packed weight tensor is cout*kh*kw*cin*4 + cout bytes (mnet_pack_weights).  The row's exponent is
 *                clamp(floor(log2 max|hi|) + 120, 11, 254) — no floor at 105: a row with 0 < max|hi| < 2^-15 is outside the format (256 W of a layer never is) —
 *                and 11 (trailing byte 0, signed-zero lo bytes as above) for a row whose every hi is +-0, e.g. a padding row. */
/* Operand range of the convolutions (mnet_conv2d_nhwc; tests/conv_range.py is this paragraph as code, tests/test_conv_range_gpu.py holds every kernel build
 * to it).  The kernels read every block the storages can hold — fp16-subnormal blocks at the floor E = 105, E = 0 blocks, blocks of one pixel or of neighbouring
 * pixels under scales far apart, weight rows 2^10 apart — and each OUTPUT, judged alone, lies within
 *     gamma * A_o + f_o + r_o      of the fp64 sum of the products its kernel family forms (finite operands, |y| inside the half range), where
 *   A_o    = the sum of the absolute values of those products: an error is measured against the output's own window, not against the largest output of the map;
 *   gamma  = the error of an fp32 accumulation, at most K * 2^-24 (K = kh * kw * cin); the kernels keep the tighter measured figure pinned in tests/conv_range.py;
 *   f_o    = 0 for MNET_F32, MNET_F16 and the MNET_F16M LDS-DMA / strip / one-wave kernels: their operands enter the MFMAs as stored, fp16 subnormals included
 *            (x_hi8 = e4m3(hi / s_x) is formed from subnormal halves as from normal ones).  MNET_F16X2 on every kernel, and MNET_F16M on the register-staged
 *            kernel (lo bytes decoded to halves), multiply f16 lo halves, which stop at the f16-subnormal step: f_o = 2^-24 * (sum |W_hi| over the taps that hold
 *            a live activation + sum |X_hi| over the taps that hold a live weight) / 256 — one step per element; the same holds for X' of an input transform;
 *   r_o    = one step of the output storage at that value: the f16 ulp; the f16 ulp of the lo half (MNET_F16X2); one e4m3 step of the scaled residual under
 *            the output block's scale (MNET_F16M); 0 for MNET_F32 and for MNET_CONV_ALGO_FLAG_F32_OUT.
 * An output whose window holds no non-zero product is exactly 0. */
typedef enum { MNET_F32 = 0, MNET_F16 = 1, MNET_F16X2 = 2, MNET_F16M = 3 } mnet_dtype;

typedef enum {
    MNET_ACT_NONE = 0,
    MNET_ACT_RELU = 1,          /* models/resnet.py:16,24,29                                   */
    MNET_ACT_LRELU = 2,         /* nn.LeakyReLU(0.2), models/networks.py:337..404              */
    MNET_ACT_LRELU_SQRT2 = 3,   /* basicsr fused_leaky_relu: sqrt(2)*lrelu_0.2, networks.py:195,241 */
    MNET_ACT_TANH = 4,          /* networks.py:321,375                                         */
    MNET_ACT_GELU = 5,          /* nn.GELU() exact erf, models/textvit_arch.py:49,88           */
    MNET_ACT_SIGMOID = 6        /* textvit_arch.py:51                                          */
} mnet_act;

enum {
    MNET_OK = 0,
    MNET_E_ARG = -1,        /* bad shape / null pointer / unsupported combination */
    MNET_E_ALIGN = -2,      /* pointer or channel count not aligned as required   */
    MNET_E_LAUNCH = -3      /* hipLaunchKernel / hipFuncSetAttribute failed       */
};

const char* mnet_last_error(void);
int mnet_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * mnet_conv2d_nhwc — implicit-GEMM convolution on the matrix cores (MFMA 16x16x32 f16 / 16x16x4 f32),
 * with fused prologue and epilogue.  One entry point covers:
 *   K1/K2/K3 dense 3x3 / 1x1 / strided convs  models/resnet.py:4-9,21-30 ; models/networks.py:336-405,501-505
 *   K4  modulated conv (activation-side modulation: y = demod[n,o] * conv(W*scale, x * s[n,i]))
 *                                              models/networks.py:281-302 (ModulatedConv2d.forward)
 *   K5  fused bias + LeakyReLU*sqrt2 epilogue  basicsr fused_act, call sites networks.py:195,241-245
 *   K7  every nn.Linear of TextViT / style MLP (1x1 conv over a [1,1,M,K] map)
 *                                              models/textvit_arch.py:34,49-60,84-107 ; networks.py:188-198
 *       the 8x8/stride-8 patch embedding is the same kernel with kh=kw=8 (textvit_arch.py:32-35)
 *   K17 channel concat without materialising it (two sources)   networks.py:415-416
 *   K11 GroupNorm+swish as an input-side affine (scale/shift per (n,c)) + swish   networks.py:508-513
 *
 * y[n,oh,ow,o] = post_scale[n,o] * act( out_scale[n,o] * sum_{r,s,i} W[o,r,s,i] * X'[n, oh*sh-ph+r, ow*sw-pw+s, i]
 *                                       + bias[o] + residual[n,oh,ow,o] )
 *   X' = X                                   if in_scale == NULL
 *   X' = f(X * in_scale[n,i] + in_shift[n,i]),  f = swish if in_swish else identity
 *   X  = channel-concat(x0[..c0], x1[..c1]);  out-of-image taps (and columns >= valid_w[n]) are zero
 *
 * Requirements: (c0+c1) % 8 == 0, c0 % 8 == 0, cout % 4 == 0, all pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t dtype;              /* mnet_dtype of x0, x1, wgt, residual, y                         */
    const void* x0; int32_t c0; /* NHWC [n,h,w,c0]                                                */
    const void* x1; int32_t c1; /* NHWC [n,h,w,c1] or NULL/0                                      */
    int32_t n, h, w;
    const void* wgt;            /* [cout][kh][kw][c0+c1]                                          */
    int32_t cout, kh, kw, stride_h, stride_w, pad_h, pad_w;
    int32_t ho, wo;             /* output spatial size (caller computes)                          */
    const float* in_scale;      /* [n][cin] or NULL                                               */
    const float* in_shift;      /* [n][cin] or NULL (treated as 0)                                */
    int32_t in_swish;
    const int32_t* valid_w;     /* [n] or NULL: input columns >= valid_w[n] read as zero — INPUT columns whatever the stride
                                 * (output column ow reads columns ow*sw-pw .. ow*sw-pw+kw-1); 0 is allowed: the image reads as zero */
    const float* out_scale;     /* [n][cout] or NULL (demodulation)                               */
    const float* bias;          /* [cout] fp32 or NULL                                            */
    const void* residual;       /* NHWC like y, or NULL                                           */
    int32_t res_mod;            /* 0, or residual pixel index = pixel % res_mod (pos-emb add)     */
    int32_t act;                /* mnet_act, applied after bias+residual                          */
    const float* post_scale;    /* [n][cout] or NULL: multiplied AFTER act — lets a StyledConv emit its
                                 * output already modulated by the NEXT layer's style (networks.py:283-284) */
    void* y;                    /* NHWC [n,ho,wo,cout]                                            */
    float* gn_partial;          /* NULL, or (ABI v4) GroupNorm partial sums of the OUTPUT, written by the epilogue that holds the values anyway:
                                 * [n*ho*wo / 32][cout / 32][2] fp32 = (sum, sum of squares) over 32 consecutive output pixels x the 32 channels of a
                                 * group (networks.py:487-493: GroupNorm(C/32 groups)), of the values as they leave the epilogue (after bias /
                                 * activation / post_scale, before the storage rounding); pixels at columns >= valid_w[n] are left out.  Fixed
                                 * reduction tree, independent of the tile configuration: the same bits for every launch size.  Removes the separate
                                 * statistics pass over the map (mnet_groupnorm_affine_from_partial folds them).  Needs an MNET_F16M launch the LDS-DMA /
                                 * strip kernels take, stride 1, cout % 32 == 0 and ho*wo % 32 == 0 — MNET_E_ARG otherwise (nothing is enqueued). */
} mnet_conv_desc;

int mnet_conv2d_nhwc(const mnet_conv_desc* d, void* stream);

/* same with an explicit kernel choice (A/B measurements, tests): AUTO picks the LDS-DMA kernel when the launch is
 * eligible (f16, (c0+c1) % 64 == 0, c0 % 64 == 0, cout >= 64, cout % 8 == 0, no in_scale, act <= LRELU_SQRT2, and a filter of
 * kh * kw <= 32 taps with kh, kw <= 8 — the tap mask of a pixel is one 32-bit word; any stride and any padding >= 0) and the
 * register-staged one otherwise (it takes every filter).
 * Address range of the LDS-DMA and strip kernels (they address a tile's activations with 31-bit byte offsets from a 64-bit per-tile base and form
 * pixel x bytes-per-pixel in a 24-bit multiply; the register-staged kernel uses 64-bit offsets throughout and has no such limit).  With
 *   I = 512 / (h * w) + 2   the images a 512-pixel tile may touch (2 for a map of more than 512 pixels; the batch n does not enter), and
 *   P = the physical halves per pixel of the wider source: max(c0, c1) for MNET_F16, twice that for MNET_F16X2 / MNET_F16M,
 *   K = kh * kw * (physical halves of c0 + c1),
 * a launch is eligible only if all of
 *   I * h * w < 2^23                 (24-bit pixel index)            2 * P < 2^23
 *   I * h * w * P * 2 < 2^31 - 1     (31-bit activation offsets)
 *   cout * K * 2 < 2^31 - 1          (31-bit weight offsets)         256 * K * 2 < 2^30
 * hold; the strip kernels further need h * w * (physical halves of c0) * 2 < 2^31 - 1 (one image per buffer descriptor).  Beyond them AUTO
 * answers MNET_CONV_ALGO_REG_STAGED and a pinned LDS-DMA or strip request is MNET_E_ARG.  Every launch needs n * h * w < 2^31 and
 * n * ho * wo < 2^31 (MNET_E_ARG "too many pixels"); element and byte offsets into x0 / x1 / residual / y are 64-bit in every kernel, so a
 * tensor may be larger than 2^32 bytes and hold more than 2^31 elements (tests/test_large_tensors_gpu.py).
 * MNET_CONV_ALGO_DMA_CFG0 + id pins one LDS-DMA tile configuration
 * (cout x pixel tile, waves, LDS stages):
 *   id 0: 256x256 16w 2st   1: 256x128 8w 3st   2: 128x256 8w 3st   3: 64x256 8w 3st   4: 128x512 16w 2st
 *      5: 64x512 8w 2st     6: 256x256 8w 2st (128x64 per wave)      — all on v_mfma_f32_16x16x32_f16 walking k in the
 *      same order (64-channel slice outer, filter tap inner): the same bits for every launch size (batch-invariant);
 *      the register-staged kernel walks k tap-outer (same products, fp32 partial sums associated differently)
 *   id 10: 128x128 8w 4st (3 slabs in flight: a lone small tile per CU exposes the load latency) — AUTO's choice when ids 1 / 2 would give fewer than 200 workgroups (one strip at a time)
 *   id 8 / 9: ids 0 / 4 with the next slab's DMA pieces issued between the two half slabs instead of right after the slab barrier
 *      (AUTO's choice for >= 65536 output pixels: +2.8 % on the 256x256 tile; same MFMA sequence, same bits)
 *   id 7: id 0 on v_mfma_f32_32x32x16_f16 (experimental)
 *   MNET_F16X2 launches: ids 0-6 and 10 as above on the split-half form, id 7 = 128x512 8w (64x128 per wave), ids 8 / 9 = ids 6 / 7
 *      with the DMA pieces issued after the first multiply group, ids 11 / 12 = ids 8 / 9 with the LDS reads placed by scheduling
 *      hints; AUTO takes the 8-wave tiles 11 (cout >= 256) / 9 (cout 128) for >= 65536 output pixels
 *   MNET_F16M launches: ids 0-5, 10 = the same tile shapes on v_mfma_f32_32x32x16_f16 + v_mfma_scale_f32_32x32x64_f8f6f4, id 6 = 256x256
 *      8w (128x64 per wave), id 7 / 8 = 128x512 8w (64x128 / 128x64 per wave), ids 11 / 12 / 13 = ids 6 / 8 / 5 with the LDS reads
 *      placed by scheduling hints; ids 15 / 9 (round 4) = ids 6 / 8 with the slab loop software-pipelined across the slab barrier (the scaled
 *      MFMAs of slab s-1 and one DMA piece of slab s+1 behind each, then the f16 MFMAs of slab s); AUTO takes 15 (cout >= 256) / 8 (cout 128) /
 *      13 (cout 64) for >= 65536 output pixels; every id runs the same MFMA sequence per output (same bytes whatever the launch size selects,
 *      signed zeros included: an absent bias adds nothing, so a -0 stays a -0);
 *      id 14: DIAGNOSTIC build (per-phase cycle sums written over the output, tools/slab_phases.py), refused unless MNET_ALLOW_DIAGNOSTIC_KERNELS=1
 *   MNET_F16 ids 11-15 ONLY: diagnostic builds used by tools/wg_timeline.py and tools/conv_bench.py; they produce WRONG results and
 *      are refused (MNET_E_ARG) unless the process sets MNET_ALLOW_DIAGNOSTIC_KERNELS=1 */
enum { MNET_CONV_ALGO_AUTO = 0, MNET_CONV_ALGO_REG_STAGED = 1, MNET_CONV_ALGO_LDS_DMA = 2,
       MNET_CONV_ALGO_SKINNY = 3 /* fp32 1x1 over <= 512 pixels straight from global memory (the TextViT linears of a small batch;
                                  * 16 x 64 tiles).  AUTO uses it when eligible; bit-identical to REG_STAGED. */,
       MNET_CONV_ALGO_DMA_CFG0 = 16,
       MNET_CONV_ALGO_STRIP_CFG0 = 32 /* + id: the 3x3 "strip" LDS-DMA kernel (one activation strip per filter row shared by its
                                        * three taps; id 0: 256x256 tile, id 1: 64x512 tile).  Eligible: 3x3/stride 1/pad 1, one
                                        * source, cout >= 256 (id 0) or < 128 (id 1), >= 65536 output pixels, whole-row tiles.
                                        * AUTO uses id 1 when eligible (id 0 measured neutral: explicit request only; MNET_F16X2: id 1 only; MNET_F16M: id 1, and id 0 as an
                                        * 8-wave 256x256 tile on explicit request — measured -3 ... -5 %).  Same k order and MFMA as the LDS-DMA kernel → identical bits. */,
       MNET_CONV_ALGO_DMA_CFG16 = 64 /* + (id - 16): LDS-DMA tile configurations 16.. (the ids 0..15 above are full):
                                       *   id 16: 256x256 8w 2st (128x64 per wave) with both half slabs' operand fragments requested up front and the
                                       *          next slab's DMA pieces issued between the halves — AUTO's f16 choice for cout >= 256, >= 65536 pixels
                                       *   id 17: the same form of the 128x512 tile (64x128 per wave)
                                       * same MFMA sequence as ids 0-6: identical bits.
                                       *   MNET_F16M launches, id 16 (round 6): the 256x256 tile with ONE wave per SIMD — 4 waves x 128x128 outputs, the accumulators
                                       *          in the accumulator register file (conv_dma_w4.hip) — AUTO's fp16+8 choice for cout >= 256, >= 65536 pixels; writes
                                       *          mnet_conv_desc.gn_partial itself; same MFMA sequence per output as the fp16+8 ids 0-15: identical bytes */,
       MNET_CONV_ALGO_FLAG_ONE_TILE = 256 /* OR-ed in: LDS-DMA kernel launched with one workgroup per tile instead of its
                                            * persistent grid (A/B measurements only; same results) */,
       MNET_CONV_ALGO_FLAG_X1_CENTER = 512 /* OR-ed in (round 4): the SECOND source x1 contributes through the filter's CENTRE tap only —
                                             * y = conv_khxkw(x0; W[:, :, :, :c0]) + conv_1x1(x1; W[:, kh/2, kw/2, c0:]) in ONE k-loop: the 1x1
                                             * skip convolution of ResTextBlockV2 (models/networks.py:504-505,514-515: h + conv_out(x)) folded
                                             * into its conv2 as extra K instead of a separate launch + a residual read.  wgt is the ordinary
                                             * [cout][kh][kw][c0+c1] tensor whose x1 part is only read at the centre tap; x1 is NHWC
                                             * [n,h,w,c1] like x0 (stride 1 launches).  LDS-DMA kernel only (MNET_E_ARG when the launch is
                                             * not eligible for it); mnet_conv2d_flops still counts x1 at every tap. */,
       MNET_CONV_ALGO_FLAG_SHUFFLE2 = 1024 /* OR-ed in: pixel-shuffle output mode — conv3x3(bilinear_x2(x)) in polyphase form.  The launch is the
                                             * 3x3 / stride 1 / pad 1 conv on the LOW-res map [n,h,w,c0] with cout = 4 C output channels, phase-major
                                             * (channel (2 py + px) C + c is phase (py,px) of channel c; wgt and bias packed accordingly), and y is
                                             * the [n,2h,2w,C] tensor: channel block b of low-res pixel (i,j) is stored as block b % (C/32) of
                                             * hi-res pixel (2i + py, 2j + px), (py,px) = b / (C/32).  gn_partial keeps its [n*h*w/32][cout/32][2]
                                             * layout — which IS [n*2h*2w/32][C/32][2] of y — with the low-res border ring (i in {0,h-1} or j in
                                             * {0,w-1}: the hi-res ring the caller rewrites, mnet_polyphase_ring_fix) left out of the sums.
                                             * MNET_F16M, one source, C % 32 == 0, h, w >= 4, w % 32 == 0, no residual / scale vectors / valid_w,
                                             * and only on the LDS-DMA builds that carry the mode (AUTO picks one; ids 10, 15, 16): MNET_E_ARG
                                             * otherwise, nothing enqueued. */,
       MNET_CONV_ALGO_FLAG_F32_OUT = 2048 /* OR-ed in: fp32 output of an MNET_F16M launch — x0 / x1 / wgt in fp16+8 as always, y is a plain fp32 [n,ho,wo,cout]
                                            * tensor (128-byte aligned; the same 4 bytes per element) that holds the value the fp16+8 launch would encode, before
                                            * its rounding: an intermediate with one reader (the tap planes of mnet_upfold3x3_f32z_nhwc, marconet_hip_upfold_f32.h)
                                            * pays neither the encode nor the decode.  Accepted only with no bias, no out_scale / post_scale, no residual, no
                                            * gn_partial, no valid_w, no input transform, act = MNET_ACT_NONE, and only where the launch resolves to the one-wave
                                            * tile (LDS-DMA id 16: AUTO names it whatever the launch size; ho * wo % 32 == 0, <= 512 k-slabs): MNET_E_ARG
                                            * otherwise, from mnet_conv2d_plan as from the launch, nothing enqueued. */,
       MNET_CONV_ALGO_FLAGS = 256 | 512 | 1024 | 2048 };
int mnet_conv2d_nhwc_ex(const mnet_conv_desc* d, int32_t algo, void* stream);

/* split-K form of the skinny kernel for a "patchify" conv (filter == stride, no padding; fp32; <= 512 output pixels) — the
 * TextViT patch embedding of a small batch (8x8 / stride 8 over [B,8,512,512]: K = 32768, 64 tokens per strip: one workgroup
 * per 16 channels would stream 2 MiB of weights alone).  K is cut into `ksplit` contiguous slices (a multiple of kh; each a
 * whole number of 16-float steps of one filter row), raw fp32 partial sums go to workspace [ksplit][n*ho*wo][cout] and a
 * second launch folds them in slice order and applies the epilogue — deterministic; differs from mnet_conv2d_nhwc only in
 * the association of the fp32 sum. */
int mnet_conv2d_splitk(const mnet_conv_desc* d, int32_t ksplit, float* workspace, void* stream);

/* the kernel that runs this launch under `algo`, without launching: MNET_CONV_ALGO_REG_STAGED, MNET_CONV_ALGO_SKINNY,
 * MNET_CONV_ALGO_DMA_CFG0 / MNET_CONV_ALGO_DMA_CFG16 + id or MNET_CONV_ALGO_STRIP_CFG0 + id; negative MNET_E_* exactly when
 * mnet_conv2d_nhwc_ex refuses the launch (bench.py buckets its timings by this).  A pinned LDS-DMA id, like AUTO's choice, is
 * handed over to another build when its own is not made for the launch (same tile shape, same bytes), and this returns the id that runs:
 *   MNET_F16M, id 16 with an activation other than NONE / LRELU / LRELU_SQRT2, ho * wo not a multiple of 32 or more than 512 k-slabs → id 15
 *   MNET_F16M, id 9 with gn_partial → id 8
 * An id with no build for the storage type (e.g. MNET_F16X2 id 13, the diagnostic ids without MNET_ALLOW_DIAGNOSTIC_KERNELS=1) is MNET_E_ARG. */
int mnet_conv2d_plan(const mnet_conv_desc* d, int32_t algo);

/* 2*MACs of the launch described by d (for roofline accounting in bench.py) */
double mnet_conv2d_flops(const mnet_conv_desc* d);

/* ---------------------------------------------------------------------------------------------
 * layout changes at the module boundary (reference tensors are NCHW fp32, models/networks.py:42,61,411)
 * ------------------------------------------------------------------------------------------- */
/* src fp32 NCHW [n,c,h,w] -> dst NHWC [n,h,w,c_ld] (channels c..c_ld-1 written as zero) */
int mnet_nchw_to_nhwc(const float* src, void* dst, int32_t dst_dtype, int32_t n, int32_t c, int32_t h,
                      int32_t w, int32_t c_ld, void* stream);
/* src NHWC [n,h,w,c_ld] (first c channels used) -> dst fp32 NCHW [n,c,h,w] */
int mnet_nhwc_to_nchw(const void* src, int32_t src_dtype, float* dst, int32_t n, int32_t c, int32_t h,
                      int32_t w, int32_t c_ld, void* stream);

/* K6: bilinear x2, align_corners=False (== polyphase [1/4,3/4] with edge clamp), NHWC, c % 4 == 0 (f32)
 * / c % 8 == 0 (f16).  nn.Upsample / F.interpolate at networks.py:268,318,360,370,415,416 */
int mnet_upsample2x_nhwc(const void* src, void* dst, int32_t dtype, int32_t n, int32_t h, int32_t w,
                         int32_t c, void* stream);
/* same, output multiplied by scale[n][c] (fp32, may be NULL): the style modulation of an up-sampling StyledConv
 * applied once per element here instead of once per filter tap inside the conv (networks.py:283-296) */
int mnet_upsample2x_scale_nhwc(const void* src, void* dst, int32_t dtype, int32_t n, int32_t h, int32_t w,
                               int32_t c, const float* scale, void* stream);
/* the same with the output in another storage type: dst_dtype == dtype, or MNET_F16 for an MNET_F16X2 / MNET_F16M input (the batched
 * driver's image-only generator level, models/networks.py:161-164, reads the 64-px prior in the mode's storage and continues in plain
 * f16 — no separate mnet_convert pass over that map) */
int mnet_upsample2x_convert_nhwc(const void* src, int32_t dtype, void* dst, int32_t dst_dtype, int32_t n, int32_t h, int32_t w,
                                 int32_t c, const float* scale, void* stream);

/* K11 apply: y = f(x * scale[n,c] + shift[n,c]), f = swish if swish else identity (shift may be NULL).
 * GroupNorm-normalise + swish once per element (networks.py:508-509,511-512) — the conv prologue form of the same
 * math costs 9 taps x Cout/128 tiles of redundant expf.  x, y NHWC [n, hw, c]; in-place (y == x) allowed. */
int mnet_affine_act_nhwc(const void* x, void* y, int32_t dtype, int32_t n, int32_t hw, int32_t c,
                         const float* scale, const float* shift, int32_t swish, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K11 GroupNorm statistics (groups of 32 channels, eps, affine), networks.py:487-490 — produces the
 * per-(n,channel) affine consumed by mnet_conv2d_nhwc's prologue:
 *   scale[n,c] = rstd[n,g]*gamma[c] ; shift[n,c] = beta[c] - mean[n,g]*rstd[n,g]*gamma[c]
 * Statistics are over h x valid_w[n] x 32 channels (biased variance), accumulated in fp64.
 * partial: caller workspace of  n * slices * (c/32) * 2  doubles.
 * ------------------------------------------------------------------------------------------- */
int mnet_groupnorm_affine(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c,
                          const int32_t* valid_w, const float* gamma, const float* beta, float eps,
                          double* partial, int32_t slices, float* scale, float* shift, void* stream);
/* the same affine from the partial sums a convolution's epilogue wrote (mnet_conv_desc.gn_partial: [n*h*w/32][c/32][2] fp32): fp64 fold in a fixed
 * order, count = h * min(valid_w[n], w) * 32 per group.  One wave per (image, group): no pass over the map. */
int mnet_groupnorm_affine_from_partial(const float* partial, int32_t n, int32_t h, int32_t w, int32_t c, const int32_t* valid_w,
                                       const float* gamma, const float* beta, float eps, float* scale, float* shift, void* stream);

/* Ring fix-up of a MNET_CONV_ALGO_FLAG_SHUFFLE2 convolution's output y [n,h2,w2,c] (MNET_F16M; h2 = 2h, w2 = 2w): hi-res rows and columns {0, 1, last two} are
 * copied from the two-launch form (up-sample + conv) run on four thin strips — top / bottom [n,4,w2,c] (low-res rows 0..1 / h-2..h-1: their hi-res rows 0..1 / 2..3 are
 * kept, all columns), left / right [n,h2,4,c] (low-res columns 0..1 / w-2..w-1: hi-res columns 0..1 / 2..3, rows 2..h2-3).  sums [n][c/32][2] (fp64) receives the sum and
 * the sum of squares of the stored ring values per (image, 32-channel group), folded in a fixed order. */
int mnet_polyphase_ring_fix(const void* top, const void* bottom, const void* left, const void* right, void* y, int32_t dtype,
                            int32_t n, int32_t h2, int32_t w2, int32_t c, double* sums, void* stream);
/* mnet_groupnorm_affine_from_partial for such an output [n,h,w,c] (hi-res): the main launch's partial sums (border ring left out) plus ring_sums */
int mnet_groupnorm_affine_from_partial_ring(const float* partial, const double* ring_sums, int32_t n, int32_t h, int32_t w, int32_t c,
                                            const float* gamma, const float* beta, float eps, float* scale, float* shift, void* stream);

/* ---------------------------------------------------------------------------------------------
 * per-glyph prior transform of TSPSRNet (networks.py:421-449 and :455-482)
 * Glyph g belongs to image g_img[g]; it covers feature columns [g_x1[g], g_x1[g]+g_w[g]) and prior
 * columns [g_y1[g], g_y1[g]+g_w[g]);  S = prior size (32 or 64) = feature height = max window width.
 * ------------------------------------------------------------------------------------------- */
/* K12+K13 crop + AdaIN + concat:  out [G,S,S,2C]
 *   out[g,y,x,0:C]  = (prior[g,y,y1+x,:] - mean_p)/std_p * std_f + mean_f   (unbiased var + 1e-5, :518-533)
 *   out[g,y,x,C:2C] = feat[img,y,x1+x,:]                                    for x < g_w[g]; 0 beyond */
int mnet_adain_crop_concat(const void* prior, const void* feat, void* out, int32_t dtype, int32_t G,
                           int32_t S, int32_t C, int32_t feat_w, const int32_t* g_img,
                           const int32_t* g_x1, const int32_t* g_y1, const int32_t* g_w, void* stream);

/* same, and additionally the GroupNorm (2C/32 groups of 32 channels, biased variance, eps) affine of the [G,S,S,2C] OUTPUT
 * over each glyph's window — norm1 of conv_32_fuse / conv_64_fuse (networks.py:508) — in closed form from the AdaIN
 * statistics the kernel has anyway (no further pass over the tensor):  scale[g,c] = rstd[g,grp]*gamma[c],
 * shift[g,c] = beta[c] - mean[g,grp]*rstd[g,grp]*gamma[c];  gamma, beta fp32 [2C];  scale, shift fp32 [G][2C] */
int mnet_adain_crop_concat_gn(const void* prior, const void* feat, void* out, int32_t dtype, int32_t G,
                              int32_t S, int32_t C, int32_t feat_w, const int32_t* g_img,
                              const int32_t* g_x1, const int32_t* g_y1, const int32_t* g_w,
                              const float* gamma, const float* beta, float eps, float* scale, float* shift, void* stream);

/* the same result from three launches that spread each glyph over `slices` workgroups — for FEW glyphs (one strip at a time:
 * the one-workgroup-per-glyph kernel above is then a 380 us latency chain).  gamma/beta/scale/shift may all be NULL (no
 * GroupNorm affine).  Scratch owned by the caller: partial fp64 [G][slices][C][4], stat fp32 [G][4][C].  Agrees with the
 * fused kernel up to the association of the fp64 statistic sums. */
int mnet_adain_crop_concat_split(const void* prior, const void* feat, void* out, int32_t dtype, int32_t G,
                                 int32_t S, int32_t C, int32_t feat_w, const int32_t* g_img,
                                 const int32_t* g_x1, const int32_t* g_y1, const int32_t* g_w,
                                 const float* gamma, const float* beta, float eps, float* scale, float* shift,
                                 double* partial, float* stat, int32_t slices, void* stream);

/* K13 ordered scatter:  out[b,y,x,:] = feat + (feat*scale[g,y,x-x1,:] + shift[g,y,x-x1,:]) for the LAST
 * glyph g of image b whose window covers x (later glyph overwrites earlier, :448,481); out = feat where
 * no window covers x.  Glyphs of image b are g_start[b] .. g_start[b+1]-1. */
int mnet_glyph_scatter_affine(const void* feat, const void* scale, const void* shift, void* out,
                              int32_t dtype, int32_t B, int32_t S, int32_t C, int32_t feat_w,
                              const int32_t* g_start, const int32_t* g_x1, const int32_t* g_w,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * TextViT pieces (fp32 only), models/textvit_arch.py
 * ------------------------------------------------------------------------------------------- */
/* K9 LayerNorm over the last dim (eps 1e-5, biased var): y[r,:] = (x[r,:]-mean)*rstd*gamma+beta */
int mnet_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t rows,
                   int32_t d, float eps, void* stream);
/* K9 token-axis LayerNorm + Linear (linear_seq_maxlen :141-144,155 ; linear_w_maxlen :59-62,72):
 *   y[b,j,d] = bias[j] + sum_t W[j,t] * LN_t(x[b,:,d])[t]      x [B,T,D], y [B,J,D], T <= 64 */
int mnet_token_mix(const float* x, const float* ln_g, const float* ln_b, const float* wgt,
                   const float* bias, float* y, int32_t B, int32_t T, int32_t D, int32_t J, float eps,
                   void* stream);
/* K8 softmax(q k^T * scale) v per (batch, head) on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products — the character
 * indices downstream stay bit-exact); qkv [B,N,3*H*64] packed (q|k|v, each '(h d)'),
 * out [B,N,H*64]; N <= 64, head dim 64   (textvit_arch.py:104-112) */
int mnet_attention(const float* qkv, float* out, int32_t B, int32_t N, int32_t H, float scale,
                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * TSPGAN pieces, models/networks.py
 * ------------------------------------------------------------------------------------------- */
/* K15 PixelNorm: y = x * rsqrt(mean(x^2, dim=1) + 1e-8)   (:170-171), x [N,D] fp32 */
int mnet_pixelnorm(const float* x, float* y, int32_t N, int32_t D, void* stream);
/* K14 SelectText: out NHWC [N,4,4*nc,C] = emb[labels[i,j],:] tiled 4x4, chars side by side (:205-215).
 * labels int64 [N,nc]; returns MNET_E_ARG-free: out-of-range labels must be rejected by the caller. */
int mnet_embed_gather(const float* emb, const int64_t* labels, void* out, int32_t dtype, int32_t N,
                      int32_t nc, int32_t C, int32_t num_classes, void* stream);
/* the same with out[i,y,x,c] multiplied by scale[i,c] (fp32 [N,C], may be NULL) before it is rounded to the storage type: the gathered
 * constant is read by nothing but the first StyledConv (:289-290), whose input modulation x * s (:284, activation side: SURVEY.md §0.5)
 * this applies — that conv then needs no modulation prologue */
int mnet_embed_gather_scaled(const float* emb, const int64_t* labels, const float* scale, void* out, int32_t dtype, int32_t N,
                             int32_t nc, int32_t C, int32_t num_classes, void* stream);
/* demod[n,o] = rsqrt( sum_i style[n,i]^2 * wsq_t[i,o] + 1e-8 ),  wsq_t[i,o] = scale^2 * sum_k W[o,i,k]^2
 * (ModulatedConv2d :284-287 rewritten for activation-side modulation); N <= 65535, cin <= 16384 (MNET_E_ARG) */
int mnet_demod(const float* style, const float* wsq_t, float* demod, int32_t N, int32_t cin,
               int32_t cout, void* stream);

/* mnet_demod with eps scaled per sample: demod[n,o] = rsqrt( sum_i style[n,i]^2 wsq_t[i,o] + 1e-8 * eps_scale[n] ) — for style rows that
 * mnet_style_rows normalised by 2^-e (eps_scale = 4^-e): the result is then exactly 2^e times mnet_demod of the original row.
 * eps_scale == NULL: mnet_demod. */
int mnet_demod_scaled(const float* style, const float* wsq_t, float* demod, int32_t N, int32_t cin, int32_t cout,
                      const float* eps_scale, void* stream);

/* argmax over the last dim (first maximal index, like torch.max(...,1)[1] in test_w.py:36) */
int mnet_argmax_rows(const float* x, int64_t* idx, int32_t rows, int32_t d, void* stream);

/* flat dtype conversion (count % 4 == 0), used where the fp16 conv stack hands over to the fp32 ViT */
int mnet_convert(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t count, void* stream);

/* K5 standalone: the operator boundary the reference itself has — basicsr.ops.fused_act.fused_leaky_relu
 * (models/networks.py:10,195,241): y = scale * leaky_relu(x + bias[(i/inner) % C], negative_slope) on a
 * contiguous fp32 tensor viewed as [outer, C, inner].  bias may be NULL.  (On the hot path this math is
 * fused into mnet_conv2d_nhwc's epilogue.) */
int mnet_fused_bias_act(const float* x, const float* bias, float* y, int64_t total, int32_t C, int32_t inner,
                        float negative_slope, float scale, void* stream);

/* ToRGB.forward (models/networks.py:313-321; call sites :148,157): modulated 1x1 conv to RGB without demodulation + bias + the
 * bilinearly up-sampled (x2, align_corners=False) RGB image of the level below, then tanh — one streaming pass over x.
 *   out[n,y,x,o] = tanh( scale_b[n] * sum_c wgt[o][c] * (x[n,y,x,c] * style[n][c]) + bias[o] + up2(skip)[n,y,x,o] ),  out[..,3] = 0
 * x NHWC [n,h,w,c] in any storage dtype (c in {64,128,256,512}); wgt fp32 [3][c] (the layer's constant scale folded); style fp32 [n][c];
 * scale_b fp32 [n] or NULL (1); bias fp32 [3]; skip fp32 [n,h/2,w/2,4] or NULL (its channel 3 is read and ignored); out fp32 [n,h,w,4].
 * Overflow rule (every storage dtype): a pre-activation that is not finite — an inf or NaN element of x, a sum that overflowed fp32 — is
 * stored as NaN, never as tanh's +-1, so that a finiteness check of the image sees it; out[..,3] stays +0 and no other pixel changes. */
int mnet_torgb(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, const float* wgt, const float* style,
               const float* scale_b, const float* bias, const float* skip, float* out, void* stream);

/* 3x3 / stride 1 / pad 1 convolution of a cin = 64 map to 3 output channels + bias (+ tanh): the last layer of TSPSRNet
 * (conv_final.6 + Tanh, models/networks.py:374-375).  x NHWC [n,h,w,64] in any storage dtype; wgt [3][3][3][64] (cout, kh, kw, cin) in
 * the same dtype for MNET_F16 / MNET_F32; bias fp32 [3]; act MNET_ACT_NONE or MNET_ACT_TANH.  Outputs (either may be NULL, not both): y_nhwc
 * [n,h,w,8] in the input dtype (channels 3..7 zero) and y_nchw fp32 [n,3,h,w] — the tensor the module returns, without a
 * separate layout pass (in f16 mode it holds the same f16-rounded values as y_nhwc).
 * A split-half (MNET_F16X2) or fp16+8 (MNET_F16M) x is decoded to fp32 while it is staged: wgt is then plain fp32 [3][3][3][64] (not the
 * packed conv-weight layout), y_nhwc is fp32 [n,h,w,8], the arithmetic is the fp32 one, and x must be 128-byte aligned.
 * Overflow rule (MNET_ACT_TANH): with a half-range input (MNET_F16, MNET_F16X2, MNET_F16M) an infinite or NaN pre-activation is stored as
 * NaN in both outputs, never as tanh's +-1, so that a finiteness check of the image sees it.  An MNET_F32 input is plain tanhf: +-inf
 * gives exactly +-1.  MNET_ACT_NONE stores the pre-activation as it is. */
int mnet_conv3x3_rgb(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t cin, const void* wgt,
                     const float* bias, int32_t act, void* y_nhwc, float* y_nchw, void* stream);

/* K19, the script's output post-processing (test_sr.py:198-200): sr*0.5+0.5 → HWC → RGB→BGR → clip(0,1)*255.
 * src NHWC [npix][c_ld] (RGB in channels 0..2, f32 or f16); dst [npix][3] BGR as float32 (dst_u8 == 0: exactly what the
 * script hands to cv2.imwrite) or uint8 (dst_u8 != 0: cv2's float→uchar conversion, round half to even) — 4x fewer bytes
 * for the device→host copy and the multi-GPU all-gather (SURVEY.md §8f NEXT-1) */
int mnet_sr_postprocess(const void* src, int32_t src_dtype, void* dst, int32_t dst_u8, int64_t npix, int32_t c_ld, void* stream);

/* a17 on the device, the script's input pre-processing (test_sr.py:98-115; the input-side counterpart of mnet_sr_postprocess): a ragged batch of
 * tightly packed uint8 RGB images [h][w][3] in ONE buffer → one launch that resizes every image to height dst_h with cv2's 8-bit INTER_CUBIC
 * arithmetic (marconet_amd/lq_io.py::resize_cubic, bit for bit: fp64 sample positions, fp32 A = -0.75 weights rounded operation by operation,
 * 11-bit integer taps, BORDER_REPLICATE, both passes in integers, clip((v + 2^21) >> 22, 0, 255)) and pastes it at the left of a canvas_w wide canvas:
 *   MNET_LQ_FORM_F32_NCHW  dst fp32 [n][3][dst_h][canvas_w] = (u8 / 255 - 0.5) / 0.5 (ToTensor + Normalize, correctly rounded fp32: torch's values);
 *                          columns >= dw are -1.0 (normalised black) — the encoder's LQ with dst_h = 32, canvas_w = 512
 *   MNET_LQ_FORM_U8_HWC    dst uint8 [n][dst_h][canvas_w][3]; columns >= dw are 0 — the panel's preview (ShowLQ, test_sr.py:99) with dst_h = 128
 * The WHOLE destination is written (no clearing by the caller).  `images`: a DEVICE table of n descriptors.  The caller computes per image only
 * scalars: dw = the resized width (<= canvas_w; larger values are clamped) and scale = 1.0 / ((double)dst_h / h), which serves both axes as in the
 * script (fx = fy).  Source indices are clamped into [0, h) x [0, w) of the image at `offset`: a table whose images lie inside src cannot take the
 * kernel out of range.  MNET_E_ARG (nothing enqueued, checked before any HIP call) for a null pointer, n <= 0, dst_h < 1, canvas_w < 1, an unknown form. */
typedef struct {
    int64_t offset;             /* byte offset of the image's first pixel in src (any alignment)   */
    int32_t h, w;               /* source size                                                      */
    int32_t dw;                 /* resized width: columns [0, dw) carry the image, the rest the fill */
    int32_t reserved;           /* 0                                                                */
    double scale;               /* 1.0 / (dst_h / h): source step per destination pixel, both axes  */
} mnet_lq_image;
enum { MNET_LQ_FORM_F32_NCHW = 0, MNET_LQ_FORM_U8_HWC = 1 };
int mnet_lq_from_u8(const uint8_t* src, const mnet_lq_image* images, int32_t n, int32_t dst_h, int32_t canvas_w, void* dst, int32_t form,
                    void* stream);

/* a17 on the device, the output side (test_sr.py:203-232; the counterpart of mnet_lq_from_u8's preview form): ONE launch composes, for every strip of
 * a batch, the panel the script saves — dst uint8 [n][512][out_w][3] in the FILE's order (RGB), the bytes of
 * marconet_amd/lq_io.py::panel_rgb_u8(panel(...)): clip(rint(panel), 0, 255) flipped BGR → RGB.  Rows of strip k, columns < show_w (the rest is 0;
 * the WHOLE destination is written):
 *     0..127   preview[preview_index][y][x][:]                      (uint8 [.][128][preview_w][3] RGB: mnet_lq_from_u8, MNET_LQ_FORM_U8_HWC)
 *   128..255   the same, with (255,0,0) in rows 128..191 where x lies in a glyph's interval [a,b) and (0,0,255) in rows 192..255 where it lies in
 *              [r,t): marks int32 [.][4] = a,b,r,t per glyph, rows glyph0 .. glyph0 + n_glyphs - 1 (the script's slices, resolved by the caller)
 *   256..383   sr_bgr[k][y][x][2-c]                                  (uint8 [n][128][sr_w][3] BGR: mnet_sr_postprocess)
 *   384..511   the strip's n_glyphs structure images side by side (prior_nhwc4 fp32 [.][128][128][4], RGB in channels 0..2, 16-byte aligned),
 *              p * 0.5 + 0.5, resized to show_w columns with cv2's INTER_LINEAR arithmetic (lq_io.resize_linear: fp64 sample position
 *              (x + 0.5) * step - 0.5, two taps, border clamp, fp32 p0 (1 - t) + p1 t, every operation rounded separately), * 255, rounded half to
 *              even and saturated; file channel c = image channel 2 - c (the script stacks this RGB row into its BGR array as it is)
 * `strips`: a DEVICE table of n descriptors; the caller computes per strip only scalars (step = 128.0 * n_glyphs / show_w).  A descriptor with
 * show_w outside [0, out_w], a negative index or n_glyphs outside [1, 65536] is written as fill and not followed; indices that lie inside the
 * tensors cannot take the kernel out of range.  MNET_E_ARG (nothing enqueued, checked before any HIP call) for a null pointer, n <= 0, out_w < 1,
 * preview_w < out_w, sr_w < 1; MNET_E_ALIGN for a misaligned prior_nhwc4 (16), strips (8) or marks (4). */
typedef struct {
    int32_t show_w;             /* the strip's width at height 128: columns [0, show_w) carry the panel, the rest is 0 */
    int32_t preview_index;      /* the strip's image in `preview`                                                      */
    int32_t glyph0, n_glyphs;   /* its structure images in `prior_nhwc4` and its rows in `marks`                       */
    double step;                /* 128.0 * n_glyphs / show_w: source step per destination column of the last row block */
} mnet_panel_strip;
int mnet_panel_u8(const uint8_t* preview, int32_t preview_w, const uint8_t* sr_bgr, int32_t sr_w, const float* prior_nhwc4,
                  const mnet_panel_strip* strips, const int32_t* marks, int32_t n, int32_t out_w, uint8_t* dst, void* stream);

/* Long text lines (no counterpart in the script: test_sr.py:108-110 refuses a strip wider than 512 px at height 32 and tells its user to crop it):
 * ONE launch joins, for every line of a batch, the restored windows of the line — dst uint8 [n_lines][rows][out_w][3] in sr's channel order, the
 * bytes of marconet_amd/long_lines.py::stitch_host.  sr uint8 [n_sr][rows][sr_w][3] (mnet_sr_postprocess: rows = 128, sr_w = 2048 in the product).
 * Line l owns windows[win0 .. win0 + n_win - 1]; window w shows columns [0, show_w) of sr[sr_index] at columns [offset, offset + show_w) of its line.
 * Column x < the line's out_w (the rest is 0; the WHOLE destination is written):
 *     in one window           sr[sr_index][y][x - offset][:]
 *     in windows k and k + 1  per channel (a (2 D - 2 t - 1) + b (2 t + 1) + D) / (2 D) in integers (csrc/stitch_blend.h), a from window k, b from
 *                             window k + 1, over the overlap [A, B) = [offset_{k+1}, offset_k + show_w_k): D = B - A, t = x - A
 * `lines`, `windows`: DEVICE tables.  A line is written as fill and not followed if a window of it has sr_index outside [0, n_sr), show_w outside
 * [1, sr_w] or a negative offset, if its offsets do not increase strictly, if a column of it lies in three windows or in none, or if n_win is outside
 * [1, 65536], win0 negative or its out_w outside [0, out_w]; the lines next to it are not affected.  Indices that lie inside the tensors cannot take
 * the kernel out of range.  MNET_E_ARG (nothing enqueued, checked before any HIP call) for a null pointer, n_lines <= 0, rows < 1, sr_w < 1 (or
 * beyond 2^22, the range of the blend's 32-bit arithmetic), out_w < 1, n_sr < 1; MNET_E_ALIGN for a table that is not 4-byte aligned. */
typedef struct {
    int32_t out_w;              /* the line's width: columns [0, out_w) carry the joined line, the rest is 0 */
    int32_t win0, n_win;        /* its windows in `windows`                                                 */
    int32_t reserved;           /* 0                                                                        */
} mnet_stitch_line;
typedef struct {
    int32_t sr_index;           /* the window's image in `sr`                                               */
    int32_t offset;             /* its first column in the line                                             */
    int32_t show_w;             /* its width: columns [0, show_w) of the image are shown                    */
    int32_t reserved;           /* 0                                                                        */
} mnet_stitch_window;
int mnet_stitch_u8(const uint8_t* sr, int32_t n_sr, int32_t rows, int32_t sr_w, const mnet_stitch_line* lines, const mnet_stitch_window* windows,
                   int32_t n_lines, int32_t out_w, uint8_t* dst, void* stream);

/* The page (no counterpart in the script, which ends at the restored strip): ONE launch brings every restored text line of a page to its rectangle
 * of the enlarged page and blends it in — the bytes of marconet_amd/pages.py::paste_host, region by region.  lines uint8 [n_lines][rows][line_w][3]
 * BGR (mnet_stitch_u8's result: rows = 128 in the product); page uint8 [page_h][page_w][3] RGB, which already holds the background (the enlarged
 * page: mnet_lq_from_u8, MNET_LQ_FORM_U8_HWC) and is modified IN PLACE, inside the regions' rectangles only.  Region r shows columns [0, src_w) of
 * lines[line_index] in the rectangle [x0, x0 + rw) x [y0, y0 + rh) of the page:
 *   1. every k x k block of the line (k x c, c < k, at a ragged right edge) → per channel (2 sum + cnt) / (2 cnt) in integers (csrc/page_blend.h):
 *      an intermediate of rows / k rows and ceil(src_w / k) columns, each value a byte;
 *   2. that intermediate → exactly rw x rh with mnet_lq_from_u8's 8-bit INTER_CUBIC arithmetic (the taps of csrc/lq_taps.h at the sampling steps
 *      scale_x, scale_y; both passes in integers; clip((v + 2^21) >> 22, 0, 255)); BGR → RGB;
 *   3. feather = 0: the pixel is that byte; else, at local (u, v), a = min(2 min(u, rw - 1 - u) + 1, 2 feather), b the same on (v, rh), m = a b,
 *      D = 4 feather^2: (bg (D - m) + fg m + D / 2) / D in integers (csrc/page_blend.h).
 * `regions`: a DEVICE table; the caller computes per region only scalars.  A region's rectangle is left untouched (the background stays; the other
 * regions are not affected) if line_index lies outside [0, n_lines), src_w outside [1, line_w], the rectangle not inside the page, rw or rh < 1,
 * feather outside [0, 1024], k is not 1, 2, 4 or 8, or rows % k != 0; a table cannot take the kernel out of its buffers.  Rectangles that overlap
 * give unspecified bytes inside the overlap and nothing outside it.  MNET_E_ARG (nothing enqueued, checked before any HIP call) for a null pointer,
 * n_lines < 1, rows < 1, line_w < 1, n_regions < 1, page_h < 1, page_w < 1, or more than 2^31 - 1 tiles (n_regions x the page's 64 x 16 tiles);
 * MNET_E_ALIGN for a table that is not 8-byte aligned. */
typedef struct {
    int32_t line_index;         /* the region's line in `lines`                                              */
    int32_t src_w;              /* the line's width: columns [0, src_w) are shown                            */
    int32_t x0, y0;             /* the rectangle's top left corner in the page                               */
    int32_t rw, rh;             /* its size                                                                  */
    int32_t feather;            /* 0 .. 1024: width of the blend ramp in page pixels, 0 for none             */
    int32_t k;                  /* the box reduction: 1, 2, 4 or 8                                           */
    double scale_x;             /* 1.0 / (rw / ceil(src_w / k)): intermediate step per destination column    */
    double scale_y;             /* 1.0 / (rh / (rows / k)): the same for rows                                */
} mnet_paste_region;
int mnet_paste_u8(const uint8_t* lines, int32_t n_lines, int32_t rows, int32_t line_w, const mnet_paste_region* regions, int32_t n_regions,
                  uint8_t* page, int32_t page_h, int32_t page_w, void* stream);

/* Finiteness guard of the half-range precision modes (the role `torch.isfinite(y).all()` would play after test_sr.py:197 — the
 * reference has no such check because its fp32 activations cannot overflow): *flag (int32, device) is set to 0 and then to 1 by any
 * thread that finds an element of x (n elements, MNET_F32 or MNET_F16) that is inf or NaN.  One streaming read of x, no atomics
 * (every writer stores the same value), no synchronisation: the caller reads the flag back when it consumes the result. */
int mnet_nonfinite_flag(const void* x, int32_t dtype, int64_t n, int32_t* flag, void* stream);

/* Precision margin guard: how far a run in a throughput mode lies from a run of the same network in a more accurate mode — the role a
 * `torch.abs(a - b).max()` (with its argmax, the norms and an isfinite count) after test_sr.py:197 would play if the script ran its forward
 * twice; the reference has no such check because it has one arithmetic.  `mode` and `ref` hold the same logical tensor [n_groups][elems_per_group]
 * (a group = one strip's map, one glyph's prior: pixel-major, channel-minor), each in its OWN storage; one record per group is written to `stats`.
 * The values compared are what the storage's reader returns (split half: float(hi) + float(lo); fp16+8: fl32(hi + lo8 * 2^(E - 138))); the difference
 * is one fp32 subtraction.  A pair with a non-finite element on either side is counted and left out of every maximum and sum: a NaN cannot hide a
 * deviation elsewhere.
 *   (mode, ref) storages: (F16 | F16M, F16X2), (F16 | F16M | F16X2 | F32, F32); anything else MNET_E_ARG.
 *   elems_per_group % 32 == 0 (a group starts on a 32-channel block), n_groups >= 1; F32 / F16 bases 16-byte, blocked storages 128-byte, stats and
 *   workspace 8-byte aligned (MNET_E_ALIGN).  Everything is checked before any HIP call.
 * One streaming pass: every workgroup of a group's MNET_CMP_SLICES(elems_per_group) slices writes one partial record to `workspace`
 * (MNET_CMP_WORKSPACE_BYTES), a second small launch folds a group's slices in slice order.  No atomics, no counters: the same bytes on every launch, and a
 * group's record does not depend on the other groups of the launch. */
typedef struct {
    float max_abs_diff;         /* max |mode - ref| over the pairs with both elements finite (0 when there is none)          */
    float max_abs_ref;          /* max |ref| over the same pairs                                                              */
    float max_abs_mode;         /* max |mode| over the same pairs                                                             */
    int32_t reserved;           /* 0                                                                                          */
    int64_t argmax_index;       /* lowest element index inside the group (pixel * C + channel) that attains max_abs_diff; -1: no finite pair */
    double sum_sq_diff;         /* sum (mode - ref)^2 and sum ref^2 over the same pairs, fp64                                 */
    double sum_sq_ref;
    int64_t nonfinite_mode;     /* elements of mode / of ref that are inf or NaN                                              */
    int64_t nonfinite_ref;
} mnet_cmp_stats;
#define MNET_CMP_WG_ELEMS 2048          /* elements one workgroup takes per trip: 256 threads x 8 */
#define MNET_CMP_MAX_SLICES 32          /* workgroups per group at most; beyond 32 * 2048 elements they make further trips */
#define MNET_CMP_SLICES(elems_per_group) \
    ((int64_t)(elems_per_group) <= MNET_CMP_WG_ELEMS ? 1 : \
     ((int64_t)(elems_per_group) + MNET_CMP_WG_ELEMS - 1) / MNET_CMP_WG_ELEMS >= MNET_CMP_MAX_SLICES ? MNET_CMP_MAX_SLICES : \
     (int)(((int64_t)(elems_per_group) + MNET_CMP_WG_ELEMS - 1) / MNET_CMP_WG_ELEMS))
#define MNET_CMP_WORKSPACE_BYTES(n_groups, elems_per_group) \
    ((size_t)(n_groups) * (size_t)MNET_CMP_SLICES(elems_per_group) * sizeof(mnet_cmp_stats))
int mnet_compare_stats(const void* mode, int32_t mode_dtype, const void* ref, int32_t ref_dtype, int32_t n_groups, int64_t elems_per_group,
                       mnet_cmp_stats* stats, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One-time weight packing on the device: from the checkpoint's tensors to the layouts above, without PyTorch
 * or a BLAS on the host side.
 * ------------------------------------------------------------------------------------------- */
/* K18: w_oihw fp32 [cout][cin][kh][kw] (the checkpoint's layout: nn.Conv2d / ModulatedConv2d[0] / nn.Linear with kh = kw = 1)
 *   → packed [cout_pad][kh][kw][cin_pad] in `dtype` (zero padded), every element = (w / sigma) * scale, where
 *   sigma = u^T (W_mat v), W_mat = w viewed as [cout][cin*kh*kw] — the eval-mode old-style torch.nn.utils.spectral_norm fold the
 *   reference recomputes on every forward (models/networks.py:14; weight_orig / weight_u / weight_v of the 33 SN convs of
 *   TSPSRNet); sn_u == sn_v == NULL: no fold (sigma = 1).  `scale`: the layer's constant factor (ModulatedConv2d
 *   1/sqrt(cin*k*k), networks.py:262,284; EqualLinear lr_mul/sqrt(in), :180,192).  MNET_F16X2 additionally stores hi/lo of
 *   256 * value (cin_pad % 32 == 0).  workspace: cout + 1 doubles (only read when sn_u != NULL); sigma is summed in fp64 in a
 *   fixed order (deterministic). */
int mnet_pack_weights(const float* w_oihw, int32_t cout, int32_t cin, int32_t kh, int32_t kw, const float* sn_u,
                      const float* sn_v, float scale, int32_t dtype, int32_t cout_pad, int32_t cin_pad, void* packed,
                      double* workspace, void* stream);
/* demodulation table of a ModulatedConv2d for activation-side modulation (input of mnet_demod):
 *   wsq_t[i][o] = sum_{r,s} (scale * w[o][i][r][s])^2,  fp32 [cin][cout]   (networks.py:284-287) */
int mnet_pack_wsq(const float* w_oihw, int32_t cout, int32_t cin, int32_t khw, float scale, float* wsq_t, void* stream);

/* mnet_gather_rows with every output row divided by 2^e, e = exponent of the row window's largest magnitude (max * 2^-e in [0.5, 1)):
 * the style rows of a modulated conv, normalised so that the modulated activations x * s stay below |x| in the half-precision
 * storage modes (ModulatedConv2d's s can be large with trained weights; models/networks.py:283-287).  Exact (power-of-two factors):
 * eps_scale[r] = 4^-e goes to mnet_demod_scaled, scale_b[r][0..bcast) = 2^e is the out_scale of a conv without demodulation (ToRGB,
 * networks.py:305-321).  eps_scale / scale_b may be NULL. */
int mnet_style_rows(const float* src, int32_t src_rows, int32_t ld, int32_t col0, int32_t ncols, const int64_t* idx,
                    int32_t rows, float* dst, float* eps_scale, float* scale_b, int32_t bcast, void* stream);

/* dst[r][0..ncols) = src[idx ? idx[r] : r][col0 .. col0+ncols)  (fp32; src [src_rows][ld]; idx int64 [rows] or NULL): every glyph
 * takes its image's row of the per-style tensors (test_sr.py:183 gives all glyphs of a strip the same w), every StyledConv its
 * column window of the one batched modulation GEMM (networks.py:141,283).  Indices are not range-checked. */
int mnet_gather_rows(const float* src, int32_t src_rows, int32_t ld, int32_t col0, int32_t ncols, const int64_t* idx,
                     int32_t rows, float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_H */
