/* marconet_hip_upfold.h — the one entry point libmarconet_hip.so exports beside the table of marconet_hip.h (C-ABI version 4, which that header and its
 * 43 entry points define and which stays as it is): an up-sampling 3x3 convolution's second half.  Plain C, like marconet_hip.h; same rules — the caller owns
 * every buffer, a call only enqueues work on the given stream, returns 0 or a negative MNET_E_*, message via mnet_last_error().
 * ctypes binding: marconet_amd/_lib.py, UPFOLD_SYMBOLS.  (The same fold with its tap planes in fp32: marconet_hip_upfold_f32.h.) */
#ifndef MARCONET_HIP_UPFOLD_H
#define MARCONET_HIP_UPFOLD_H

#include "marconet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The "fold" of conv3x3(bilinear_x2(x)) in tap-conv form (an addition beside ABI v4: nothing in marconet_hip.h changes).  The channel contraction runs on the LOW-res map as one 1x1 convolution with 9 C
 * output channels, tap-major — z [n,h,w,9 C], channel t C + c = sum_i W[c, ky, kx, i] x[.., i] with t = 3 ky + kx (mnet_conv2d_nhwc with the rows of the weight
 * tensor reordered: a quarter of the MACs of the conv on the up-sampled map, which is never written) — and this streaming kernel sums the nine up-sampled, shifted
 * planes and applies the conv epilogue's contract:
 *   y[n,Y,X,c] = post_scale[n,c] * act( out_scale[n,c] * sum_{ky,kx} (U z_{ky,kx})[n, Y + ky - 1, X + kx - 1, c] + bias[c] ),     y [n,2h,2w,c]
 * U = the bilinear x2 of mnet_upsample2x_nhwc (1/4, 3/4 weights, align_corners=False, edge clamp); terms outside the hi-res map are zero (the conv's zero padding),
 * so the identity with conv3x3(U x) is exact at the borders as well.  fp32 sums in a fixed order per output (batch-invariant bytes), one rounding to storage.
 * The fold takes all four storages, MNET_F32, MNET_F16, MNET_F16X2 (split half) and MNET_F16M (fp16+8), with their alignment rules: z and y in the same storage
 * `dtype`, 16-byte aligned, c % 8 == 0 (f32: c % 4 == 0); blocked storages: c % 32 == 0, 128-byte aligned.  Maps with w * 9 c >= 2^29 or h * w * (c / 8) * 4
 * >= 2^31 (f32: c / 4) are refused with MNET_E_ARG.  act: MNET_ACT_NONE, MNET_ACT_LRELU or
 * MNET_ACT_LRELU_SQRT2; out_scale, bias, post_scale: fp32, 16-byte aligned, each may be NULL. */
int mnet_upfold3x3_nhwc(const void* z, void* y, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c,
                        const float* out_scale, const float* bias, int32_t act, const float* post_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_UPFOLD_H */
