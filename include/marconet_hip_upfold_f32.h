/* marconet_hip_upfold_f32.h — the fold of marconet_hip_upfold.h with its tap planes in fp32: one more entry point beside the table of marconet_hip.h (C-ABI
 * version 4 and its 43 entry points stay as they are, and so does marconet_hip_upfold.h).  Plain C; same rules — the caller owns every buffer, a call only
 * enqueues work on the given stream, returns 0 or a negative MNET_E_*, message via mnet_last_error().
 * ctypes binding: marconet_amd/_lib.py, UPFOLD_F32Z_SYMBOLS. */
#ifndef MARCONET_HIP_UPFOLD_F32_H
#define MARCONET_HIP_UPFOLD_F32_H

#include "marconet_hip_upfold.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mnet_upfold3x3_nhwc with z and y in DIFFERENT storages: z [n,h,w,9 c] is plain fp32 — what mnet_conv2d_nhwc_ex writes under MNET_CONV_ALGO_FLAG_F32_OUT, the
 * tap planes before any rounding to a storage — and y [n,2h,2w,c] is `ydtype`, which must be MNET_F16M (fp16+8).  z is an intermediate that only this kernel
 * reads and fp16+8 costs 4 bytes per element like fp32: with fp32 planes a loaded chunk is already the decoded value.  Same thread-to-work map, same fp32
 * sums in the same (P + C) + N order, same epilogue contract
 *   y[n,Y,X,c] = post_scale[n,c] * act( out_scale[n,c] * sum_{ky,kx} (U z_{ky,kx})[n, Y + ky - 1, X + kx - 1, c] + bias[c] )
 * and the same refusals as mnet_upfold3x3_nhwc on MNET_F16M: c % 32 == 0, z and y 128-byte aligned, maps with w * 9 c >= 2^29 or h * w * (c / 8) * 4 >= 2^31
 * refused with MNET_E_ARG; act: MNET_ACT_NONE, MNET_ACT_LRELU or MNET_ACT_LRELU_SQRT2; out_scale, bias, post_scale: fp32, 16-byte aligned, each may be NULL.
 * Batch-invariant bytes: one image alone gives the bytes it gives in a batch. */
int mnet_upfold3x3_f32z_nhwc(const float* z, void* y, int32_t ydtype, int32_t n, int32_t h, int32_t w, int32_t c,
                             const float* out_scale, const float* bias, int32_t act, const float* post_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARCONET_HIP_UPFOLD_F32_H */
