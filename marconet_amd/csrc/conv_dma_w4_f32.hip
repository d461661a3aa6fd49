// The one-wave-per-SIMD 256x256 fp16+8 tile (conv_dma_w4.hip) built with the MNET_CONV_ALGO_FLAG_F32_OUT output mode: fp16+8 operands, the accumulator's value
// (* 2^-8) stored as fp32 [N,Ho,Wo,cout] — the tap planes of an up-conv's tap-conv form, an intermediate that only the fold reads (upfold_kernels.hip).  A
// translation unit of its own: the production builds of the tile keep their code, their names and their count.  Same slab loop, same MFMA sequence per output:
// the fp32 value IS the value the fp16+8 build encodes.
#define MNET_W4_F32_TU 1
#include "conv_dma_w4.hip"
