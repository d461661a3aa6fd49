// The one-wave-per-SIMD 256x256 fp16+8 tile (conv_dma_w4.hip) built with the MNET_CONV_ALGO_FLAG_SHUFFLE2 output mode: cout = 4 C phase-major on the low-res map, stored
// as the [N,2H,2W,C] tensor (conv o bilinear x2 in polyphase form).  A translation unit of its own: the production builds of the tile keep their code, their names and
// their count.  Same slab loop, same MFMA sequence per output.
#define MNET_W4_SHUF_TU 1
#include "conv_dma_w4.hip"
