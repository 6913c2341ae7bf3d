// Instantiations of the LDS-DMA implicit-GEMM convolution kernel (conv_igemm_dma_kernel.h; design notes in
// conv_igemm_dma.hip): f32 activations, plain and phase form, epilogue EPI_SPLITK (a slice of the K loop per block, raw
// accumulators to the workspace) -- the 64x64 tile, both K-chunk row sizes.
#define RS_CONV_INSTANTIATE
#include "conv_igemm_dma_kernel.h"

RS_CONV_DEFINE_SPLITK_LAUNCHER(rs_conv_launch_f32_plain_splitk, false)
RS_CONV_DEFINE_SPLITK_LAUNCHER(rs_conv_launch_f32_phase_splitk, true)
