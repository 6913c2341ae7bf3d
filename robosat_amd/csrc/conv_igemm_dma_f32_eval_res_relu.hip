// Instantiations of the LDS-DMA implicit-GEMM convolution kernel (conv_igemm_dma_kernel.h; design notes in
// conv_igemm_dma.hip): f32 activations, direct form, epilogue EPI_EVAL with the kind fixed at compile time -- scale + shift + residual + ReLU --
// on the four fp32 tiles, both K-chunk row sizes, table and FAST1 prologue.
#define RS_CONV_INSTANTIATE
#include "conv_igemm_dma_kernel.h"

RS_CONV_DEFINE_KIND_LAUNCHER(rs_conv_launch_f32_eval_res_relu, EK_RES_RELU)
