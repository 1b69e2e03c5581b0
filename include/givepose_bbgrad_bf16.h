/* givepose_bbgrad_bf16.h -- the mixed-precision forms of the backbone backward family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * An addition to givepose_bbgrad.h (gpb_), whose conventions, tables and layouts apply unchanged.  The entry points here carry the
 * prefix gpbm_ and take a trailing `precision`:
 *
 *   GPB_PREC_F32   every contraction is the k-ordered fp32 fmaf chain of the gpb_ entry points: the same kernels, the same bits.
 *   GPB_PREC_BF16  what torch.autocast(bfloat16) gives elsewhere: the six dense contractions of a ConvNeXt block -- fc1 and fc2
 *                  forward, d h = (g . gamma W2) GELU'(h), d W2 = gamma (g^T a), fc1's dX, d W1 = d h^T LN_out -- multiply bf16
 *                  operands and add in fp32 (csrc/grad_gemm_bf16.hpp, v_mfma_f32_32x32x16_bf16).  Everything else is the fp32 code
 *                  of the gpb_ family: the depth-wise 7x7, the LayerNorms, the GELU map, every ordered row sum, the stem and
 *                  downsample patch convs.  Gradients need no loss scaling: bf16 has fp32's exponent range.
 *
 * The contract of a bf16 contraction.  Every operand element is the fp32 value the gpb_ code reads or forms (LN(dwout), GELU(h),
 * gamma W2, d h, ...), rounded to bf16 with round-to-nearest-even while the tile is staged; memory holds fp32 only, and a saved table
 * has the same shapes and dtypes in both modes: a table written in one mode is accepted by the backward of the other.  An element
 * outside the tensor is an exact 0.  The products are added in fp32 accumulators and the store functor (bias, GELU, the layer scale,
 * GELU') sees the fp32 sum.  The split of k depends on the shape alone, the partial sums are merged in order by a second launch, and
 * there is no atomic: equal inputs give equal bits, and scaling the upstream gradient by a power of two scales every gradient by it
 * bit for bit (short of overflow and underflow).  The split differs from the fp32 form's (128 x 128 tiles), so the workspace sizes
 * differ too: ask the query of the precision in use.
 *
 * An unknown precision is refused (GP_ERR_INVALID and a message), and its size query answers 0.
 */
#ifndef GIVEPOSE_BBGRAD_BF16_H
#define GIVEPOSE_BBGRAD_BF16_H

#include "givepose_bbgrad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPB_PREC_F32 0
#define GPB_PREC_BF16 1

/* C (M,N) row-major fp32 = op(A) op(B) by the bf16 contraction above: A is (M,K) row-major, or (K,M) when trans_a; B is (K,N)
 * row-major, or (N,K) when trans_b.  A piece callable on its own, like those of givepose_bbgrad.h. */
long long gpbm_matmul_bf16_workspace(int M, int N, int K);
int gpbm_matmul_bf16(const float* a, const float* b, int M, int N, int K, int trans_a, int trans_b, float* c, void* ws, long long ws_bytes,
                     void* stream);

/* gpb_block_workspace / gpb_block_forward_save / gpb_block_backward with a precision. */
long long gpbm_block_workspace(int N, int H, int W, int C, int precision);
int gpbm_block_forward_save(const float* x, const gpb_block_params* params, int N, int H, int W, int C, float* dwout, float* mean,
                            float* rstd, float* h, float* y2, float* out, void* ws, long long ws_bytes, void* stream, int precision);
int gpbm_block_backward(const float* g, const float* x, const gpb_block_params* params, const float* dwout, const float* mean,
                        const float* rstd, const float* h, const float* y2, int N, int H, int W, int C, const gpb_block_params* grads,
                        float* dx, void* ws, long long ws_bytes, void* stream, int precision);

/* gpb_backbone_forward_save / gpb_backbone_backward and their size queries with a precision. */
long long gpbm_backbone_forward_workspace(const int* dims, const int* depths, int n_stages, int B, int S, int precision);
int gpbm_backbone_forward_save(const float* img, float* const* params, const int* dims, const int* depths, int n_stages, int B, int S,
                               float* const* saved, float* feat, void* ws, long long ws_bytes, void* stream, int precision);
long long gpbm_backbone_backward_workspace(const int* dims, const int* depths, int n_stages, int B, int S, int precision);
int gpbm_backbone_backward(float* const* params, float* const* saved, const float* img, const float* g_feat, const int* dims,
                           const int* depths, int n_stages, int B, int S, float* const* grads, float* d_img, void* ws, long long ws_bytes,
                           void* stream, int precision);

#ifdef __cplusplus
}
#endif
#endif
