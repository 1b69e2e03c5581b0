/* givepose_xyzgrad_bf16.h -- the mixed-precision forms of the coordinate-head backward family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * An addition to givepose_xyzgrad.h (gpx_), whose conventions, structs and layouts apply unchanged.  The entry points here carry the
 * prefix gpxm_ and take a trailing `precision`:
 *
 *   GPX_PREC_F32   every contraction is the k-ordered fp32 fmaf chain of the gpx_ entry points: the same kernels, the same bits.
 *   GPX_PREC_BF16  the 21 contractions of the 3x3 layers of a head -- forward, dX and dW of the stride-2 transposed conv and of the six
 *                  stride-1 convs -- multiply bf16 operands and add in fp32 (csrc/grad_gemm_bf16.hpp, v_mfma_f32_32x32x16_bf16), as
 *                  torch.autocast(bfloat16) does elsewhere.  Everything else is the fp32 code of the gpx_ family with its bits:
 *                  GroupNorm + GELU and their backward, the bilinear x2 in both directions, and the whole 1x1 output conv (forward,
 *                  dX, dW, db: with 3 output channels a 128-wide tile would be wasted on it).  Gradients need no loss scaling: bf16
 *                  has fp32's exponent range.
 *
 * The contract of a bf16 contraction is that of givepose_bbgrad_bf16.h.  Every operand element is the fp32 value the gpx_ code reads
 * through its view (a window of the input, a gathered output gradient, a weight), rounded to bf16 with round-to-nearest-even while
 * the tile is staged; memory holds fp32 only, and a gpx_xyz_saved table has the same shapes and dtypes in both modes: a table written
 * in one mode is accepted by the backward of the other.  An element outside the map (padding, a tap without an output pixel) is an
 * exact 0.  The products are added in fp32 accumulators and the store functor sees the fp32 sum.  The split of k depends on the shape
 * alone, the partial sums are merged in order by a second launch, and there is no atomic: equal inputs give equal bits, and scaling
 * the upstream gradient by a power of two scales every gradient by it bit for bit (short of overflow and underflow).  The split
 * differs from the fp32 form's (128 x 128 tiles) and depends on B, so the workspace sizes differ -- ask the query of the precision in
 * use -- and a crop's result is not bitwise independent of the other crops of the call.
 *
 * An unknown precision is refused (GP_ERR_INVALID and a message), and its size query answers 0.
 */
#ifndef GIVEPOSE_XYZGRAD_BF16_H
#define GIVEPOSE_XYZGRAD_BF16_H

#include "givepose_xyzgrad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_PREC_F32 0
#define GPX_PREC_BF16 1

/* gpx_conv3x3s1_workspace / _forward / _backward with a precision. */
long long gpxm_conv3x3s1_workspace(int B, int Cin, int Cout, int H, int precision);
int gpxm_conv3x3s1_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, void* ws, long long ws_bytes,
                           void* stream, int precision);
int gpxm_conv3x3s1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW,
                            void* ws, long long ws_bytes, void* stream, int precision);

/* gpx_deconv3x3s2_workspace / _forward / _backward with a precision. */
long long gpxm_deconv3x3s2_workspace(int B, int Cin, int Cout, int H, int precision);
int gpxm_deconv3x3s2_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, void* ws, long long ws_bytes,
                             void* stream, int precision);
int gpxm_deconv3x3s2_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW,
                              void* ws, long long ws_bytes, void* stream, int precision);

/* gpx_xyz_forward_save / gpx_xyz_backward and their size queries with a precision. */
long long gpxm_xyz_forward_workspace(int B, int Cin, int H0, int precision);
int gpxm_xyz_forward_save(const float* feat, const gpx_xyz_params* w, int B, int Cin, int H0, const gpx_xyz_saved* saved, void* ws,
                          long long ws_bytes, void* stream, int precision);
long long gpxm_xyz_backward_workspace(int B, int Cin, int H0, int precision);
int gpxm_xyz_backward(const gpx_xyz_params* w, const gpx_xyz_saved* saved, const float* feat, const float* g_coor, int B, int Cin,
                      int H0, const gpx_xyz_params* grads, float* g_feat, void* ws, long long ws_bytes, void* stream, int precision);

#ifdef __cplusplus
}
#endif
#endif
