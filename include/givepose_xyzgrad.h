/* givepose_xyzgrad.h -- the coordinate-head backward family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * Backward of TopDownXyzHead (network/xyz_head.py:195-366 with its defaults: ConvTranspose2d(Cin,256,3,s2,p1,op1) + GroupNorm(32) +
 * GELU, six times conv3x3 + GroupNorm(32) + GELU with UpsamplingBilinear2d(2) before the third and the fifth, a 1x1 out layer with
 * bias), the class of xyz_nocs_head (Cin 1024) and xyz_deform_head (Cin 512): from the gradient of the (B,3,8 H0,8 H0) coordinate
 * map to the gradient of all 23 parameter tensors and of the (B,Cin,H0,H0) input feature.  In the network H0 is 8.
 *
 * The family has its own header and prefix (gpx_) next to givepose_headgrad.h (gph_), whose conventions apply unchanged: device
 * pointers, caller-owned buffers, no allocation, no synchronisation, no copy to the host, a hipStream_t `stream`, 0 or a negative
 * gp_status, gp_last_error().  Every entry point that needs scratch memory takes `ws` (256-byte aligned) and `ws_bytes`, and has
 * a size query next to it (0 for a shape the entry point refuses).
 *
 * All arithmetic is fp32.  Every tensor is in the reference's own layout: activations NCHW, conv weights OIHW, the transposed
 * conv's weight (Cin,Cout,3,3) as nn.ConvTranspose2d stores it.  No layout is packed, so a gradient lies under the index of its
 * parameter.
 *
 * Every long contraction runs on the LDS-tiled v_mfma_f32_32x32x2_f32 kernel this family shares with gph_* (csrc/grad_gemm.hpp):
 * bit for bit a k-ordered fmaf chain over the terms that exist, split over k into at most GPH_MAX_SPLIT chains by a rule of the
 * shape alone, whose partial sums are added in the order of k.  There is no floating-point atomic anywhere: equal inputs give
 * equal bits, and every result is linear in the upstream gradient bit for bit (g scaled by 2 scales it by 2).
 *
 * Memory.  gpx_xyz_forward_save writes, per crop at H0 = 8: the pre-norm and post-GELU maps of the 7 normalised layers (3 at
 * 16 x 16, 2 at 32 x 32, 2 at 64 x 64: 21.5 MB), the two upsampled maps (5 MB), mean / rstd and the result: about 27 MB per crop.
 * gpx_xyz_backward needs two more maps of the largest size (8 MB per crop) plus the split partial sums.
 */
#ifndef GIVEPOSE_XYZGRAD_H
#define GIVEPOSE_XYZGRAD_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_FEAT 256      /* channels of every layer of the head */
#define GPX_GROUPS 32     /* GroupNorm groups (8 channels each), eps 1e-5 */
#define GPX_LAYERS 7      /* normalised layers: the transposed conv and six convs */

/* The 23 parameter tensors of one head, in the reference's shapes.  The same struct holds the weights (read) and their
 * gradients (written). */
typedef struct gpx_xyz_params {
    float* deconv_w;       /* features.0.weight (Cin,256,3,3) */
    float* conv_w[6];      /* features.{3,4,6,7,9,10}.conv.weight (256,256,3,3) */
    float* gn_w[7];        /* features.1.weight, features.{3,4,6,7,9,10}.norm.weight (256) */
    float* gn_b[7];        /* features.1.bias, features.{3,4,6,7,9,10}.norm.bias (256) */
    float *out_w, *out_b;  /* out_layer.weight (3,256,1,1), out_layer.bias (3) */
} gpx_xyz_params;

/* What the forward saves for the backward (all fp32, written by gpx_xyz_forward_save, read by gpx_xyz_backward).  Layer l runs
 * at R_l = H0 * {2,2,2,4,4,8,8}[l]. */
typedef struct gpx_xyz_saved {
    float* pre[7];         /* pre-norm outputs (B,256,R_l,R_l) */
    float* mean[7];        /* GroupNorm mean per (crop, group): (B,32) */
    float* rstd[7];        /* 1 / sqrt(var + 1e-5), (B,32) */
    float* act[7];         /* post-GELU outputs, shapes of pre[] */
    float* up[2];          /* the bilinear x2 of act[2] (B,256,4 H0,4 H0) and of act[4] (B,256,8 H0,8 H0) */
    float* coor;           /* (B,3,8 H0,8 H0): the head's result */
} gpx_xyz_saved;

/* ---- the pieces, each callable on its own ---- */

/* Y = conv2d(X, Wt, stride 1, padding 1) without bias: X (B,Cin,H,H), Wt (Cout,Cin,3,3), Y (B,Cout,H,H), any H >= 1.
 *   forward: contraction (ci,kh,kw).  backward: dX (B,Cin,H,H) in gather form (an input pixel collects the up to 9 Cout taps whose
 *   output pixel exists; an absent one is an exact 0), contraction (co,kh,kw); dW (Cout,Cin,3,3), contraction (b,oh,ow).  dX or dW
 *   may be null.  One size query serves both. */
long long gpx_conv3x3s1_workspace(int B, int Cin, int Cout, int H);
int gpx_conv3x3s1_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, void* ws, long long ws_bytes,
                          void* stream);
int gpx_conv3x3s1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW,
                           void* ws, long long ws_bytes, void* stream);

/* Y = conv_transpose2d(X, Wt, stride 2, padding 1, output_padding 1) without bias: X (B,Cin,H,H), Wt (Cin,Cout,3,3),
 * Y (B,Cout,2H,2H), oh = 2 ih - 1 + kh.  The forward is the stride-2 conv's dX gather with X in the role of dY (contraction
 * (ci,kh,kw)); dX is the stride-2 conv of dY (contraction (co,kh,kw)); dW (Cin,Cout,3,3) is the stride-2 conv's dW with the
 * operand roles exchanged (contraction (b,ih,iw)).  dX or dW may be null. */
long long gpx_deconv3x3s2_workspace(int B, int Cin, int Cout, int H);
int gpx_deconv3x3s2_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, void* ws, long long ws_bytes,
                            void* stream);
int gpx_deconv3x3s2_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW,
                             void* ws, long long ws_bytes, void* stream);

/* Backward of out = GELU(GroupNorm_G(x)) (exact erf GELU, eps 1e-5), x (B,C,HW) NCHW, C a multiple of G, given the saved x,
 * mean and rstd (B,G), gamma and beta (C).  The pre-activation u = (x - mean) rstd gamma + beta is formed by the device function
 * gpx_xyz_forward_save uses; dGELU = Phi(u) + u phi(u) with erff / expf; dx is the three-term form
 * rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)) over the C/G x HW elements of a group; dgamma, dbeta (C) are sums over HW
 * inside a wave (each lane its elements in turn, xor tree), the group means add the waves in a fixed order, and the crops are
 * added in order.  One workgroup per (crop, group).  dx must not overlap any input. */
long long gpx_gn_gelu_backward_workspace(int B, int C);
int gpx_gn_gelu_backward(const float* dout, const float* x, const float* mean, const float* rstd, const float* gamma,
                         const float* beta, int B, int C, int HW, int G, float* dx, float* dgamma, float* dbeta, void* ws,
                         long long ws_bytes, void* stream);

/* UpsamplingBilinear2d(scale 2) (align_corners = True) in fp32: x (B,C,H,H) -> y (B,C,2H,2H), and its transpose dy -> dx.  One
 * device function gives (i0, frac) of an output index for both, so the backward is the transpose of the forward that ran; each
 * input pixel sums the output pixels whose taps include it in the order of (oh, ow). */
int gpx_upsample_bilinear2x_forward(const float* x, int B, int C, int H, float* y, void* stream);
int gpx_upsample_bilinear2x_backward(const float* dy, int B, int C, int H, float* dx, void* stream);

/* Backward of Y = conv2d(X, Wt) + bias with a 1x1 kernel: X (B,Cin,HW), Wt (Cout,Cin), dY (B,Cout,HW), Cout <= 64.
 *   dX (B,Cin,HW): a chain over Cout; dW (Cout,Cin): a chain over the B HW pixels in order (split and merged in order);
 *   db (Cout): each lane its pixels in turn, xor tree, the four waves in order.  Each may be null. */
long long gpx_conv1x1_backward_workspace(int B, int Cin, int Cout, int HW);
int gpx_conv1x1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int HW, float* dX, float* dW,
                         float* db, void* ws, long long ws_bytes, void* stream);

/* ---- the head ---- */

/* TopDownXyzHead.forward in fp32 on feat (B,Cin,H0,H0), writing every tensor of `saved`. */
long long gpx_xyz_forward_workspace(int B, int Cin, int H0);
int gpx_xyz_forward_save(const float* feat, const gpx_xyz_params* w, int B, int Cin, int H0, const gpx_xyz_saved* saved, void* ws,
                         long long ws_bytes, void* stream);

/* From g_coor (B,3,8 H0,8 H0) to the gradient of every parameter (grads, all 23 written in full) and to g_feat (B,Cin,H0,H0);
 * feat and saved are what gpx_xyz_forward_save read and wrote for the same parameters. */
long long gpx_xyz_backward_workspace(int B, int Cin, int H0);
int gpx_xyz_backward(const gpx_xyz_params* w, const gpx_xyz_saved* saved, const float* feat, const float* g_coor, int B, int Cin,
                     int H0, const gpx_xyz_params* grads, float* g_feat, void* ws, long long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
