/* givepose_headgrad.h -- the pose-head backward family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * Backward of ConvPnPNet (network/conv_pnp_net.py:18-201; flat_op "flatten", mask_attention_type "none" or "mul"): from the
 * gradients of pred_rot (B,rot_dim) and pred_t (B,3), which givepose_grad.h produces, to the gradient of every pnp_net.*
 * parameter and the head's contribution to d ivfc_coor.  The backward of the other modules is not here.
 *
 * The family has its own header and prefix (gph_) next to givepose_hip.h, givepose_align.h, givepose_loss.h and givepose_grad.h;
 * the symbols live in the same library and follow the same conventions (device pointers, caller-owned buffers, no allocation,
 * no synchronisation, no copy to the host, a hipStream_t `stream`, 0 or a negative gp_status, gp_last_error()).  Every entry
 * point that needs scratch memory takes `ws` (256-byte aligned) and `ws_bytes`, and has a size query next to it.
 *
 * All arithmetic is fp32, whatever the forward's compute type: the backward linearises the fp32 head at the given input.  Every
 * tensor is in the reference's own layout: activations NCHW, conv weights OIHW, linear weights (out, in) with fc1's columns in
 * the NCHW flatten order c*64 + hw.  No layout is packed, so a gradient lies under the index of its parameter.
 *
 * Every contraction with a long reduction is one LDS-tiled kernel on v_mfma_f32_32x32x2_f32, whose result is bit for bit a
 * k-ordered fmaf chain.  A contraction may be split over k into at most GPH_MAX_SPLIT chains, whose partial sums are added in
 * the order of k by a second launch; the split depends on the shape alone.  There is no floating-point atomic anywhere: equal
 * inputs give equal bits, and every result is linear in the upstream gradient bit for bit (g scaled by 2 scales it by 2).
 */
#ifndef GIVEPOSE_HEADGRAD_H
#define GIVEPOSE_HEADGRAD_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPH_MAX_SPLIT 8   /* partial sums of one contraction, merged in k order */
#define GPH_FEAT 128      /* channels of the three conv layers */
#define GPH_GROUPS 32     /* GroupNorm groups (4 channels each), eps 1e-5 */
#define GPH_RES 64        /* the maps are 64 x 64; the layers run at 32, 16 and 8 */

/* The 23 parameter tensors of pnp_net, in the reference's shapes.  The same struct holds the weights (read) and their
 * gradients (written). */
typedef struct gph_pnp_params {
    float* conv_w[3];      /* features.{0,3,6}.weight: (128,5,3,3), (128,128,3,3), (128,128,3,3) */
    float* gn_w[3];        /* features.{1,4,7}.weight (128) */
    float* gn_b[3];        /* features.{1,4,7}.bias (128) */
    float *fc1_w, *fc1_b;      /* (1024,8192), (1024) */
    float *fc1z_w, *fc1z_b;    /* fc1_z */
    float *fc2_w, *fc2_b;      /* (256,1024), (256) */
    float *fc2z_w, *fc2z_b;    /* fc2_z */
    float *fcr_w, *fcr_b;      /* fc_r (rot_dim,256), (rot_dim) */
    float *fct_w, *fct_b;      /* fc_t (2,256), (2) */
    float *fcz_w, *fcz_b;      /* fc_z (1,256), (1) */
} gph_pnp_params;

/* What the forward saves for the backward (all fp32, written by gph_pnp_forward_save, read by gph_pnp_backward). */
typedef struct gph_pnp_saved {
    float* x0;             /* (B,5,64,64): cat(ivfc, roi_coord_2d), times the mask when one is given */
    float* conv[3];        /* pre-norm conv outputs (B,128,32,32), (B,128,16,16), (B,128,8,8) */
    float* mean[3];        /* GroupNorm mean per (crop, group): (B,32) */
    float* rstd[3];        /* 1 / sqrt(var + 1e-5), (B,32) */
    float* act[3];         /* post-ReLU outputs, shapes of conv[] */
    float* h1;             /* (B,2048): LeakyReLU(0.1) outputs of fc1 (columns 0..1023) and fc1_z (1024..2047) */
    float* h2;             /* (B,256): LeakyReLU output of fc2 */
    float* h2z;            /* (B,256): LeakyReLU output of fc2_z */
    float* pred_rot;       /* (B,rot_dim) */
    float* pred_t;         /* (B,3): fc_t's two columns, then fc_z's */
} gph_pnp_saved;

/* ---- the pieces, each callable on its own ---- */

/* Backward of Y = act(X W^T + b), X (M,K) with row stride ldx, W (N,K), act = LeakyReLU(0.1) when Y is given, else none.
 *   dY (M,N) row stride lddy; Y (M,N) row stride ldy or null: the saved OUTPUT, the gate is 1 where Y > 0 and 0.1 elsewhere
 *   -> dX (M,K) row stride lddx = (dY o gate) W, added to what dX holds when accumulate != 0 (MFMA, contraction N);
 *      dW (N,K) = (dY o gate)^T X, a chain over the M rows in order; db (N) likewise.  dX, dW and db may each be null. */
long long gph_linear_backward_workspace(int M, int N, int K);
int gph_linear_backward(const float* dY, int lddy, const float* Y, int ldy, const float* W, const float* X, int ldx, int M, int N,
                        int K, int accumulate, float* dX, int lddx, float* dW, float* db, void* ws, long long ws_bytes, void* stream);

/* Backward of out = ReLU(GroupNorm(x)), x (B,C,HW) NCHW, groups of 4 channels, given the saved output, mean and rstd (B,C/4).
 *   the gate is out > 0; dx is the three-term form rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)) over the 4 HW elements of
 *   a group; dgamma, dbeta (C) are sums over HW inside a wave (each lane its elements in turn, xor tree) and then over the
 *   crops in order.  dx may alias dout.  One workgroup per (crop, group), one wave per channel. */
long long gph_gn_relu_backward_workspace(int B, int C);
int gph_gn_relu_backward(const float* dout, const float* out, const float* x, const float* mean, const float* rstd,
                         const float* gamma, int B, int C, int HW, float* dx, float* dgamma, float* dbeta, void* ws,
                         long long ws_bytes, void* stream);

/* Backward of a 3x3 stride-2 pad-1 conv without bias, X (B,Cin,H,H) -> (B,Cout,H/2,H/2), H even, Wt (Cout,Cin,3,3).
 *   dX (B,cin_dx,H,H): the first cin_dx <= Cin input channels, in gather form (an input pixel collects the taps whose output
 *       pixel exists; a tap without one contributes an exact 0), contraction (co,kh,kw) on MFMA; multiplied by mask (B,H,H)
 *       when mask is given.  dW (Cout,Cin,3,3): contraction over (b,oh,ow) on MFMA.  Either may be null. */
long long gph_conv3x3s2_backward_workspace(int B, int Cin, int Cout, int H, int cin_dx);
int gph_conv3x3s2_backward(const float* dY, const float* X, const float* Wt, const float* mask, int B, int Cin, int Cout, int H,
                           int cin_dx, float* dX, float* dW, void* ws, long long ws_bytes, void* stream);

/* ---- the head ---- */

/* ConvPnPNet.forward in fp32 on ivfc (B,3,64,64), roi_coord_2d (B,2,64,64) and mask (B,1,64,64) or null
 * (mask_attention_type "mul": all five channels are multiplied), writing every tensor of `saved`. */
long long gph_pnp_forward_workspace(int B, int rot_dim);
int gph_pnp_forward_save(const float* ivfc, const float* roi_coord_2d, const float* mask, const gph_pnp_params* w, int B,
                         int rot_dim, const gph_pnp_saved* saved, void* ws, long long ws_bytes, void* stream);

/* From g_pred_rot (B,rot_dim) and g_pred_t (B,3) to the gradient of every parameter (grads, all 23 written in full) and to
 * g_ivfc (B,3,64,64), the head's part of d ivfc_coor (times the mask when one is given; roi_coord_2d and the mask get none).
 * The gradients of fc1 and fc1_z into the flattened feature are added, fc1's first. */
long long gph_pnp_backward_workspace(int B, int rot_dim);
int gph_pnp_backward(const gph_pnp_params* w, const gph_pnp_saved* saved, const float* mask, const float* g_pred_rot,
                     const float* g_pred_t, int B, int rot_dim, const gph_pnp_params* grads, float* g_ivfc, void* ws,
                     long long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
