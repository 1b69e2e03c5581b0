/* givepose_encgrad.h -- the map-encoder backward family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * Backward of MAPEncoder with use_dcn = 'dcnv3' (network/conv_pnp_net.py:254-332, network/dcnv3.py:23-38,
 * network/ops_dcnv3/modules/dcnv3.py:318-356): three layers of conv1x1 (3 -> 256, then 256 -> 256, with bias) + DCNv3 (3x3, stride 2,
 * pad 1, dilation 1, 4 groups of 64 channels, offset_scale 1) + GroupNorm(32, eps 1e-5) + ReLU, from the gradient of the
 * (N,256,R/8,R/8) map to the gradient of all 48 parameter tensors and of the (N,3,R,R) coordinate map, plus the backward of a 1x1
 * conv with any number of output channels (feat_reducer).  DCNv3_C.bn is in the state_dict and is never applied: it has no entry.
 *
 * The family has its own header and prefix (gpe_) next to givepose_headgrad.h (gph_) and givepose_xyzgrad.h (gpx_), whose conventions
 * apply unchanged: device pointers, caller-owned buffers, no allocation, no synchronisation, no copy to the host, a hipStream_t
 * `stream`, 0 or a negative gp_status, gp_last_error().  Every entry point that needs scratch memory takes `ws` (256-byte aligned)
 * and `ws_bytes`, and has a size query next to it (0 for a shape the entry point refuses).
 *
 * All arithmetic is fp32.  Parameters and their gradients are in the reference's own shapes and layouts ((out, in) linear weights,
 * OIHW conv weights, the depth-wise weight (C,1,3,3)).  The coordinate map, the result and the GroupNorm tensors are NCHW; inside a
 * layer the reference's module is channels-last, and so is what is saved there: rows (n,h,w) x channels.
 *
 * The coupling.  offset and mask are produced at the layer's full resolution and the stride-2 core consumes them as flat buffers:
 * it reads the first N Ho Wo rows of the (N,H,W) row space of ONE call -- a coupling batch -- and nothing else.  d offset and
 * d mask are zero outside that prefix, so the offset / mask branch (the two Linears, GELU, LayerNorm, depth-wise 3x3) is saved and
 * differentiated over the prefix rows only.  The prefix is a flat row range that may end anywhere; the depth-wise conv zero-pads
 * per image.  gpe_map_encoder_* handle one coupling batch: the caller runs one call per batch of the forward that ran.
 *
 * Every contraction runs on the functor GEMM of csrc/grad_gemm.hpp (k-ordered fmaf chains, splits merged in order).  Sums over rows
 * (bias, LayerNorm and depth-wise gradients) are ordered: each lane takes its rows in turn, the four waves of a workgroup are added
 * as (w0 + w1) + (w2 + w3), and the workgroups' partial sums are added in order.
 *
 * Determinism.  d xp, the gradient of the sampled map, is a data-dependent scatter with fp32 atomic adds (as gp_dcnv3_backward and
 * the reference do), so everything upstream of a scatter inherits its ordering: this family does NOT claim bit-repeatable results
 * or bitwise linearity.  Without any atomic, and therefore equal between runs bit for bit: in every operator everything but d xp;
 * in the encoder the gradients of the LAST layer's GroupNorm, output_proj, offset, mask, LayerNorm and depth-wise parameters.  Its
 * input_proj and conv gradients, every gradient of the two layers below and d coor follow a scatter.  (givepose_encgrad_ordered.h adds an
 * opt-in mode in which d xp is an ordered sum and every output is equal bits between runs; the entry points here are its atomic mode.)
 *
 * Memory.  gpe_map_encoder_forward_save writes per crop at R = 64: layer 0 two maps of 64 x 64 x 256 (8 MB), three prefix maps of
 * 1024 x 256 (3 MB), offset and mask (0.4 MB), the pre-norm and the output map (2 MB); a quarter of that for each layer after:
 * about 17.7 MB per crop.
 */
#ifndef GIVEPOSE_ENCGRAD_H
#define GIVEPOSE_ENCGRAD_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_FEAT 256          /* channels of every layer */
#define GPE_DCN_GROUPS 4      /* DCNv3 groups */
#define GPE_DCN_CHANNELS 64   /* channels per DCNv3 group */
#define GPE_TAPS 9            /* 3 x 3 sampling points: offset rows are 4 x 9 x 2 = 72 wide, mask rows 4 x 9 = 36 */
#define GPE_GN_GROUPS 32      /* GroupNorm groups, eps 1e-5 */
#define GPE_LAYERS 3

/* The 16 parameter tensors of one layer (features.{0,3,6}.* and the GroupNorm features.{1,4,7}.*), in the reference's shapes.
 * The same struct holds the weights (read) and their gradients (written). */
typedef struct gpe_layer_params {
    float *conv_w, *conv_b;      /* conv.weight (256,Cin,1,1), conv.bias (256): Cin 3 in layer 0, 256 after */
    float *dw_w, *dw_b;          /* dcnv3.dw_conv.0.weight (256,1,3,3), .bias (256) */
    float *ln_w, *ln_b;          /* dcnv3.dw_conv.1.1.weight, .bias (256): LayerNorm, eps 1e-6 */
    float *off_w, *off_b;        /* dcnv3.offset.weight (72,256), .bias (72) */
    float *mask_w, *mask_b;      /* dcnv3.mask.weight (36,256), .bias (36) */
    float *in_w, *in_b;          /* dcnv3.input_proj.weight (256,256), .bias (256) */
    float *out_w, *out_b;        /* dcnv3.output_proj.weight (256,256), .bias (256) */
    float *gn_w, *gn_b;          /* the GroupNorm after the layer (256) */
} gpe_layer_params;

typedef struct gpe_enc_params {
    gpe_layer_params layer[GPE_LAYERS];
} gpe_enc_params;

/* What the forward saves of one layer with input resolution H (R, R/2, R/4), Ho = H/2, n_pixels = N Ho Ho (all fp32). */
typedef struct gpe_layer_saved {
    float* x;                    /* conv1x1 output, NHWC (N,H,H,256) */
    float* xp;                   /* input_proj(x), NHWC (N,H,H,256): the map the core samples */
    float* dwout;                /* depth-wise 3x3 + bias of the prefix rows (n_pixels,256) */
    float *ln_mean, *ln_rstd;    /* LayerNorm statistics of the prefix rows (n_pixels) */
    float* x1;                   /* GELU(LN(dwout)) (n_pixels,256) */
    float* offset;               /* (n_pixels,72): per group and tap (w, h) */
    float* mask;                 /* (n_pixels,36): softmax probabilities per group */
    float* y;                    /* core output (n_pixels,256) = NHWC (N,Ho,Ho,256) */
    float* pre;                  /* output_proj(y), NCHW (N,256,Ho,Ho): the GroupNorm's input */
    float *gn_mean, *gn_rstd;    /* (N,32) */
    float* act;                  /* ReLU(GroupNorm(pre)), NCHW (N,256,Ho,Ho): the layer's output */
} gpe_layer_saved;

typedef struct gpe_enc_saved {
    gpe_layer_saved layer[GPE_LAYERS];
} gpe_enc_saved;

/* ---- the pieces, each callable on its own ---- */

/* Linear over rows: Y = X Wt^T + b with X (rows,Cin), Wt (Cout,Cin), b (Cout, may be null), any rows, Cin, Cout >= 1.
 *   forward: a chain over Cin.  backward: dX (rows,Cin) a chain over Cout; dW (Cout,Cin) a chain over the rows (split and merged
 *   in order); db (Cout) the ordered row sum.  dX, dW, db may each be null.  One size query serves both. */
long long gpe_linear_workspace(int rows, int Cin, int Cout);
int gpe_linear_forward(const float* X, const float* Wt, const float* b, int rows, int Cin, int Cout, float* Y, void* ws,
                       long long ws_bytes, void* stream);
int gpe_linear_backward(const float* dY, const float* X, const float* Wt, int rows, int Cin, int Cout, float* dX, float* dW, float* db,
                        void* ws, long long ws_bytes, void* stream);

/* x1 = GELU(LayerNorm_eps1e-6(dw3x3(xin) + b)) on the first n_pixels rows of the (N,H,W) row space of xin (N,H,W,C), C a multiple
 * of 64 up to 256, 1 <= n_pixels <= N H W.  The 3x3 stride-1 conv zero-pads per image and reads every pixel of an image the prefix
 * reaches.  forward_save writes dwout, x1 (n_pixels,C), mean, rstd (n_pixels).
 * backward: from d x1 (n_pixels,C) to d xin (N,H,W,C) -- written in full, a gather over the up to 9 prefix neighbours of the same
 * image, an exact 0 where no prefix row reaches --, d dw_w (C,1,3,3), d dw_b, d ln_w, d ln_b (C). */
int gpe_dwln_forward_save(const float* xin, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, int N, int H,
                          int W, int C, int n_pixels, float* dwout, float* mean, float* rstd, float* x1, void* stream);
long long gpe_dwln_backward_workspace(int N, int H, int W, int C, int n_pixels);
int gpe_dwln_backward(const float* dx1, const float* xin, const float* dwout, const float* mean, const float* rstd, const float* dw_w,
                      const float* ln_w, const float* ln_b, int N, int H, int W, int C, int n_pixels, float* dxin, float* d_dw_w,
                      float* d_dw_b, float* d_ln_w, float* d_ln_b, void* ws, long long ws_bytes, void* stream);

/* The DCNv3 core of this geometry on xp (N,H,W,256): Ho = (H - 1) / 2 + 1, Wo likewise, rows = N Ho Wo; offset (rows,72) and the mask
 * LOGITS (rows,36) are the first rows of the flat buffers.  forward: the softmax over the 9 taps of a group is fused in; writes the
 * probabilities mask (rows,36) and y (rows,256).
 * backward: from d y (rows,256), the saved offset rows and probabilities to d xp (N,H,W,256) (zero-filled here, then fp32 atomic
 * adds), d offset (rows,72) and d mask-logits (rows,36), the softmax backward m (gm - sum m gm) fused in; every d offset / d mask
 * element has exactly one writer, a tap outside the image gives exact zeros.  One wavefront per (row, group). */
int gpe_dcnv3_core_forward(const float* xp, const float* offset, const float* mask_logits, int N, int H, int W, float* mask, float* y,
                           void* stream);
int gpe_dcnv3_core_backward(const float* xp, const float* offset, const float* mask, const float* dy, int N, int H, int W, float* dxp,
                            float* doffset, float* dmask_logits, void* stream);

/* out = ReLU(GroupNorm_G(x)), x (B,C,HW) NCHW, C a multiple of G, eps 1e-5; and its backward given the saved x, mean, rstd (B,G): d is 0
 * where the pre-activation is not > 0, then the three-term form and the ordering of gpx_gn_gelu_backward. */
int gpe_gn_relu_forward(const float* x, const float* gamma, const float* beta, int B, int C, int HW, int G, float* out, float* mean,
                        float* rstd, void* stream);
long long gpe_gn_relu_backward_workspace(int B, int C);
int gpe_gn_relu_backward(const float* dout, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         int B, int C, int HW, int G, float* dx, float* dgamma, float* dbeta, void* ws, long long ws_bytes, void* stream);

/* Backward of Y = conv2d(X, Wt) + bias with a 1x1 kernel and any Cout: X (B,Cin,HW), Wt (Cout,Cin), dY (B,Cout,HW).
 *   dX (B,Cin,HW): a chain over Cout; dW (Cout,Cin): a chain over the B HW pixels; db (Cout): the ordered sum.  Each may be null. */
long long gpe_conv1x1_backward_workspace(int B, int Cin, int Cout, int HW);
int gpe_conv1x1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int HW, float* dX, float* dW,
                         float* db, void* ws, long long ws_bytes, void* stream);

/* ---- the encoder, one coupling batch ---- */

/* MAPEncoder.forward in fp32 on coor (N,3,R,R), R a multiple of 8, writing every tensor of `saved`; saved->layer[2].act
 * (N,256,R/8,R/8) is the result. */
long long gpe_map_encoder_forward_workspace(int N, int R);
int gpe_map_encoder_forward_save(const float* coor, const gpe_enc_params* w, int N, int R, const gpe_enc_saved* saved, void* ws,
                                 long long ws_bytes, void* stream);

/* From g_feat (N,256,R/8,R/8) to the gradient of every parameter (grads, all 48 written in full) and to g_coor (N,3,R,R); coor
 * and saved are what gpe_map_encoder_forward_save read and wrote for the same parameters. */
long long gpe_map_encoder_backward_workspace(int N, int R);
int gpe_map_encoder_backward(const gpe_enc_params* w, const gpe_enc_saved* saved, const float* coor, const float* g_feat, int N, int R,
                             const gpe_enc_params* grads, float* g_coor, void* ws, long long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
