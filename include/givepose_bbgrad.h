/* givepose_bbgrad.h -- the backbone backward family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * Forward-that-saves and backward of the ConvNeXt backbone (timm convnext, FeatureListNet(out_indices=(3,)) as called by
 * network/backbone.py:36-46): stem conv 4x4 stride 4 + LayerNorm over channels; per stage s > 0 LayerNorm + conv 2x2 stride 2; per
 * block x + gamma * fc2(GELU(fc1(LN(dw7x7(x))))), every LayerNorm with eps 1e-6.  From the gradient of the (B,C_last,S/32,S/32) map to
 * the gradient of every parameter tensor and of the (B,3,S,S) image.  drop_path is 0 and there is neither BatchNorm nor Dropout:
 * train mode computes what this forward computes.
 *
 * The family has its own header and prefix (gpb_) next to givepose_headgrad.h (gph_), givepose_xyzgrad.h (gpx_) and
 * givepose_encgrad.h (gpe_), whose conventions apply unchanged: device pointers, caller-owned buffers, no allocation, no
 * synchronisation, no copy to the host, a hipStream_t `stream`, 0 or a negative gp_status, gp_last_error().  Every entry point that
 * needs scratch memory takes `ws` (256-byte aligned) and `ws_bytes`, and has a size query next to it that runs the entry point's own
 * host code in dry mode (0 for a shape the entry point refuses).
 *
 * All arithmetic is fp32.  Parameters and their gradients are in the reference's own shapes and layouts: conv_dw.weight (C,1,7,7),
 * (out, in) linear weights, OIHW stem and downsample weights.  The image, feat and their gradients are NCHW; inside the family an
 * activation is channels-last: rows (b,h,w) x C.  The moves between the two are operand views and store functors of the GEMM
 * (csrc/grad_gemm.hpp), never a transpose kernel.
 *
 * Shapes.  Any number of stages (1 .. GPB_MAX_STAGES), any depths >= 1, every dim a multiple of 64 (a lane holds a channel in the
 * depth-wise kernels, a wavefront a 64-channel slab), any square image side S that is a multiple of 4 2^(stages - 1).  No kernel
 * assumes a map size or a channel count of the network.
 *
 * Determinism.  There is no floating-point atomic in this family.  Every contraction is a k-ordered fmaf chain of the functor GEMM
 * (splits merged in order); every sum over rows is ordered: a lane takes its rows in turn, the four waves of a workgroup are added
 * as (w0 + w1) + (w2 + w3), and the workgroups' partial sums are added in order by a second launch.  Equal inputs give equal bits,
 * and scaling the upstream gradient by a power of two scales every gradient by it bit for bit (short of overflow and underflow).
 *
 * Memory.  gpb_backbone_forward_save writes per block the input x, the depth-wise output, the fc1 pre-activation h (4C wide) and
 * the fc2 output y2: 7 C floats per row and the two LayerNorm statistics.  ConvNeXt-Base at 256 x 256: 176.7 MB per crop,
 * 11.3 GB at B = 64 (givepose_amd.bb_grad.saved_bytes counts it).
 */
#ifndef GIVEPOSE_BBGRAD_H
#define GIVEPOSE_BBGRAD_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPB_MAX_STAGES 8
#define GPB_STEM_PATCH 4      /* stem conv 4x4 stride 4 */
#define GPB_DOWN_PATCH 2      /* downsample conv 2x2 stride 2 */

/* Parameter tables.  A table is an array of float* in state_dict order: gpb_stem_params, then per stage s [gpb_down_params if
 * s > 0, then depths[s] gpb_block_params].  The same layout holds the weights (read) and their gradients (written in full). */
typedef struct gpb_stem_params {
    float *conv_w, *conv_b;      /* stem_0.weight (C0,3,4,4), .bias (C0) */
    float *ln_w, *ln_b;          /* stem_1.weight, .bias (C0) */
} gpb_stem_params;

typedef struct gpb_down_params {
    float *ln_w, *ln_b;          /* stages_s.downsample.0.weight, .bias (C_{s-1}) */
    float *conv_w, *conv_b;      /* stages_s.downsample.1.weight (C_s,C_{s-1},2,2), .bias (C_s) */
} gpb_down_params;

typedef struct gpb_block_params {
    float* gamma;                /* stages_s.blocks.b.gamma (C) */
    float *dw_w, *dw_b;          /* conv_dw.weight (C,1,7,7), .bias (C) */
    float *ln_w, *ln_b;          /* norm.weight, .bias (C) */
    float *fc1_w, *fc1_b;        /* mlp.fc1.weight (4C,C), .bias (4C) */
    float *fc2_w, *fc2_b;        /* mlp.fc2.weight (C,4C), .bias (C) */
} gpb_block_params;

/* Saved tables: an array of float* -- gpb_norm_saved of the stem, then per stage s [gpb_norm_saved of the downsample if s > 0, then
 * depths[s] gpb_block_saved].  rows = B H W of the map the entry belongs to. */
typedef struct gpb_norm_saved {
    float* pre;                  /* the LayerNorm's input (rows,C): the stem conv's output / the stage input before the downsample */
    float *mean, *rstd;          /* (rows) */
} gpb_norm_saved;

typedef struct gpb_block_saved {
    float* x;                    /* the block's input (rows,C) */
    float* dwout;                /* dw7x7(x) + bias (rows,C): the LayerNorm's input */
    float *mean, *rstd;          /* (rows) */
    float* h;                    /* the fc1 pre-activation (rows,4C) */
    float* y2;                   /* the fc2 output (rows,C) */
} gpb_block_saved;

/* ---- the pieces, each callable on its own ---- */

/* Depth-wise 7x7, stride 1, pad 3 on x (N,H,W,C) channels-last, H and W independent, C a multiple of 64.
 *   forward: y = dw7x7(x) + b, a chain of bias then the taps in (kh, kw) order; a tap outside the image is skipped or adds an exact 0.
 *   backward: dx (N,H,W,C) a gather of dy with flipped taps (no scatter); dw (C,1,7,7): 49 ordered sums per channel over the N H W
 *   rows, accumulated in registers (a lane per channel), a workgroup per row chunk, the chunks merged in order; db (C) likewise.  A
 *   tap that meets no pixel anywhere (maps smaller than the window) gets an exact 0. */
int gpb_dw7_forward(const float* x, const float* w, const float* b, int N, int H, int W, int C, float* y, void* stream);
long long gpb_dw7_backward_workspace(int N, int H, int W, int C);
int gpb_dw7_backward(const float* dy, const float* x, const float* w, int N, int H, int W, int C, float* dx, float* dw, float* db, void* ws,
                     long long ws_bytes, void* stream);

/* LayerNorm over channels, eps 1e-6, on x (rows,C), C a multiple of 64.  forward_save writes y, mean and rstd (rows).
 * backward: the three-term form at the SAVED statistics (they are not recomputed): dx (rows,C), dw = sum dy xhat and db = sum dy
 * as ordered row sums. */
int gpb_layernorm_forward_save(const float* x, const float* w, const float* b, int rows, int C, float* y, float* mean, float* rstd,
                               void* stream);
long long gpb_layernorm_backward_workspace(int rows, int C);
int gpb_layernorm_backward(const float* dy, const float* x, const float* mean, const float* rstd, const float* w, int rows, int C,
                           float* dx, float* dw, float* db, void* ws, long long ws_bytes, void* stream);

/* Patch conv: kernel p x p, stride p, no padding (non-overlapping patches), through the view rows (b,oh,ow) x columns (ci,kh,kw), so
 * that the OIHW weight is a plain (Cout, Cin p p) matrix.  nchw != 0: x and dx are (N,Cin,H,W) (the stem from the image); else
 * (N,H,W,Cin) rows (the downsample).  y and dy are rows (N H/p W/p, Cout).  H and W multiples of p.
 *   backward: dx through a store functor, every input element written exactly once; dw (Cout,Cin,p,p) a chain over the output rows;
 *   db the ordered row sum.  dx, dw, db may each be null. */
long long gpb_patch_conv_workspace(int N, int H, int W, int Cin, int Cout, int p, int nchw);
int gpb_patch_conv_forward(const float* x, const float* w, const float* b, int N, int H, int W, int Cin, int Cout, int p, int nchw,
                           float* y, void* ws, long long ws_bytes, void* stream);
int gpb_patch_conv_backward(const float* dy, const float* x, const float* w, int N, int H, int W, int Cin, int Cout, int p, int nchw,
                            float* dx, float* dw, float* db, void* ws, long long ws_bytes, void* stream);

/* One block on x (N,H,W,C): out = x + gamma * fc2(GELU(fc1(LN(dw7x7(x))))).  `params` / `grads` are gpb_block_params.
 *   forward_save writes dwout, mean, rstd, h, y2 (gpb_block_saved without x) and out (rows,C).
 *   backward: from g = d out (rows,C) to the nine parameter gradients and dx = g + (the depth-wise dX), added in that order.
 *   a = GELU(h) is formed once into the workspace (fc2's dW reads it); d h = (d y2 . W2) GELU'(h) in the dX GEMM's store functor;
 *   d gamma the ordered row sum of g y2; d y2 = g gamma is never materialised: d W2 = gamma (g^T a) scales in its store functor and
 *   d h contracts g with gamma W2 (formed once per block in the workspace).
 * One size query serves both. */
long long gpb_block_workspace(int N, int H, int W, int C);
int gpb_block_forward_save(const float* x, const gpb_block_params* params, int N, int H, int W, int C, float* dwout, float* mean,
                           float* rstd, float* h, float* y2, float* out, void* ws, long long ws_bytes, void* stream);
int gpb_block_backward(const float* g, const float* x, const gpb_block_params* params, const float* dwout, const float* mean,
                       const float* rstd, const float* h, const float* y2, int N, int H, int W, int C, const gpb_block_params* grads,
                       float* dx, void* ws, long long ws_bytes, void* stream);

/* ---- the backbone ---- */

/* The number of float* entries of a parameter table (0 for a refused configuration); a saved table has
 * 3 n_stages + 6 sum(depths) entries. */
int gpb_param_count(const int* depths, int n_stages);

/* img (B,3,S,S) NCHW -> feat (B,C_last,S/2^(n_stages+1),.) NCHW, writing every tensor of the saved table. */
long long gpb_backbone_forward_workspace(const int* dims, const int* depths, int n_stages, int B, int S);
int gpb_backbone_forward_save(const float* img, float* const* params, const int* dims, const int* depths, int n_stages, int B, int S,
                              float* const* saved, float* feat, void* ws, long long ws_bytes, void* stream);

/* From g_feat (NCHW, like feat) to the gradient of every parameter (grads: a parameter table, every tensor written in full) and
 * d_img (B,3,S,S); params, saved and img are what gpb_backbone_forward_save read and wrote. */
long long gpb_backbone_backward_workspace(const int* dims, const int* depths, int n_stages, int B, int S);
int gpb_backbone_backward(float* const* params, float* const* saved, const float* img, const float* g_feat, const int* dims,
                          const int* depths, int n_stages, int B, int S, float* const* grads, float* d_img, void* ws, long long ws_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
