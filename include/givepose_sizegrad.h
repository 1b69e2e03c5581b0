/* givepose_sizegrad.h -- the train-mode size head of libgivepose_hip.so (gfx950 / MI355X).
 *
 * SizeHead (network/pose_head.py:17-42) as the training loop runs it, under network.train() (engine/train.py:36): BatchNorm1d
 * normalises with the statistics of the batch and Dropout(0.2) is active.  gp_size_head (givepose_hip.h) is the eval-mode head: the
 * running statistics folded into conv1, no dropout.  This family is the other function: a forward that saves what the backward needs,
 * the backward, and the update of the running statistics.
 *
 * The family has its own header and prefix (gps_) next to givepose_optim.h (gpo_), whose conventions apply: device pointers to
 * caller-owned buffers, no allocation on the device, no synchronisation, no copy to the host, a hipStream_t `stream`, 0 or a negative
 * gp_status, gp_last_error(), `ws` (256-byte aligned) / `ws_bytes` with a size query that answers 0 for what the entry point refuses.
 *
 * Sizes.  feat is (B,C,HW); F = feat_ts hidden channels; the output dimension is 3.  B >= 2 (one value per channel has no variance:
 * torch refuses it too), C a multiple of 64 and at most GPS_MAX_C, HW >= 1, F a multiple of 16 (gp_size_head's constraint).
 *
 * Forward (GPS_FORWARD_LAUNCHES launches, whatever B):
 *   1. pooled[b,c] = max_hw feat[b,c,hw];  arg[b,c] = the LOWEST hw that attains the maximum.  The tie rule is this library's: torch
 *      documents none.  feat is read once, NHWC (fp16 or fp32: the layout and dtype the network's forward holds) or NCHW fp32.
 *   2. h = pooled W1^T + b1 (B,F);  per channel over the batch, two passes: mean = sum_b h / B, var = sum_b (h - mean)^2 / B (biased),
 *      rstd = 1 / sqrt(var + GPS_BN_EPS), xhat = (h - mean) rstd, y = gamma xhat + beta;  d = relu(y) keep / (1 - p), p = 0.2, so
 *      the factor is exactly 1.25.  h is fp32; the statistics, xhat and y are formed from it in fp64 and y is rounded once (see
 *      Arithmetic).  One workgroup owns GPS_CHUNK channels for all B rows: a wave computes the rows' dot products (the
 *      lanes split C, a fixed butterfly adds them), then wave w owns channel w of the chunk and its lanes split the rows.
 *   3. out = d W2^T + b2 (B,3), and size = out + mean_size / |mean_size| where mean_size is given (network/PoseNet.py:199-202).
 *   Also saved: mean and the unbiased variance sum_b (h - mean)^2 / (B - 1), which the running statistics take.
 *
 * The dropout mask is an input.  Explicit: keep_in, (B,F) bytes, non-zero = kept.  Seeded (keep_in null): unit idx = b F + f is kept iff
 *     x = seed_lo ^ (idx * 0x9E3779B9) ^ rotl32(seed_hi, 16);                       (32-bit arithmetic, seed = seed_hi : seed_lo)
 *     x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16;   (the murmur3 finaliser)
 *     x >= GPS_DROP_THRESHOLD = floor(0.2 * 2^32).
 * The rule needs no state.  Either way saved.keep receives the mask that was used (0 / 1), and the backward reads it there.
 *
 * Backward from g_out (B,3) (GPS_BACKWARD_LAUNCHES launches, whatever B):
 *   1. per channel (the same ownership): dd = g_out W2, dy = dd keep / (1 - p) [d > 0], dgamma = sum_b dy xhat, dbeta = sum_b dy,
 *      dW2 = g_out^T d, db2 = sum_b g_out, and with dxhat = dy gamma
 *          dh = rstd / B (B dxhat - sum_b dxhat - xhat sum_b dxhat xhat),     db1 = sum_b dh   (analytically 0; returned as computed)
 *   2. dW1 = dh^T pooled (F,C): a thread per element, the rows added in order.
 *   3. dpooled = dh W1, and d feat[b,c,hw] = dpooled[b,c] at hw = arg[b,c], +0.0 elsewhere: (B,C,HW) fp32 NCHW, every element
 *      written by this launch (no memset, no scatter).
 *
 * Arithmetic.  Every tensor is fp32 and so are the contractions.  The per-channel batch statistics and their backward (mean, var, rstd,
 * xhat, the sums over b of step 1 of the backward, dh) are formed in fp64 from the fp32 h, which torch's CPU BatchNorm does too for
 * float32 input (its accumulation type is double): dh is a difference of the size (1 - xhat^2) of its terms, and with a channel
 * variance of a few tens of eps the fp32 rounding of mean alone costs four digits of dh.  The saved statistics are fp32 pairs hi + lo
 * (mean, mean_lo; rstd, rstd_lo), so the backward reads the forward's fp64 values back; xhat is recomputed from the saved h.
 * No atomic; every sum is added in an order that depends on the shapes alone (a lane adds its terms in index
 * order, the lanes of a wave by a fixed butterfly, the four partial sums of a workgroup as (p0 + p1) + (p2 + p3)): equal inputs give
 * equal bits wherever the buffers lie.
 */
#ifndef GIVEPOSE_SIZEGRAD_H
#define GIVEPOSE_SIZEGRAD_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPS_CHUNK 4                     /* hidden channels per workgroup of the statistics kernels: one per wave */
#define GPS_MAX_C 4096                  /* the chunk's rows of W1 are staged in LDS: GPS_CHUNK * C floats */
#define GPS_FORWARD_LAUNCHES 3          /* pool, hidden + statistics + dropout, out */
#define GPS_BACKWARD_LAUNCHES 3         /* per-channel sums and dh, dW1, dpooled + d feat */
#define GPS_DROP_THRESHOLD 858993459u   /* floor(0.2 * 2^32) */
#define GPS_BN_EPS 1e-5                /* double, as nn.BatchNorm1d holds it */

typedef struct gps_params {             /* size_head's six tensors, weights or their gradients */
    float *w1, *b1;                     /* conv1 (F,C), (F,) */
    float *w2, *b2;                     /* conv2 (3,F), (3,) */
    float *gamma, *beta;                /* bn1 (F,), (F,) */
} gps_params;

typedef struct gps_saved {
    float* pooled;                      /* (B,C) */
    int* arg;                           /* (B,C) the lowest hw of the maximum */
    float* h;                           /* (B,F) conv1's output, the input of bn1 */
    float *mean, *mean_lo;              /* (F,) each: the batch mean as hi + lo; mean is the statistic the running mean takes */
    float *rstd, *rstd_lo;              /* (F,) each */
    float* d;                           /* (B,F) relu(y) keep / (1 - p) */
    unsigned char* keep;                /* (B,F) the mask used, 0 / 1 */
    float* out;                         /* (B,3) the head's output */
    float* var_unbiased;                /* (F,) */
} gps_saved;

/* feat: dtype GP_F32 or GP_F16; nhwc != 0: (B,HW,C), else (B,C,HW), which must be GP_F32.  keep_in null: the seeded rule with `seed`.
 * mean_size / size (both null or both given, (B,3)): size = out + mean_size / |mean_size|. */
int gps_size_forward_save(const void* feat, int dtype, int nhwc, const gps_params* params, const unsigned char* keep_in,
                          unsigned long long seed, const float* mean_size, int B, int C, int HW, int F, const gps_saved* saved, float* size,
                          void* stream);

long long gps_size_backward_workspace(int B, int C, int HW, int F);
int gps_size_backward(const gps_params* params, const gps_saved* saved, const float* g_out, int B, int C, int HW, int F,
                      const gps_params* grads, float* d_feat, void* ws, long long ws_bytes, void* stream);

/* nn.BatchNorm1d's update in train mode: running_mean = (1 - momentum) running_mean + momentum mean, running_var the same with the
 * unbiased variance, num_batches_tracked (one int64, may be null) += 1.  One launch. */
int gps_bn_running_update(float* running_mean, float* running_var, long long* num_batches_tracked, const float* mean,
                          const float* var_unbiased, int F, double momentum, void* stream);

#ifdef __cplusplus
}
#endif
#endif
