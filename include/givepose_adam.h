/* givepose_adam.h -- Adam and AdamW of libgivepose_hip.so (gfx950 / MI355X).
 *
 * The two other choices of the training loop's FLAGS.optimizer_type (engine/train.py:66-72): torch.optim.AdamW(param_list, lr) and
 * torch.optim.Adam(param_list), after clip_grad_norm_(parameters, max_norm) with the 2-norm.  All tensors of a step are served by
 * GPAD_STEP_LAUNCHES launches, whatever the number of tensors.
 *
 * The family has its own header and prefix (gpad_) next to givepose_optim.h (gpo_), whose conventions apply unchanged: a HOST table of
 * gpad_tensor, one entry per parameter stepped, with device pointers inside; the entry point checks the table on the host, cuts every
 * tensor into flat chunks of at most GPO_CHUNK elements and sends tensor and chunk table to the head of the workspace with ONE
 * asynchronous copy; no allocation, no synchronisation, nothing back to the host, no floating-point atomic; 0 or a negative gp_status,
 * gp_last_error(), `ws` (256-byte aligned) / `ws_bytes` with a size query that answers 0 for what the entry point refuses.
 *
 * Launches.  (1) reduce: the chunks' sums of squares of g, in the order givepose_optim.h gives a tensor that is not centralised, so that
 * the norm has the bits of gpo_clip_grad_norm on equal data.  (2) finalize: the norm and coef = min(1, max_norm / (norm + 1e-6)), or
 * exactly 1 for max_norm <= 0.  (3) update.  The gradients are read, not scaled.
 *
 * Per element, all fp32, one rounding per operation (no fused multiply-add), in the order of torch.optim.adam._single_tensor_adam:
 *     g' = coef * g
 *     GPAD_MODE_ADAM  and weight_decay != 0:   g' = g' + wd * p
 *     GPAD_MODE_ADAMW and weight_decay != 0:   p  = p * decay                 decay = fp32(1 - lr * wd)
 *     m  = m + omb1 * (g' - m)                                                omb1 = fp32(1 - beta1)
 *     v  = v * beta2 + (omb2 * g') * g'                                       omb2 = fp32(1 - beta2)
 *     amsgrad:  vmax = max(vmax, v),  u = vmax;   else u = v
 *     den = sqrt(u) / bc2_sqrt + eps                                          bc2_sqrt = fp32((1 - beta2^step)^0.5)
 *     p  = p - step_size * (m / den)                                          step_size = fp32(lr / (1 - beta1^step))
 * The square root and the quotients are correctly rounded.  step_size, bc2_sqrt and decay are formed by the caller in double and rounded
 * once; they are per tensor because a tensor without a gradient is skipped and keeps its own step count.
 * p, g, m, v (and vmax under amsgrad) are each read once, and p, m, v (and vmax) written once.  Where a quad of four elements is 16-byte
 * aligned in every buffer it moves as one 16-byte access, else as four 4-byte ones with the same arithmetic: equal inputs give equal
 * bits wherever the buffers lie.
 */
#ifndef GIVEPOSE_ADAM_H
#define GIVEPOSE_ADAM_H

#include "givepose_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPAD_STEP_LAUNCHES 3     /* gpad_adam_step: reduce, finalize, update */
#define GPAD_MAX_TENSORS 65536
#define GPAD_MODE_ADAM 0         /* weight decay is added to the gradient */
#define GPAD_MODE_ADAMW 1        /* weight decay multiplies the parameter */

typedef struct gpad_tensor {
    float *p, *g, *m, *v, *vmax;     /* parameter, gradient, exp_avg, exp_avg_sq, max_exp_avg_sq: n floats each, 4-byte aligned;
                                        vmax is read under amsgrad only and may be null otherwise */
    long long n;                     /* elements, >= 1 */
    float step_size, bc2_sqrt;       /* lr / (1 - beta1^step), (1 - beta2^step)^0.5 of this tensor's step */
    float decay;                     /* 1 - lr * weight_decay (read in GPAD_MODE_ADAMW with weight_decay != 0) */
    int pad;
} gpad_tensor;

typedef struct gpad_hyper {          /* doubles, as torch holds them: 1 - beta is formed in double and rounded once */
    double beta1, beta2, eps, weight_decay;
    double max_norm;                 /* clip_grad_norm_'s max_norm; <= 0: no clipping (the coefficient is exactly 1) */
    int mode;                        /* GPAD_MODE_* */
    int amsgrad;                     /* 0 or 1 */
} gpad_hyper;

/* One clip + Adam / AdamW step over the n tensors of the host table `tensors`.  `scalars` (device, 2 floats, may be null) receives the
 * total 2-norm of the gradients and the clip coefficient. */
long long gpad_adam_step_workspace(const gpad_tensor* tensors, int n, const gpad_hyper* hyper);
int gpad_adam_step(const gpad_tensor* tensors, int n, const gpad_hyper* hyper, float* scalars, void* ws, long long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
