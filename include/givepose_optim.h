/* givepose_optim.h -- the optimiser family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * What the training loop does after backward() (engine/train.py:117-129): clip_grad_norm_(parameters, max_norm) with the 2-norm, then
 * one step of Ranger (tools/torch_utils/solver/ranger2020.py: RAdam + Lookahead + gradient centralisation, gc_loc = True) over every
 * parameter that has a gradient.  All tensors of a step are served by a fixed number of launches: GPO_STEP_LAUNCHES, whatever the
 * number of tensors.
 *
 * The family has its own header and prefix (gpo_) next to givepose_bbgrad.h (gpb_), whose conventions apply: device pointers to
 * caller-owned buffers, no allocation on the device, no synchronisation, no copy to the host, a hipStream_t `stream`, 0 or a negative
 * gp_status, gp_last_error(), `ws` (256-byte aligned) / `ws_bytes` with a size query that answers 0 for what the entry point refuses.
 *
 * The tensor table.  The caller passes a HOST array of gpo_tensor, one entry per distinct parameter that takes part in this step; the
 * pointers inside an entry are device pointers.  The entry point checks the table on the host, cuts every tensor into chunks of at most
 * GPO_CHUNK elements (the chunk table: a workgroup's tensor, offset and count), and sends both tables to the head of the workspace
 * with ONE asynchronous copy; the kernels read them there.  Nothing comes back to the host.
 *
 * Chunks.  A centralised tensor (rows > 0) with row_len <= GPO_CHUNK is cut into runs of whole rows: wave w of the workgroup takes the
 * run's rows w, w + 4, ... in turn.  A longer row is cut into segments of GPO_CHUNK elements, each served by a whole workgroup, and its
 * sum is the segments' sums added in order.  A tensor that is not centralised (rows == 0) is cut into flat segments.
 *
 * Arithmetic.  All fp32, no floating-point atomic.  Inside a row or a segment, element i belongs to lane (i / 4) % 64 of the wave (or
 * to thread (i / 4) % 256 of the workgroup for a segment): a lane adds its elements in index order, the lanes are added by a fixed
 * butterfly, the four waves as (w0 + w1) + (w2 + w3), the chunks' sums of squares in a fixed order by the second launch.  The order
 * depends on the shapes alone -- not on pointer alignment: where a quad of four elements is 16-byte aligned in every buffer it is moved
 * by one 16-byte load or store, else by four 4-byte ones, with the same arithmetic.  Equal inputs give equal bits.
 *
 * Per element, with coef the clip coefficient (1 without clipping) and mean the row mean of the gradient (centralised tensors):
 *     g' = coef (g - mean)           (the clipped gradient minus its own row mean; a row of length 1 gives an exact 0)
 *     v  = beta2 v + (1 - beta2) g' g'
 *     m  = beta1 m + (1 - beta1) g'
 *     G  = m / (sqrt(v) + eps) if the tensor's step is rectified, else m;     G += weight_decay p if weight_decay != 0
 *          (on an unrectified step the reference's G is exp_avg itself, ranger2020.py:225-228, so the decay term stays in m: m = G.
 *           build_optimizer uses weight_decay = 0, where none of this runs)
 *     p -= step_lr G                                 (step_lr: the host's step_size * lr, ranger2020.py:192-214, rounded to fp32)
 *     if lookahead:  slow += alpha (p - slow);  p = slow
 * p, g, m, v (and slow on a lookahead step) are each read once, and p, m, v (and slow) written once.
 */
#ifndef GIVEPOSE_OPTIM_H
#define GIVEPOSE_OPTIM_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPO_CHUNK 4096          /* elements per workgroup: 16 per lane, four 16-byte accesses per buffer */
#define GPO_STEP_LAUNCHES 3     /* gpo_ranger_step: reduce, finalize, update */
#define GPO_CLIP_LAUNCHES 3     /* gpo_clip_grad_norm: reduce, finalize, scale */
#define GPO_MAX_TENSORS 65536
#define GPO_FLAG_RECTIFIED 1    /* N_sma > N_sma_threshhold at this tensor's step */
#define GPO_FLAG_LOOKAHEAD 2    /* this tensor's step is a multiple of k */

typedef struct gpo_tensor {
    float *p, *g, *m, *v, *slow;     /* parameter, gradient, exp_avg, exp_avg_sq, slow_buffer: n floats each, 4-byte aligned */
    long long n;                     /* elements, >= 1 */
    int rows, row_len;               /* gradient centralisation: rows * row_len == n; rows == 0: not centralised */
    int flags;                       /* GPO_FLAG_* */
    float step_lr;                   /* step_size * lr of this tensor's step */
} gpo_tensor;

typedef struct gpo_hyper {           /* doubles, as the reference holds them: 1 - beta is formed in double and rounded once */
    double beta1, beta2, eps, alpha, weight_decay;
    double max_norm;                 /* clip_grad_norm_'s max_norm; <= 0: no clipping (the coefficient is exactly 1) */
} gpo_hyper;

/* One clip + Ranger step over the n tensors of the host table `tensors`.  `scalars` (device, 2 floats, may be null) receives the total
 * 2-norm of the gradients and the clip coefficient min(1, max_norm / (norm + 1e-6)).  The gradients are read, not scaled. */
long long gpo_ranger_step_workspace(const gpo_tensor* tensors, int n);
int gpo_ranger_step(const gpo_tensor* tensors, int n, const gpo_hyper* hyper, float* scalars, void* ws, long long ws_bytes, void* stream);

/* torch.nn.utils.clip_grad_norm_(., max_norm, norm_type = 2): scales the gradients in place by min(1, max_norm / (norm + 1e-6)) and
 * leaves the norm and the coefficient in `scalars` (device, 2 floats).  Only g and n of an entry are read. */
long long gpo_clip_grad_norm_workspace(const gpo_tensor* tensors, int n);
int gpo_clip_grad_norm(const gpo_tensor* tensors, int n, float max_norm, float* scalars, void* ws, long long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
