/* givepose_accum.h -- the gradient-accumulation family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * What the training loop does between backward() and optimizer.step() when FLAGS.accumulate > 1 or when more than one rank trains
 * (engine/train.py:117-131): the micro-step's gradients, scaled by 1 / accumulate, are added to the accumulated ones, and
 * clip_grad_norm_(parameters, max_norm) scales the ACCUMULATED gradients in place on every micro-step -- so the next micro-step adds to
 * an already clipped buffer.  The gradients of a step arrive as hundreds of separate tensors; this family adds them into slices of one
 * flat, persistent buffer, norms and clips that buffer in GPC_ACCUM_LAUNCHES launches whatever the number of tensors, and so leaves one
 * buffer that a single all_reduce can exchange between ranks.
 *
 * The family has its own header and prefix (gpc_) next to givepose_optim.h (gpo_), whose conventions apply: a HOST table of gpo_tensor
 * (the struct is reused; the pointers inside are device pointers), both device tables sent to the head of the workspace with ONE
 * asynchronous copy, no allocation on the device, no synchronisation, no copy to the host, a hipStream_t `stream`, 0 or a negative
 * gp_status, gp_last_error(), `ws` (256-byte aligned) / `ws_bytes` with a size query that answers 0 for what the entry point refuses.
 *
 * Fields of an entry that are read: p, the accumulator slice (the destination, n floats); g, this micro-step's gradient (n floats) or
 * NULL; n; flags (GPC_FLAG_OVERWRITE or 0).  m, v, slow, rows, row_len and step_lr are ignored.
 *
 * Arithmetic, all fp32, no atomic; scale * g and the addition to a are two roundings, never one fused operation, and the sum of squares
 * is accumulated by the very expression of gpo_clip_grad_norm's reduce pass.  Per element, with a the accumulator:
 *     g != NULL, GPC_FLAG_OVERWRITE:   a = scale * g                 (the first addition of a window; scale == 1 keeps the bits of g)
 *     g != NULL, otherwise:            a = a + scale * g             (one multiply, one add: not fused)
 *     g == NULL:                       a stays                       (a parameter with an accumulated gradient that received none on
 *                                                                     this micro-step: clip_grad_norm_ still counts and scales it)
 *     norm = sqrt(sum over all entries of the NEW a squared),   coef = min(1, max_norm / (norm + 1e-6))   (max_norm <= 0: exactly 1)
 *     a = a * coef                                               (not issued for max_norm <= 0)
 * g == NULL together with GPC_FLAG_OVERWRITE is refused.
 *
 * Order.  Every tensor is cut into flat segments of GPO_CHUNK elements, a workgroup each (no centralisation here).  Inside a segment
 * element i belongs to thread (i / 4) % 256: a thread adds the squares of its elements in index order, the lanes of a wave are added by
 * a fixed butterfly, the four waves as (w0 + w1) + (w2 + w3), the segments' sums in table order by the second launch -- the map and the
 * order of gpo_clip_grad_norm.  So an accumulate with GPC_FLAG_OVERWRITE on every entry, scale == 1 and max_norm == m leaves the bits
 * that copying g and then gpo_clip_grad_norm(m) over a table of the same tensors in the same order leaves: the data and both scalars.
 * The order depends on the shapes alone, not on pointer alignment: where a quad of four elements is 16-byte aligned in p and in g it
 * moves as one 16-byte access, else as four 4-byte ones, with the same arithmetic.  Equal inputs give equal bits.
 */
#ifndef GIVEPOSE_ACCUM_H
#define GIVEPOSE_ACCUM_H

#include "givepose_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPC_ACCUM_LAUNCHES 3    /* gpc_grad_accumulate: accumulate, finalize, scale (two without clipping) */
#define GPC_FLAG_OVERWRITE 4    /* a = scale * g instead of a = a + scale * g (distinct from the GPO_FLAG_* bits) */

/* One accumulation over the n entries of the host table `tensors`.  `scalars` (device, 2 floats, may be null) receives the 2-norm of the
 * accumulated gradients before the scaling and the coefficient. */
long long gpc_grad_accumulate_workspace(const gpo_tensor* tensors, int n);
int gpc_grad_accumulate(const gpo_tensor* tensors, int n, float scale, float max_norm, float* scalars, void* ws, long long ws_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
