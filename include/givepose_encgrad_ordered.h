/* givepose_encgrad_ordered.h -- the map-encoder backward with a selectable d xp scatter (prefix gpeo_), next to givepose_encgrad.h.
 *
 * givepose_encgrad.h scatters d xp, the gradient of the map the DCNv3 core samples, with fp32 atomic adds: the terms of one element
 * arrive in an order that changes from run to run, and so do the last bits of everything downstream of a scatter.  The entry
 * points here take a trailing `scatter`:
 *
 *   GPE_SCATTER_ATOMIC    the code of the gpe_ entry points, which are wrappers of these at this value: same launches, same
 *                         workspace, same results to rounding.
 *   GPE_SCATTER_ORDERED   d xp element (b, h, w, g, lane) is the sum of the SAME terms, added in a fixed order:
 *                           term     c = fmul(w_k, tg), tg = fmul(dy[(row 4 + g) 64 + lane], mask[(row 4 + g) 9 + q]), for every output
 *                                    row, tap q = 0..8 and corner k = 1..4 whose corner pixel is (b, h, w), with
 *                                    w_1 = fmul(hh, hw), w_2 = fmul(hh, lw), w_3 = fmul(lh, hw), w_4 = fmul(lh, lw) and the locations,
 *                                    lh, lw, hh = 1 - lh, hw = 1 - lw formed as the atomic kernel forms them;
 *                           order    ascending source id s = (row 9 + q) 4 + (k - 1);
 *                           sum      acc = +0, then acc = fadd(acc, c) per term: each product and each sum rounded on its own (no
 *                                    fused multiply-add); an element nothing reaches is +0.
 *                         d offset and d mask-logits are the atomic mode's, bit for bit.  Two calls on the same inputs give equal
 *                         bits in every output; there is no floating-point atomic and no zero-fill of d xp (every element is
 *                         written once by the wavefront that owns it).  Any list length is handled: all 36 rows sources of a group
 *                         may fall on one pixel (slowly: one wavefront adds them one after the other).
 *
 * The ordered mode builds an inverted index per call in the workspace: per destination (b, h, w, g) a counter and a segment start
 * (2 N H W 4 ints), the scan's tile sums, and room for one 32-bit id per corner (144 rows ints): at R = 64 about 0.7 MB per crop
 * in layer 0 and a quarter of that in each layer after.  The encoder carves a layer's index out of that layer's own scratch, so its
 * workspace grows by layer 0's.
 *
 * Conventions are givepose_encgrad.h's.  An unknown `scatter` is refused by name (gp_last_error()), and its size query answers 0.
 */
#ifndef GIVEPOSE_ENCGRAD_ORDERED_H
#define GIVEPOSE_ENCGRAD_ORDERED_H

#include "givepose_encgrad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPE_SCATTER_ATOMIC 0
#define GPE_SCATTER_ORDERED 1

/* gpe_dcnv3_core_backward with the scatter mode and a workspace (GPE_SCATTER_ATOMIC needs none: ws may be null, the query answers
 * 0 as it does for a shape the entry point refuses). */
long long gpeo_dcnv3_core_backward_workspace(int N, int H, int W, int scatter);
int gpeo_dcnv3_core_backward(const float* xp, const float* offset, const float* mask, const float* dy, int N, int H, int W, float* dxp,
                             float* doffset, float* dmask_logits, void* stream, int scatter, void* ws, long long ws_bytes);

/* gpe_map_encoder_backward with the scatter mode; the workspace of GPE_SCATTER_ORDERED is larger by the index of layer 0. */
long long gpeo_map_encoder_backward_workspace(int N, int R, int scatter);
int gpeo_map_encoder_backward(const gpe_enc_params* w, const gpe_enc_saved* saved, const float* coor, const float* g_feat, int N, int R,
                              const gpe_enc_params* grads, float* g_coor, void* ws, long long ws_bytes, void* stream, int scatter);

#ifdef __cplusplus
}
#endif
#endif
