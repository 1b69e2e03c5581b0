// What encgrad.hip calls of encscatter.hip: the ordered d xp of the specialised DCNv3 core (include/givepose_encgrad_ordered.h).
#ifndef GIVEPOSE_ENCSCATTER_HPP
#define GIVEPOSE_ENCSCATTER_HPP

#include <hip/hip_runtime.h>

namespace encscatter {

// floats (4-byte words) of workspace an ordered d xp of xp (N,H,W,256) takes; the shape is one core_ok accepts
long ordered_dxp_ws_floats(long N, long H, long W);

// d xp (N,H,W,256), every element written here: per destination the terms fmul(w_k, fmul(dy, mask)) added from +0 in ascending
// order of the source id (row 9 + q) 4 + (k - 1).  offset (rows,72), mask (rows,36) probabilities, dy (rows,256); ws 256-byte
// aligned, at least ordered_dxp_ws_floats words.
int ordered_dxp(const float* offset, const float* mask, const float* dy, int N, int H, int W, float* dxp, float* ws, long ws_floats,
                hipStream_t s, const char* name);

}  // namespace encscatter
#endif
