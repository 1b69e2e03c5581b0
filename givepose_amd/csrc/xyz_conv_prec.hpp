// The contractions of the coordinate-head family in a precision (include/givepose_xyzgrad_bf16.h, gpxm_*): the stride-1 window view
// of xyzgrad.hip and gemm_px, which sends a contraction to the fp32 functor GEMM (grad_gemm.hpp: the gpx_ kernels and bits) or, for
// GPX_PREC_BF16, to its bf16-operand form (the 128 x 128 kernel on v_mfma_f32_32x32x16_bf16) with the same views and store functors.
// The contract of the bf16 form is stated in that kernel's header and in DESIGN.md 1j / 1k.
#ifndef GIVEPOSE_XYZ_CONV_PREC_HPP
#define GIVEPOSE_XYZ_CONV_PREC_HPP

#include "grad_gemm_bf16.hpp"
#include "../../include/givepose_xyzgrad_bf16.h"

namespace {

// (B,C,H,H) as rows (b,h,w) x columns (c,kh,kw): the element at (h - 1 + kh, w - 1 + kw) -- the im2col view of a stride-1 pad-1 conv
// input -- or with flip at (h + 1 - kh, w + 1 - kw) -- the gathered view of its output gradient --, an exact 0 outside the map.
// The tile loader keeps a thread on one row for a whole contraction, so the compiler hoists the divisions of r out of the k loop.
struct WindowS1 {
    const float* p; int C, H, flip;
    static constexpr bool FAST_C = false;
    __device__ __forceinline__ float operator()(int r, int c) const {
        const int hw = H * H, b = r / hw, px = r - b * hw, h = px / H, w = px - h * H;
        const int ch = c / 9, t0 = c - ch * 9, t = flip ? 8 - t0 : t0, kh = t / 3, kw = t - kh * 3;
        const int y = h - 1 + kh, x = w - 1 + kw;
        if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)H) return 0.0f;
        return p[(((long)b * C + ch) * H + y) * H + x];
    }
};

// The window as A (forward and dX): what depends on the pixel -- the address of (b, 0, h, w) and which of the nine taps lie inside the
// map -- is formed once per thread; an element (c, kh, kw) is then one bit of the mask and the wave-uniform offset c HW + (kh - 1) H +
// (kw - 1) from that address.
template <> struct Bf16Rows<WindowS1> {
    static constexpr bool value = (GP_BF16_WIDE_MASK & 2) != 0;
    struct State { const float* base; unsigned taps; };
    static __device__ __forceinline__ State init(const WindowS1& f, int r, int R) {
        if (r >= R) return State{f.p, 0u};
        const int H = f.H, hw = H * H, b = r / hw, px = r - b * hw, h = px / H, w = px - h * H;
        unsigned taps = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int y = h - 1 + t / 3, x = w - 1 + t % 3;
            if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)H) taps |= 1u << t;
        }
        return State{f.p + (((long)b * f.C * H + h) * H + w), taps};
    }
    static __device__ __forceinline__ float get(const WindowS1& f, const State& st, int c) {
        const int ch = c / 9, t0 = c - ch * 9, t = f.flip ? 8 - t0 : t0, kh = t / 3, kw = t - kh * 3;
        if (!((st.taps >> t) & 1u)) return 0.0f;
        return st.base[(long)ch * f.H * f.H + (kh - 1) * f.H + (kw - 1)];
    }
};

bool xyz_prec_ok(int p) { return p == GPX_PREC_F32 || p == GPX_PREC_BF16; }

// the partial sums of a contraction in a precision: the two forms tile, and so split, differently
long gemm_px_ws_floats(int prec, long M, long N, long K) { return prec == GPX_PREC_BF16 ? gemm_bf16_ws_floats(M, N, K) : gemm_ws_floats(M, N, K); }

template <class AF, class BF, class EP>
int gemm_px(int prec, const AF& A, const BF& Bm, const EP& ep, long M, long N, long K, float* ws, long ws_floats, hipStream_t s,
            const char* name) {
    if (prec == GPX_PREC_BF16) return gemm_bf16(A, Bm, ep, M, N, K, ws, ws_floats, s, name);
    return gemm(A, Bm, ep, M, N, K, ws, ws_floats, s, name);
}

}  // namespace

#endif
