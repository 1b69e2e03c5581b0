// The functor GEMM of the backward families (gph_* in pnpgrad.hip, gpx_* in xyzgrad.hip), shared by inclusion.
//
// One LDS-tiled GEMM kernel on v_mfma_f32_32x32x2_f32 serves every long contraction.  Its operands are functors that map
// (row, column) of a logical matrix to an address -- a plain matrix, an NCHW tensor read as (pixels, channels), the im2col
// view of a conv input, the gathered view of a conv output gradient -- so no operand is ever materialised.  An element
// outside the tensor (padding, a tap without an output pixel, the ragged edge of a tile) is an exact 0, and fma(0, b, acc)
// leaves acc unchanged, so each result is the fmaf chain over the terms that exist, in the order of k.
//
// Everything lives in an unnamed namespace: each translation unit that includes this header gets its own instantiations.
#ifndef GIVEPOSE_GRAD_GEMM_HPP
#define GIVEPOSE_GRAD_GEMM_HPP

#include "common.hpp"
#include "../../include/givepose_headgrad.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TM = 64, TN = 64, TK = 32, WG = 256;

// ---------------------------------------------------------------------------------- operand views: element (r, c)
// FAST_C: consecutive c are adjacent in memory (the tile loader then walks c with the lane index, else r)
struct MatRow {      // p[r * ld + c]
    const float* p; long ld;
    static constexpr bool FAST_C = true;
    __device__ __forceinline__ float operator()(int r, int c) const { return p[(long)r * ld + c]; }
};
struct MatCol {      // p[c * ld + r]
    const float* p; long ld;
    static constexpr bool FAST_C = false;
    __device__ __forceinline__ float operator()(int r, int c) const { return p[(long)c * ld + r]; }
};
struct Nchw {        // (B,C,HW) read as rows (b, pixel) x columns c
    const float* p; int C, HW;
    static constexpr bool FAST_C = false;
    __device__ __forceinline__ float operator()(int r, int c) const {
        const int b = r / HW, px = r - b * HW;
        return p[((long)b * C + c) * HW + px];
    }
};
struct Im2col {      // conv input (B,Cin,H,H) as rows (b,oh,ow) x columns (ci,kh,kw): 3x3, stride 2, pad 1
    const float* x; int Cin, H, Ho;
    static constexpr bool FAST_C = false;
    __device__ __forceinline__ float operator()(int r, int c) const {
        const int hw = Ho * Ho, b = r / hw, px = r - b * hw, oh = px / Ho, ow = px - oh * Ho;
        const int ci = c / 9, t = c - ci * 9, kh = t / 3, kw = t - kh * 3;
        const int ih = 2 * oh - 1 + kh, iw = 2 * ow - 1 + kw;
        if ((unsigned)ih >= (unsigned)H || (unsigned)iw >= (unsigned)H) return 0.0f;
        return x[(((long)b * Cin + ci) * H + ih) * H + iw];
    }
};
struct GatherDY {    // conv output gradient (B,Cout,Ho,Ho) as rows (b,ih,iw) x columns (co,kh,kw): the tap's output pixel, or 0
    const float* dy; int Cout, H, Ho;
    static constexpr bool FAST_C = false;
    __device__ __forceinline__ float operator()(int r, int c) const {
        const int hw = H * H, b = r / hw, px = r - b * hw, ih = px / H, iw = px - ih * H;
        const int co = c / 9, t = c - co * 9, kh = t / 3, kw = t - kh * 3;
        const int th = ih + 1 - kh, tw = iw + 1 - kw;      // = 2 oh, 2 ow
        if (th < 0 || tw < 0 || (th & 1) || (tw & 1)) return 0.0f;
        const int oh = th >> 1, ow = tw >> 1;
        if (oh >= Ho || ow >= Ho) return 0.0f;             // no bottom / right padding at even sizes
        return dy[(((long)b * Cout + co) * Ho + oh) * Ho + ow];
    }
};
struct WeightDx {    // OIHW weights as rows (co,kh,kw) x columns ci
    const float* w; int Cin;
    static constexpr bool FAST_C = false;
    __device__ __forceinline__ float operator()(int r, int c) const {
        const int co = r / 9, t = r - co * 9;
        return w[((long)co * Cin + c) * 9 + t];
    }
};
template <class F> struct Tr {
    F f;
    static constexpr bool FAST_C = !F::FAST_C;
    __device__ __forceinline__ float operator()(int r, int c) const { return f(c, r); }
};

// ---------------------------------------------------------------------------------- result stores: element (m, n)
// M_FAST: consecutive m are adjacent in memory (the kernel then puts m on the lane index of the MFMA result)
struct EpRow {       // C[m * ld + n] = act(v + bias[n] (+ C))
    float* C; long ld; const float* bias; int lrelu, accumulate;
    static constexpr bool M_FAST = false;
    __device__ __forceinline__ void operator()(int m, int n, float v) const {
        const long i = (long)m * ld + n;
        if (bias) v += bias[n];
        if (accumulate) v = C[i] + v;
        if (lrelu) v = v > 0.0f ? v : 0.1f * v;
        C[i] = v;
    }
};
struct EpNchw {      // rows (b, pixel) -> C (B,Cc,HW), times scale[m] when given
    float* C; int Cc, HW; const float* scale;
    static constexpr bool M_FAST = true;
    __device__ __forceinline__ void operator()(int m, int n, float v) const {
        const int b = m / HW, px = m - b * HW;
        C[((long)b * Cc + n) * HW + px] = scale ? v * scale[m] : v;
    }
};

// ---------------------------------------------------------------------------------- the GEMM
// C(m, n) = sum_k A(m, k) B(k, n), k in [z kchunk, min(K, (z + 1) kchunk)).  64 x 64 tile, four waves of 32 x 32, k in steps of
// 32 through LDS ([k][m] and [k][n] images, one row of pad), the next step's operands fetched under the MFMAs.  With one chunk
// the result goes through the store functor, else to part[z][m][n] for gemm_merge_kernel.
template <class F, bool FAST_C>
__device__ __forceinline__ void tile_fetch(const F& f, int r0, int R, int c0, int C1, float (&v)[8], bool rows_are_k) {
    // A: rows m, columns k (rows_are_k false).  B: rows k, columns n (rows_are_k true).  The tile is 64 (m or n) x 32 (k).
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int r, c;
        if (!rows_are_k) {     // 64 rows x 32 columns
            if (FAST_C) { c = t & 31; r = (t >> 5) + 8 * i; } else { r = t & 63; c = (t >> 6) + 4 * i; }
        } else {               // 32 rows x 64 columns
            if (FAST_C) { c = t & 63; r = (t >> 6) + 4 * i; } else { r = t & 31; c = (t >> 5) + 8 * i; }
        }
        const int gr = r0 + r, gc = c0 + c;
        v[i] = (gr < R && gc < C1) ? f(gr, gc) : 0.0f;
    }
}
template <bool FAST_C>
__device__ __forceinline__ void tile_put(float (*S)[TM + 1], const float (&v)[8], bool rows_are_k) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int r, c;
        if (!rows_are_k) {
            if (FAST_C) { c = t & 31; r = (t >> 5) + 8 * i; } else { r = t & 63; c = (t >> 6) + 4 * i; }
            S[c][r] = v[i];      // [k][m]
        } else {
            if (FAST_C) { c = t & 63; r = (t >> 6) + 4 * i; } else { r = t & 31; c = (t >> 5) + 8 * i; }
            S[r][c] = v[i];      // [k][n]
        }
    }
}

template <class AF, class BF, class EP>
__global__ __launch_bounds__(WG) void gemm_kernel(AF A, BF Bm, EP ep, int M, int N, int K, int kchunk, float* __restrict__ part) {
    __shared__ float As[TK][TM + 1];
    __shared__ float Bs[TK][TN + 1];
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
    const int kbeg = blockIdx.z * kchunk, kend = min(K, kbeg + kchunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int l32 = lane & 31, half = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    float ra[8], rb[8];
    tile_fetch<AF, AF::FAST_C>(A, m0, M, kbeg, kend, ra, false);
    tile_fetch<BF, BF::FAST_C>(Bm, kbeg, kend, n0, N, rb, true);
    for (int k0 = kbeg; k0 < kend; k0 += TK) {
        __syncthreads();
        tile_put<AF::FAST_C>(As, ra, false);
        tile_put<BF::FAST_C>(Bs, rb, true);
        __syncthreads();
        if (k0 + TK < kend) {
            tile_fetch<AF, AF::FAST_C>(A, m0, M, k0 + TK, kend, ra, false);
            tile_fetch<BF, BF::FAST_C>(Bm, k0 + TK, kend, n0, N, rb, true);
        }
#pragma unroll
        for (int kk = 0; kk < TK; kk += 2) {
            const float a = As[kk + half][wm + l32], b = Bs[kk + half][wn + l32];
            // the MFMA puts its second operand's index on the lane: m when the store wants m adjacent, else n
            if (EP::M_FAST) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b, a, acc, 0, 0, 0);
            else acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    const bool split = gridDim.z > 1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * half;      // index of the first operand, l32 that of the second
        const int m = m0 + wm + (EP::M_FAST ? l32 : i), n = n0 + wn + (EP::M_FAST ? i : l32);
        if (m < M && n < N) {
            if (split) part[((long)blockIdx.z * M + m) * N + n] = acc[r];
            else ep(m, n, acc[r]);
        }
    }
}

template <class EP>
__global__ __launch_bounds__(WG) void gemm_merge_kernel(const float* __restrict__ part, EP ep, int M, int N, int S) {
    const long MN = (long)M * N, idx = (long)blockIdx.x * WG + threadIdx.x;
    if (idx >= MN) return;
    // m adjacent in the output: walk m with the lane
    const int m = EP::M_FAST ? (int)(idx % M) : (int)(idx / N), n = EP::M_FAST ? (int)(idx / M) : (int)(idx % N);
    const long e = (long)m * N + n;
    float v = part[e];
    for (int s = 1; s < S; ++s) v += part[s * MN + e];
    ep(m, n, v);
}

// the split of a contraction depends on the shape alone: problems with few tiles are cut into up to GPH_MAX_SPLIT chunks of k
void gemm_split(long M, long N, long K, int& S, int& kchunk) {
    S = 1;
    kchunk = TK;
    if (M <= 0 || N <= 0 || K <= 0) return;      // not a GEMM: the callers refuse it, the size queries answer 0
    const long tiles = (long)cdiv(M, TM) * cdiv(N, TN);
    long s = 1;
    if (tiles < 256) s = 512 / tiles < GPH_MAX_SPLIT ? 512 / tiles : GPH_MAX_SPLIT;
    kchunk = cdiv(cdiv(K, s), TK) * TK;
    S = cdiv(K, kchunk);
}
long gemm_ws_floats(long M, long N, long K) {
    int S, kc;
    gemm_split(M, N, K, S, kc);
    return S > 1 ? (long)S * M * N : 0;
}
long up64(long n) { return (n + 63) / 64 * 64; }

#define GPH_CHECK(name)                                                                                   \
    do {                                                                                                  \
        hipError_t e__ = hipGetLastError();                                                               \
        if (e__ != hipSuccess) return gp_fail(GP_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e__));     \
    } while (0)
#define GPH_TRY(call)            \
    do {                         \
        int rc__ = (call);       \
        if (rc__ != 0) return rc__; \
    } while (0)

template <class AF, class BF, class EP>
int gemm(const AF& A, const BF& Bm, const EP& ep, long M, long N, long K, float* ws, long ws_floats, hipStream_t s, const char* name) {
    GP_REQUIRE(M > 0 && N > 0 && K > 0 && M < (1L << 30) && cdiv(N, TN) <= 65535, "%s: bad GEMM shape %ld x %ld x %ld", name, M, N, K);
    int S, kchunk;
    gemm_split(M, N, K, S, kchunk);
    GP_REQUIRE(S == 1 || (ws && ws_floats >= (long)S * M * N), "%s: workspace too small (%ld floats, %ld needed)", name, ws_floats,
               (long)S * M * N);
    hipLaunchKernelGGL((gemm_kernel<AF, BF, EP>), dim3(cdiv(M, TM), cdiv(N, TN), S), dim3(WG), 0, s, A, Bm, ep, (int)M, (int)N, (int)K,
                       kchunk, ws);
    GPH_CHECK(name);
    if (S > 1) {
        hipLaunchKernelGGL((gemm_merge_kernel<EP>), dim3(cdiv(M * N, WG)), dim3(WG), 0, s, (const float*)ws, ep, (int)M, (int)N, S);
        GPH_CHECK(name);
    }
    return 0;
}

}  // namespace

#endif
