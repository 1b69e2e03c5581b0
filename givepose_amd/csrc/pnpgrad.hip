// Pose-head backward family (include/givepose_headgrad.h, prefix gph_): ConvPnPNet forward-that-saves and its backward in fp32.
//
// One LDS-tiled GEMM kernel on v_mfma_f32_32x32x2_f32 serves every long contraction.  Its operands are functors that map
// (row, column) of a logical matrix to an address -- a plain matrix, an NCHW tensor read as (pixels, channels), the im2col
// view of a conv input, the gathered view of a conv output gradient -- so no operand is ever materialised.  An element
// outside the tensor (padding, a tap without an output pixel, the ragged edge of a tile) is an exact 0, and fma(0, b, acc)
// leaves acc unchanged, so each result is the fmaf chain over the terms that exist, in the order of k.
#include "common.hpp"
#include "../../include/givepose_headgrad.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TM = 64, TN = 64, TK = 32, WG = 256;
constexpr int FEAT = GPH_FEAT, RES = GPH_RES;

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

// ---------------------------------------------------------------------------------- linear layers
// g = dY o gate (slope 0.1 where the saved output is <= 0), and db = sum over the rows in order
__global__ __launch_bounds__(WG) void linear_gate_kernel(const float* __restrict__ dY, int lddy, const float* __restrict__ Y, int ldy,
                                                         int M, int N, float* __restrict__ g, float* __restrict__ db) {
    const int n = blockIdx.x * WG + threadIdx.x;
    if (n >= N) return;
    float s = 0.0f;
    for (int b = 0; b < M; ++b) {
        float v = dY[(long)b * lddy + n];
        if (Y) v = Y[(long)b * ldy + n] > 0.0f ? v : 0.1f * v;
        g[(long)b * N + n] = v;
        s += v;
    }
    if (db) db[n] = s;
}

// dW[n][k] = sum_b g[b][n] X[b][k]: the contraction has the length of the batch, so this is a stream of outer products bounded
// by its store.  A thread owns one k and eight rows n: X is read once per eight rows (from L2), g through the scalar unit.
constexpr int DW_ROWS = 8;
__global__ __launch_bounds__(WG) void linear_dw_kernel(const float* __restrict__ g, const float* __restrict__ X, int ldx, int M, int N,
                                                       int K, float* __restrict__ dW) {
    const int k = blockIdx.x * WG + threadIdx.x, n0 = blockIdx.y * DW_ROWS;
    if (k >= K) return;
    float acc[DW_ROWS];
#pragma unroll
    for (int j = 0; j < DW_ROWS; ++j) acc[j] = 0.0f;
    for (int b = 0; b < M; ++b) {
        const float x = X[(long)b * ldx + k];
#pragma unroll
        for (int j = 0; j < DW_ROWS; ++j)
            if (n0 + j < N) acc[j] = fmaf(g[(long)b * N + n0 + j], x, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < DW_ROWS; ++j)
        if (n0 + j < N) dW[(long)(n0 + j) * K + k] = acc[j];
}

long linear_bwd_ws_floats(long M, long N, long K) { return up64(M * N) + gemm_ws_floats(M, K, N); }

int linear_backward(const float* dY, int lddy, const float* Y, int ldy, const float* W, const float* X, int ldx, int M, int N, int K,
                    int accumulate, float* dX, int lddx, float* dW, float* db, float* ws, long ws_floats, hipStream_t s) {
    GP_REQUIRE(dY && M > 0 && N > 0 && K > 0 && lddy >= N && (!Y || ldy >= N), "gph_linear_backward: bad arguments (M %d N %d K %d)", M, N, K);
    GP_REQUIRE((!dX || (W && lddx >= K)) && (!dW || (X && ldx >= K)), "gph_linear_backward: dX needs W, dW needs X");
    GP_REQUIRE(ws && ws_floats >= linear_bwd_ws_floats(M, N, K), "gph_linear_backward: workspace too small");
    float* g = ws;
    hipLaunchKernelGGL(linear_gate_kernel, dim3(cdiv(N, WG)), dim3(WG), 0, s, dY, lddy, Y, ldy, M, N, g, db);
    GPH_CHECK("gph_linear_backward");
    if (dW) {
        hipLaunchKernelGGL(linear_dw_kernel, dim3(cdiv(K, WG), cdiv(N, DW_ROWS)), dim3(WG), 0, s, (const float*)g, X, ldx, M, N, K, dW);
        GPH_CHECK("gph_linear_backward");
    }
    if (dX)      // (M x N) (N x K): W's rows are the k of the contraction
        GPH_TRY(gemm(MatRow{g, N}, MatRow{W, K}, EpRow{dX, lddx, nullptr, 0, accumulate}, M, K, N, ws + up64((long)M * N),
                     ws_floats - up64((long)M * N), s, "gph_linear_backward"));
    return 0;
}

int linear_forward(const float* X, int ldx, const float* W, const float* bias, int M, int N, int K, int lrelu, float* Yo, int ldy,
                   float* ws, long ws_floats, hipStream_t s) {
    return gemm(MatRow{X, ldx}, MatCol{W, K}, EpRow{Yo, ldy, bias, lrelu, 0}, M, N, K, ws, ws_floats, s, "gph_pnp_forward_save");
}

// ---------------------------------------------------------------------------------- GroupNorm (groups of 4 channels) + ReLU
// One workgroup per (crop, group), wave w owns channel 4 g + w: HW adjacent floats.  Sums: each lane its elements in turn, the
// xor tree of group_sum over the wave, the four waves as (w0 + w1) + (w2 + w3).
__device__ __forceinline__ float four_waves(float* sh, float v, int wave, int lane) {
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(WG) void gn_relu_forward_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int C, int HW, float* __restrict__ out,
                                                             float* __restrict__ mean, float* __restrict__ rstd) {
    __shared__ float sh[4];
    const int G = C >> 2, b = blockIdx.x / G, g = blockIdx.x - b * G, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = 4 * g + wave;
    const long base = ((long)b * C + c) * HW;
    const float inv_n = 1.0f / (float)(4 * HW);
    float s = 0.0f;
    for (int i = lane; i < HW; i += 64) s += x[base + i];
    const float mu = four_waves(sh, group_sum(s, 64), wave, lane) * inv_n;
    float q = 0.0f;
    for (int i = lane; i < HW; i += 64) {
        const float d = x[base + i] - mu;
        q = fmaf(d, d, q);
    }
    const float var = four_waves(sh, group_sum(q, 64), wave, lane) * inv_n;
    const float rs = 1.0f / sqrtf(var + 1e-5f);
    if (threadIdx.x == 0) {
        mean[blockIdx.x] = mu;
        rstd[blockIdx.x] = rs;
    }
    const float ga = gamma[c], be = beta[c];
    for (int i = lane; i < HW; i += 64) out[base + i] = fmaxf(fmaf((x[base + i] - mu) * rs, ga, be), 0.0f);
}

__global__ __launch_bounds__(WG) void gn_relu_backward_kernel(const float* dout, const float* __restrict__ out,
                                                              const float* __restrict__ x, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, const float* __restrict__ gamma, int C,
                                                              int HW, float* dx, float* __restrict__ pgamma, float* __restrict__ pbeta) {
    __shared__ float sh[4];
    const int G = C >> 2, b = blockIdx.x / G, g = blockIdx.x - b * G, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = 4 * g + wave;
    const long base = ((long)b * C + c) * HW;
    const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x], ga = gamma[c];
    float sdy = 0.0f, sdx = 0.0f;
    for (int i = lane; i < HW; i += 64) {
        const float dy = out[base + i] > 0.0f ? dout[base + i] : 0.0f;
        const float xh = (x[base + i] - mu) * rs;
        sdy += dy;
        sdx = fmaf(dy, xh, sdx);
    }
    sdy = group_sum(sdy, 64);
    sdx = group_sum(sdx, 64);
    if (lane == 0) {
        pbeta[(long)b * C + c] = sdy;
        pgamma[(long)b * C + c] = sdx;
    }
    const float inv_n = 1.0f / (float)(4 * HW);
    const float m1 = four_waves(sh, ga * sdy, wave, lane) * inv_n;      // mean of dxhat over the group
    const float m2 = four_waves(sh, ga * sdx, wave, lane) * inv_n;      // mean of dxhat xhat
    for (int i = lane; i < HW; i += 64) {
        const float dy = out[base + i] > 0.0f ? dout[base + i] : 0.0f;
        const float xh = (x[base + i] - mu) * rs;
        dx[base + i] = rs * ((dy * ga - m1) - xh * m2);
    }
}

__global__ __launch_bounds__(WG) void gn_param_reduce_kernel(const float* __restrict__ pgamma, const float* __restrict__ pbeta, int B,
                                                             int C, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * WG + threadIdx.x;
    if (c >= C) return;
    float sg = 0.0f, sb = 0.0f;
    for (int b = 0; b < B; ++b) {
        sg += pgamma[(long)b * C + c];
        sb += pbeta[(long)b * C + c];
    }
    if (dgamma) dgamma[c] = sg;
    if (dbeta) dbeta[c] = sb;
}

long gn_bwd_ws_floats(long B, long C) { return 2 * up64(B * C); }

int gn_relu_backward(const float* dout, const float* out, const float* x, const float* mean, const float* rstd, const float* gamma, int B,
                     int C, int HW, float* dx, float* dgamma, float* dbeta, float* ws, long ws_floats, hipStream_t s) {
    GP_REQUIRE(dout && out && x && mean && rstd && gamma && dx, "gph_gn_relu_backward: null pointer");
    GP_REQUIRE(B > 0 && C > 0 && (C & 3) == 0 && HW > 0 && (long)B * (C >> 2) < (1L << 30), "gph_gn_relu_backward: bad shape B %d C %d HW %d", B,
               C, HW);
    GP_REQUIRE(ws && ws_floats >= gn_bwd_ws_floats(B, C), "gph_gn_relu_backward: workspace too small");
    float *pg = ws, *pb = ws + up64((long)B * C);
    hipLaunchKernelGGL(gn_relu_backward_kernel, dim3(B * (C >> 2)), dim3(WG), 0, s, dout, out, x, mean, rstd, gamma, C, HW, dx, pg, pb);
    GPH_CHECK("gph_gn_relu_backward");
    hipLaunchKernelGGL(gn_param_reduce_kernel, dim3(cdiv(C, WG)), dim3(WG), 0, s, (const float*)pg, (const float*)pb, B, C, dgamma, dbeta);
    GPH_CHECK("gph_gn_relu_backward");
    return 0;
}

// ---------------------------------------------------------------------------------- 3x3 stride-2 pad-1 conv
long conv_bwd_ws_floats(long B, long Cin, long Cout, long H, long cin_dx) {
    const long Ho = H / 2, a = gemm_ws_floats(Cout, Cin * 9, B * Ho * Ho), d = cin_dx > 0 ? gemm_ws_floats(B * H * H, cin_dx, Cout * 9) : 0;
    return a > d ? a : d;
}

int conv_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Yo, float* ws, long ws_floats, hipStream_t s) {
    const int Ho = H / 2;
    return gemm(Im2col{X, Cin, H, Ho}, MatCol{Wt, (long)Cin * 9}, EpNchw{Yo, Cout, Ho * Ho, nullptr}, (long)B * Ho * Ho, Cout, (long)Cin * 9, ws,
                ws_floats, s, "gph_pnp_forward_save");
}

int conv_backward(const float* dY, const float* X, const float* Wt, const float* mask, int B, int Cin, int Cout, int H, int cin_dx,
                  float* dX, float* dW, float* ws, long ws_floats, hipStream_t s) {
    GP_REQUIRE(dY && B > 0 && Cin > 0 && Cout > 0 && H > 0 && (H & 1) == 0 && cin_dx >= 0 && cin_dx <= Cin && (long)B * H * H < (1L << 30),
               "gph_conv3x3s2_backward: bad shape B %d Cin %d Cout %d H %d cin_dx %d", B, Cin, Cout, H, cin_dx);
    GP_REQUIRE((!dW || X) && (!dX || (Wt && cin_dx > 0)), "gph_conv3x3s2_backward: dW needs X, dX needs the weights and cin_dx > 0");
    const int Ho = H / 2;
    if (dW)      // (Cout x m) (m x Cin 9), m = (b,oh,ow)
        GPH_TRY(gemm(Tr<Nchw>{Nchw{dY, Cout, Ho * Ho}}, Im2col{X, Cin, H, Ho}, EpRow{dW, (long)Cin * 9, nullptr, 0, 0}, Cout, (long)Cin * 9,
                     (long)B * Ho * Ho, ws, ws_floats, s, "gph_conv3x3s2_backward"));
    if (dX)      // ((b,ih,iw) x (co,kh,kw)) ((co,kh,kw) x ci)
        GPH_TRY(gemm(GatherDY{dY, Cout, H, Ho}, WeightDx{Wt, Cin}, EpNchw{dX, cin_dx, H * H, mask}, (long)B * H * H, cin_dx, (long)Cout * 9, ws,
                     ws_floats, s, "gph_conv3x3s2_backward"));
    return 0;
}

// ---------------------------------------------------------------------------------- the head
__global__ __launch_bounds__(WG) void pnp_input_kernel(const float* __restrict__ ivfc, const float* __restrict__ coord,
                                                       const float* __restrict__ mask, long total, float* __restrict__ x0) {
    const long idx = (long)blockIdx.x * WG + threadIdx.x;
    if (idx >= total) return;
    const int NP = RES * RES;
    const int px = (int)(idx % NP), c = (int)(idx / NP % 5);
    const long b = idx / (5 * NP);
    float v = c < 3 ? ivfc[(b * 3 + c) * NP + px] : coord[(b * 2 + (c - 3)) * NP + px];
    if (mask) v *= mask[b * NP + px];
    x0[idx] = v;
}

bool params_complete(const gph_pnp_params* p) {
    if (!p) return false;
    for (int i = 0; i < 3; ++i)
        if (!p->conv_w[i] || !p->gn_w[i] || !p->gn_b[i]) return false;
    return p->fc1_w && p->fc1_b && p->fc1z_w && p->fc1z_b && p->fc2_w && p->fc2_b && p->fc2z_w && p->fc2z_b && p->fcr_w && p->fcr_b &&
           p->fct_w && p->fct_b && p->fcz_w && p->fcz_b;
}
bool saved_complete(const gph_pnp_saved* v) {
    if (!v || !v->x0 || !v->h1 || !v->h2 || !v->h2z || !v->pred_rot || !v->pred_t) return false;
    for (int i = 0; i < 3; ++i)
        if (!v->conv[i] || !v->mean[i] || !v->rstd[i] || !v->act[i]) return false;
    return true;
}

long max2(long a, long b) { return a > b ? a : b; }

long pnp_fwd_ws_floats(long B, long rot_dim) {
    long w = 0;
    for (int li = 0; li < 3; ++li) {
        const long Ho = RES >> (li + 1);
        w = max2(w, gemm_ws_floats(B * Ho * Ho, FEAT, (li ? FEAT : 5) * 9));
    }
    w = max2(w, gemm_ws_floats(B, 1024, 8192));
    w = max2(w, gemm_ws_floats(B, 256, 1024));
    w = max2(w, gemm_ws_floats(B, rot_dim, 256));
    w = max2(w, gemm_ws_floats(B, 2, 256));
    w = max2(w, gemm_ws_floats(B, 1, 256));
    return up64(w);
}

// offsets (floats) of the backward's own buffers inside its workspace
struct BwdLayout {
    long dh2, dh2z, dh1, da[3], dc[3], scratch, scratch_floats, total;
};
BwdLayout bwd_layout(long B, long rot_dim) {
    BwdLayout L;
    long o = 0;
    auto take = [&](long n) { long at = o; o += up64(n); return at; };
    L.dh2 = take(B * 256);
    L.dh2z = take(B * 256);
    L.dh1 = take(B * 2048);
    for (int li = 0; li < 3; ++li) {
        const long Ho = RES >> (li + 1);
        L.da[li] = take(B * FEAT * Ho * Ho);
        L.dc[li] = take(B * FEAT * Ho * Ho);
    }
    long w = max2(linear_bwd_ws_floats(B, rot_dim, 256), max2(linear_bwd_ws_floats(B, 2, 256), linear_bwd_ws_floats(B, 1, 256)));
    w = max2(w, max2(linear_bwd_ws_floats(B, 256, 1024), linear_bwd_ws_floats(B, 1024, 8192)));
    w = max2(w, gn_bwd_ws_floats(B, FEAT));
    w = max2(w, max2(conv_bwd_ws_floats(B, FEAT, FEAT, 16, FEAT), conv_bwd_ws_floats(B, FEAT, FEAT, 32, FEAT)));
    w = max2(w, conv_bwd_ws_floats(B, 5, FEAT, RES, 3));
    L.scratch = o;
    L.scratch_floats = up64(w);
    L.total = o + L.scratch_floats;
    return L;
}

bool aligned256(const void* p) { return ((uintptr_t)p & 255) == 0; }

}  // namespace

extern "C" {

long long gph_linear_backward_workspace(int M, int N, int K) {
    return M > 0 && N > 0 && K > 0 ? 4LL * linear_bwd_ws_floats(M, N, K) : 0;
}

int gph_linear_backward(const float* dY, int lddy, const float* Y, int ldy, const float* W, const float* X, int ldx, int M, int N, int K,
                        int accumulate, float* dX, int lddx, float* dW, float* db, void* ws, long long ws_bytes, void* stream) {
    GP_REQUIRE(!ws || aligned256(ws), "gph_linear_backward: the workspace is not 256-byte aligned");
    return linear_backward(dY, lddy, Y, ldy, W, X, ldx, M, N, K, accumulate, dX, lddx, dW, db, (float*)ws, (long)(ws_bytes / 4),
                           (hipStream_t)stream);
}

long long gph_gn_relu_backward_workspace(int B, int C) { return B > 0 && C > 0 ? 4LL * gn_bwd_ws_floats(B, C) : 0; }

int gph_gn_relu_backward(const float* dout, const float* out, const float* x, const float* mean, const float* rstd, const float* gamma,
                         int B, int C, int HW, float* dx, float* dgamma, float* dbeta, void* ws, long long ws_bytes, void* stream) {
    GP_REQUIRE(!ws || aligned256(ws), "gph_gn_relu_backward: the workspace is not 256-byte aligned");
    return gn_relu_backward(dout, out, x, mean, rstd, gamma, B, C, HW, dx, dgamma, dbeta, (float*)ws, (long)(ws_bytes / 4),
                            (hipStream_t)stream);
}

long long gph_conv3x3s2_backward_workspace(int B, int Cin, int Cout, int H, int cin_dx) {
    const bool ok = B > 0 && Cin > 0 && Cout > 0 && H >= 2 && !(H & 1) && cin_dx >= 0 && cin_dx <= Cin;      // what the entry point accepts
    return ok ? 4LL * up64(conv_bwd_ws_floats(B, Cin, Cout, H, cin_dx)) : 0;
}

int gph_conv3x3s2_backward(const float* dY, const float* X, const float* Wt, const float* mask, int B, int Cin, int Cout, int H,
                           int cin_dx, float* dX, float* dW, void* ws, long long ws_bytes, void* stream) {
    GP_REQUIRE(!ws || aligned256(ws), "gph_conv3x3s2_backward: the workspace is not 256-byte aligned");
    return conv_backward(dY, X, Wt, mask, B, Cin, Cout, H, cin_dx, dX, dW, (float*)ws, (long)(ws_bytes / 4), (hipStream_t)stream);
}

long long gph_pnp_forward_workspace(int B, int rot_dim) { return B > 0 && rot_dim > 0 ? 4LL * pnp_fwd_ws_floats(B, rot_dim) : 0; }

int gph_pnp_forward_save(const float* ivfc, const float* roi_coord_2d, const float* mask, const gph_pnp_params* w, int B, int rot_dim,
                         const gph_pnp_saved* sv, void* ws, long long ws_bytes, void* stream) {
    GP_REQUIRE(ivfc && roi_coord_2d && params_complete(w) && saved_complete(sv), "gph_pnp_forward_save: null pointer");
    GP_REQUIRE(B > 0 && B <= 4096 && rot_dim > 0 && rot_dim <= 64, "gph_pnp_forward_save: bad shape B %d rot_dim %d", B, rot_dim);
    GP_REQUIRE(!ws || aligned256(ws), "gph_pnp_forward_save: the workspace is not 256-byte aligned");
    GP_REQUIRE(ws_bytes / 4 >= pnp_fwd_ws_floats(B, rot_dim) && (ws || ws_bytes == 0), "gph_pnp_forward_save: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float* f = (float*)ws;
    const long wf = (long)(ws_bytes / 4);
    const long total = (long)B * 5 * RES * RES;
    hipLaunchKernelGGL(pnp_input_kernel, dim3(cdiv(total, WG)), dim3(WG), 0, s, ivfc, roi_coord_2d, mask, total, sv->x0);
    GPH_CHECK("gph_pnp_forward_save");
    const float* in = sv->x0;
    for (int li = 0; li < 3; ++li) {
        const int H = RES >> li, Ho = H / 2;
        GPH_TRY(conv_forward(in, w->conv_w[li], B, li ? FEAT : 5, FEAT, H, sv->conv[li], f, wf, s));
        hipLaunchKernelGGL(gn_relu_forward_kernel, dim3(B * GPH_GROUPS), dim3(WG), 0, s, (const float*)sv->conv[li], (const float*)w->gn_w[li],
                           (const float*)w->gn_b[li], FEAT, Ho * Ho, sv->act[li], sv->mean[li], sv->rstd[li]);
        GPH_CHECK("gph_pnp_forward_save");
        in = sv->act[li];
    }
    GPH_TRY(linear_forward(sv->act[2], 8192, w->fc1_w, w->fc1_b, B, 1024, 8192, 1, sv->h1, 2048, f, wf, s));
    GPH_TRY(linear_forward(sv->act[2], 8192, w->fc1z_w, w->fc1z_b, B, 1024, 8192, 1, sv->h1 + 1024, 2048, f, wf, s));
    GPH_TRY(linear_forward(sv->h1, 2048, w->fc2_w, w->fc2_b, B, 256, 1024, 1, sv->h2, 256, f, wf, s));
    GPH_TRY(linear_forward(sv->h1 + 1024, 2048, w->fc2z_w, w->fc2z_b, B, 256, 1024, 1, sv->h2z, 256, f, wf, s));
    GPH_TRY(linear_forward(sv->h2, 256, w->fcr_w, w->fcr_b, B, rot_dim, 256, 0, sv->pred_rot, rot_dim, f, wf, s));
    GPH_TRY(linear_forward(sv->h2, 256, w->fct_w, w->fct_b, B, 2, 256, 0, sv->pred_t, 3, f, wf, s));
    GPH_TRY(linear_forward(sv->h2z, 256, w->fcz_w, w->fcz_b, B, 1, 256, 0, sv->pred_t + 2, 3, f, wf, s));
    return 0;
}

long long gph_pnp_backward_workspace(int B, int rot_dim) { return B > 0 && rot_dim > 0 ? 4LL * bwd_layout(B, rot_dim).total : 0; }

int gph_pnp_backward(const gph_pnp_params* w, const gph_pnp_saved* sv, const float* mask, const float* g_pred_rot, const float* g_pred_t,
                     int B, int rot_dim, const gph_pnp_params* gr, float* g_ivfc, void* ws, long long ws_bytes, void* stream) {
    GP_REQUIRE(params_complete(w) && saved_complete(sv) && params_complete(gr) && g_pred_rot && g_pred_t && g_ivfc,
               "gph_pnp_backward: null pointer");
    GP_REQUIRE(B > 0 && B <= 4096 && rot_dim > 0 && rot_dim <= 64, "gph_pnp_backward: bad shape B %d rot_dim %d", B, rot_dim);
    const BwdLayout L = bwd_layout(B, rot_dim);
    GP_REQUIRE(ws && aligned256(ws) && ws_bytes / 4 >= L.total, "gph_pnp_backward: workspace missing, unaligned or too small");
    hipStream_t s = (hipStream_t)stream;
    float* f = (float*)ws;
    float *dh2 = f + L.dh2, *dh2z = f + L.dh2z, *dh1 = f + L.dh1, *sc = f + L.scratch;
    const long sf = L.scratch_floats;
    // the three output layers: pred_rot = fc_r(h2), pred_t = [fc_t(h2) | fc_z(h2z)]
    GPH_TRY(linear_backward(g_pred_rot, rot_dim, nullptr, 0, w->fcr_w, sv->h2, 256, B, rot_dim, 256, 0, dh2, 256, gr->fcr_w, gr->fcr_b, sc, sf, s));
    GPH_TRY(linear_backward(g_pred_t, 3, nullptr, 0, w->fct_w, sv->h2, 256, B, 2, 256, 1, dh2, 256, gr->fct_w, gr->fct_b, sc, sf, s));
    GPH_TRY(linear_backward(g_pred_t + 2, 3, nullptr, 0, w->fcz_w, sv->h2z, 256, B, 1, 256, 0, dh2z, 256, gr->fcz_w, gr->fcz_b, sc, sf, s));
    GPH_TRY(linear_backward(dh2, 256, sv->h2, 256, w->fc2_w, sv->h1, 2048, B, 256, 1024, 0, dh1, 2048, gr->fc2_w, gr->fc2_b, sc, sf, s));
    GPH_TRY(linear_backward(dh2z, 256, sv->h2z, 256, w->fc2z_w, sv->h1 + 1024, 2048, B, 256, 1024, 0, dh1 + 1024, 2048, gr->fc2z_w, gr->fc2z_b,
                            sc, sf, s));
    // fc1 and fc1_z read the same flattened feature: the second adds to the first
    float* da3 = f + L.da[2];
    GPH_TRY(linear_backward(dh1, 2048, sv->h1, 2048, w->fc1_w, sv->act[2], 8192, B, 1024, 8192, 0, da3, 8192, gr->fc1_w, gr->fc1_b, sc, sf, s));
    GPH_TRY(linear_backward(dh1 + 1024, 2048, sv->h1 + 1024, 2048, w->fc1z_w, sv->act[2], 8192, B, 1024, 8192, 1, da3, 8192, gr->fc1z_w,
                            gr->fc1z_b, sc, sf, s));
    for (int li = 2; li >= 0; --li) {
        const int H = RES >> li, Ho = H / 2;
        float* dc = f + L.dc[li];
        GPH_TRY(gn_relu_backward(f + L.da[li], sv->act[li], sv->conv[li], sv->mean[li], sv->rstd[li], w->gn_w[li], B, FEAT, Ho * Ho, dc,
                                 gr->gn_w[li], gr->gn_b[li], sc, sf, s));
        if (li > 0)
            GPH_TRY(conv_backward(dc, sv->act[li - 1], w->conv_w[li], nullptr, B, FEAT, FEAT, H, FEAT, f + L.da[li - 1], gr->conv_w[li], sc, sf, s));
        else      // the first conv: all of dW, dX for the three ivfc channels only, times the mask
            GPH_TRY(conv_backward(dc, sv->x0, w->conv_w[0], mask, B, 5, FEAT, H, 3, g_ivfc, gr->conv_w[0], sc, sf, s));
    }
    return 0;
}

}  // extern "C"
