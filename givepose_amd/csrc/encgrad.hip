// Map-encoder backward family (include/givepose_encgrad.h, prefix gpe_): MAPEncoder's forward-that-saves and its backward in fp32,
// and the 1x1 conv backward with any number of output channels.
//
// Every contraction is a view on the functor GEMM of grad_gemm.hpp: a Linear over rows is MatRow x MatCol, the layer's conv1x1 is
// the same operator with the NCHW map read as rows (Nchw) or written as NCHW (EpNchw), so the layout moves of coor and d coor are
// views, not kernels.  What is not a contraction: the ordered row sums (colsum), the depth-wise 3x3 + LayerNorm + GELU on a flat
// prefix, the DCNv3 core of this geometry (one wavefront per (row, group), a lane per channel) and GroupNorm + ReLU.
//
// d xp of the core is scattered with fp32 atomics here, or left to the ordered sum of encscatter.hip (givepose_encgrad_ordered.h, gpeo_*:
// the gpe_ entry points are the gpeo_ ones at GPE_SCATTER_ATOMIC).
//
// The size queries and the entry points run the same host code: a Scratch in `dry` mode only records what a run would take.
#include "grad_gemm.hpp"
#include "../../include/givepose_encgrad_ordered.h"
#include "encscatter.hpp"

namespace {

constexpr int FEAT = GPE_FEAT, DG = GPE_DCN_GROUPS, DD = GPE_DCN_CHANNELS, TAPS = GPE_TAPS, GNG = GPE_GN_GROUPS, LAYERS = GPE_LAYERS;
constexpr int OFFW = DG * TAPS * 2, MASKW = DG * TAPS;
constexpr int MAXJ = 4;               // channels per lane of the depth-wise / LayerNorm kernels: C <= 64 MAXJ
constexpr int COLSUM_CHUNK = 256;     // rows per workgroup of an ordered row sum
constexpr int DWLN_ROWS = 64;         // rows per workgroup of the LayerNorm backward

struct EpNchwBias {  // rows (b, pixel) -> C (B,Cc,HW), plus bias[n]
    float* C; int Cc, HW; const float* bias;
    static constexpr bool M_FAST = true;
    __device__ __forceinline__ void operator()(int m, int n, float v) const {
        const int b = m / HW, px = m - b * HW;
        C[((long)b * Cc + n) * HW + px] = v + bias[n];
    }
};

long max2(long a, long b) { return a > b ? a : b; }
bool aligned256(const void* p) { return ((uintptr_t)p & 255) == 0; }

// the workspace of a call: take() carves what lives to the end of the call, want() announces what one step needs behind that
struct Scratch {
    float* base; long size; bool dry; long used = 0, need = 0;
    Scratch(void* ws, long long bytes, bool d) : base((float*)ws), size((long)(bytes / 4)), dry(d) {}
    float* take(long n) {
        float* p = base + used;
        used += up64(n);
        need = max2(need, used);
        return p;
    }
    void want(long n) { need = max2(need, used + up64(n)); }
    float* rest() const { return base + used; }
    long rest_floats() const { return size - used; }
};

template <class AF, class BF, class EP>
int gemm_s(const AF& A, const BF& Bm, const EP& ep, long M, long N, long K, Scratch& sc, hipStream_t s, const char* name) {
    sc.want(gemm_ws_floats(M, N, K));
    if (sc.dry) return 0;
    return gemm(A, Bm, ep, M, N, K, sc.rest(), sc.rest_floats(), s, name);
}

// ---------------------------------------------------------------------------------- ordered row sums
// out[c] = sum_r f(r, c).  Workgroup (column tile, row chunk): lane = column, wave w takes the chunk's rows w, w + 4, ... in turn,
// the waves are added as (w0 + w1) + (w2 + w3); the chunks' partial sums are added in order by rows_merge_kernel.
template <class F>
__global__ __launch_bounds__(WG) void colsum_kernel(F f, int rows, int cols, float* __restrict__ part) {
    __shared__ float sh[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * COLSUM_CHUNK, r1 = min(rows, r0 + COLSUM_CHUNK);
    float s = 0.0f;
    if (col < cols)
        for (int r = r0 + wave; r < r1; r += 4) s += f(r, col);
    sh[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && col < cols) part[(long)blockIdx.y * cols + col] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

__global__ __launch_bounds__(WG) void rows_merge_kernel(const float* __restrict__ part, int n, int cols, float* __restrict__ out) {
    const int c = blockIdx.x * WG + threadIdx.x;
    if (c >= cols) return;
    float s = part[c];
    for (int i = 1; i < n; ++i) s += part[(long)i * cols + c];
    out[c] = s;
}

bool colsum_ok(long rows, long cols) { return rows > 0 && cols > 0 && rows < (1L << 23) && cols < (1L << 22); }

template <class F>
int colsum_s(const F& f, long rows, long cols, float* out, Scratch& sc, hipStream_t s, const char* name) {
    const int chunks = cdiv(rows, COLSUM_CHUNK);
    sc.want((long)chunks * cols);
    if (sc.dry) return 0;
    GP_REQUIRE(colsum_ok(rows, cols) && sc.rest_floats() >= (long)chunks * cols, "%s: bad row sum %ld x %ld or workspace too small", name,
               rows, cols);
    hipLaunchKernelGGL((colsum_kernel<F>), dim3(cdiv(cols, 64), chunks), dim3(WG), 0, s, f, (int)rows, (int)cols, sc.rest());
    GPH_CHECK(name);
    hipLaunchKernelGGL(rows_merge_kernel, dim3(cdiv(cols, WG)), dim3(WG), 0, s, (const float*)sc.rest(), chunks, (int)cols, out);
    GPH_CHECK(name);
    return 0;
}

// ---------------------------------------------------------------------------------- Linear over rows
bool linear_ok(long rows, long Cin, long Cout) { return rows > 0 && rows < (1L << 23) && Cin > 0 && Cin <= 65536 && Cout > 0 && Cout <= 65536; }

int linear_forward(const float* X, const float* Wt, const float* b, long rows, int Cin, int Cout, float* Y, Scratch& sc, hipStream_t s,
                   const char* name) {
    return gemm_s(MatRow{X, Cin}, MatCol{Wt, Cin}, EpRow{Y, Cout, b, 0, 0}, rows, Cout, Cin, sc, s, name);
}

// accumulate: dX += (the sum of two branches)
int linear_backward(const float* dY, const float* X, const float* Wt, long rows, int Cin, int Cout, float* dX, int accumulate, float* dW,
                    float* db, Scratch& sc, hipStream_t s, const char* name) {
    if (dX)      // (rows x Cout) (Cout x Cin)
        GPH_TRY(gemm_s(MatRow{dY, Cout}, MatRow{Wt, Cin}, EpRow{dX, Cin, nullptr, 0, accumulate}, rows, Cin, Cout, sc, s, name));
    if (dW)      // (Cout x rows) (rows x Cin)
        GPH_TRY(gemm_s(Tr<MatRow>{MatRow{dY, Cout}}, MatRow{X, Cin}, EpRow{dW, Cin, nullptr, 0, 0}, Cout, Cin, rows, sc, s, name));
    if (db) GPH_TRY(colsum_s(MatRow{dY, Cout}, rows, Cout, db, sc, s, name));
    return 0;
}

// ---------------------------------------------------------------------------------- depth-wise 3x3 + LayerNorm + GELU on a prefix
__device__ __forceinline__ float ln_pre(float xh, float ga, float be) { return fmaf(xh, ga, be); }
__device__ __forceinline__ float gelu_value(float u) { return 0.5f * u * (1.0f + erff(u * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_slope(float u) {      // Phi(u) + u phi(u)
    const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * expf(-0.5f * u * u);
    return fmaf(u, pdf, cdf);
}

// one wavefront per prefix row; lane l owns the channels l, l + 64, ...
__global__ __launch_bounds__(WG) void dwln_forward_kernel(const float* __restrict__ xin, const float* __restrict__ dw_w,
                                                          const float* __restrict__ dw_b, const float* __restrict__ ln_w,
                                                          const float* __restrict__ ln_b, int H, int W, int C, int n_pixels,
                                                          float* __restrict__ dwout, float* __restrict__ mean, float* __restrict__ rstd,
                                                          float* __restrict__ x1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * 4 + wave;
    if (r >= n_pixels) return;      // wave-uniform
    const int hw = H * W, n = (int)(r / hw), px = (int)(r - (long)n * hw), h = px / W, w = px - h * W, nj = C >> 6;
    const float inv_c = 1.0f / (float)C;
    float u[MAXJ], s = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        u[j] = 0.0f;
        if (j < nj) {
            const int c = lane + 64 * j;
            float a = dw_b[c];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int y = h - 1 + t / 3, x = w - 1 + t % 3;
                if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) a = fmaf(xin[(((long)n * H + y) * W + x) * C + c], dw_w[c * 9 + t], a);
            }
            u[j] = a;
            s += a;
        }
    }
    const float mu = group_sum(s, 64) * inv_c;
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
        if (j < nj) {
            const float d = u[j] - mu;
            q = fmaf(d, d, q);
        }
    const float rs = 1.0f / sqrtf(group_sum(q, 64) * inv_c + 1e-6f);
    if (lane == 0) {
        mean[r] = mu;
        rstd[r] = rs;
    }
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
        if (j < nj) {
            const int c = lane + 64 * j;
            dwout[r * C + c] = u[j];
            x1[r * C + c] = gelu_value(ln_pre((u[j] - mu) * rs, ln_w[c], ln_b[c]));
        }
}

// Workgroup = DWLN_ROWS prefix rows, wave w its rows w, w + 4, ... in turn: du = d dwout (three-term LayerNorm backward of
// dy = d x1 GELU'(pre)), and this workgroup's part of d ln_w = sum dy xhat and d ln_b = sum dy, the waves added as (w0 + w1) + (w2 + w3).
__global__ __launch_bounds__(WG) void dwln_backward_rows_kernel(const float* __restrict__ dx1, const float* __restrict__ dwout,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ ln_w, const float* __restrict__ ln_b, int C,
                                                                int n_pixels, float* __restrict__ du, float* __restrict__ pg,
                                                                float* __restrict__ pb) {
    __shared__ float sh[4][2][64 * MAXJ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nj = C >> 6;
    const float inv_c = 1.0f / (float)C;
    float ga[MAXJ], be[MAXJ], ag[MAXJ], ab[MAXJ];
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        ga[j] = j < nj ? ln_w[lane + 64 * j] : 0.0f;
        be[j] = j < nj ? ln_b[lane + 64 * j] : 0.0f;
        ag[j] = ab[j] = 0.0f;
    }
    const long r0 = (long)blockIdx.x * DWLN_ROWS, r1 = min((long)n_pixels, r0 + DWLN_ROWS);
    for (long r = r0 + wave; r < r1; r += 4) {
        const float mu = mean[r], rs = rstd[r];
        float xh[MAXJ], dxh[MAXJ], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            xh[j] = dxh[j] = 0.0f;
            if (j < nj) {
                const long e = r * C + lane + 64 * j;
                xh[j] = (dwout[e] - mu) * rs;
                const float dy = dx1[e] * gelu_slope(ln_pre(xh[j], ga[j], be[j]));
                ag[j] = fmaf(dy, xh[j], ag[j]);
                ab[j] += dy;
                dxh[j] = dy * ga[j];
                s1 += dxh[j];
                s2 = fmaf(dxh[j], xh[j], s2);
            }
        }
        const float m1 = group_sum(s1, 64) * inv_c, m2 = group_sum(s2, 64) * inv_c;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j)
            if (j < nj) du[r * C + lane + 64 * j] = rs * ((dxh[j] - m1) - xh[j] * m2);
    }
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        sh[wave][0][lane + 64 * j] = ag[j];
        sh[wave][1][lane + 64 * j] = ab[j];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += WG) {
        pg[(long)blockIdx.x * C + c] = (sh[0][0][c] + sh[1][0][c]) + (sh[2][0][c] + sh[3][0][c]);
        pb[(long)blockIdx.x * C + c] = (sh[0][1][c] + sh[1][1][c]) + (sh[2][1][c] + sh[3][1][c]);
    }
}

// d xin of pixel (n,y,x): the prefix rows (n, y + 1 - kh, x + 1 - kw) whose window holds it, with the tap's weight
__global__ __launch_bounds__(WG) void dwln_dx_kernel(const float* __restrict__ du, const float* __restrict__ dw_w, long total, int H, int W,
                                                     int C, int n_pixels, float* __restrict__ dxin) {
    const long idx = (long)blockIdx.x * WG + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long pix = idx / C;
    const int hw = H * W, n = (int)(pix / hw), px = (int)(pix - (long)n * hw), h = px / W, w = px - h * W;
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int y = h + 1 - t / 3, x = w + 1 - t % 3;
        if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) continue;
        const long rr = ((long)n * H + y) * W + x;
        if (rr < n_pixels) acc = fmaf(du[rr * C + c], dw_w[c * 9 + t], acc);
    }
    dxin[idx] = acc;
}

struct DwGrad {      // element (prefix row r, (c, tap)) of d dw_w's sum: du[r, c] times the tap's input pixel, an exact 0 in the padding
    const float *du, *xin; int H, W, C;
    __device__ __forceinline__ float operator()(int r, int j) const {
        const int c = j / 9, t = j - c * 9, hw = H * W, n = r / hw, px = r - n * hw, h = px / W, w = px - h * W;
        const int y = h - 1 + t / 3, x = w - 1 + t % 3;
        if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return 0.0f;
        return du[(long)r * C + c] * xin[(((long)n * H + y) * W + x) * C + c];
    }
};

bool dwln_ok(long N, long H, long W, long C, long np) {
    return N > 0 && H > 0 && W > 0 && H <= 4096 && W <= 4096 && C > 0 && C % 64 == 0 && C <= 64 * MAXJ && N * H * W < (1L << 23) && np >= 1 &&
           np <= N * H * W;
}

int dwln_forward(const float* xin, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, int H, int W, int C, int np,
                 float* dwout, float* mean, float* rstd, float* x1, hipStream_t s, const char* name) {
    hipLaunchKernelGGL(dwln_forward_kernel, dim3(cdiv(np, 4)), dim3(WG), 0, s, xin, dw_w, dw_b, ln_w, ln_b, H, W, C, np, dwout, mean, rstd, x1);
    GPH_CHECK(name);
    return 0;
}

int dwln_backward(const float* dx1, const float* xin, const float* dwout, const float* mean, const float* rstd, const float* dw_w,
                  const float* ln_w, const float* ln_b, int N, int H, int W, int C, int np, float* dxin, float* d_dw_w, float* d_dw_b,
                  float* d_ln_w, float* d_ln_b, Scratch& sc, hipStream_t s, const char* name) {
    const long keep = sc.used;
    const int blocks = cdiv(np, DWLN_ROWS);
    float* du = sc.take((long)np * C);
    float* pg = sc.take((long)blocks * C);
    float* pb = sc.take((long)blocks * C);
    if (!sc.dry) {
        hipLaunchKernelGGL(dwln_backward_rows_kernel, dim3(blocks), dim3(WG), 0, s, dx1, dwout, mean, rstd, ln_w, ln_b, C, np, du, pg, pb);
        GPH_CHECK(name);
        hipLaunchKernelGGL(rows_merge_kernel, dim3(cdiv(C, WG)), dim3(WG), 0, s, (const float*)pg, blocks, C, d_ln_w);
        GPH_CHECK(name);
        hipLaunchKernelGGL(rows_merge_kernel, dim3(cdiv(C, WG)), dim3(WG), 0, s, (const float*)pb, blocks, C, d_ln_b);
        GPH_CHECK(name);
        const long total = (long)N * H * W * C;
        hipLaunchKernelGGL(dwln_dx_kernel, dim3(cdiv(total, WG)), dim3(WG), 0, s, (const float*)du, dw_w, total, H, W, C, np, dxin);
        GPH_CHECK(name);
    }
    GPH_TRY(colsum_s(DwGrad{du, xin, H, W, C}, np, (long)C * 9, d_dw_w, sc, s, name));
    GPH_TRY(colsum_s(MatRow{du, C}, np, C, d_dw_b, sc, s, name));
    sc.used = keep;
    return 0;
}

// ---------------------------------------------------------------------------------- the DCNv3 core: 3x3, stride 2, pad 1, G 4, D 64
// dcnv3_im2col_cuda.cuh:216-282 / :386-487 at this geometry, in the arithmetic of csrc/dcnv3_any.hip: tap q = 3 i + j (i along w,
// the outer loop), location w = (2 wo - 1) + (i + offset[2 q]), h = (2 ho - 1) + (j + offset[2 q + 1]).
struct Tap {
    bool valid, o1, o2, o3, o4;
    float lh, lw, hh, hw;
    long a1;
};
__device__ __forceinline__ Tap tap_of(float w, float h, int H, int W) {
    Tap t;
    t.valid = h > -1.0f && w > -1.0f && h < (float)H && w < (float)W;
    const int h_low = (int)floorf(h), w_low = (int)floorf(w);
    t.lh = h - (float)h_low;
    t.lw = w - (float)w_low;
    t.hh = 1.0f - t.lh;
    t.hw = 1.0f - t.lw;
    const bool top = h_low >= 0, bot = h_low + 1 <= H - 1, lef = w_low >= 0, rig = w_low + 1 <= W - 1;
    t.o1 = t.valid && top && lef;
    t.o2 = t.valid && top && rig;
    t.o3 = t.valid && bot && lef;
    t.o4 = t.valid && bot && rig;
    t.a1 = t.valid ? ((long)h_low * W + w_low) * FEAT : 0;
    return t;
}

__global__ __launch_bounds__(WG) void core_forward_kernel(const float* __restrict__ xp, const float* __restrict__ offset,
                                                          const float* __restrict__ logits, int H, int W, int Ho, int Wo, long rows,
                                                          float* __restrict__ mask, float* __restrict__ y) {
    const long wid = ((long)blockIdx.x * WG + threadIdx.x) >> 6;      // (row, group)
    const int lane = threadIdx.x & 63;
    if (wid >= rows * DG) return;      // wave-uniform
    const int g = (int)(wid % DG);
    const long row = wid / DG;
    const int wo = (int)(row % Wo), ho = (int)(row / Wo % Ho), b = (int)(row / ((long)Wo * Ho));
    const float* off = offset + wid * (TAPS * 2);
    const float* lg = logits + wid * TAPS;
    float m[TAPS], mx = lg[0];
#pragma unroll
    for (int q = 1; q < TAPS; ++q) mx = fmaxf(mx, lg[q]);
    float sum = 0.0f;
#pragma unroll
    for (int q = 0; q < TAPS; ++q) {
        m[q] = expf(lg[q] - mx);
        sum += m[q];
    }
#pragma unroll
    for (int q = 0; q < TAPS; ++q) m[q] = m[q] / sum;
    if (lane < TAPS) {
        float v = m[0];
#pragma unroll
        for (int q = 1; q < TAPS; ++q) v = lane == q ? m[q] : v;
        mask[wid * TAPS + lane] = v;
    }
    const float* im = xp + (long)b * H * W * FEAT + g * DD + lane;
    const long ws_ = FEAT, hs_ = (long)W * FEAT;
    float acc = 0.0f;
#pragma unroll
    for (int q = 0; q < TAPS; ++q) {
        const float w = (float)(2 * wo - 1) + ((float)(q / 3) + off[2 * q]);
        const float h = (float)(2 * ho - 1) + ((float)(q % 3) + off[2 * q + 1]);
        const Tap t = tap_of(w, h, H, W);
        const float v1 = t.o1 ? im[t.a1] : 0.0f, v2 = t.o2 ? im[t.a1 + ws_] : 0.0f;
        const float v3 = t.o3 ? im[t.a1 + hs_] : 0.0f, v4 = t.o4 ? im[t.a1 + hs_ + ws_] : 0.0f;
        acc += (t.hh * t.hw * v1 + t.hh * t.lw * v2 + t.lh * t.hw * v3 + t.lh * t.lw * v4) * m[q];
    }
    y[wid * DD + lane] = acc;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// SCATTER false (GPE_SCATTER_ORDERED): d xp is left to encscatter.hip, everything else is the same code
template <bool SCATTER>
__global__ __launch_bounds__(WG) void core_backward_kernel(const float* __restrict__ xp, const float* __restrict__ offset,
                                                           const float* __restrict__ mask, const float* __restrict__ dy, int H, int W,
                                                           int Ho, int Wo, long rows, float* dxp, float* __restrict__ doffset,
                                                           float* __restrict__ dlogits) {
    const long wid = ((long)blockIdx.x * WG + threadIdx.x) >> 6;      // (row, group)
    const int lane = threadIdx.x & 63;
    if (wid >= rows * DG) return;      // wave-uniform
    const int g = (int)(wid % DG);
    const long row = wid / DG;
    const int wo = (int)(row % Wo), ho = (int)(row / Wo % Ho), b = (int)(row / ((long)Wo * Ho));
    const float* off = offset + wid * (TAPS * 2);
    const float* mk = mask + wid * TAPS;
    const long img = (long)b * H * W * FEAT + g * DD + lane;
    const float* im = xp + img;
    float* gim = dxp + img;
    const long ws_ = FEAT, hs_ = (long)W * FEAT;
    const float top_grad = dy[wid * DD + lane];
    float gm[TAPS], mq[TAPS], dot = 0.0f;
#pragma unroll
    for (int q = 0; q < TAPS; ++q) {
        const float w = (float)(2 * wo - 1) + ((float)(q / 3) + off[2 * q]);
        const float h = (float)(2 * ho - 1) + ((float)(q % 3) + off[2 * q + 1]);
        const Tap t = tap_of(w, h, H, W);      // wave-uniform
        mq[q] = mk[q];
        const float tg = top_grad * mq[q];
        const float w1 = t.hh * t.hw, w2 = t.hh * t.lw, w3 = t.lh * t.hw, w4 = t.lh * t.lw;
        float v1 = 0.0f, v2 = 0.0f, v3 = 0.0f, v4 = 0.0f, ghc = 0.0f, gwc = 0.0f;
        if (t.o1) { v1 = im[t.a1]; ghc -= t.hw * v1; gwc -= t.hh * v1; if (SCATTER) atomicAdd(gim + t.a1, w1 * tg); }
        if (t.o2) { v2 = im[t.a1 + ws_]; ghc -= t.lw * v2; gwc += t.hh * v2; if (SCATTER) atomicAdd(gim + t.a1 + ws_, w2 * tg); }
        if (t.o3) { v3 = im[t.a1 + hs_]; ghc += t.hw * v3; gwc -= t.lh * v3; if (SCATTER) atomicAdd(gim + t.a1 + hs_, w3 * tg); }
        if (t.o4) { v4 = im[t.a1 + hs_ + ws_]; ghc += t.lw * v4; gwc += t.lh * v4; if (SCATTER) atomicAdd(gim + t.a1 + hs_ + ws_, w4 * tg); }
        gm[q] = wave_sum(top_grad * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4));
        const float gw = wave_sum(gwc * tg), gh = wave_sum(ghc * tg);
        if (lane == 0) {      // the one writer of this (row, group, tap); zeros for a tap outside the image
            doffset[wid * (TAPS * 2) + 2 * q] = gw;
            doffset[wid * (TAPS * 2) + 2 * q + 1] = gh;
        }
        dot = fmaf(mq[q], gm[q], dot);
    }
    if (lane < TAPS) {      // softmax backward: m (gm - sum m gm)
        float v = mq[0] * (gm[0] - dot);
#pragma unroll
        for (int q = 1; q < TAPS; ++q) v = lane == q ? mq[q] * (gm[q] - dot) : v;
        dlogits[wid * TAPS + lane] = v;
    }
}

bool core_ok(long N, long H, long W) { return N > 0 && H > 0 && W > 0 && H <= 4096 && W <= 4096 && N * H * W < (1L << 23); }

int core_forward(const float* xp, const float* offset, const float* logits, int N, int H, int W, float* mask, float* y, hipStream_t s,
                 const char* name) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long rows = (long)N * Ho * Wo;
    hipLaunchKernelGGL(core_forward_kernel, dim3(cdiv(rows * DG, 4)), dim3(WG), 0, s, xp, offset, logits, H, W, Ho, Wo, rows, mask, y);
    GPH_CHECK(name);
    return 0;
}

bool scatter_ok(int scatter) { return scatter == GPE_SCATTER_ATOMIC || scatter == GPE_SCATTER_ORDERED; }

long index_floats(int scatter, long N, long H, long W) {
    return scatter == GPE_SCATTER_ORDERED ? encscatter::ordered_dxp_ws_floats(N, H, W) : 0;
}

// index: index_floats() words of the caller's scratch (the ordered mode's inverted index), null in the atomic mode
int core_backward(const float* xp, const float* offset, const float* mask, const float* dy, int N, int H, int W, float* dxp, float* doffset,
                  float* dlogits, int scatter, float* index, hipStream_t s, const char* name) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long rows = (long)N * Ho * Wo;
    if (scatter == GPE_SCATTER_ORDERED) {
        hipLaunchKernelGGL(core_backward_kernel<false>, dim3(cdiv(rows * DG, 4)), dim3(WG), 0, s, xp, offset, mask, dy, H, W, Ho, Wo, rows, dxp,
                           doffset, dlogits);
        GPH_CHECK(name);
        return encscatter::ordered_dxp(offset, mask, dy, N, H, W, dxp, index, index_floats(scatter, N, H, W), s, name);
    }
    const hipError_t e = hipMemsetAsync(dxp, 0, (size_t)N * H * W * FEAT * sizeof(float), s);
    if (e != hipSuccess) return gp_fail(GP_ERR_RUNTIME, "%s: hipMemsetAsync: %s", name, hipGetErrorString(e));
    hipLaunchKernelGGL(core_backward_kernel<true>, dim3(cdiv(rows * DG, 4)), dim3(WG), 0, s, xp, offset, mask, dy, H, W, Ho, Wo, rows, dxp, doffset,
                       dlogits);
    GPH_CHECK(name);
    return 0;
}

// ---------------------------------------------------------------------------------- GroupNorm + ReLU
// The kernels of gpx_gn_gelu_* (xyzgrad.hip) with the ReLU gate in the place of the GELU: one workgroup per (crop, group), wave w
// owns the group's channels w, w + 4, ...; sums: each lane its elements in turn, the xor tree, a wave's channels in turn, the four
// waves as (w0 + w1) + (w2 + w3).
__device__ __forceinline__ float four_waves(float* sh, float v, int wave, int lane) {
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ float gn_pre(float x, float mu, float rs, float ga, float be) { return fmaf((x - mu) * rs, ga, be); }

__global__ __launch_bounds__(WG) void gn_relu_forward_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int C, int HW, int G, float* __restrict__ out,
                                                             float* __restrict__ mean, float* __restrict__ rstd) {
    __shared__ float sh[4];
    const int cpg = C / G, b = blockIdx.x / G, g = blockIdx.x - b * G, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long gbase = ((long)b * C + (long)g * cpg) * HW;
    const float inv_n = 1.0f / ((float)cpg * (float)HW);
    float s = 0.0f;
    for (int ch = wave; ch < cpg; ch += 4)
        for (int i = lane; i < HW; i += 64) s += x[gbase + (long)ch * HW + i];
    const float mu = four_waves(sh, group_sum(s, 64), wave, lane) * inv_n;
    float q = 0.0f;
    for (int ch = wave; ch < cpg; ch += 4)
        for (int i = lane; i < HW; i += 64) {
            const float d = x[gbase + (long)ch * HW + i] - mu;
            q = fmaf(d, d, q);
        }
    const float var = four_waves(sh, group_sum(q, 64), wave, lane) * inv_n;
    const float rs = 1.0f / sqrtf(var + 1e-5f);
    if (threadIdx.x == 0) {
        mean[blockIdx.x] = mu;
        rstd[blockIdx.x] = rs;
    }
    for (int ch = wave; ch < cpg; ch += 4) {
        const float ga = gamma[g * cpg + ch], be = beta[g * cpg + ch];
        const long base = gbase + (long)ch * HW;
        for (int i = lane; i < HW; i += 64) out[base + i] = fmaxf(gn_pre(x[base + i], mu, rs, ga, be), 0.0f);
    }
}

__global__ __launch_bounds__(WG) void gn_relu_backward_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, int C, int HW,
                                                              int G, float* dx, float* __restrict__ pgamma, float* __restrict__ pbeta) {
    __shared__ float sh[4];
    const int cpg = C / G, b = blockIdx.x / G, g = blockIdx.x - b * G, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long gbase = ((long)b * C + (long)g * cpg) * HW;
    const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x];
    float a1 = 0.0f, a2 = 0.0f;
    for (int ch = wave; ch < cpg; ch += 4) {
        const int c = g * cpg + ch;
        const float ga = gamma[c], be = beta[c];
        const long base = gbase + (long)ch * HW;
        float sdy = 0.0f, sdx = 0.0f;
        for (int i = lane; i < HW; i += 64) {
            const float xv = x[base + i];
            const float dy = gn_pre(xv, mu, rs, ga, be) > 0.0f ? dout[base + i] : 0.0f;
            dx[base + i] = dy;
            sdy += dy;
            sdx = fmaf(dy, (xv - mu) * rs, sdx);
        }
        sdy = group_sum(sdy, 64);
        sdx = group_sum(sdx, 64);
        if (lane == 0) {
            pbeta[(long)b * C + c] = sdy;
            pgamma[(long)b * C + c] = sdx;
        }
        a1 = fmaf(ga, sdy, a1);
        a2 = fmaf(ga, sdx, a2);
    }
    const float inv_n = 1.0f / ((float)cpg * (float)HW);
    const float m1 = four_waves(sh, a1, wave, lane) * inv_n;
    const float m2 = four_waves(sh, a2, wave, lane) * inv_n;
    for (int ch = wave; ch < cpg; ch += 4) {
        const float ga = gamma[g * cpg + ch];
        const long base = gbase + (long)ch * HW;
        for (int i = lane; i < HW; i += 64) {
            const float xh = (x[base + i] - mu) * rs;
            dx[base + i] = rs * ((dx[base + i] * ga - m1) - xh * m2);
        }
    }
}

bool gn_ok(long B, long C, long HW, long G) {
    return B > 0 && C > 0 && HW > 0 && G > 0 && C % G == 0 && B * G < (1L << 30) && HW < (1L << 28) && C <= 65536;
}

int gn_relu_forward(const float* x, const float* gamma, const float* beta, int B, int C, int HW, int G, float* out, float* mean, float* rstd,
                    hipStream_t s, const char* name) {
    hipLaunchKernelGGL(gn_relu_forward_kernel, dim3(B * G), dim3(WG), 0, s, x, gamma, beta, C, HW, G, out, mean, rstd);
    GPH_CHECK(name);
    return 0;
}

int gn_relu_backward(const float* dout, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int B,
                     int C, int HW, int G, float* dx, float* dgamma, float* dbeta, Scratch& sc, hipStream_t s, const char* name) {
    const long keep = sc.used;
    float* pg = sc.take((long)B * C);
    float* pb = sc.take((long)B * C);
    if (!sc.dry) {
        hipLaunchKernelGGL(gn_relu_backward_kernel, dim3(B * G), dim3(WG), 0, s, dout, x, mean, rstd, gamma, beta, C, HW, G, dx, pg, pb);
        GPH_CHECK(name);
        hipLaunchKernelGGL(rows_merge_kernel, dim3(cdiv(C, WG)), dim3(WG), 0, s, (const float*)pg, B, C, dgamma);
        GPH_CHECK(name);
        hipLaunchKernelGGL(rows_merge_kernel, dim3(cdiv(C, WG)), dim3(WG), 0, s, (const float*)pb, B, C, dbeta);
        GPH_CHECK(name);
    }
    sc.used = keep;
    return 0;
}

// ---------------------------------------------------------------------------------- 1x1 conv, NCHW, any Cout
bool conv1x1_ok(long B, long Cin, long Cout, long HW) {
    return B > 0 && Cin > 0 && Cout > 0 && HW > 0 && B * HW < (1L << 23) && Cin <= 65536 && Cout <= 65536;
}

int conv1x1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int HW, float* dX, float* dW, float* db,
                     Scratch& sc, hipStream_t s, const char* name) {
    const long m = (long)B * HW;
    if (dX)      // ((b, pixel) x Cout) (Cout x Cin)
        GPH_TRY(gemm_s(Nchw{dY, Cout, HW}, MatRow{Wt, Cin}, EpNchw{dX, Cin, HW, nullptr}, m, Cin, Cout, sc, s, name));
    if (dW)      // (Cout x m) (m x Cin)
        GPH_TRY(gemm_s(Tr<Nchw>{Nchw{dY, Cout, HW}}, Nchw{X, Cin, HW}, EpRow{dW, Cin, nullptr, 0, 0}, Cout, Cin, m, sc, s, name));
    if (db) GPH_TRY(colsum_s(Nchw{dY, Cout, HW}, m, Cout, db, sc, s, name));
    return 0;
}

// ---------------------------------------------------------------------------------- the encoder
bool enc_ok(long N, long R) { return N > 0 && N <= 4096 && R >= 8 && R <= 512 && R % 8 == 0 && N * R * R < (1L << 23); }

bool layer_params_complete(const gpe_layer_params& p) {
    return p.conv_w && p.conv_b && p.dw_w && p.dw_b && p.ln_w && p.ln_b && p.off_w && p.off_b && p.mask_w && p.mask_b && p.in_w && p.in_b &&
           p.out_w && p.out_b && p.gn_w && p.gn_b;
}
bool params_complete(const gpe_enc_params* p) {
    if (!p) return false;
    for (int l = 0; l < LAYERS; ++l)
        if (!layer_params_complete(p->layer[l])) return false;
    return true;
}
bool saved_complete(const gpe_enc_saved* v) {
    if (!v) return false;
    for (int l = 0; l < LAYERS; ++l) {
        const gpe_layer_saved& s = v->layer[l];
        if (!s.x || !s.xp || !s.dwout || !s.ln_mean || !s.ln_rstd || !s.x1 || !s.offset || !s.mask || !s.y || !s.pre || !s.gn_mean ||
            !s.gn_rstd || !s.act)
            return false;
    }
    return true;
}

const gpe_enc_params NO_PARAMS = {};
const gpe_enc_saved NO_SAVED = {};

int enc_forward(const float* coor, const gpe_enc_params* w, int N, int R, const gpe_enc_saved* sv, Scratch& sc, hipStream_t s,
                const char* name) {
    const float* in = coor;
    int Cin = 3, H = R;
    for (int l = 0; l < LAYERS; ++l) {
        const gpe_layer_params& p = w->layer[l];
        const gpe_layer_saved& v = sv->layer[l];
        const int Ho = H / 2;
        const long rows = (long)N * H * H, np = (long)N * Ho * Ho, keep = sc.used;
        float* logits = sc.take(np * MASKW);
        GPH_TRY(gemm_s(Nchw{in, Cin, H * H}, MatCol{p.conv_w, Cin}, EpRow{v.x, FEAT, p.conv_b, 0, 0}, rows, FEAT, Cin, sc, s, name));
        GPH_TRY(linear_forward(v.x, p.in_w, p.in_b, rows, FEAT, FEAT, v.xp, sc, s, name));
        if (!sc.dry)
            GPH_TRY(dwln_forward(v.x, p.dw_w, p.dw_b, p.ln_w, p.ln_b, H, H, FEAT, (int)np, v.dwout, v.ln_mean, v.ln_rstd, v.x1, s, name));
        GPH_TRY(linear_forward(v.x1, p.off_w, p.off_b, np, FEAT, OFFW, v.offset, sc, s, name));
        GPH_TRY(linear_forward(v.x1, p.mask_w, p.mask_b, np, FEAT, MASKW, logits, sc, s, name));
        if (!sc.dry) GPH_TRY(core_forward(v.xp, v.offset, logits, N, H, H, v.mask, v.y, s, name));
        GPH_TRY(gemm_s(MatRow{v.y, FEAT}, MatCol{p.out_w, FEAT}, EpNchwBias{v.pre, FEAT, Ho * Ho, p.out_b}, np, FEAT, FEAT, sc, s, name));
        if (!sc.dry) GPH_TRY(gn_relu_forward(v.pre, p.gn_w, p.gn_b, N, FEAT, Ho * Ho, GNG, v.act, v.gn_mean, v.gn_rstd, s, name));
        sc.used = keep;
        in = v.act;
        Cin = FEAT;
        H = Ho;
    }
    return 0;
}

int enc_backward(const gpe_enc_params* w, const gpe_enc_saved* sv, const float* coor, const float* g_feat, int N, int R,
                 const gpe_enc_params* gr, float* g_coor, int scatter, Scratch& sc, hipStream_t s, const char* name) {
    // the gradient of layer l's input map is layer l - 1's upstream gradient: two buffers that live across layers
    float* dmap[LAYERS] = {g_coor, sc.take((long)N * FEAT * (R / 2) * (R / 2)), sc.take((long)N * FEAT * (R / 4) * (R / 4))};
    const float* da = g_feat;
    for (int l = LAYERS - 1; l >= 0; --l) {
        const gpe_layer_params &p = w->layer[l], &g = gr->layer[l];
        const gpe_layer_saved& v = sv->layer[l];
        const int H = R >> l, Ho = H / 2, Cin = l ? FEAT : 3;
        const float* in = l ? sv->layer[l - 1].act : coor;
        const long rows = (long)N * H * H, np = (long)N * Ho * Ho, keep = sc.used;
        float* dpre = sc.take(np * FEAT);       // NCHW (N,256,Ho,Ho)
        float* dy = sc.take(np * FEAT);
        float* dxp = sc.take(rows * FEAT);
        float* doff = sc.take(np * OFFW);
        float* dml = sc.take(np * MASKW);
        float* dx1 = sc.take(np * FEAT);
        float* dx = sc.take(rows * FEAT);
        float* index = scatter == GPE_SCATTER_ORDERED ? sc.take(index_floats(scatter, N, H, H)) : nullptr;
        GPH_TRY(gn_relu_backward(da, v.pre, v.gn_mean, v.gn_rstd, p.gn_w, p.gn_b, N, FEAT, Ho * Ho, GNG, dpre, g.gn_w, g.gn_b, sc, s, name));
        // output_proj on the rows of the NCHW gradient
        const Nchw dout{dpre, FEAT, Ho * Ho};
        GPH_TRY(gemm_s(dout, MatRow{p.out_w, FEAT}, EpRow{dy, FEAT, nullptr, 0, 0}, np, FEAT, FEAT, sc, s, name));
        GPH_TRY(gemm_s(Tr<Nchw>{dout}, MatRow{v.y, FEAT}, EpRow{g.out_w, FEAT, nullptr, 0, 0}, FEAT, FEAT, np, sc, s, name));
        GPH_TRY(colsum_s(dout, np, FEAT, g.out_b, sc, s, name));
        if (!sc.dry) GPH_TRY(core_backward(v.xp, v.offset, v.mask, dy, N, H, H, dxp, doff, dml, scatter, index, s, name));
        // the offset / mask branch, prefix rows only: d x1 is the sum of the two Linears' parts, in this order
        GPH_TRY(linear_backward(doff, v.x1, p.off_w, np, FEAT, OFFW, dx1, 0, g.off_w, g.off_b, sc, s, name));
        GPH_TRY(linear_backward(dml, v.x1, p.mask_w, np, FEAT, MASKW, dx1, 1, g.mask_w, g.mask_b, sc, s, name));
        GPH_TRY(dwln_backward(dx1, v.x, v.dwout, v.ln_mean, v.ln_rstd, p.dw_w, p.ln_w, p.ln_b, N, H, H, FEAT, (int)np, dx, g.dw_w, g.dw_b, g.ln_w,
                              g.ln_b, sc, s, name));
        // d x = the depth-wise branch's part (written in full above) + input_proj's part
        GPH_TRY(linear_backward(dxp, v.x, p.in_w, rows, FEAT, FEAT, dx, 1, g.in_w, g.in_b, sc, s, name));
        // the layer's conv1x1 on the rows of the NCHW input
        GPH_TRY(gemm_s(Tr<MatRow>{MatRow{dx, FEAT}}, Nchw{in, Cin, H * H}, EpRow{g.conv_w, Cin, nullptr, 0, 0}, FEAT, Cin, rows, sc, s, name));
        GPH_TRY(colsum_s(MatRow{dx, FEAT}, rows, FEAT, g.conv_b, sc, s, name));
        GPH_TRY(gemm_s(MatRow{dx, FEAT}, MatRow{p.conv_w, Cin}, EpNchw{dmap[l], Cin, H * H, nullptr}, rows, Cin, FEAT, sc, s, name));
        sc.used = keep;
        da = dmap[l];
    }
    return 0;
}

// the second pass of an entry point: the dry pass gave `need`
#define GPE_WS_CHECK(dry, ws, ws_bytes, name)                                                                                   \
    GP_REQUIRE((dry).need == 0 || ((ws) && aligned256(ws) && (ws_bytes) / 4 >= (dry).need),                                      \
               "%s: workspace missing, unaligned or too small (%lld bytes, %ld needed)", name, (long long)(ws_bytes), 4 * (dry).need)

}  // namespace

extern "C" {

long long gpe_linear_workspace(int rows, int Cin, int Cout) {
    if (!linear_ok(rows, Cin, Cout)) return 0;
    Scratch d(nullptr, 0, true);
    linear_forward(nullptr, nullptr, nullptr, rows, Cin, Cout, nullptr, d, nullptr, "");
    float one;
    linear_backward(nullptr, nullptr, nullptr, rows, Cin, Cout, &one, 0, &one, &one, d, nullptr, "");
    return 4LL * d.need;
}

int gpe_linear_forward(const float* X, const float* Wt, const float* b, int rows, int Cin, int Cout, float* Y, void* ws, long long ws_bytes,
                       void* stream) {
    const char* name = "gpe_linear_forward";
    GP_REQUIRE(X && Wt && Y && linear_ok(rows, Cin, Cout), "%s: bad arguments (rows %d Cin %d Cout %d)", name, rows, Cin, Cout);
    Scratch d(nullptr, 0, true), sc(ws, ws_bytes, false);
    linear_forward(X, Wt, b, rows, Cin, Cout, Y, d, nullptr, name);
    GPE_WS_CHECK(d, ws, ws_bytes, name);
    return linear_forward(X, Wt, b, rows, Cin, Cout, Y, sc, (hipStream_t)stream, name);
}

int gpe_linear_backward(const float* dY, const float* X, const float* Wt, int rows, int Cin, int Cout, float* dX, float* dW, float* db,
                        void* ws, long long ws_bytes, void* stream) {
    const char* name = "gpe_linear_backward";
    GP_REQUIRE(dY && linear_ok(rows, Cin, Cout), "%s: bad arguments (rows %d Cin %d Cout %d)", name, rows, Cin, Cout);
    GP_REQUIRE((!dW || X) && (!dX || Wt), "%s: dW needs X, dX needs the weights", name);
    Scratch d(nullptr, 0, true), sc(ws, ws_bytes, false);
    linear_backward(dY, X, Wt, rows, Cin, Cout, dX, 0, dW, db, d, nullptr, name);
    GPE_WS_CHECK(d, ws, ws_bytes, name);
    return linear_backward(dY, X, Wt, rows, Cin, Cout, dX, 0, dW, db, sc, (hipStream_t)stream, name);
}

int gpe_dwln_forward_save(const float* xin, const float* dw_w, const float* dw_b, const float* ln_w, const float* ln_b, int N, int H, int W,
                          int C, int n_pixels, float* dwout, float* mean, float* rstd, float* x1, void* stream) {
    const char* name = "gpe_dwln_forward_save";
    GP_REQUIRE(xin && dw_w && dw_b && ln_w && ln_b && dwout && mean && rstd && x1, "%s: null pointer", name);
    GP_REQUIRE(dwln_ok(N, H, W, C, n_pixels), "%s: bad shape N %d H %d W %d C %d n_pixels %d", name, N, H, W, C, n_pixels);
    return dwln_forward(xin, dw_w, dw_b, ln_w, ln_b, H, W, C, n_pixels, dwout, mean, rstd, x1, (hipStream_t)stream, name);
}

long long gpe_dwln_backward_workspace(int N, int H, int W, int C, int n_pixels) {
    if (!dwln_ok(N, H, W, C, n_pixels)) return 0;
    Scratch d(nullptr, 0, true);
    dwln_backward(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N, H, W, C, n_pixels, nullptr, nullptr, nullptr, nullptr,
                  nullptr, d, nullptr, "");
    return 4LL * d.need;
}

int gpe_dwln_backward(const float* dx1, const float* xin, const float* dwout, const float* mean, const float* rstd, const float* dw_w,
                      const float* ln_w, const float* ln_b, int N, int H, int W, int C, int n_pixels, float* dxin, float* d_dw_w,
                      float* d_dw_b, float* d_ln_w, float* d_ln_b, void* ws, long long ws_bytes, void* stream) {
    const char* name = "gpe_dwln_backward";
    GP_REQUIRE(dx1 && xin && dwout && mean && rstd && dw_w && ln_w && ln_b && dxin && d_dw_w && d_dw_b && d_ln_w && d_ln_b, "%s: null pointer",
               name);
    GP_REQUIRE(dwln_ok(N, H, W, C, n_pixels), "%s: bad shape N %d H %d W %d C %d n_pixels %d", name, N, H, W, C, n_pixels);
    GP_REQUIRE(ws && aligned256(ws) && ws_bytes >= gpe_dwln_backward_workspace(N, H, W, C, n_pixels),
               "%s: workspace missing, unaligned or too small", name);
    Scratch sc(ws, ws_bytes, false);
    return dwln_backward(dx1, xin, dwout, mean, rstd, dw_w, ln_w, ln_b, N, H, W, C, n_pixels, dxin, d_dw_w, d_dw_b, d_ln_w, d_ln_b, sc,
                         (hipStream_t)stream, name);
}

int gpe_dcnv3_core_forward(const float* xp, const float* offset, const float* mask_logits, int N, int H, int W, float* mask, float* y,
                           void* stream) {
    const char* name = "gpe_dcnv3_core_forward";
    GP_REQUIRE(xp && offset && mask_logits && mask && y, "%s: null pointer", name);
    GP_REQUIRE(core_ok(N, H, W), "%s: bad shape N %d H %d W %d", name, N, H, W);
    return core_forward(xp, offset, mask_logits, N, H, W, mask, y, (hipStream_t)stream, name);
}

long long gpeo_dcnv3_core_backward_workspace(int N, int H, int W, int scatter) {
    if (!core_ok(N, H, W) || !scatter_ok(scatter)) return 0;
    return 4LL * up64(index_floats(scatter, N, H, W));
}

int gpeo_dcnv3_core_backward(const float* xp, const float* offset, const float* mask, const float* dy, int N, int H, int W, float* dxp,
                             float* doffset, float* dmask_logits, void* stream, int scatter, void* ws, long long ws_bytes) {
    const char* name = scatter == GPE_SCATTER_ATOMIC ? "gpe_dcnv3_core_backward" : "gpeo_dcnv3_core_backward";
    GP_REQUIRE(scatter_ok(scatter), "%s: unknown scatter mode %d (GPE_SCATTER_ATOMIC 0, GPE_SCATTER_ORDERED 1)", name, scatter);
    GP_REQUIRE(xp && offset && mask && dy && dxp && doffset && dmask_logits, "%s: null pointer", name);
    GP_REQUIRE(core_ok(N, H, W), "%s: bad shape N %d H %d W %d", name, N, H, W);
    const long long need = gpeo_dcnv3_core_backward_workspace(N, H, W, scatter);
    GP_REQUIRE(need == 0 || (ws && aligned256(ws) && ws_bytes >= need), "%s: workspace missing, unaligned or too small (%lld bytes, %lld needed)",
               name, ws_bytes, need);
    return core_backward(xp, offset, mask, dy, N, H, W, dxp, doffset, dmask_logits, scatter, need ? (float*)ws : nullptr, (hipStream_t)stream,
                         name);
}

int gpe_dcnv3_core_backward(const float* xp, const float* offset, const float* mask, const float* dy, int N, int H, int W, float* dxp,
                            float* doffset, float* dmask_logits, void* stream) {
    return gpeo_dcnv3_core_backward(xp, offset, mask, dy, N, H, W, dxp, doffset, dmask_logits, stream, GPE_SCATTER_ATOMIC, nullptr, 0);
}

int gpe_gn_relu_forward(const float* x, const float* gamma, const float* beta, int B, int C, int HW, int G, float* out, float* mean,
                        float* rstd, void* stream) {
    const char* name = "gpe_gn_relu_forward";
    GP_REQUIRE(x && gamma && beta && out && mean && rstd && gn_ok(B, C, HW, G), "%s: bad GroupNorm arguments", name);
    return gn_relu_forward(x, gamma, beta, B, C, HW, G, out, mean, rstd, (hipStream_t)stream, name);
}

long long gpe_gn_relu_backward_workspace(int B, int C) { return B > 0 && C > 0 ? 8LL * up64((long)B * C) : 0; }

int gpe_gn_relu_backward(const float* dout, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         int B, int C, int HW, int G, float* dx, float* dgamma, float* dbeta, void* ws, long long ws_bytes, void* stream) {
    const char* name = "gpe_gn_relu_backward";
    GP_REQUIRE(dout && x && mean && rstd && gamma && beta && dx && dgamma && dbeta, "%s: null pointer", name);
    GP_REQUIRE(gn_ok(B, C, HW, G), "%s: bad shape B %d C %d HW %d G %d", name, B, C, HW, G);
    GP_REQUIRE(ws && aligned256(ws) && ws_bytes >= gpe_gn_relu_backward_workspace(B, C), "%s: workspace missing, unaligned or too small", name);
    Scratch sc(ws, ws_bytes, false);
    return gn_relu_backward(dout, x, mean, rstd, gamma, beta, B, C, HW, G, dx, dgamma, dbeta, sc, (hipStream_t)stream, name);
}

long long gpe_conv1x1_backward_workspace(int B, int Cin, int Cout, int HW) {
    if (!conv1x1_ok(B, Cin, Cout, HW)) return 0;
    Scratch d(nullptr, 0, true);
    float one;
    conv1x1_backward(nullptr, nullptr, nullptr, B, Cin, Cout, HW, &one, &one, &one, d, nullptr, "");
    return 4LL * d.need;
}

int gpe_conv1x1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int HW, float* dX, float* dW, float* db,
                         void* ws, long long ws_bytes, void* stream) {
    const char* name = "gpe_conv1x1_backward";
    GP_REQUIRE(dY && conv1x1_ok(B, Cin, Cout, HW), "%s: bad arguments (B %d Cin %d Cout %d HW %d)", name, B, Cin, Cout, HW);
    GP_REQUIRE((!dW || X) && (!dX || Wt), "%s: dW needs X, dX needs the weights", name);
    Scratch d(nullptr, 0, true), sc(ws, ws_bytes, false);
    conv1x1_backward(dY, X, Wt, B, Cin, Cout, HW, dX, dW, db, d, nullptr, name);
    GPE_WS_CHECK(d, ws, ws_bytes, name);
    return conv1x1_backward(dY, X, Wt, B, Cin, Cout, HW, dX, dW, db, sc, (hipStream_t)stream, name);
}

long long gpe_map_encoder_forward_workspace(int N, int R) {
    if (!enc_ok(N, R)) return 0;
    Scratch d(nullptr, 0, true);
    enc_forward(nullptr, &NO_PARAMS, N, R, &NO_SAVED, d, nullptr, "");
    return 4LL * d.need;
}

int gpe_map_encoder_forward_save(const float* coor, const gpe_enc_params* w, int N, int R, const gpe_enc_saved* saved, void* ws,
                                 long long ws_bytes, void* stream) {
    const char* name = "gpe_map_encoder_forward_save";
    GP_REQUIRE(coor && params_complete(w) && saved_complete(saved), "%s: null pointer", name);
    GP_REQUIRE(enc_ok(N, R), "%s: bad shape N %d R %d", name, N, R);
    GP_REQUIRE(ws && aligned256(ws) && ws_bytes >= gpe_map_encoder_forward_workspace(N, R), "%s: workspace missing, unaligned or too small", name);
    Scratch sc(ws, ws_bytes, false);
    return enc_forward(coor, w, N, R, saved, sc, (hipStream_t)stream, name);
}

long long gpeo_map_encoder_backward_workspace(int N, int R, int scatter) {
    if (!enc_ok(N, R) || !scatter_ok(scatter)) return 0;
    Scratch d(nullptr, 0, true);
    enc_backward(&NO_PARAMS, &NO_SAVED, nullptr, nullptr, N, R, &NO_PARAMS, nullptr, scatter, d, nullptr, "");
    return 4LL * d.need;
}

int gpeo_map_encoder_backward(const gpe_enc_params* w, const gpe_enc_saved* saved, const float* coor, const float* g_feat, int N, int R,
                              const gpe_enc_params* grads, float* g_coor, void* ws, long long ws_bytes, void* stream, int scatter) {
    const char* name = scatter == GPE_SCATTER_ATOMIC ? "gpe_map_encoder_backward" : "gpeo_map_encoder_backward";
    GP_REQUIRE(scatter_ok(scatter), "%s: unknown scatter mode %d (GPE_SCATTER_ATOMIC 0, GPE_SCATTER_ORDERED 1)", name, scatter);
    GP_REQUIRE(params_complete(w) && saved_complete(saved) && params_complete(grads) && coor && g_feat && g_coor, "%s: null pointer", name);
    GP_REQUIRE(enc_ok(N, R), "%s: bad shape N %d R %d", name, N, R);
    GP_REQUIRE(ws && aligned256(ws) && ws_bytes >= gpeo_map_encoder_backward_workspace(N, R, scatter),
               "%s: workspace missing, unaligned or too small", name);
    Scratch sc(ws, ws_bytes, false);
    return enc_backward(w, saved, coor, g_feat, N, R, grads, g_coor, scatter, sc, (hipStream_t)stream, name);
}

long long gpe_map_encoder_backward_workspace(int N, int R) { return gpeo_map_encoder_backward_workspace(N, R, GPE_SCATTER_ATOMIC); }

int gpe_map_encoder_backward(const gpe_enc_params* w, const gpe_enc_saved* saved, const float* coor, const float* g_feat, int N, int R,
                             const gpe_enc_params* grads, float* g_coor, void* ws, long long ws_bytes, void* stream) {
    return gpeo_map_encoder_backward(w, saved, coor, g_feat, N, R, grads, g_coor, ws, ws_bytes, stream, GPE_SCATTER_ATOMIC);
}

}  // extern "C"
