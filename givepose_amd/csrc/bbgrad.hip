// Backbone backward family (include/givepose_bbgrad.h, prefix gpb_): the ConvNeXt backbone's forward-that-saves and its backward in
// fp32, and the operators they are made of.
//
// Inside the family an activation is channels-last rows (b,h,w) x C.  Every contraction is a view on the functor GEMM of
// grad_gemm.hpp: a Linear over rows is MatRow x MatCol, a patch conv reads its input through Patch (rows (b,oh,ow) x columns
// (ci,kh,kw), so the OIHW weight is a plain matrix) and writes its input gradient through EpPatch, the last block's output and its
// gradient are NCHW through EpFc2<true> and Nchw.  d y2 = g gamma is never formed: the scale is applied in d W2's store functor
// (EpRowScaleM) and folded into W2 for d h = (g . gamma W2) GELU'(h), whose store functor is EpGeluBack -- a product inside an operand
// view would have to wait for its loads, which then no longer stream under the MFMAs.  What is not a contraction: the ordered row sums (the kernels of encgrad.hip, restated here: that file and
// grad_gemm.hpp are untouched), LayerNorm over rows, the GELU map and the depth-wise 7x7 kernels.
//
// The depth-wise 7x7 kernels are built around data movement.  A lane holds a channel, so every load and store of a wavefront is one
// contiguous 256-byte row segment.  Forward and dX (the same kernel, taps flipped): a wavefront computes a DW_TH x DW_TW tile of
// output pixels for its 64 channels from registers -- the 49 weights, the tile's accumulators, and one input row of DW_TW + 6 pixels
// at a time, which is loaded once and feeds every output row of the tile whose window holds it: (DW_TH + 6)(DW_TW + 6) loads for
// DW_TH DW_TW outputs, 7 per output in the place of 49.  dW: 49 + 1 accumulators per lane over a chunk of rows.
//
// Precision (include/givepose_bbgrad_bf16.h, gpbm_*): the six dense contractions of a block go through gemm_p, which runs the fp32 chain
// above or, for GPB_PREC_BF16, the bf16-operand form of the same functor GEMM (grad_gemm_bf16.hpp) with the same views, store functors and
// workspace layout.  The patch convs, the row sums and everything that is not a contraction are fp32 in both modes.
//
// There is no atomic in this file.  The size queries and the entry points run the same host code: a Scratch in `dry` mode only
// records what a run would take.
#include "grad_gemm.hpp"
#include "grad_gemm_bf16.hpp"
#include "../../include/givepose_bbgrad.h"
#include "../../include/givepose_bbgrad_bf16.h"

namespace {

constexpr int COLSUM_CHUNK = 256;     // rows per workgroup of an ordered row sum
constexpr int DW_TH = 2, DW_TW = 8;   // output tile of a wavefront of the depth-wise kernels
constexpr int TAPS = 49;
constexpr int STEM_CIN = 3;

long max2(long a, long b) { return a > b ? a : b; }
bool aligned256(const void* p) { return ((uintptr_t)p & 255) == 0; }

// the workspace of a call: take() carves what lives to the end of the call, want() announces what one step needs behind that
struct Scratch {
    float* base; long size; bool dry; int prec; long used = 0, need = 0;      // prec: GPB_PREC_* of the block contractions (gemm_p)
    Scratch(void* ws, long long bytes, bool d, int p = GPB_PREC_F32) : base((float*)ws), size((long)(bytes / 4)), dry(d), prec(p) {}
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

// the six contractions of a block: in the call's precision, fp32 chains or bf16 operands with fp32 sums (grad_gemm_bf16.hpp)
template <class AF, class BF, class EP>
int gemm_p(const AF& A, const BF& Bm, const EP& ep, long M, long N, long K, Scratch& sc, hipStream_t s, const char* name) {
    if (sc.prec == GPB_PREC_F32) return gemm_s(A, Bm, ep, M, N, K, sc, s, name);
    sc.want(gemm_bf16_ws_floats(M, N, K));
    if (sc.dry) return 0;
    return gemm_bf16(A, Bm, ep, M, N, K, sc.rest(), sc.rest_floats(), s, name);
}
bool prec_ok(int p) { return p == GPB_PREC_F32 || p == GPB_PREC_BF16; }

// ---------------------------------------------------------------------------------- views and store functors of this family
struct Patch {       // non-overlapping p x p patches as rows (b,oh,ow) x columns (ci,kh,kw); sb, sc, sy, sx: element strides of b, ci, y, x
    const float* x; int Ho, Wo, p; long sb, sc, sy, sx;
    static constexpr bool FAST_C = true;
    __device__ __forceinline__ long at(int r, int c) const {
        const int hw = Ho * Wo, b = r / hw, px = r - b * hw, oh = px / Wo, ow = px - oh * Wo;
        const int pp = p * p, ci = c / pp, t = c - ci * pp, kh = t / p, kw = t - kh * p;
        return b * sb + ci * sc + (long)(oh * p + kh) * sy + (long)(ow * p + kw) * sx;
    }
    __device__ __forceinline__ float operator()(int r, int c) const { return x[at(r, c)]; }
};
struct EpPatch {     // the same index map as a store: every input element has exactly one (m, n)
    float* x; Patch v;
    static constexpr bool M_FAST = false;
    __device__ __forceinline__ void operator()(int m, int n, float val) const { x[v.at(m, n)] = val; }
};
template <class G> struct Scaled {      // g(r, c) s[c]: d y2 = g gamma
    G g; const float* s;
    static constexpr bool FAST_C = G::FAST_C;
    __device__ __forceinline__ float operator()(int r, int c) const { return g(r, c) * s[c]; }
};
template <class G> struct Prod {        // g(r, c) y[r, c]: the terms of d gamma
    G g; const float* y; long ld;
    __device__ __forceinline__ float operator()(int r, int c) const { return g(r, c) * y[(long)r * ld + c]; }
};
struct LnGw {        // dy[r, c] xhat[r, c] at the saved statistics: the terms of a LayerNorm's d weight
    const float *dy, *x, *mean, *rstd; long ld;
    __device__ __forceinline__ float operator()(int r, int c) const {
        const long i = (long)r * ld + c;
        return dy[i] * ((x[i] - mean[r]) * rstd[r]);
    }
};

__device__ __forceinline__ float gelu_value(float u) { return 0.5f * u * (1.0f + erff(u * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_slope(float u) {      // Phi(u) + u phi(u)
    const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * expf(-0.5f * u * u);
    return fmaf(u, pdf, cdf);
}

struct EpFc1 {       // h = v + bias (saved) and a = GELU(h) (fc2's operand)
    float *h, *a; long ld; const float* bias;
    static constexpr bool M_FAST = false;
    __device__ __forceinline__ void operator()(int m, int n, float v) const {
        const long i = (long)m * ld + n;
        v += bias[n];
        h[i] = v;
        a[i] = gelu_value(v);
    }
};
template <bool NCHW> struct EpFc2 {      // y2 = v + bias (saved) and out = x + gamma y2, as rows or as (B,C,HW)
    float* y2; const float *x, *bias, *gamma; float* out; int C, HW;
    static constexpr bool M_FAST = NCHW;
    __device__ __forceinline__ void operator()(int m, int n, float v) const {
        const long i = (long)m * C + n;
        v += bias[n];
        y2[i] = v;
        const float o = x[i] + gamma[n] * v;
        if (NCHW) {
            const int b = m / HW, px = m - b * HW;
            out[((long)b * C + n) * HW + px] = o;
        } else {
            out[i] = o;
        }
    }
};
struct EpRowScaleM { // C[m * ld + n] = v s[m]: d W2 = gamma (g^T a), the layer scale applied once per element after the chain
    float* C; long ld; const float* s;
    static constexpr bool M_FAST = false;
    __device__ __forceinline__ void operator()(int m, int n, float v) const { C[(long)m * ld + n] = v * s[m]; }
};
struct EpGeluBack {  // d h = v GELU'(h)
    float* dh; const float* h; long ld;
    static constexpr bool M_FAST = false;
    __device__ __forceinline__ void operator()(int m, int n, float v) const {
        const long i = (long)m * ld + n;
        dh[i] = v * gelu_slope(h[i]);
    }
};

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

bool rows_ok(long rows) { return rows > 0 && rows < (1L << 23); }      // 65535 chunks of 256 rows in grid.y, and int row indices
bool chan_ok(long C) { return C > 0 && C % 64 == 0 && C <= 16384; }

template <class F>
int colsum_s(const F& f, long rows, long cols, float* out, Scratch& sc, hipStream_t s, const char* name) {
    const int chunks = cdiv(rows, COLSUM_CHUNK);
    sc.want((long)chunks * cols);
    if (sc.dry) return 0;
    GP_REQUIRE(rows_ok(rows) && cols > 0 && cols < (1L << 22) && sc.rest_floats() >= (long)chunks * cols,
               "%s: bad row sum %ld x %ld or workspace too small", name, rows, cols);
    hipLaunchKernelGGL((colsum_kernel<F>), dim3(cdiv(cols, 64), chunks), dim3(WG), 0, s, f, (int)rows, (int)cols, sc.rest());
    GPH_CHECK(name);
    hipLaunchKernelGGL(rows_merge_kernel, dim3(cdiv(cols, WG)), dim3(WG), 0, s, (const float*)sc.rest(), chunks, (int)cols, out);
    GPH_CHECK(name);
    return 0;
}

// ---------------------------------------------------------------------------------- LayerNorm over rows, eps 1e-6
// One wavefront per row, lane l the channels l, l + 64, ...; the row (at most a few KB) is read again from the cache for the
// second moment and the result, so that C is not bounded by a register array.  SAVED: normalise with the given statistics.
template <bool SAVED>
__global__ __launch_bounds__(WG) void ln_forward_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                        long rows, int C, float* __restrict__ y, float* mean, float* rstd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * 4 + wave;
    if (r >= rows) return;      // wave-uniform
    const float* xr = x + r * C;
    float mu, rs;
    if (SAVED) {
        mu = mean[r];
        rs = rstd[r];
    } else {
        const float inv_c = 1.0f / (float)C;
        float s = 0.0f;
        for (int c = lane; c < C; c += 64) s += xr[c];
        mu = group_sum(s, 64) * inv_c;
        float q = 0.0f;
        for (int c = lane; c < C; c += 64) {
            const float d = xr[c] - mu;
            q = fmaf(d, d, q);
        }
        rs = 1.0f / sqrtf(group_sum(q, 64) * inv_c + 1e-6f);
        if (lane == 0) {
            mean[r] = mu;
            rstd[r] = rs;
        }
    }
    for (int c = lane; c < C; c += 64) y[r * C + c] = fmaf((xr[c] - mu) * rs, w[c], b[c]);
}

// dx = rstd ((dxh - mean(dxh)) - xhat mean(dxh xhat)), dxh = dy w, at the saved statistics
__global__ __launch_bounds__(WG) void ln_dx_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                   const float* __restrict__ rstd, const float* __restrict__ w, long rows, int C,
                                                   float* __restrict__ dx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * 4 + wave;
    if (r >= rows) return;      // wave-uniform
    const float mu = mean[r], rs = rstd[r], inv_c = 1.0f / (float)C;
    const float *xr = x + r * C, *dr = dy + r * C;
    float s1 = 0.0f, s2 = 0.0f;
    for (int c = lane; c < C; c += 64) {
        const float xh = (xr[c] - mu) * rs, dxh = dr[c] * w[c];
        s1 += dxh;
        s2 = fmaf(dxh, xh, s2);
    }
    const float m1 = group_sum(s1, 64) * inv_c, m2 = group_sum(s2, 64) * inv_c;
    for (int c = lane; c < C; c += 64) {
        const float xh = (xr[c] - mu) * rs, dxh = dr[c] * w[c];
        dx[r * C + c] = rs * ((dxh - m1) - xh * m2);
    }
}

int ln_forward(const float* x, const float* w, const float* b, long rows, int C, float* y, float* mean, float* rstd, bool saved, hipStream_t s,
               const char* name) {
    if (saved) hipLaunchKernelGGL(ln_forward_kernel<true>, dim3(cdiv(rows, 4)), dim3(WG), 0, s, x, w, b, rows, C, y, mean, rstd);
    else hipLaunchKernelGGL(ln_forward_kernel<false>, dim3(cdiv(rows, 4)), dim3(WG), 0, s, x, w, b, rows, C, y, mean, rstd);
    GPH_CHECK(name);
    return 0;
}

// dx must not alias dy or x
int ln_backward(const float* dy, const float* x, const float* mean, const float* rstd, const float* w, long rows, int C, float* dx, float* dw,
                float* db, Scratch& sc, hipStream_t s, const char* name) {
    if (!sc.dry) {
        hipLaunchKernelGGL(ln_dx_kernel, dim3(cdiv(rows, 4)), dim3(WG), 0, s, dy, x, mean, rstd, w, rows, C, dx);
        GPH_CHECK(name);
    }
    GPH_TRY(colsum_s(LnGw{dy, x, mean, rstd, C}, rows, C, dw, sc, s, name));
    GPH_TRY(colsum_s(MatRow{dy, C}, rows, C, db, sc, s, name));
    return 0;
}

// ---------------------------------------------------------------------------------- GELU map
__global__ __launch_bounds__(WG) void gelu_map_kernel(const float* __restrict__ h, long n, float* __restrict__ a) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i < n) a[i] = gelu_value(h[i]);
}

// out[r, c] = s[r] w[r, c]: gamma folded into W2 for the d h contraction
__global__ __launch_bounds__(WG) void scale_rows_kernel(const float* __restrict__ w, const float* __restrict__ s, long n, int cols,
                                                        float* __restrict__ out) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i < n) out[i] = s[i / cols] * w[i];
}

// ---------------------------------------------------------------------------------- depth-wise 7x7, pad 3, channels-last
// Workgroup: four wavefronts, each a DW_TH x DW_TW tile of output pixels of one image for the 64 channels of slab blockIdx.y.
// out(h, w) = bias + sum_{kh,kw} in(h - 3 + kh, w - 3 + kw) wt[kh][kw] in (kh, kw) order; FLIP reads the taps as wt[6 - kh][6 - kw]
// (the gather of d x); RES adds the accumulated value to res(row, c): res + acc.  A row outside the image is skipped, a column
// outside it is an exact 0 operand.
struct NoRes {
    __device__ __forceinline__ float operator()(int, int) const { return 0.0f; }
};
template <bool FLIP, bool RES, class G>
__global__ __launch_bounds__(WG) void dw7_kernel(const float* __restrict__ in, const float* __restrict__ wt, const float* __restrict__ bias,
                                                 G res, int N, int H, int W, int C, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.y * 64 + lane;
    const int th = (H + DW_TH - 1) / DW_TH, tw = (W + DW_TW - 1) / DW_TW;
    const long tile = (long)blockIdx.x * 4 + wave;
    if (tile >= (long)N * th * tw) return;      // wave-uniform
    const int n = (int)(tile / (th * tw)), rem = (int)(tile - (long)n * th * tw), h0 = (rem / tw) * DW_TH, w0 = (rem % tw) * DW_TW;
    float wreg[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t) wreg[t] = wt[c * TAPS + (FLIP ? TAPS - 1 - t : t)];
    float acc[DW_TH][DW_TW];
    const float b0 = bias ? bias[c] : 0.0f;
#pragma unroll
    for (int oh = 0; oh < DW_TH; ++oh)
#pragma unroll
        for (int ow = 0; ow < DW_TW; ++ow) acc[oh][ow] = b0;
#pragma unroll
    for (int iy = 0; iy < DW_TH + 6; ++iy) {
        const int y = h0 - 3 + iy;
        if ((unsigned)y < (unsigned)H) {      // wave-uniform
            float row[DW_TW + 6];
#pragma unroll
            for (int ix = 0; ix < DW_TW + 6; ++ix) {
                const int x = w0 - 3 + ix;
                row[ix] = (unsigned)x < (unsigned)W ? in[(((long)n * H + y) * W + x) * C + c] : 0.0f;
            }
#pragma unroll
            for (int oh = 0; oh < DW_TH; ++oh) {
                const int kh = iy - oh;
                if (kh >= 0 && kh < 7) {
#pragma unroll
                    for (int ow = 0; ow < DW_TW; ++ow)
#pragma unroll
                        for (int kw = 0; kw < 7; ++kw) acc[oh][ow] = fmaf(row[ow + kw], wreg[kh * 7 + kw], acc[oh][ow]);
                }
            }
        }
    }
#pragma unroll
    for (int oh = 0; oh < DW_TH; ++oh)
#pragma unroll
        for (int ow = 0; ow < DW_TW; ++ow) {
            const int h = h0 + oh, w = w0 + ow;
            if (h < H && w < W) {
                const long r = ((long)n * H + h) * W + w;
                out[r * C + c] = RES ? res((int)r, c) + acc[oh][ow] : acc[oh][ow];
            }
        }
}

// d wt[c][kh][kw] = sum_r dy[r, c] x(r's pixel + (kh - 3, kw - 3), c) and d bias[c] = sum_r dy[r, c] over the rows of chunk blockIdx.y:
// lane = channel of slab blockIdx.x, 49 + 1 accumulators in registers, wave w the chunk's rows w, w + 4, ... in turn, the waves added
// as (w0 + w1) + (w2 + w3).  A tap outside the image is skipped: an accumulator no pixel ever meets stays an exact 0.
__global__ __launch_bounds__(WG) void dw7_dw_kernel(const float* __restrict__ dy, const float* __restrict__ x, int H, int W, int C, long rows,
                                                    int chunk, float* __restrict__ partw, float* __restrict__ partb) {
    __shared__ float sh[2][TAPS + 1][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    const long r0 = (long)blockIdx.y * chunk, r1 = min(rows, r0 + chunk);
    const int hw = H * W;
    float acc[TAPS], ab = 0.0f;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) acc[t] = 0.0f;
    for (long r = r0 + wave; r < r1; r += 4) {
        const int n = (int)(r / hw), px = (int)(r - (long)n * hw), h = px / W, w = px - h * W;
        const float d = dy[r * C + c];
        ab += d;
#pragma unroll
        for (int kh = 0; kh < 7; ++kh) {
            const int y = h - 3 + kh;
            if ((unsigned)y < (unsigned)H) {      // wave-uniform, as the next
#pragma unroll
                for (int kw = 0; kw < 7; ++kw) {
                    const int xx = w - 3 + kw;
                    if ((unsigned)xx < (unsigned)W) acc[kh * 7 + kw] = fmaf(d, x[(((long)n * H + y) * W + xx) * C + c], acc[kh * 7 + kw]);
                }
            }
        }
    }
    if (wave & 1) {
#pragma unroll
        for (int t = 0; t < TAPS; ++t) sh[wave >> 1][t][lane] = acc[t];
        sh[wave >> 1][TAPS][lane] = ab;
    }
    __syncthreads();
    if (!(wave & 1)) {
#pragma unroll
        for (int t = 0; t < TAPS; ++t) acc[t] += sh[wave >> 1][t][lane];
        ab += sh[wave >> 1][TAPS][lane];
    }
    __syncthreads();
    if (wave == 2) {
#pragma unroll
        for (int t = 0; t < TAPS; ++t) sh[0][t][lane] = acc[t];
        sh[0][TAPS][lane] = ab;
    }
    __syncthreads();
    if (wave == 0) {
        float* pw = partw + ((long)blockIdx.y * C + c) * TAPS;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) pw[t] = acc[t] + sh[0][t][lane];
        partb[(long)blockIdx.y * C + c] = ab + sh[0][TAPS][lane];
    }
}

bool dw7_ok(long N, long H, long W, long C) {
    return N > 0 && H > 0 && W > 0 && H <= 4096 && W <= 4096 && chan_ok(C) && rows_ok(N * H * W) && N * H * W * C < (1L << 40);
}
// the rows of a d weight chunk depend on the shape alone: at most 512 chunks, at least 32 rows each
int dw7_chunk(long rows) { return (int)max2(32, (cdiv(rows, 512) + 3) / 4 * 4); }

template <bool FLIP, bool RES, class G>
int dw7_run(const float* in, const float* wt, const float* bias, const G& res, int N, int H, int W, int C, float* out, hipStream_t s,
            const char* name) {
    const long tiles = (long)N * cdiv(H, DW_TH) * cdiv(W, DW_TW);
    hipLaunchKernelGGL((dw7_kernel<FLIP, RES, G>), dim3(cdiv(tiles, 4), C / 64), dim3(WG), 0, s, in, wt, bias, res, N, H, W, C, out);
    GPH_CHECK(name);
    return 0;
}

int dw7_dwdb(const float* dy, const float* x, int N, int H, int W, int C, float* dw, float* db, Scratch& sc, hipStream_t s, const char* name) {
    const long rows = (long)N * H * W, keep = sc.used;
    const int chunk = dw7_chunk(rows), chunks = cdiv(rows, chunk);
    float* pw = sc.take((long)chunks * C * TAPS);
    float* pb = sc.take((long)chunks * C);
    if (!sc.dry) {
        hipLaunchKernelGGL(dw7_dw_kernel, dim3(C / 64, chunks), dim3(WG), 0, s, dy, x, H, W, C, rows, chunk, pw, pb);
        GPH_CHECK(name);
        hipLaunchKernelGGL(rows_merge_kernel, dim3(cdiv((long)C * TAPS, WG)), dim3(WG), 0, s, (const float*)pw, chunks, C * TAPS, dw);
        GPH_CHECK(name);
        hipLaunchKernelGGL(rows_merge_kernel, dim3(cdiv(C, WG)), dim3(WG), 0, s, (const float*)pb, chunks, C, db);
        GPH_CHECK(name);
    }
    sc.used = keep;
    return 0;
}

// ---------------------------------------------------------------------------------- patch conv
bool patch_ok(long N, long H, long W, long Cin, long Cout, long p) {
    return N > 0 && p >= 1 && p <= 16 && H > 0 && W > 0 && H % p == 0 && W % p == 0 && H <= 8192 && W <= 8192 && Cin > 0 && Cin <= 16384 &&
           Cout > 0 && Cout <= 16384 && rows_ok(N * (H / p) * (W / p)) && N * H * W * Cin < (1L << 40);
}
Patch patch_view(const float* x, int H, int W, int Cin, int p, int nchw) {
    if (nchw) return Patch{x, H / p, W / p, p, (long)Cin * H * W, (long)H * W, (long)W, 1};
    return Patch{x, H / p, W / p, p, (long)H * W * Cin, 1, (long)W * Cin, (long)Cin};
}

int patch_forward(const float* x, const float* w, const float* b, int N, int H, int W, int Cin, int Cout, int p, int nchw, float* y,
                  Scratch& sc, hipStream_t s, const char* name) {
    const long rows = (long)N * (H / p) * (W / p), K = (long)Cin * p * p;
    return gemm_s(patch_view(x, H, W, Cin, p, nchw), MatCol{w, K}, EpRow{y, Cout, b, 0, 0}, rows, Cout, K, sc, s, name);
}

int patch_backward(const float* dy, const float* x, const float* w, int N, int H, int W, int Cin, int Cout, int p, int nchw, float* dx,
                   float* dw, float* db, Scratch& sc, hipStream_t s, const char* name) {
    const long rows = (long)N * (H / p) * (W / p), K = (long)Cin * p * p;
    if (dx)      // (rows x Cout) (Cout x K), stored through the patch map
        GPH_TRY(gemm_s(MatRow{dy, Cout}, MatRow{w, K}, EpPatch{dx, patch_view(dx, H, W, Cin, p, nchw)}, rows, K, Cout, sc, s, name));
    if (dw)      // (Cout x rows) (rows x K)
        GPH_TRY(gemm_s(Tr<MatRow>{MatRow{dy, Cout}}, patch_view(x, H, W, Cin, p, nchw), EpRow{dw, K, nullptr, 0, 0}, Cout, K, rows, sc, s, name));
    if (db) GPH_TRY(colsum_s(MatRow{dy, Cout}, rows, Cout, db, sc, s, name));
    return 0;
}

// ---------------------------------------------------------------------------------- the block
bool block_ok(long N, long H, long W, long C) { return dw7_ok(N, H, W, C) && N * H * W * C * 4 < (1L << 40); }

const gpb_block_params NO_BLOCK = {};
bool block_complete(const gpb_block_params* p) {
    return p && p->gamma && p->dw_w && p->dw_b && p->ln_w && p->ln_b && p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b;
}

// out: rows (N H W, C), or (N,C,H,W) when out_nchw
int block_forward(const float* x, const gpb_block_params& p, int N, int H, int W, int C, float* dwout, float* mean, float* rstd, float* h,
                  float* y2, float* out, bool out_nchw, Scratch& sc, hipStream_t s, const char* name) {
    const long rows = (long)N * H * W, keep = sc.used;
    const int C4 = 4 * C;
    float* z = sc.take(rows * C);
    float* a = sc.take(rows * C4);
    if (!sc.dry) {
        GPH_TRY((dw7_run<false, false>(x, p.dw_w, p.dw_b, NoRes{}, N, H, W, C, dwout, s, name)));
        GPH_TRY(ln_forward(dwout, p.ln_w, p.ln_b, rows, C, z, mean, rstd, false, s, name));
    }
    GPH_TRY(gemm_p(MatRow{z, C}, MatCol{p.fc1_w, C}, EpFc1{h, a, C4, p.fc1_b}, rows, C4, C, sc, s, name));
    if (out_nchw)
        GPH_TRY(gemm_p(MatRow{a, C4}, MatCol{p.fc2_w, C4}, EpFc2<true>{y2, x, p.fc2_b, p.gamma, out, C, H * W}, rows, C, C4, sc, s, name));
    else
        GPH_TRY(gemm_p(MatRow{a, C4}, MatCol{p.fc2_w, C4}, EpFc2<false>{y2, x, p.fc2_b, p.gamma, out, C, H * W}, rows, C, C4, sc, s, name));
    sc.used = keep;
    return 0;
}

// g: the view of d out as rows x C (MatRow, or Nchw for the last block).  dx = g + (the depth-wise dX).
template <class G>
int block_backward(const G& g, const float* x, const gpb_block_params& p, const float* dwout, const float* mean, const float* rstd,
                   const float* h, const float* y2, int N, int H, int W, int C, const gpb_block_params& gr, float* dx, Scratch& sc,
                   hipStream_t s, const char* name) {
    const long rows = (long)N * H * W, keep = sc.used;
    const int C4 = 4 * C;
    float* a = sc.take(rows * C4);      // GELU(h), then d h
    float* z = sc.take(rows * C);       // LN(dwout), then d dwout
    float* dz = sc.take(rows * C);
    float* w2s = sc.take((long)C * C4);      // gamma[c] W2[c, :]
    if (!sc.dry) {
        hipLaunchKernelGGL(gelu_map_kernel, dim3(cdiv(rows * C4, WG)), dim3(WG), 0, s, h, rows * C4, a);
        GPH_CHECK(name);
        hipLaunchKernelGGL(scale_rows_kernel, dim3(cdiv((long)C * C4, WG)), dim3(WG), 0, s, p.fc2_w, p.gamma, (long)C * C4, C4, w2s);
        GPH_CHECK(name);
        GPH_TRY(ln_forward(dwout, p.ln_w, p.ln_b, rows, C, z, const_cast<float*>(mean), const_cast<float*>(rstd), true, s, name));
    }
    GPH_TRY(colsum_s(Prod<G>{g, y2, C}, rows, C, gr.gamma, sc, s, name));
    // fc2 with d y2 = g gamma never formed: the scale leaves the contractions, whose operands then stream under the MFMAs as plain
    // loads.  d W2 = gamma (g^T a) in the store functor, d b2 the row sum of g gamma, d h = g (gamma W2) GELU'(h) over a
    GPH_TRY(gemm_p(Tr<G>{g}, MatRow{a, C4}, EpRowScaleM{gr.fc2_w, C4, p.gamma}, C, C4, rows, sc, s, name));
    GPH_TRY(colsum_s(Scaled<G>{g, p.gamma}, rows, C, gr.fc2_b, sc, s, name));
    float* dh = a;
    GPH_TRY(gemm_p(g, MatRow{w2s, C4}, EpGeluBack{dh, h, C4}, rows, C4, C, sc, s, name));
    // fc1
    GPH_TRY(gemm_p(Tr<MatRow>{MatRow{dh, C4}}, MatRow{z, C}, EpRow{gr.fc1_w, C, nullptr, 0, 0}, C4, C, rows, sc, s, name));
    GPH_TRY(colsum_s(MatRow{dh, C4}, rows, C4, gr.fc1_b, sc, s, name));
    GPH_TRY(gemm_p(MatRow{dh, C4}, MatRow{p.fc1_w, C}, EpRow{dz, C, nullptr, 0, 0}, rows, C, C4, sc, s, name));
    // LayerNorm at the saved statistics, d dwout over z
    float* du = z;
    GPH_TRY(ln_backward(dz, dwout, mean, rstd, p.ln_w, rows, C, du, gr.ln_w, gr.ln_b, sc, s, name));
    // depth-wise: the parameter sums, then dx = g + gather
    GPH_TRY(dw7_dwdb(du, x, N, H, W, C, gr.dw_w, gr.dw_b, sc, s, name));
    if (!sc.dry) GPH_TRY((dw7_run<true, true>(du, p.dw_w, nullptr, g, N, H, W, C, dx, s, name)));
    sc.used = keep;
    return 0;
}

// ---------------------------------------------------------------------------------- the backbone
struct Net {
    int n, dims[GPB_MAX_STAGES], depths[GPB_MAX_STAGES], B, S;
    int side(int s) const { return S / (GPB_STEM_PATCH << s); }
    long rows(int s) const { return (long)B * side(s) * side(s); }
};

bool net_ok(const int* dims, const int* depths, int n, long B, long S, Net& net) {
    if (!dims || !depths || n < 1 || n > GPB_MAX_STAGES || B < 1 || S < 1 || S > 8192) return false;
    if (S % (GPB_STEM_PATCH << (n - 1))) return false;
    net.n = n;
    net.B = (int)B;
    net.S = (int)S;
    for (int s = 0; s < n; ++s) {
        if (!chan_ok(dims[s]) || depths[s] < 1 || depths[s] > 4096) return false;
        net.dims[s] = dims[s];
        net.depths[s] = depths[s];
    }
    for (int s = 0; s < n; ++s)
        if (!block_ok(B, net.side(s), net.side(s), dims[s])) return false;
    return patch_ok(B, S, S, STEM_CIN, dims[0], GPB_STEM_PATCH);
}

int param_count(const int* depths, int n) {
    if (!depths || n < 1 || n > GPB_MAX_STAGES) return 0;
    long c = 4;
    for (int s = 0; s < n; ++s) {
        if (depths[s] < 1 || depths[s] > 4096) return 0;
        c += (s ? 4 : 0) + 9L * depths[s];
    }
    return (int)c;
}
int saved_count(const Net& net) {
    int c = 0;
    for (int s = 0; s < net.n; ++s) c += 3 + 6 * net.depths[s];
    return c;
}
bool table_complete(float* const* t, int n) {
    if (!t) return false;
    for (int i = 0; i < n; ++i)
        if (!t[i]) return false;
    return true;
}

// walks of the tables: the offsets of stage s's downsample and of its first block
struct Walk {
    int down_p[GPB_MAX_STAGES], block_p[GPB_MAX_STAGES], down_s[GPB_MAX_STAGES], block_s[GPB_MAX_STAGES];
    explicit Walk(const Net& net) {
        int p = 4, v = 3;
        for (int s = 0; s < net.n; ++s) {
            down_p[s] = p;
            down_s[s] = v;
            if (s) p += 4, v += 3;
            block_p[s] = p;
            block_s[s] = v;
            p += 9 * net.depths[s];
            v += 6 * net.depths[s];
        }
    }
};
// in dry mode the tables are null: every pointer read from them is null and never dereferenced
template <class T> const T& entry(float* const* t, int at, const T& none) { return t ? *reinterpret_cast<const T*>(t + at) : none; }
const gpb_stem_params NO_STEM = {};
const gpb_down_params NO_DOWN = {};
const gpb_norm_saved NO_NORM = {};
const gpb_block_saved NO_BSAVED = {};

int net_forward(const float* img, float* const* P, const Net& net, float* const* V, float* feat, Scratch& sc, hipStream_t s, const char* name) {
    const Walk wk(net);
    const gpb_stem_params& st = entry(P, 0, NO_STEM);
    const gpb_norm_saved& sv = entry(V, 0, NO_NORM);
    GPH_TRY(patch_forward(img, st.conv_w, st.conv_b, net.B, net.S, net.S, STEM_CIN, net.dims[0], GPB_STEM_PATCH, 1, sv.pre, sc, s, name));
    if (!sc.dry) GPH_TRY(ln_forward(sv.pre, st.ln_w, st.ln_b, net.rows(0), net.dims[0], entry(V, wk.block_s[0], NO_BSAVED).x, sv.mean, sv.rstd, false, s, name));
    for (int st_i = 0; st_i < net.n; ++st_i) {
        const int C = net.dims[st_i], H = net.side(st_i);
        if (st_i) {
            const gpb_down_params& d = entry(P, wk.down_p[st_i], NO_DOWN);
            const gpb_norm_saved& dv = entry(V, wk.down_s[st_i], NO_NORM);
            const int Cp = net.dims[st_i - 1], Hp = net.side(st_i - 1);
            const long keep = sc.used;
            float* z = sc.take(net.rows(st_i - 1) * Cp);
            if (!sc.dry) GPH_TRY(ln_forward(dv.pre, d.ln_w, d.ln_b, net.rows(st_i - 1), Cp, z, dv.mean, dv.rstd, false, s, name));
            GPH_TRY(patch_forward(z, d.conv_w, d.conv_b, net.B, Hp, Hp, Cp, C, GPB_DOWN_PATCH, 0, entry(V, wk.block_s[st_i], NO_BSAVED).x, sc, s, name));
            sc.used = keep;
        }
        for (int b = 0; b < net.depths[st_i]; ++b) {
            const gpb_block_params& p = entry(P, wk.block_p[st_i] + 9 * b, NO_BLOCK);
            const gpb_block_saved& v = entry(V, wk.block_s[st_i] + 6 * b, NO_BSAVED);
            const bool last_of_stage = b == net.depths[st_i] - 1, last = last_of_stage && st_i == net.n - 1;
            // the block's output is the next block's input, the next downsample's pre-norm map, or feat
            float* out = last ? feat
                              : last_of_stage ? entry(V, wk.down_s[st_i + 1], NO_NORM).pre : entry(V, wk.block_s[st_i] + 6 * (b + 1), NO_BSAVED).x;
            GPH_TRY(block_forward(v.x, p, net.B, H, H, C, v.dwout, v.mean, v.rstd, v.h, v.y2, out, last, sc, s, name));
        }
    }
    return 0;
}

int net_backward(float* const* P, float* const* V, const float* img, const float* g_feat, const Net& net, float* const* Gr, float* d_img,
                 Scratch& sc, hipStream_t s, const char* name) {
    const Walk wk(net);
    // the gradient of a block's input is the upstream gradient of what came before it: two buffers of the largest map
    long biggest = 0;
    for (int st_i = 0; st_i < net.n; ++st_i) biggest = max2(biggest, net.rows(st_i) * net.dims[st_i]);
    float* buf[2] = {sc.take(biggest), sc.take(biggest)};
    int cur = 0;
    bool first = true;
    for (int st_i = net.n - 1; st_i >= 0; --st_i) {
        const int C = net.dims[st_i], H = net.side(st_i);
        for (int b = net.depths[st_i] - 1; b >= 0; --b) {
            const gpb_block_params &p = entry(P, wk.block_p[st_i] + 9 * b, NO_BLOCK), &g = entry(Gr, wk.block_p[st_i] + 9 * b, NO_BLOCK);
            const gpb_block_saved& v = entry(V, wk.block_s[st_i] + 6 * b, NO_BSAVED);
            if (first)
                GPH_TRY(block_backward(Nchw{g_feat, C, H * H}, v.x, p, v.dwout, v.mean, v.rstd, v.h, v.y2, net.B, H, H, C, g, buf[cur], sc, s, name));
            else
                GPH_TRY(block_backward(MatRow{buf[cur ^ 1], C}, v.x, p, v.dwout, v.mean, v.rstd, v.h, v.y2, net.B, H, H, C, g, buf[cur], sc, s, name));
            first = false;
            cur ^= 1;
        }
        const float* gin = buf[cur ^ 1];      // d (the stage's first block input), rows x C
        if (st_i) {
            const gpb_down_params &d = entry(P, wk.down_p[st_i], NO_DOWN), &g = entry(Gr, wk.down_p[st_i], NO_DOWN);
            const gpb_norm_saved& dv = entry(V, wk.down_s[st_i], NO_NORM);
            const int Cp = net.dims[st_i - 1], Hp = net.side(st_i - 1);
            const long rp = net.rows(st_i - 1), keep = sc.used;
            float* z = sc.take(rp * Cp);
            float* dz = sc.take(rp * Cp);
            if (!sc.dry) GPH_TRY(ln_forward(dv.pre, d.ln_w, d.ln_b, rp, Cp, z, dv.mean, dv.rstd, true, s, name));
            GPH_TRY(patch_backward(gin, z, d.conv_w, net.B, Hp, Hp, Cp, C, GPB_DOWN_PATCH, 0, dz, g.conv_w, g.conv_b, sc, s, name));
            GPH_TRY(ln_backward(dz, dv.pre, dv.mean, dv.rstd, d.ln_w, rp, Cp, buf[cur], g.ln_w, g.ln_b, sc, s, name));
            sc.used = keep;
            cur ^= 1;
        } else {
            const gpb_stem_params &t = entry(P, 0, NO_STEM), &g = entry(Gr, 0, NO_STEM);
            const gpb_norm_saved& tv = entry(V, 0, NO_NORM);
            GPH_TRY(ln_backward(gin, tv.pre, tv.mean, tv.rstd, t.ln_w, net.rows(0), C, buf[cur], g.ln_w, g.ln_b, sc, s, name));
            GPH_TRY(patch_backward(buf[cur], img, t.conv_w, net.B, net.S, net.S, STEM_CIN, C, GPB_STEM_PATCH, 1, d_img, g.conv_w, g.conv_b, sc, s, name));
        }
    }
    return 0;
}

// the second pass of an entry point: the dry pass gave `need`
#define GPB_WS_CHECK(dry, ws, ws_bytes, name)                                                                                   \
    GP_REQUIRE((dry).need == 0 || ((ws) && aligned256(ws) && (ws_bytes) / 4 >= (dry).need),                                      \
               "%s: workspace missing, unaligned or too small (%lld bytes, %ld needed)", name, (long long)(ws_bytes), 4 * (dry).need)

// ---------------------------------------------------------------------------------- the entry points of the block and the backbone
// One body serves the fp32 entry point and its precision-taking form: `name` is the caller's, `prec` a GPB_PREC_* value.
long long block_workspace(int N, int H, int W, int C, int prec) {
    if (!block_ok(N, H, W, C) || !prec_ok(prec)) return 0;
    Scratch d(nullptr, 0, true, prec);
    block_forward(nullptr, NO_BLOCK, N, H, W, C, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false, d, nullptr, "");
    block_backward(MatRow{nullptr, C}, nullptr, NO_BLOCK, nullptr, nullptr, nullptr, nullptr, nullptr, N, H, W, C, NO_BLOCK, nullptr, d, nullptr, "");
    return 4LL * d.need;
}

int block_forward_save(const float* x, const gpb_block_params* params, int N, int H, int W, int C, float* dwout, float* mean, float* rstd,
                       float* h, float* y2, float* out, void* ws, long long ws_bytes, void* stream, int prec, const char* name) {
    GP_REQUIRE(prec_ok(prec), "%s: unknown precision %d (GPB_PREC_F32 or GPB_PREC_BF16)", name, prec);
    GP_REQUIRE(x && block_complete(params) && dwout && mean && rstd && h && y2 && out, "%s: null pointer", name);
    GP_REQUIRE(block_ok(N, H, W, C), "%s: bad shape N %d H %d W %d C %d (C must be a multiple of 64)", name, N, H, W, C);
    GP_REQUIRE(ws && aligned256(ws) && ws_bytes >= block_workspace(N, H, W, C, prec), "%s: workspace missing, unaligned or too small", name);
    Scratch sc(ws, ws_bytes, false, prec);
    return block_forward(x, *params, N, H, W, C, dwout, mean, rstd, h, y2, out, false, sc, (hipStream_t)stream, name);
}

int block_backward_entry(const float* g, const float* x, const gpb_block_params* params, const float* dwout, const float* mean,
                         const float* rstd, const float* h, const float* y2, int N, int H, int W, int C, const gpb_block_params* grads,
                         float* dx, void* ws, long long ws_bytes, void* stream, int prec, const char* name) {
    GP_REQUIRE(prec_ok(prec), "%s: unknown precision %d (GPB_PREC_F32 or GPB_PREC_BF16)", name, prec);
    GP_REQUIRE(g && x && block_complete(params) && dwout && mean && rstd && h && y2 && block_complete(grads) && dx, "%s: null pointer", name);
    GP_REQUIRE(dx != g, "%s: dx must not alias g", name);
    GP_REQUIRE(block_ok(N, H, W, C), "%s: bad shape N %d H %d W %d C %d (C must be a multiple of 64)", name, N, H, W, C);
    GP_REQUIRE(ws && aligned256(ws) && ws_bytes >= block_workspace(N, H, W, C, prec), "%s: workspace missing, unaligned or too small", name);
    Scratch sc(ws, ws_bytes, false, prec);
    return block_backward(MatRow{g, C}, x, *params, dwout, mean, rstd, h, y2, N, H, W, C, *grads, dx, sc, (hipStream_t)stream, name);
}

long long backbone_forward_workspace(const int* dims, const int* depths, int n_stages, int B, int S, int prec) {
    Net net;
    if (!net_ok(dims, depths, n_stages, B, S, net) || !prec_ok(prec)) return 0;
    Scratch d(nullptr, 0, true, prec);
    net_forward(nullptr, nullptr, net, nullptr, nullptr, d, nullptr, "");
    return 4LL * d.need;
}

int backbone_forward_save(const float* img, float* const* params, const int* dims, const int* depths, int n_stages, int B, int S,
                          float* const* saved, float* feat, void* ws, long long ws_bytes, void* stream, int prec, const char* name) {
    Net net;
    GP_REQUIRE(prec_ok(prec), "%s: unknown precision %d (GPB_PREC_F32 or GPB_PREC_BF16)", name, prec);
    if (dims)
        for (int s = 0; s < n_stages && s < GPB_MAX_STAGES; ++s)
            GP_REQUIRE(dims[s] > 0 && dims[s] % 64 == 0, "%s: dims[%d] = %d is not a multiple of 64", name, s, dims[s]);
    GP_REQUIRE(net_ok(dims, depths, n_stages, B, S, net), "%s: bad configuration (stages %d B %d S %d)", name, n_stages, B, S);
    GP_REQUIRE(img && feat && table_complete(params, param_count(depths, n_stages)) && table_complete(saved, saved_count(net)),
               "%s: null pointer", name);
    GP_REQUIRE(ws && aligned256(ws) && ws_bytes >= backbone_forward_workspace(dims, depths, n_stages, B, S, prec),
               "%s: workspace missing, unaligned or too small", name);
    Scratch sc(ws, ws_bytes, false, prec);
    return net_forward(img, params, net, saved, feat, sc, (hipStream_t)stream, name);
}

long long backbone_backward_workspace(const int* dims, const int* depths, int n_stages, int B, int S, int prec) {
    Net net;
    if (!net_ok(dims, depths, n_stages, B, S, net) || !prec_ok(prec)) return 0;
    Scratch d(nullptr, 0, true, prec);
    net_backward(nullptr, nullptr, nullptr, nullptr, net, nullptr, nullptr, d, nullptr, "");
    return 4LL * d.need;
}

int backbone_backward_entry(float* const* params, float* const* saved, const float* img, const float* g_feat, const int* dims,
                            const int* depths, int n_stages, int B, int S, float* const* grads, float* d_img, void* ws, long long ws_bytes,
                            void* stream, int prec, const char* name) {
    Net net;
    GP_REQUIRE(prec_ok(prec), "%s: unknown precision %d (GPB_PREC_F32 or GPB_PREC_BF16)", name, prec);
    if (dims)
        for (int s = 0; s < n_stages && s < GPB_MAX_STAGES; ++s)
            GP_REQUIRE(dims[s] > 0 && dims[s] % 64 == 0, "%s: dims[%d] = %d is not a multiple of 64", name, s, dims[s]);
    GP_REQUIRE(net_ok(dims, depths, n_stages, B, S, net), "%s: bad configuration (stages %d B %d S %d)", name, n_stages, B, S);
    const int np = param_count(depths, n_stages);
    GP_REQUIRE(img && g_feat && d_img && table_complete(params, np) && table_complete(grads, np) && table_complete(saved, saved_count(net)),
               "%s: null pointer", name);
    GP_REQUIRE(ws && aligned256(ws) && ws_bytes >= backbone_backward_workspace(dims, depths, n_stages, B, S, prec),
               "%s: workspace missing, unaligned or too small", name);
    Scratch sc(ws, ws_bytes, false, prec);
    return net_backward(params, saved, img, g_feat, net, grads, d_img, sc, (hipStream_t)stream, name);
}

}  // namespace

extern "C" {

int gpb_dw7_forward(const float* x, const float* w, const float* b, int N, int H, int W, int C, float* y, void* stream) {
    const char* name = "gpb_dw7_forward";
    GP_REQUIRE(x && w && b && y, "%s: null pointer", name);
    GP_REQUIRE(dw7_ok(N, H, W, C), "%s: bad shape N %d H %d W %d C %d (C must be a multiple of 64)", name, N, H, W, C);
    return dw7_run<false, false>(x, w, b, NoRes{}, N, H, W, C, y, (hipStream_t)stream, name);
}

long long gpb_dw7_backward_workspace(int N, int H, int W, int C) {
    if (!dw7_ok(N, H, W, C)) return 0;
    Scratch d(nullptr, 0, true);
    dw7_dwdb(nullptr, nullptr, N, H, W, C, nullptr, nullptr, d, nullptr, "");
    return 4LL * d.need;
}

int gpb_dw7_backward(const float* dy, const float* x, const float* w, int N, int H, int W, int C, float* dx, float* dw, float* db, void* ws,
                     long long ws_bytes, void* stream) {
    const char* name = "gpb_dw7_backward";
    GP_REQUIRE(dy && x && w && dx && dw && db, "%s: null pointer", name);
    GP_REQUIRE(dw7_ok(N, H, W, C), "%s: bad shape N %d H %d W %d C %d (C must be a multiple of 64)", name, N, H, W, C);
    Scratch d(nullptr, 0, true), sc(ws, ws_bytes, false);
    dw7_dwdb(nullptr, nullptr, N, H, W, C, nullptr, nullptr, d, nullptr, name);
    GPB_WS_CHECK(d, ws, ws_bytes, name);
    GPH_TRY(dw7_dwdb(dy, x, N, H, W, C, dw, db, sc, (hipStream_t)stream, name));
    return dw7_run<true, false>(dy, w, nullptr, NoRes{}, N, H, W, C, dx, (hipStream_t)stream, name);
}

int gpb_layernorm_forward_save(const float* x, const float* w, const float* b, int rows, int C, float* y, float* mean, float* rstd,
                               void* stream) {
    const char* name = "gpb_layernorm_forward_save";
    GP_REQUIRE(x && w && b && y && mean && rstd, "%s: null pointer", name);
    GP_REQUIRE(rows_ok(rows) && chan_ok(C), "%s: bad shape rows %d C %d (C must be a multiple of 64)", name, rows, C);
    return ln_forward(x, w, b, rows, C, y, mean, rstd, false, (hipStream_t)stream, name);
}

long long gpb_layernorm_backward_workspace(int rows, int C) {
    if (!rows_ok(rows) || !chan_ok(C)) return 0;
    Scratch d(nullptr, 0, true);
    ln_backward(nullptr, nullptr, nullptr, nullptr, nullptr, rows, C, nullptr, nullptr, nullptr, d, nullptr, "");
    return 4LL * d.need;
}

int gpb_layernorm_backward(const float* dy, const float* x, const float* mean, const float* rstd, const float* w, int rows, int C,
                           float* dx, float* dw, float* db, void* ws, long long ws_bytes, void* stream) {
    const char* name = "gpb_layernorm_backward";
    GP_REQUIRE(dy && x && mean && rstd && w && dx && dw && db, "%s: null pointer", name);
    GP_REQUIRE(dx != dy && dx != x, "%s: dx must not alias dy or x", name);
    GP_REQUIRE(rows_ok(rows) && chan_ok(C), "%s: bad shape rows %d C %d (C must be a multiple of 64)", name, rows, C);
    Scratch d(nullptr, 0, true), sc(ws, ws_bytes, false);
    ln_backward(nullptr, nullptr, nullptr, nullptr, nullptr, rows, C, nullptr, nullptr, nullptr, d, nullptr, name);
    GPB_WS_CHECK(d, ws, ws_bytes, name);
    return ln_backward(dy, x, mean, rstd, w, rows, C, dx, dw, db, sc, (hipStream_t)stream, name);
}

long long gpb_patch_conv_workspace(int N, int H, int W, int Cin, int Cout, int p, int nchw) {
    if (!patch_ok(N, H, W, Cin, Cout, p)) return 0;
    Scratch d(nullptr, 0, true);
    float one;
    patch_forward(nullptr, nullptr, nullptr, N, H, W, Cin, Cout, p, nchw, nullptr, d, nullptr, "");
    patch_backward(nullptr, nullptr, nullptr, N, H, W, Cin, Cout, p, nchw, &one, &one, &one, d, nullptr, "");
    return 4LL * d.need;
}

int gpb_patch_conv_forward(const float* x, const float* w, const float* b, int N, int H, int W, int Cin, int Cout, int p, int nchw,
                           float* y, void* ws, long long ws_bytes, void* stream) {
    const char* name = "gpb_patch_conv_forward";
    GP_REQUIRE(x && w && y, "%s: null pointer", name);
    GP_REQUIRE(patch_ok(N, H, W, Cin, Cout, p), "%s: bad shape N %d H %d W %d Cin %d Cout %d p %d", name, N, H, W, Cin, Cout, p);
    Scratch d(nullptr, 0, true), sc(ws, ws_bytes, false);
    patch_forward(x, w, b, N, H, W, Cin, Cout, p, nchw, y, d, nullptr, name);
    GPB_WS_CHECK(d, ws, ws_bytes, name);
    return patch_forward(x, w, b, N, H, W, Cin, Cout, p, nchw, y, sc, (hipStream_t)stream, name);
}

int gpb_patch_conv_backward(const float* dy, const float* x, const float* w, int N, int H, int W, int Cin, int Cout, int p, int nchw,
                            float* dx, float* dw, float* db, void* ws, long long ws_bytes, void* stream) {
    const char* name = "gpb_patch_conv_backward";
    GP_REQUIRE(dy && patch_ok(N, H, W, Cin, Cout, p), "%s: bad arguments (N %d H %d W %d Cin %d Cout %d p %d)", name, N, H, W, Cin, Cout, p);
    GP_REQUIRE((!dw || x) && (!dx || w), "%s: dw needs x, dx needs the weights", name);
    Scratch d(nullptr, 0, true), sc(ws, ws_bytes, false);
    patch_backward(dy, x, w, N, H, W, Cin, Cout, p, nchw, dx, dw, db, d, nullptr, name);
    GPB_WS_CHECK(d, ws, ws_bytes, name);
    return patch_backward(dy, x, w, N, H, W, Cin, Cout, p, nchw, dx, dw, db, sc, (hipStream_t)stream, name);
}

long long gpb_block_workspace(int N, int H, int W, int C) { return block_workspace(N, H, W, C, GPB_PREC_F32); }

int gpb_block_forward_save(const float* x, const gpb_block_params* params, int N, int H, int W, int C, float* dwout, float* mean,
                           float* rstd, float* h, float* y2, float* out, void* ws, long long ws_bytes, void* stream) {
    return block_forward_save(x, params, N, H, W, C, dwout, mean, rstd, h, y2, out, ws, ws_bytes, stream, GPB_PREC_F32, "gpb_block_forward_save");
}

int gpb_block_backward(const float* g, const float* x, const gpb_block_params* params, const float* dwout, const float* mean,
                       const float* rstd, const float* h, const float* y2, int N, int H, int W, int C, const gpb_block_params* grads,
                       float* dx, void* ws, long long ws_bytes, void* stream) {
    return block_backward_entry(g, x, params, dwout, mean, rstd, h, y2, N, H, W, C, grads, dx, ws, ws_bytes, stream, GPB_PREC_F32,
                                "gpb_block_backward");
}

int gpb_param_count(const int* depths, int n_stages) { return param_count(depths, n_stages); }

long long gpb_backbone_forward_workspace(const int* dims, const int* depths, int n_stages, int B, int S) {
    return backbone_forward_workspace(dims, depths, n_stages, B, S, GPB_PREC_F32);
}

int gpb_backbone_forward_save(const float* img, float* const* params, const int* dims, const int* depths, int n_stages, int B, int S,
                              float* const* saved, float* feat, void* ws, long long ws_bytes, void* stream) {
    return backbone_forward_save(img, params, dims, depths, n_stages, B, S, saved, feat, ws, ws_bytes, stream, GPB_PREC_F32,
                                 "gpb_backbone_forward_save");
}

long long gpb_backbone_backward_workspace(const int* dims, const int* depths, int n_stages, int B, int S) {
    return backbone_backward_workspace(dims, depths, n_stages, B, S, GPB_PREC_F32);
}

int gpb_backbone_backward(float* const* params, float* const* saved, const float* img, const float* g_feat, const int* dims,
                          const int* depths, int n_stages, int B, int S, float* const* grads, float* d_img, void* ws, long long ws_bytes,
                          void* stream) {
    return backbone_backward_entry(params, saved, img, g_feat, dims, depths, n_stages, B, S, grads, d_img, ws, ws_bytes, stream, GPB_PREC_F32,
                                   "gpb_backbone_backward");
}

/* ---- the precision-taking forms (include/givepose_bbgrad_bf16.h) ---- */

long long gpbm_matmul_bf16_workspace(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return 4LL * up64(gemm_bf16_ws_floats(M, N, K));
}

int gpbm_matmul_bf16(const float* a, const float* b, int M, int N, int K, int trans_a, int trans_b, float* c, void* ws, long long ws_bytes,
                     void* stream) {
    const char* name = "gpbm_matmul_bf16";
    GP_REQUIRE(a && b && c, "%s: null pointer", name);
    GP_REQUIRE(M > 0 && N > 0 && K > 0 && (long)M * N < (1L << 40) && (long)M * K < (1L << 40) && (long)K * N < (1L << 40),
               "%s: bad shape M %d N %d K %d", name, M, N, K);
    const long need = gemm_bf16_ws_floats(M, N, K);
    GP_REQUIRE(need == 0 || (ws && aligned256(ws) && ws_bytes / 4 >= need), "%s: workspace missing, unaligned or too small (%lld bytes, %ld needed)",
               name, ws_bytes, 4 * need);
    const EpRow ep{c, N, nullptr, 0, 0};
    float* w = (float*)ws;
    const long wf = (long)(ws_bytes / 4);
    hipStream_t s = (hipStream_t)stream;
    if (trans_a) {
        if (trans_b) return gemm_bf16(MatCol{a, M}, MatCol{b, K}, ep, M, N, K, w, wf, s, name);
        return gemm_bf16(MatCol{a, M}, MatRow{b, N}, ep, M, N, K, w, wf, s, name);
    }
    if (trans_b) return gemm_bf16(MatRow{a, K}, MatCol{b, K}, ep, M, N, K, w, wf, s, name);
    return gemm_bf16(MatRow{a, K}, MatRow{b, N}, ep, M, N, K, w, wf, s, name);
}

long long gpbm_block_workspace(int N, int H, int W, int C, int precision) { return block_workspace(N, H, W, C, precision); }

int gpbm_block_forward_save(const float* x, const gpb_block_params* params, int N, int H, int W, int C, float* dwout, float* mean,
                            float* rstd, float* h, float* y2, float* out, void* ws, long long ws_bytes, void* stream, int precision) {
    return block_forward_save(x, params, N, H, W, C, dwout, mean, rstd, h, y2, out, ws, ws_bytes, stream, precision, "gpbm_block_forward_save");
}

int gpbm_block_backward(const float* g, const float* x, const gpb_block_params* params, const float* dwout, const float* mean,
                        const float* rstd, const float* h, const float* y2, int N, int H, int W, int C, const gpb_block_params* grads,
                        float* dx, void* ws, long long ws_bytes, void* stream, int precision) {
    return block_backward_entry(g, x, params, dwout, mean, rstd, h, y2, N, H, W, C, grads, dx, ws, ws_bytes, stream, precision,
                                "gpbm_block_backward");
}

long long gpbm_backbone_forward_workspace(const int* dims, const int* depths, int n_stages, int B, int S, int precision) {
    return backbone_forward_workspace(dims, depths, n_stages, B, S, precision);
}

int gpbm_backbone_forward_save(const float* img, float* const* params, const int* dims, const int* depths, int n_stages, int B, int S,
                               float* const* saved, float* feat, void* ws, long long ws_bytes, void* stream, int precision) {
    return backbone_forward_save(img, params, dims, depths, n_stages, B, S, saved, feat, ws, ws_bytes, stream, precision,
                                 "gpbm_backbone_forward_save");
}

long long gpbm_backbone_backward_workspace(const int* dims, const int* depths, int n_stages, int B, int S, int precision) {
    return backbone_backward_workspace(dims, depths, n_stages, B, S, precision);
}

int gpbm_backbone_backward(float* const* params, float* const* saved, const float* img, const float* g_feat, const int* dims,
                           const int* depths, int n_stages, int B, int S, float* const* grads, float* d_img, void* ws, long long ws_bytes,
                           void* stream, int precision) {
    return backbone_backward_entry(params, saved, img, g_feat, dims, depths, n_stages, B, S, grads, d_img, ws, ws_bytes, stream, precision,
                                   "gpbm_backbone_backward");
}

}  // extern "C"
