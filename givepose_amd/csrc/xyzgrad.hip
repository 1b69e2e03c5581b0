// Coordinate-head backward family (include/givepose_xyzgrad.h, prefix gpx_): TopDownXyzHead forward-that-saves and its backward in
// fp32.
//
// Every contraction is a view on the functor GEMM of grad_gemm.hpp.  The stride-1 conv adds one operand view (WindowS1, plain or
// with the taps flipped); the transposed conv adds none: with oh = 2 ih - 1 + kh its forward is the stride-2 conv's dX gather
// (GatherDY) with the input in the role of dY, its dX is the stride-2 conv (Im2col) of dY, its dW the stride-2 conv's dW with the
// operand roles exchanged -- and its (Cin,Cout,3,3) weight is the OIHW weight of that stride-2 conv as it stands, so WeightDx,
// MatCol and EpRow address it and its gradient directly.
//
// Precision (include/givepose_xyzgrad_bf16.h, gpxm_*): the 21 contractions of the 3x3 layers go through gemm_px (xyz_conv_prec.hpp), which
// runs the fp32 chain or, for GPX_PREC_BF16, the bf16-operand form of the same functor GEMM with the same views and store functors.  The
// 1x1 output conv, GroupNorm + GELU, the bilinear x2 and every reduction are fp32 in both.  The gpx_ entry points are the same bodies at
// GPX_PREC_F32.
#include "grad_gemm.hpp"
#include "xyz_conv_prec.hpp"
#include "../../include/givepose_xyzgrad.h"

namespace {

constexpr int FEAT = GPX_FEAT, GROUPS = GPX_GROUPS, LAYERS = GPX_LAYERS;

// ---------------------------------------------------------------------------------- views and stores of this family
// WindowS1, the view of the stride-1 conv, lives in xyz_conv_prec.hpp
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

// ---------------------------------------------------------------------------------- 3x3 stride-1 pad-1 conv
long conv_s1_ws_floats(long B, long Cin, long Cout, long H, int prec) {
    const long m = B * H * H;
    return max2(gemm_px_ws_floats(prec, m, Cout, Cin * 9),
                max2(gemm_px_ws_floats(prec, Cout, Cin * 9, m), gemm_px_ws_floats(prec, m, Cin, Cout * 9)));
}
bool conv_shape_ok(long B, long Cin, long Cout, long H) {
    return B > 0 && Cin > 0 && Cout > 0 && H > 0 && H <= 4096 && B * H * H < (1L << 28) && Cin <= 65536 && Cout <= 65536;
}

int conv_s1_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, float* ws, long wf, hipStream_t s,
                    int prec, const char* name) {
    GP_REQUIRE(X && Wt && Y && conv_shape_ok(B, Cin, Cout, H), "%s: bad arguments (B %d Cin %d Cout %d H %d)", name, B, Cin, Cout, H);
    return gemm_px(prec, WindowS1{X, Cin, H, 0}, MatCol{Wt, (long)Cin * 9}, EpNchw{Y, Cout, H * H, nullptr}, (long)B * H * H, Cout,
                   (long)Cin * 9, ws, wf, s, name);
}

int conv_s1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW, float* ws,
                     long wf, hipStream_t s, int prec, const char* name) {
    GP_REQUIRE(dY && conv_shape_ok(B, Cin, Cout, H), "%s: bad arguments (B %d Cin %d Cout %d H %d)", name, B, Cin, Cout, H);
    GP_REQUIRE((!dW || X) && (!dX || Wt), "%s: dW needs X, dX needs the weights", name);
    if (dW)      // (Cout x m) (m x Cin 9), m = (b,oh,ow)
        GPH_TRY(gemm_px(prec, Tr<Nchw>{Nchw{dY, Cout, H * H}}, WindowS1{X, Cin, H, 0}, EpRow{dW, (long)Cin * 9, nullptr, 0, 0}, Cout,
                        (long)Cin * 9, (long)B * H * H, ws, wf, s, name));
    if (dX)      // ((b,ih,iw) x (co,kh,kw)) ((co,kh,kw) x ci)
        GPH_TRY(gemm_px(prec, WindowS1{dY, Cout, H, 1}, WeightDx{Wt, Cin}, EpNchw{dX, Cin, H * H, nullptr}, (long)B * H * H, Cin,
                        (long)Cout * 9, ws, wf, s, name));
    return 0;
}

// ---------------------------------------------------------------------------------- 3x3 stride-2 transposed conv
// X (B,Cin,H,H), Wt (Cin,Cout,3,3), Y (B,Cout,2H,2H).  In the stride-2 conv that maps Y's shape to X's, Wt is the OIHW weight.
long deconv_ws_floats(long B, long Cin, long Cout, long H, int prec) {
    const long m = B * H * H;
    return max2(gemm_px_ws_floats(prec, 4 * m, Cout, Cin * 9),
                max2(gemm_px_ws_floats(prec, m, Cin, Cout * 9), gemm_px_ws_floats(prec, Cin, Cout * 9, m)));
}

int deconv_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, float* ws, long wf, hipStream_t s,
                   int prec, const char* name) {
    GP_REQUIRE(X && Wt && Y && conv_shape_ok(B, Cin, Cout, 2L * H), "%s: bad arguments (B %d Cin %d Cout %d H %d)", name, B, Cin, Cout, H);
    return gemm_px(prec, GatherDY{X, Cin, 2 * H, H}, WeightDx{Wt, Cout}, EpNchw{Y, Cout, 4 * H * H, nullptr}, (long)B * 4 * H * H, Cout,
                   (long)Cin * 9, ws, wf, s, name);
}

int deconv_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW, float* ws,
                    long wf, hipStream_t s, int prec, const char* name) {
    GP_REQUIRE(dY && conv_shape_ok(B, Cin, Cout, 2L * H), "%s: bad arguments (B %d Cin %d Cout %d H %d)", name, B, Cin, Cout, H);
    GP_REQUIRE((!dW || X) && (!dX || Wt), "%s: dW needs X, dX needs the weights", name);
    if (dW)      // (Cin x m) (m x Cout 9), m = (b,ih,iw): rows (ci), columns (co,kh,kw) -- the weight's own order
        GPH_TRY(gemm_px(prec, Tr<Nchw>{Nchw{X, Cin, H * H}}, Im2col{dY, Cout, 2 * H, H}, EpRow{dW, (long)Cout * 9, nullptr, 0, 0}, Cin,
                        (long)Cout * 9, (long)B * H * H, ws, wf, s, name));
    if (dX)      // ((b,ih,iw) x (co,kh,kw)) ((co,kh,kw) x ci)
        GPH_TRY(gemm_px(prec, Im2col{dY, Cout, 2 * H, H}, MatCol{Wt, (long)Cout * 9}, EpNchw{dX, Cin, H * H, nullptr}, (long)B * H * H, Cin,
                        (long)Cout * 9, ws, wf, s, name));
    return 0;
}

// ---------------------------------------------------------------------------------- GroupNorm + GELU
// One workgroup per (crop, group); wave w owns the group's channels w, w + 4, ...: HW adjacent floats each.  Sums: each lane its
// elements in turn, the xor tree of group_sum over the wave, a wave's channels in turn, the four waves as (w0 + w1) + (w2 + w3).
__device__ __forceinline__ float four_waves(float* sh, float v, int wave, int lane) {
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// the pre-activation, formed in one place for the forward and the backward
__device__ __forceinline__ float gn_pre(float x, float mu, float rs, float ga, float be) { return fmaf((x - mu) * rs, ga, be); }
__device__ __forceinline__ float gelu_value(float u) { return 0.5f * u * (1.0f + erff(u * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_slope(float u) {      // Phi(u) + u phi(u)
    const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * expf(-0.5f * u * u);
    return fmaf(u, pdf, cdf);
}

__global__ __launch_bounds__(WG) void gn_gelu_forward_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
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
        for (int i = lane; i < HW; i += 64) out[base + i] = gelu_value(gn_pre(x[base + i], mu, rs, ga, be));
    }
}

// First pass: dy = dout GELU'(u) goes to dx, and the sums.  Second pass (the same thread rereads what it wrote): the three terms.
__global__ __launch_bounds__(WG) void gn_gelu_backward_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, int C, int HW,
                                                              int G, float* dx, float* __restrict__ pgamma, float* __restrict__ pbeta) {
    __shared__ float sh[4];
    const int cpg = C / G, b = blockIdx.x / G, g = blockIdx.x - b * G, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long gbase = ((long)b * C + (long)g * cpg) * HW;
    const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x];
    float a1 = 0.0f, a2 = 0.0f;      // this wave's part of sum dxhat and sum dxhat xhat
    for (int ch = wave; ch < cpg; ch += 4) {
        const int c = g * cpg + ch;
        const float ga = gamma[c], be = beta[c];
        const long base = gbase + (long)ch * HW;
        float sdy = 0.0f, sdx = 0.0f;
        for (int i = lane; i < HW; i += 64) {
            const float xv = x[base + i];
            const float dy = dout[base + i] * gelu_slope(gn_pre(xv, mu, rs, ga, be));
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
    const float m1 = four_waves(sh, a1, wave, lane) * inv_n;      // mean of dxhat over the group
    const float m2 = four_waves(sh, a2, wave, lane) * inv_n;      // mean of dxhat xhat
    for (int ch = wave; ch < cpg; ch += 4) {
        const float ga = gamma[g * cpg + ch];
        const long base = gbase + (long)ch * HW;
        for (int i = lane; i < HW; i += 64) {
            const float xh = (x[base + i] - mu) * rs;
            dx[base + i] = rs * ((dx[base + i] * ga - m1) - xh * m2);
        }
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
bool gn_shape_ok(long B, long C, long HW, long G) {
    return B > 0 && C > 0 && HW > 0 && G > 0 && C % G == 0 && B * G < (1L << 30) && HW < (1L << 28) && C <= 65536;
}

int gn_gelu_forward(const float* x, const float* gamma, const float* beta, int B, int C, int HW, int G, float* out, float* mean, float* rstd,
                    hipStream_t s, const char* name) {
    GP_REQUIRE(x && gamma && beta && out && mean && rstd && gn_shape_ok(B, C, HW, G), "%s: bad GroupNorm arguments", name);
    hipLaunchKernelGGL(gn_gelu_forward_kernel, dim3(B * G), dim3(WG), 0, s, x, gamma, beta, C, HW, G, out, mean, rstd);
    GPH_CHECK(name);
    return 0;
}

int gn_gelu_backward(const float* dout, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, int B,
                     int C, int HW, int G, float* dx, float* dgamma, float* dbeta, float* ws, long wf, hipStream_t s, const char* name) {
    GP_REQUIRE(dout && x && mean && rstd && gamma && beta && dx, "%s: null pointer", name);
    GP_REQUIRE(gn_shape_ok(B, C, HW, G), "%s: bad shape B %d C %d HW %d G %d", name, B, C, HW, G);
    GP_REQUIRE(ws && wf >= gn_bwd_ws_floats(B, C), "%s: workspace too small", name);
    float *pg = ws, *pb = ws + up64((long)B * C);
    hipLaunchKernelGGL(gn_gelu_backward_kernel, dim3(B * G), dim3(WG), 0, s, dout, x, mean, rstd, gamma, beta, C, HW, G, dx, pg, pb);
    GPH_CHECK(name);
    hipLaunchKernelGGL(gn_param_reduce_kernel, dim3(cdiv(C, WG)), dim3(WG), 0, s, (const float*)pg, (const float*)pb, B, C, dgamma, dbeta);
    GPH_CHECK(name);
    return 0;
}

// ---------------------------------------------------------------------------------- bilinear x2, align_corners = True
// Output index o of 2H reads input i0 with weight 1 - frac and i0 + 1 with weight frac, where o (H - 1) / (2H - 1) = i0 + frac
// in fp32 as torch forms it; at the last input index there is no second tap (frac 0).
__device__ __forceinline__ void up_source(int o, int H, int& i0, float& frac) {
    const float scale = H > 1 ? (float)(H - 1) / (float)(2 * H - 1) : 0.0f;
    const float s = scale * (float)o;
    i0 = (int)s;
    frac = s - (float)i0;
    if (i0 >= H - 1) {
        i0 = H - 1;
        frac = 0.0f;
    }
}

__global__ __launch_bounds__(WG) void upsample_forward_kernel(const float* __restrict__ x, long total, int H, float* __restrict__ y) {
    const long idx = (long)blockIdx.x * WG + threadIdx.x;
    if (idx >= total) return;
    const int Ho = 2 * H, ow = (int)(idx % Ho), oh = (int)(idx / Ho % Ho);
    const long plane = idx / ((long)Ho * Ho);
    int h0, w0;
    float fh, fw;
    up_source(oh, H, h0, fh);
    up_source(ow, H, w0, fw);
    const int h1 = min(h0 + 1, H - 1), w1 = min(w0 + 1, H - 1);
    const float* p = x + plane * H * H;
    const float top = (1.0f - fw) * p[h0 * H + w0] + fw * p[h0 * H + w1];
    const float bot = (1.0f - fw) * p[h1 * H + w0] + fw * p[h1 * H + w1];
    y[idx] = (1.0f - fh) * top + fh * bot;
}

// weight of input index i in output index o (0 when o is outside the map or has no tap at i)
__device__ __forceinline__ float up_weight(int o, int i, int H) {
    if (o < 0 || o >= 2 * H) return 0.0f;
    int i0;
    float f;
    up_source(o, H, i0, f);
    return i0 == i ? 1.0f - f : (i0 + 1 == i ? f : 0.0f);
}

// o (H - 1) / (2H - 1) lies in [o / 2 - 1 / 2, o / 2], so the outputs with a tap at i are among 2 i - 2 .. 2 i + 3
constexpr int UP_CAND = 6;
__global__ __launch_bounds__(WG) void upsample_backward_kernel(const float* __restrict__ dy, long total, int H, float* __restrict__ dx) {
    const long idx = (long)blockIdx.x * WG + threadIdx.x;
    if (idx >= total) return;
    const int iw = (int)(idx % H), ih = (int)(idx / H % H), Ho = 2 * H;
    const long plane = idx / ((long)H * H);
    float wh[UP_CAND], ww[UP_CAND];
#pragma unroll
    for (int j = 0; j < UP_CAND; ++j) {
        wh[j] = up_weight(2 * ih - 2 + j, ih, H);
        ww[j] = up_weight(2 * iw - 2 + j, iw, H);
    }
    const float* p = dy + plane * Ho * Ho;
    float acc = 0.0f;
#pragma unroll
    for (int jh = 0; jh < UP_CAND; ++jh) {
        if (wh[jh] == 0.0f) continue;
        const int oh = 2 * ih - 2 + jh;
#pragma unroll
        for (int jw = 0; jw < UP_CAND; ++jw)
            if (ww[jw] != 0.0f) acc = fmaf(wh[jh] * ww[jw], p[oh * Ho + 2 * iw - 2 + jw], acc);
    }
    dx[idx] = acc;
}

bool up_shape_ok(long B, long C, long H) { return B > 0 && C > 0 && H > 0 && H <= 8192 && B * C < (1L << 31) && B * C * H * H < (1L << 36); }

int upsample_forward(const float* x, int B, int C, int H, float* y, hipStream_t s, const char* name) {
    GP_REQUIRE(x && y && up_shape_ok(B, C, H), "%s: bad upsample arguments (B %d C %d H %d)", name, B, C, H);
    const long total = (long)B * C * 4 * H * H;
    hipLaunchKernelGGL(upsample_forward_kernel, dim3(cdiv(total, WG)), dim3(WG), 0, s, x, total, H, y);
    GPH_CHECK(name);
    return 0;
}
int upsample_backward(const float* dy, int B, int C, int H, float* dx, hipStream_t s, const char* name) {
    GP_REQUIRE(dy && dx && up_shape_ok(B, C, H), "%s: bad upsample arguments (B %d C %d H %d)", name, B, C, H);
    const long total = (long)B * C * H * H;
    hipLaunchKernelGGL(upsample_backward_kernel, dim3(cdiv(total, WG)), dim3(WG), 0, s, dy, total, H, dx);
    GPH_CHECK(name);
    return 0;
}

// ---------------------------------------------------------------------------------- 1x1 conv with bias
__global__ __launch_bounds__(WG) void conv1x1_dx_kernel(const float* __restrict__ dY, const float* __restrict__ Wt, long total, int Cin,
                                                        int Cout, int HW, float* __restrict__ dX) {
    const long idx = (long)blockIdx.x * WG + threadIdx.x;
    if (idx >= total) return;
    const int px = (int)(idx % HW), c = (int)(idx / HW % Cin);
    const long b = idx / ((long)HW * Cin);
    float v = 0.0f;
    for (int o = 0; o < Cout; ++o) v = fmaf(dY[(b * Cout + o) * HW + px], Wt[(long)o * Cin + c], v);
    dX[idx] = v;
}

// db[o]: one workgroup per o; each thread its pixels (b, px) in turn, the xor tree, the four waves in order
__global__ __launch_bounds__(WG) void conv1x1_db_kernel(const float* __restrict__ dY, int B, int Cout, int HW, float* __restrict__ db) {
    __shared__ float sh[4];
    const int o = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s = 0.0f;
    for (int b = 0; b < B; ++b) {
        const float* p = dY + ((long)b * Cout + o) * HW;
        for (int i = threadIdx.x; i < HW; i += WG) s += p[i];
    }
    const float v = four_waves(sh, group_sum(s, 64), wave, lane);
    if (threadIdx.x == 0) db[o] = v;
}

bool conv1x1_shape_ok(long B, long Cin, long Cout, long HW) {
    return B > 0 && Cin > 0 && Cout > 0 && Cout <= 64 && HW > 0 && B * HW < (1L << 30) && Cin <= 65536;
}
long conv1x1_fwd_ws_floats(long B, long Cin, long Cout, long HW) { return gemm_ws_floats(B * HW, Cout, Cin); }
long conv1x1_bwd_ws_floats(long B, long Cin, long Cout, long HW) { return gemm_ws_floats(Cout, Cin, B * HW); }

int conv1x1_forward(const float* X, const float* Wt, const float* bias, int B, int Cin, int Cout, int HW, float* Y, float* ws, long wf,
                    hipStream_t s, const char* name) {
    return gemm(Nchw{X, Cin, HW}, MatCol{Wt, Cin}, EpNchwBias{Y, Cout, HW, bias}, (long)B * HW, Cout, Cin, ws, wf, s, name);
}

int conv1x1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int HW, float* dX, float* dW, float* db,
                     float* ws, long wf, hipStream_t s, const char* name) {
    GP_REQUIRE(dY && conv1x1_shape_ok(B, Cin, Cout, HW), "%s: bad arguments (B %d Cin %d Cout %d HW %d)", name, B, Cin, Cout, HW);
    GP_REQUIRE((!dW || X) && (!dX || Wt), "%s: dW needs X, dX needs the weights", name);
    if (dX) {
        const long total = (long)B * Cin * HW;
        hipLaunchKernelGGL(conv1x1_dx_kernel, dim3(cdiv(total, WG)), dim3(WG), 0, s, dY, Wt, total, Cin, Cout, HW, dX);
        GPH_CHECK(name);
    }
    if (dW)      // (Cout x m) (m x Cin), m = (b, pixel)
        GPH_TRY(gemm(Tr<Nchw>{Nchw{dY, Cout, HW}}, Nchw{X, Cin, HW}, EpRow{dW, Cin, nullptr, 0, 0}, Cout, Cin, (long)B * HW, ws, wf, s, name));
    if (db) {
        hipLaunchKernelGGL(conv1x1_db_kernel, dim3(Cout), dim3(WG), 0, s, dY, B, Cout, HW, db);
        GPH_CHECK(name);
    }
    return 0;
}

// ---------------------------------------------------------------------------------- the head
constexpr int MUL[LAYERS] = {2, 2, 2, 4, 4, 8, 8};      // layer l runs at H0 * MUL[l]

bool params_complete(const gpx_xyz_params* p) {
    if (!p || !p->deconv_w || !p->out_w || !p->out_b) return false;
    for (int i = 0; i < 6; ++i)
        if (!p->conv_w[i]) return false;
    for (int i = 0; i < LAYERS; ++i)
        if (!p->gn_w[i] || !p->gn_b[i]) return false;
    return true;
}
bool saved_complete(const gpx_xyz_saved* v) {
    if (!v || !v->up[0] || !v->up[1] || !v->coor) return false;
    for (int i = 0; i < LAYERS; ++i)
        if (!v->pre[i] || !v->mean[i] || !v->rstd[i] || !v->act[i]) return false;
    return true;
}
bool head_shape_ok(long B, long Cin, long H0) { return B > 0 && B <= 4096 && Cin > 0 && Cin <= 8192 && H0 > 0 && H0 <= 64 && B * 64 * H0 * H0 < (1L << 28); }

long head_fwd_ws_floats(long B, long Cin, long H0, int prec) {
    long w = gemm_px_ws_floats(prec, B * 4 * H0 * H0, FEAT, Cin * 9);
    for (int l = 1; l < LAYERS; ++l) w = max2(w, gemm_px_ws_floats(prec, B * MUL[l] * MUL[l] * H0 * H0, FEAT, FEAT * 9));
    w = max2(w, conv1x1_fwd_ws_floats(B, FEAT, 3, 64 * H0 * H0));
    return up64(w);
}

// the backward's workspace: two maps of the largest size, which every step reads one of and writes the other, and the scratch
struct BwdLayout {
    long p, q, scratch, scratch_floats, total;
};
BwdLayout bwd_layout(long B, long Cin, long H0, int prec) {
    BwdLayout L;
    const long big = up64(B * FEAT * 64 * H0 * H0);
    L.p = 0;
    L.q = big;
    L.scratch = 2 * big;
    long w = max2(deconv_ws_floats(B, Cin, FEAT, H0, prec), gn_bwd_ws_floats(B, FEAT));
    for (int l = 1; l < LAYERS; ++l) w = max2(w, conv_s1_ws_floats(B, FEAT, FEAT, MUL[l] * H0, prec));
    w = max2(w, conv1x1_bwd_ws_floats(B, FEAT, 3, 64 * H0 * H0));
    L.scratch_floats = up64(w);
    L.total = L.scratch + L.scratch_floats;
    return L;
}

// ---------------------------------------------------------------------------------- the entry points' bodies
// One body serves a gpx_ entry point and its precision-taking form: `name` is the caller's, `prec` a GPX_PREC_* value.
#define XYZ_PREC_REQUIRE(prec, name) GP_REQUIRE(xyz_prec_ok(prec), "%s: unknown precision %d (GPX_PREC_F32 or GPX_PREC_BF16)", name, prec)

long long conv_s1_workspace(int B, int Cin, int Cout, int H, int prec) {
    return conv_shape_ok(B, Cin, Cout, H) && xyz_prec_ok(prec) ? 4LL * up64(conv_s1_ws_floats(B, Cin, Cout, H, prec)) : 0;
}
int conv_s1_forward_entry(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, void* ws, long long ws_bytes,
                          void* stream, int prec, const char* name) {
    XYZ_PREC_REQUIRE(prec, name);
    GP_REQUIRE(!ws || aligned256(ws), "%s: the workspace is not 256-byte aligned", name);
    return conv_s1_forward(X, Wt, B, Cin, Cout, H, Y, (float*)ws, (long)(ws_bytes / 4), (hipStream_t)stream, prec, name);
}
int conv_s1_backward_entry(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW, void* ws,
                           long long ws_bytes, void* stream, int prec, const char* name) {
    XYZ_PREC_REQUIRE(prec, name);
    GP_REQUIRE(!ws || aligned256(ws), "%s: the workspace is not 256-byte aligned", name);
    return conv_s1_backward(dY, X, Wt, B, Cin, Cout, H, dX, dW, (float*)ws, (long)(ws_bytes / 4), (hipStream_t)stream, prec, name);
}

long long deconv_workspace(int B, int Cin, int Cout, int H, int prec) {
    return conv_shape_ok(B, Cin, Cout, 2L * H) && xyz_prec_ok(prec) ? 4LL * up64(deconv_ws_floats(B, Cin, Cout, H, prec)) : 0;
}
int deconv_forward_entry(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, void* ws, long long ws_bytes,
                         void* stream, int prec, const char* name) {
    XYZ_PREC_REQUIRE(prec, name);
    GP_REQUIRE(!ws || aligned256(ws), "%s: the workspace is not 256-byte aligned", name);
    return deconv_forward(X, Wt, B, Cin, Cout, H, Y, (float*)ws, (long)(ws_bytes / 4), (hipStream_t)stream, prec, name);
}
int deconv_backward_entry(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW, void* ws,
                          long long ws_bytes, void* stream, int prec, const char* name) {
    XYZ_PREC_REQUIRE(prec, name);
    GP_REQUIRE(!ws || aligned256(ws), "%s: the workspace is not 256-byte aligned", name);
    return deconv_backward(dY, X, Wt, B, Cin, Cout, H, dX, dW, (float*)ws, (long)(ws_bytes / 4), (hipStream_t)stream, prec, name);
}

long long head_forward_workspace(int B, int Cin, int H0, int prec) {
    return head_shape_ok(B, Cin, H0) && xyz_prec_ok(prec) ? 4LL * head_fwd_ws_floats(B, Cin, H0, prec) : 0;
}
int head_forward_save(const float* feat, const gpx_xyz_params* w, int B, int Cin, int H0, const gpx_xyz_saved* sv, void* ws,
                      long long ws_bytes, void* stream, int prec, const char* name) {
    XYZ_PREC_REQUIRE(prec, name);
    GP_REQUIRE(feat && params_complete(w) && saved_complete(sv), "%s: null pointer", name);
    GP_REQUIRE(head_shape_ok(B, Cin, H0), "%s: bad shape B %d Cin %d H0 %d", name, B, Cin, H0);
    GP_REQUIRE(!ws || aligned256(ws), "%s: the workspace is not 256-byte aligned", name);
    GP_REQUIRE(ws_bytes / 4 >= head_fwd_ws_floats(B, Cin, H0, prec) && (ws || ws_bytes == 0), "%s: workspace too small", name);
    hipStream_t s = (hipStream_t)stream;
    float* f = (float*)ws;
    const long wf = (long)(ws_bytes / 4);
    GPH_TRY(deconv_forward(feat, w->deconv_w, B, Cin, FEAT, H0, sv->pre[0], f, wf, s, prec, name));
    const float* in = nullptr;
    for (int l = 0; l < LAYERS; ++l) {
        const int H = MUL[l] * H0;
        if (l == 3 || l == 5) {      // UpsamplingBilinear2d in front of the third and the fifth conv
            float* up = sv->up[(l - 3) / 2];
            GPH_TRY(upsample_forward(in, B, FEAT, H / 2, up, s, name));
            in = up;
        }
        if (l > 0) GPH_TRY(conv_s1_forward(in, w->conv_w[l - 1], B, FEAT, FEAT, H, sv->pre[l], f, wf, s, prec, name));
        GPH_TRY(gn_gelu_forward(sv->pre[l], w->gn_w[l], w->gn_b[l], B, FEAT, H * H, GROUPS, sv->act[l], sv->mean[l], sv->rstd[l], s, name));
        in = sv->act[l];
    }
    return conv1x1_forward(in, w->out_w, w->out_b, B, FEAT, 3, 64 * H0 * H0, sv->coor, f, wf, s, name);
}

long long head_backward_workspace(int B, int Cin, int H0, int prec) {
    return head_shape_ok(B, Cin, H0) && xyz_prec_ok(prec) ? 4LL * bwd_layout(B, Cin, H0, prec).total : 0;
}
int head_backward(const gpx_xyz_params* w, const gpx_xyz_saved* sv, const float* feat, const float* g_coor, int B, int Cin, int H0,
                  const gpx_xyz_params* gr, float* g_feat, void* ws, long long ws_bytes, void* stream, int prec, const char* name) {
    XYZ_PREC_REQUIRE(prec, name);
    GP_REQUIRE(params_complete(w) && saved_complete(sv) && params_complete(gr) && feat && g_coor && g_feat, "%s: null pointer", name);
    GP_REQUIRE(head_shape_ok(B, Cin, H0), "%s: bad shape B %d Cin %d H0 %d", name, B, Cin, H0);
    const BwdLayout L = bwd_layout(B, Cin, H0, prec);
    GP_REQUIRE(ws && aligned256(ws) && ws_bytes / 4 >= L.total, "%s: workspace missing, unaligned or too small", name);
    hipStream_t s = (hipStream_t)stream;
    float* f = (float*)ws;
    float *da = f + L.p, *dc = f + L.q, *sc = f + L.scratch;      // da: gradient of a layer's output, dc: of its pre-norm map
    const long sf = L.scratch_floats;
    GPH_TRY(conv1x1_backward(g_coor, sv->act[LAYERS - 1], w->out_w, B, FEAT, 3, 64 * H0 * H0, da, gr->out_w, gr->out_b, sc, sf, s, name));
    for (int l = LAYERS - 1; l >= 0; --l) {
        const int H = MUL[l] * H0;
        GPH_TRY(gn_gelu_backward(da, sv->pre[l], sv->mean[l], sv->rstd[l], w->gn_w[l], w->gn_b[l], B, FEAT, H * H, GROUPS, dc, gr->gn_w[l],
                                 gr->gn_b[l], sc, sf, s, name));
        if (l == 0) break;
        const bool up = l == 3 || l == 5;
        const float* in = up ? sv->up[(l - 3) / 2] : sv->act[l - 1];
        GPH_TRY(conv_s1_backward(dc, in, w->conv_w[l - 1], B, FEAT, FEAT, H, da, gr->conv_w[l - 1], sc, sf, s, prec, name));
        if (up) {      // back through the upsample: da (H) -> dc (H / 2) -> da for the layer below
            GPH_TRY(upsample_backward(da, B, FEAT, H / 2, dc, s, name));
            float* t = da;
            da = dc;
            dc = t;
        }
    }
    return deconv_backward(dc, feat, w->deconv_w, B, Cin, FEAT, H0, g_feat, gr->deconv_w, sc, sf, s, prec, name);
}

}  // namespace

extern "C" {

long long gpx_conv3x3s1_workspace(int B, int Cin, int Cout, int H) { return conv_s1_workspace(B, Cin, Cout, H, GPX_PREC_F32); }

int gpx_conv3x3s1_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, void* ws, long long ws_bytes,
                          void* stream) {
    return conv_s1_forward_entry(X, Wt, B, Cin, Cout, H, Y, ws, ws_bytes, stream, GPX_PREC_F32, "gpx_conv3x3s1_forward");
}

int gpx_conv3x3s1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW, void* ws,
                           long long ws_bytes, void* stream) {
    return conv_s1_backward_entry(dY, X, Wt, B, Cin, Cout, H, dX, dW, ws, ws_bytes, stream, GPX_PREC_F32, "gpx_conv3x3s1_backward");
}

long long gpx_deconv3x3s2_workspace(int B, int Cin, int Cout, int H) { return deconv_workspace(B, Cin, Cout, H, GPX_PREC_F32); }

int gpx_deconv3x3s2_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, void* ws, long long ws_bytes,
                            void* stream) {
    return deconv_forward_entry(X, Wt, B, Cin, Cout, H, Y, ws, ws_bytes, stream, GPX_PREC_F32, "gpx_deconv3x3s2_forward");
}

int gpx_deconv3x3s2_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW,
                             void* ws, long long ws_bytes, void* stream) {
    return deconv_backward_entry(dY, X, Wt, B, Cin, Cout, H, dX, dW, ws, ws_bytes, stream, GPX_PREC_F32, "gpx_deconv3x3s2_backward");
}

long long gpx_gn_gelu_backward_workspace(int B, int C) { return B > 0 && C > 0 ? 4LL * gn_bwd_ws_floats(B, C) : 0; }

int gpx_gn_gelu_backward(const float* dout, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         int B, int C, int HW, int G, float* dx, float* dgamma, float* dbeta, void* ws, long long ws_bytes, void* stream) {
    GP_REQUIRE(!ws || aligned256(ws), "gpx_gn_gelu_backward: the workspace is not 256-byte aligned");
    return gn_gelu_backward(dout, x, mean, rstd, gamma, beta, B, C, HW, G, dx, dgamma, dbeta, (float*)ws, (long)(ws_bytes / 4),
                            (hipStream_t)stream, "gpx_gn_gelu_backward");
}

int gpx_upsample_bilinear2x_forward(const float* x, int B, int C, int H, float* y, void* stream) {
    return upsample_forward(x, B, C, H, y, (hipStream_t)stream, "gpx_upsample_bilinear2x_forward");
}

int gpx_upsample_bilinear2x_backward(const float* dy, int B, int C, int H, float* dx, void* stream) {
    return upsample_backward(dy, B, C, H, dx, (hipStream_t)stream, "gpx_upsample_bilinear2x_backward");
}

long long gpx_conv1x1_backward_workspace(int B, int Cin, int Cout, int HW) {
    return conv1x1_shape_ok(B, Cin, Cout, HW) ? 4LL * up64(conv1x1_bwd_ws_floats(B, Cin, Cout, HW)) : 0;
}

int gpx_conv1x1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int HW, float* dX, float* dW, float* db,
                         void* ws, long long ws_bytes, void* stream) {
    GP_REQUIRE(!ws || aligned256(ws), "gpx_conv1x1_backward: the workspace is not 256-byte aligned");
    return conv1x1_backward(dY, X, Wt, B, Cin, Cout, HW, dX, dW, db, (float*)ws, (long)(ws_bytes / 4), (hipStream_t)stream,
                            "gpx_conv1x1_backward");
}

long long gpx_xyz_forward_workspace(int B, int Cin, int H0) { return head_forward_workspace(B, Cin, H0, GPX_PREC_F32); }

int gpx_xyz_forward_save(const float* feat, const gpx_xyz_params* w, int B, int Cin, int H0, const gpx_xyz_saved* sv, void* ws,
                         long long ws_bytes, void* stream) {
    return head_forward_save(feat, w, B, Cin, H0, sv, ws, ws_bytes, stream, GPX_PREC_F32, "gpx_xyz_forward_save");
}

long long gpx_xyz_backward_workspace(int B, int Cin, int H0) { return head_backward_workspace(B, Cin, H0, GPX_PREC_F32); }

int gpx_xyz_backward(const gpx_xyz_params* w, const gpx_xyz_saved* sv, const float* feat, const float* g_coor, int B, int Cin, int H0,
                     const gpx_xyz_params* gr, float* g_feat, void* ws, long long ws_bytes, void* stream) {
    return head_backward(w, sv, feat, g_coor, B, Cin, H0, gr, g_feat, ws, ws_bytes, stream, GPX_PREC_F32, "gpx_xyz_backward");
}

/* ---- the precision-taking forms (include/givepose_xyzgrad_bf16.h) ---- */
long long gpxm_conv3x3s1_workspace(int B, int Cin, int Cout, int H, int precision) { return conv_s1_workspace(B, Cin, Cout, H, precision); }

int gpxm_conv3x3s1_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, void* ws, long long ws_bytes,
                           void* stream, int precision) {
    return conv_s1_forward_entry(X, Wt, B, Cin, Cout, H, Y, ws, ws_bytes, stream, precision, "gpxm_conv3x3s1_forward");
}

int gpxm_conv3x3s1_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW,
                            void* ws, long long ws_bytes, void* stream, int precision) {
    return conv_s1_backward_entry(dY, X, Wt, B, Cin, Cout, H, dX, dW, ws, ws_bytes, stream, precision, "gpxm_conv3x3s1_backward");
}

long long gpxm_deconv3x3s2_workspace(int B, int Cin, int Cout, int H, int precision) { return deconv_workspace(B, Cin, Cout, H, precision); }

int gpxm_deconv3x3s2_forward(const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* Y, void* ws, long long ws_bytes,
                             void* stream, int precision) {
    return deconv_forward_entry(X, Wt, B, Cin, Cout, H, Y, ws, ws_bytes, stream, precision, "gpxm_deconv3x3s2_forward");
}

int gpxm_deconv3x3s2_backward(const float* dY, const float* X, const float* Wt, int B, int Cin, int Cout, int H, float* dX, float* dW,
                              void* ws, long long ws_bytes, void* stream, int precision) {
    return deconv_backward_entry(dY, X, Wt, B, Cin, Cout, H, dX, dW, ws, ws_bytes, stream, precision, "gpxm_deconv3x3s2_backward");
}

long long gpxm_xyz_forward_workspace(int B, int Cin, int H0, int precision) { return head_forward_workspace(B, Cin, H0, precision); }

int gpxm_xyz_forward_save(const float* feat, const gpx_xyz_params* w, int B, int Cin, int H0, const gpx_xyz_saved* sv, void* ws,
                          long long ws_bytes, void* stream, int precision) {
    return head_forward_save(feat, w, B, Cin, H0, sv, ws, ws_bytes, stream, precision, "gpxm_xyz_forward_save");
}

long long gpxm_xyz_backward_workspace(int B, int Cin, int H0, int precision) { return head_backward_workspace(B, Cin, H0, precision); }

int gpxm_xyz_backward(const gpx_xyz_params* w, const gpx_xyz_saved* sv, const float* feat, const float* g_coor, int B, int Cin, int H0,
                      const gpx_xyz_params* gr, float* g_feat, void* ws, long long ws_bytes, void* stream, int precision) {
    return head_backward(w, sv, feat, g_coor, B, Cin, H0, gr, g_feat, ws, ws_bytes, stream, precision, "gpxm_xyz_backward");
}

}  // extern "C"
