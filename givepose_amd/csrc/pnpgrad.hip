// Pose-head backward family (include/givepose_headgrad.h, prefix gph_): ConvPnPNet forward-that-saves and its backward in fp32.
//
// Every long contraction runs on the functor GEMM of grad_gemm.hpp (one LDS-tiled kernel on v_mfma_f32_32x32x2_f32, the builtin
// __builtin_amdgcn_mfma_f32_32x32x2f32, whose operands are address functors); this file holds the layers that are not contractions
// and the head.
#include "grad_gemm.hpp"

namespace {

constexpr int FEAT = GPH_FEAT, RES = GPH_RES;

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
