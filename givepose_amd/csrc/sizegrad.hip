// The train-mode size head (include/givepose_sizegrad.h, gps_*): SizeHead with batch-statistics BatchNorm1d and an explicit or seeded
// dropout mask -- forward that saves, backward, running-statistics update.
//
//   pool_kernel      a workgroup per (crop, 64 channels): max over hw and the lowest hw that attains it, feat read once
//   hidden_kernel    a workgroup per GPS_CHUNK hidden channels, all B rows: h, the batch statistics, relu, dropout
//   out_kernel       a wave per crop: out = d W2^T + b2 (+ the normalised mean size)
//   chan_kernel      the same ownership as hidden_kernel: every sum over the batch of the backward, and dh
//   dw1_kernel       a thread per element of dW1 = dh^T pooled
//   dfeat_kernel     a workgroup per (crop, 64 channels): dpooled = dh W1, then every element of d feat
//   running_kernel   the running statistics
//
// The maps are small (B F is 8 k elements at B = 64) and the batch statistics couple all crops of a channel, so the contractions are
// dedicated kernels shaped around that ownership, not the functor GEMM of grad_gemm.hpp: a GEMM would put h and dh through memory
// between three more launches and buy nothing at B x 1024 x 128.
#include "common.hpp"
#include "../../include/givepose_sizegrad.h"

// Sums are written out as fma / + in a fixed order; nothing may be re-associated or fused behind the code's back.
#pragma clang fp contract(off)

namespace {

constexpr int WG = 256;
constexpr float DROP_SCALE = 1.25f;      // 1 / (1 - 0.2), exact

__device__ __forceinline__ float wave_sum(float v) {      // a fixed butterfly: every lane gets the same total
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// a double as two floats, hi + lo: the saved statistics keep fp32 buffers and lose nothing the backward needs
__device__ __forceinline__ void split(double v, float& hi, float& lo) {
    hi = (float)v;
    lo = (float)(v - (double)hi);
}

__device__ __forceinline__ unsigned keep_hash(unsigned lo, unsigned hi, unsigned idx) {
    unsigned x = lo ^ (idx * 0x9E3779B9u) ^ ((hi << 16) | (hi >> 16));
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// ---------------------------------------------------------------------------------- forward
// Thread (channel cl of 64, part of 4) walks hw = part, part + 4, ...; NHWC: a wave reads 64 consecutive channels of one pixel, NCHW:
// four lanes share a channel's row.  The four candidates of a channel meet in LDS: the larger value wins, of equal values the lower hw.
template <typename T, bool NHWC>
__global__ __launch_bounds__(WG) void pool_kernel(const T* __restrict__ feat, float* __restrict__ pooled, int* __restrict__ arg, int C, int HW) {
    __shared__ float sv[WG];
    __shared__ int si[WG];
    const int t = threadIdx.x, groups = C >> 6;
    const int b = blockIdx.x / groups, c0 = (blockIdx.x - b * groups) << 6;
    const int cl = NHWC ? (t & 63) : (t >> 2), part = NHWC ? (t >> 6) : (t & 3);
    const long long base = NHWC ? (long long)b * HW * C + c0 + cl : ((long long)b * C + c0 + cl) * HW;
    const long long step = NHWC ? C : 1;
    float best = 0.0f;
    int bi = -1;
    for (int hw = part; hw < HW; hw += 4) {
        const float v = (float)feat[base + hw * step];
        if (bi < 0 || v > best) best = v, bi = hw;
    }
    sv[part * 64 + cl] = best, si[part * 64 + cl] = bi;
    __syncthreads();
    if (t < 64) {
        float v = sv[t];      // part 0 holds hw = 0: never empty
        int i = si[t];
#pragma unroll
        for (int p = 1; p < 4; ++p) {
            const float v2 = sv[p * 64 + t];
            const int i2 = si[p * 64 + t];
            if (i2 >= 0 && (v2 > v || (v2 == v && i2 < i))) v = v2, i = i2;
        }
        pooled[(long long)b * C + c0 + t] = v;
        arg[(long long)b * C + c0 + t] = i;
    }
}

__global__ __launch_bounds__(WG) void hidden_kernel(const float* __restrict__ pooled, gps_params P, const unsigned char* __restrict__ keep_in,
                                                    unsigned seed_lo, unsigned seed_hi, int B, int C, int F, gps_saved S) {
    extern __shared__ __attribute__((aligned(16))) float w1s[];      // GPS_CHUNK rows of W1
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, f0 = blockIdx.x * GPS_CHUNK;
    for (int i = t; i < GPS_CHUNK * C; i += WG) w1s[i] = P.w1[(long long)f0 * C + i];
    __syncthreads();
    // h: wave w takes the rows w, w + 4, ...; the lanes split C
    for (int b = wave; b < B; b += 4) {
        const float* __restrict__ x = pooled + (long long)b * C;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        for (int c = lane; c < C; c += 64) {
            const float v = x[c];
            a0 = fmaf(v, w1s[c], a0);
            a1 = fmaf(v, w1s[C + c], a1);
            a2 = fmaf(v, w1s[2 * C + c], a2);
            a3 = fmaf(v, w1s[3 * C + c], a3);
        }
        a0 = wave_sum(a0), a1 = wave_sum(a1), a2 = wave_sum(a2), a3 = wave_sum(a3);
        if (lane < GPS_CHUNK) S.h[(long long)b * F + f0 + lane] = (lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3) + P.b1[f0 + lane];
    }
    __threadfence_block();
    __syncthreads();      // h of every row of this chunk is written; from here wave w owns channel f0 + w and its lanes split the rows
    // The statistics are formed in fp64 from the fp32 h (as torch's CPU BatchNorm does for float32 input: its accumulation type is
    // double).  In fp32 the rounding of mean alone leaves xhat^2 short of what 1 - xhat^2 needs when a channel's variance is small.
    const int f = f0 + wave;
    const float* hc = S.h + f;
    double s = 0.0;
    for (int b = lane; b < B; b += 64) s += (double)hc[(long long)b * F];
    const double mean = wave_sum(s) / (double)B;
    double q = 0.0;
    for (int b = lane; b < B; b += 64) {
        const double dl = (double)hc[(long long)b * F] - mean;
        q = fma(dl, dl, q);
    }
    q = wave_sum(q);
    const double rstd = 1.0 / sqrt(q / (double)B + GPS_BN_EPS);
    const double gam = P.gamma[f], bet = P.beta[f];
    for (int b = lane; b < B; b += 64) {
        const long long o = (long long)b * F + f;
        const float y = (float)fma(gam, ((double)hc[(long long)b * F] - mean) * rstd, bet);
        const bool k = keep_in ? keep_in[o] != 0 : keep_hash(seed_lo, seed_hi, (unsigned)o) >= GPS_DROP_THRESHOLD;
        S.d[o] = (k && y > 0.0f) ? y * DROP_SCALE : 0.0f;
        S.keep[o] = k ? 1 : 0;
    }
    if (lane == 0) {
        split(mean, S.mean[f], S.mean_lo[f]);
        split(rstd, S.rstd[f], S.rstd_lo[f]);
        S.var_unbiased[f] = (float)(q / (double)(B - 1));
    }
}

__global__ __launch_bounds__(WG) void out_kernel(const float* __restrict__ d, const float* __restrict__ w2, const float* __restrict__ b2,
                                                 const float* __restrict__ mean_size, float* __restrict__ out, float* __restrict__ size, int B, int F) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float a[3] = {0.0f, 0.0f, 0.0f};
    for (int f = lane; f < F; f += 64) {
        const float v = d[(long long)b * F + f];
#pragma unroll
        for (int j = 0; j < 3; ++j) a[j] = fmaf(v, w2[j * F + f], a[j]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] = wave_sum(a[j]);
    if (lane < 3) {
        const float o = (lane == 0 ? a[0] : lane == 1 ? a[1] : a[2]) + b2[lane];
        out[b * 3 + lane] = o;
        if (size) {
            const float m0 = mean_size[b * 3], m1 = mean_size[b * 3 + 1], m2 = mean_size[b * 3 + 2];
            size[b * 3 + lane] = o + mean_size[b * 3 + lane] / sqrtf(m0 * m0 + m1 * m1 + m2 * m2);
        }
    }
}

// ---------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(WG) void chan_kernel(gps_params P, gps_saved S, const float* __restrict__ g_out, int B, int F, gps_params G,
                                                  float* __restrict__ dh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.x * GPS_CHUNK + wave;
    const float w0 = P.w2[f], w1 = P.w2[F + f], w2 = P.w2[2 * F + f];
    // the batch sums and dh in fp64 from the saved fp32 h and the saved statistics (hi + lo), as in the forward
    const double gam = P.gamma[f], mean = (double)S.mean[f] + (double)S.mean_lo[f], rstd = (double)S.rstd[f] + (double)S.rstd_lo[f];
    double s1 = 0.0, s2 = 0.0, dbeta = 0.0, dgamma = 0.0;
    float u0 = 0.0f, u1 = 0.0f, u2 = 0.0f;
    for (int b = lane; b < B; b += 64) {
        const long long o = (long long)b * F + f;
        const float g0 = g_out[b * 3], g1 = g_out[b * 3 + 1], g2 = g_out[b * 3 + 2], dv = S.d[o];
        const double xv = ((double)S.h[o] - mean) * rstd;
        const float dd = fmaf(g2, w2, fmaf(g1, w1, g0 * w0));
        const float dy = (S.keep[o] && dv > 0.0f) ? dd * DROP_SCALE : 0.0f;
        const double dx = (double)dy * gam;
        s1 += dx, s2 = fma(dx, xv, s2), dbeta += (double)dy, dgamma = fma((double)dy, xv, dgamma);
        u0 = fmaf(g0, dv, u0), u1 = fmaf(g1, dv, u1), u2 = fmaf(g2, dv, u2);
    }
    s1 = wave_sum(s1), s2 = wave_sum(s2), dbeta = wave_sum(dbeta), dgamma = wave_sum(dgamma);
    u0 = wave_sum(u0), u1 = wave_sum(u1), u2 = wave_sum(u2);
    const double k = rstd / (double)B;
    double db1 = 0.0;
    for (int b = lane; b < B; b += 64) {
        const long long o = (long long)b * F + f;
        const float g0 = g_out[b * 3], g1 = g_out[b * 3 + 1], g2 = g_out[b * 3 + 2], dv = S.d[o];
        const double xv = ((double)S.h[o] - mean) * rstd;
        const float dd = fmaf(g2, w2, fmaf(g1, w1, g0 * w0));
        const float dy = (S.keep[o] && dv > 0.0f) ? dd * DROP_SCALE : 0.0f;
        const float v = (float)(k * (((double)B * ((double)dy * gam) - s1) - xv * s2));
        dh[o] = v;
        db1 += (double)v;
    }
    db1 = wave_sum(db1);
    if (lane == 0) {
        G.gamma[f] = (float)dgamma, G.beta[f] = (float)dbeta, G.b1[f] = (float)db1;
        G.w2[f] = u0, G.w2[F + f] = u1, G.w2[2 * F + f] = u2;
    }
    if (blockIdx.x == 0 && wave < 3) {      // db2 = sum_b g_out
        float a = 0.0f;
        for (int b = lane; b < B; b += 64) a += g_out[b * 3 + wave];
        a = wave_sum(a);
        if (lane == 0) G.b2[wave] = a;
    }
}

__global__ __launch_bounds__(WG) void dw1_kernel(const float* __restrict__ dh, const float* __restrict__ pooled, float* __restrict__ dw1, int B,
                                                 int C, int F) {
    const int idx = blockIdx.x * WG + threadIdx.x;      // F C is a multiple of 1024
    const int f = idx / C, c = idx - f * C;
    float a = 0.0f;
    for (int b = 0; b < B; ++b) a = fmaf(dh[(long long)b * F + f], pooled[(long long)b * C + c], a);
    dw1[idx] = a;
}

__global__ __launch_bounds__(WG) void dfeat_kernel(const float* __restrict__ dh, const float* __restrict__ w1, const int* __restrict__ arg,
                                                   float* __restrict__ d_feat, int C, int HW, int F) {
    __shared__ float part[WG];
    __shared__ float dp[64];
    __shared__ int sa[64];
    const int t = threadIdx.x, cl = t & 63, p = t >> 6, groups = C >> 6;
    const int b = blockIdx.x / groups, c0 = (blockIdx.x - b * groups) << 6;
    float a = 0.0f;
    for (int f = p; f < F; f += 4) a = fmaf(dh[(long long)b * F + f], w1[(long long)f * C + c0 + cl], a);
    part[t] = a;
    __syncthreads();
    if (t < 64) {
        dp[t] = (part[t] + part[64 + t]) + (part[128 + t] + part[192 + t]);
        sa[t] = arg[(long long)b * C + c0 + t];
    }
    __syncthreads();
    float* __restrict__ out = d_feat + ((long long)b * C + c0) * HW;      // the 64 channels' maps are one contiguous run
    const int n = 64 * HW;
    for (int i = t; i < n; i += WG) {
        const int c = i / HW, hw = i - c * HW;
        out[i] = hw == sa[c] ? dp[c] : 0.0f;
    }
}

__global__ __launch_bounds__(WG) void running_kernel(float* __restrict__ rm, float* __restrict__ rv, long long* __restrict__ nbt,
                                                     const float* __restrict__ mean, const float* __restrict__ var, int F, float mom, float keep) {
    const int f = blockIdx.x * WG + threadIdx.x;
    if (f < F) {
        rm[f] = fmaf(mom, mean[f], keep * rm[f]);
        rv[f] = fmaf(mom, var[f], keep * rv[f]);
    }
    if (f == 0 && nbt) nbt[0] += 1;
}

// ---------------------------------------------------------------------------------- host
bool al4(const void* p) { return p && ((uintptr_t)p & 3) == 0; }

int check_sizes(const char* name, int B, int C, int HW, int F) {
    GP_REQUIRE(B >= 2, "%s: B = %d: the batch statistics need more than 1 value per channel (B >= 2)", name, B);
    GP_REQUIRE(B <= (1 << 20), "%s: B = %d", name, B);
    GP_REQUIRE(C >= 64 && C % 64 == 0 && C <= GPS_MAX_C, "%s: C = %d is not a multiple of 64 in 64 .. %d", name, C, GPS_MAX_C);
    GP_REQUIRE(HW >= 1 && HW <= (1 << 20), "%s: HW = %d", name, HW);
    GP_REQUIRE(F >= 16 && F % 16 == 0 && F <= (1 << 16), "%s: F = %d is not a multiple of 16", name, F);
    GP_REQUIRE((long long)B * (C / 64) < (1LL << 31) && (long long)B * F < (1LL << 31) && (long long)64 * HW < (1LL << 31),
               "%s: B = %d, C = %d, HW = %d, F = %d: too many workgroups or hidden units", name, B, C, HW, F);
    return 0;
}

int check_params(const char* name, const char* what, const gps_params* p) {
    GP_REQUIRE(p && al4(p->w1) && al4(p->b1) && al4(p->w2) && al4(p->b2) && al4(p->gamma) && al4(p->beta), "%s: %s: a null or misaligned pointer",
               name, what);
    return 0;
}

int check_saved(const char* name, const gps_saved* s) {
    GP_REQUIRE(s && al4(s->pooled) && al4(s->arg) && al4(s->h) && al4(s->mean) && al4(s->mean_lo) && al4(s->rstd) && al4(s->rstd_lo) && al4(s->d) &&
                   s->keep && al4(s->out) && al4(s->var_unbiased),
               "%s: saved: a null or misaligned pointer", name);
    return 0;
}

#define GPS_CHECK(name)                                                                               \
    do {                                                                                              \
        hipError_t e__ = hipGetLastError();                                                           \
        if (e__ != hipSuccess) return gp_fail(GP_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e__)); \
    } while (0)

}  // namespace

extern "C" {

int gps_size_forward_save(const void* feat, int dtype, int nhwc, const gps_params* params, const unsigned char* keep_in, unsigned long long seed,
                          const float* mean_size, int B, int C, int HW, int F, const gps_saved* saved, float* size, void* stream) {
    const char* name = "gps_size_forward_save";
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_sizes(name, B, C, HW, F)) return rc;
    GP_REQUIRE(dtype == GP_F32 || dtype == GP_F16, "%s: dtype %d (GP_F32 or GP_F16)", name, dtype);
    GP_REQUIRE(nhwc || dtype == GP_F32, "%s: an NCHW feature must be GP_F32", name);
    GP_REQUIRE(feat && ((uintptr_t)feat & (dtype == GP_F16 ? 1 : 3)) == 0, "%s: feat is null or misaligned", name);
    GP_REQUIRE((mean_size == nullptr) == (size == nullptr) && (!size || (al4(mean_size) && al4(size))), "%s: mean_size and size go together", name);
    if (int rc = check_params(name, "params", params)) return rc;
    if (int rc = check_saved(name, saved)) return rc;
    const dim3 pg((unsigned)(B * (C / 64))), wg(WG);
    if (!nhwc) hipLaunchKernelGGL((pool_kernel<float, false>), pg, wg, 0, s, (const float*)feat, saved->pooled, saved->arg, C, HW);
    else if (dtype == GP_F16) hipLaunchKernelGGL((pool_kernel<half_t, true>), pg, wg, 0, s, (const half_t*)feat, saved->pooled, saved->arg, C, HW);
    else hipLaunchKernelGGL((pool_kernel<float, true>), pg, wg, 0, s, (const float*)feat, saved->pooled, saved->arg, C, HW);
    GPS_CHECK(name);
    hipLaunchKernelGGL(hidden_kernel, dim3(F / GPS_CHUNK), wg, (size_t)GPS_CHUNK * C * sizeof(float), s, (const float*)saved->pooled, *params, keep_in,
                       (unsigned)(seed & 0xFFFFFFFFu), (unsigned)(seed >> 32), B, C, F, *saved);
    GPS_CHECK(name);
    hipLaunchKernelGGL(out_kernel, dim3((B + 3) / 4), wg, 0, s, (const float*)saved->d, (const float*)params->w2, (const float*)params->b2, mean_size,
                       saved->out, size, B, F);
    GPS_CHECK(name);
    return 0;
}

long long gps_size_backward_workspace(int B, int C, int HW, int F) {
    if (check_sizes("gps_size_backward_workspace", B, C, HW, F)) return 0;
    return ((long long)B * F * 4 + 255) / 256 * 256;      // dh
}

int gps_size_backward(const gps_params* params, const gps_saved* saved, const float* g_out, int B, int C, int HW, int F, const gps_params* grads,
                      float* d_feat, void* ws, long long ws_bytes, void* stream) {
    const char* name = "gps_size_backward";
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_sizes(name, B, C, HW, F)) return rc;
    if (int rc = check_params(name, "params", params)) return rc;
    if (int rc = check_params(name, "grads", grads)) return rc;
    if (int rc = check_saved(name, saved)) return rc;
    GP_REQUIRE(al4(g_out) && al4(d_feat), "%s: g_out or d_feat is null or misaligned", name);
    const long long need = gps_size_backward_workspace(B, C, HW, F);
    GP_REQUIRE(ws && ((uintptr_t)ws & 255) == 0 && ws_bytes >= need, "%s: workspace of %lld bytes (256-byte aligned) needed, %lld given", name, need,
               ws_bytes);
    float* dh = (float*)ws;
    hipLaunchKernelGGL(chan_kernel, dim3(F / GPS_CHUNK), dim3(WG), 0, s, *params, *saved, g_out, B, F, *grads, dh);
    GPS_CHECK(name);
    hipLaunchKernelGGL(dw1_kernel, dim3((unsigned)((long long)F * C / WG)), dim3(WG), 0, s, (const float*)dh, (const float*)saved->pooled, grads->w1, B,
                       C, F);
    GPS_CHECK(name);
    hipLaunchKernelGGL(dfeat_kernel, dim3((unsigned)(B * (C / 64))), dim3(WG), 0, s, (const float*)dh, (const float*)params->w1,
                       (const int*)saved->arg, d_feat, C, HW, F);
    GPS_CHECK(name);
    return 0;
}

int gps_bn_running_update(float* running_mean, float* running_var, long long* num_batches_tracked, const float* mean, const float* var_unbiased,
                          int F, double momentum, void* stream) {
    const char* name = "gps_bn_running_update";
    GP_REQUIRE(al4(running_mean) && al4(running_var) && al4(mean) && al4(var_unbiased), "%s: a null or misaligned pointer", name);
    GP_REQUIRE(((uintptr_t)num_batches_tracked & 7) == 0, "%s: num_batches_tracked is misaligned", name);
    GP_REQUIRE(F >= 1 && F <= (1 << 24) && momentum >= 0.0 && momentum <= 1.0, "%s: F = %d, momentum = %g", name, F, momentum);
    hipLaunchKernelGGL(running_kernel, dim3((F + WG - 1) / WG), dim3(WG), 0, (hipStream_t)stream, running_mean, running_var, num_batches_tracked, mean,
                       var_unbiased, F, (float)momentum, (float)(1.0 - momentum));
    GPS_CHECK(name);
    return 0;
}

}  // extern "C"
