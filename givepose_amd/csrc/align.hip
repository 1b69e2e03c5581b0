// Pose from the NOCS map and depth: RANSAC Umeyama alignment on the device (include/givepose_align.h; the reference's
// pose_from_umeyama, tools/umeyama.py:17-60, arithmetic in tools/align_utils.py:10-104).  Three launches per call of
// pose_from_umeyama_device, all crops at once:
//   align_backproject_kernel   one workgroup per crop: float32 back-projection of every pixel, and the masked pixels compacted in
//                              row-major order (wave ballot + prefix counts over the 4 waves; no atomics)
//   align_hypotheses_kernel    grid (crop, slice of HYP_PER_WG hypotheses): lane h of every wave fits hypothesis h of the slice
//                              (5-point Umeyama, all 16 in parallel), then the workgroup's threads, each holding 16 points of
//                              the crop in registers, count the inliers of one hypothesis after the other (ballot + popcount)
//   align_finish_kernel        one workgroup per crop: thread 0 replays the reference's sequential rule on the 128 counts, then
//                              the inlier flags of the winner and the final Umeyama fit, two passes (centroids, centred covariance)
//                              with a fixed reduction order: the thread's 16 points in turn, xor tree over the wave, the 4 waves
//                              as (w0 + w1) + (w2 + w3)
// float64 throughout after the back-projection.  The kernels are latency-bound (a 3x3 Jacobi SVD per hypothesis, 128 x 4096
// residuals per crop); nothing is tuned, and no LDS staging is needed: a thread's 16 points are 96 float registers.
#include "common.hpp"
#include "../../include/givepose_align.h"
#include "align_math.hpp"

namespace {

constexpr int NPIX = GPA_MAX_POINTS;
constexpr int WG = 256;                    // threads of every kernel here
constexpr int PER_THREAD = NPIX / WG;      // 16 points (pixels) per thread: point k * WG + tid, so that a wave reads consecutive points
constexpr int HYP_PER_WG = 16;             // hypotheses per workgroup of align_hypotheses_kernel: one per lane of a 16-lane row
constexpr int HYP_SLICES = GPA_MAX_ITER / HYP_PER_WG;
static_assert(GPA_RES * GPA_RES == NPIX && NPIX % WG == 0 && GPA_MAX_ITER % HYP_PER_WG == 0 && GPA_HYP_STRIDE >= 13, "layout");

__global__ __launch_bounds__(WG) void align_backproject_kernel(const float* __restrict__ xyz, const float* __restrict__ coor,
                                                               const float* __restrict__ camK, const float* __restrict__ depth,
                                                               const unsigned char* __restrict__ mask, int valid_depth_only,
                                                               float* __restrict__ points, int* __restrict__ index,
                                                               int* __restrict__ n_points, float* __restrict__ pc) {
    __shared__ int s_wave[WG / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float fx = camK[b * 9 + 0], fy = camK[b * 9 + 4], ux = camK[b * 9 + 2], uy = camK[b * 9 + 5];
    float* P = points + (long)b * 6 * NPIX;
    int* I = index + (long)b * NPIX;
    int base = 0;                          // points kept before this round of WG pixels (the same in every thread)
    for (int k = 0; k < PER_THREAD; ++k) {
        const int i = k * WG + tid;
        const float d = depth[(long)b * NPIX + i];
        // (x_label - ux) * depth / fx: three correctly rounded float32 operations, none of which can contract
        const float x = __fdiv_rn(__fmul_rn(__fsub_rn(coor[((long)b * 2 + 0) * NPIX + i], ux), d), fx);
        const float y = __fdiv_rn(__fmul_rn(__fsub_rn(coor[((long)b * 2 + 1) * NPIX + i], uy), d), fy);
        if (pc) {
            float* o = pc + ((long)b * NPIX + i) * 3;
            o[0] = x; o[1] = y; o[2] = d;
        }
        const bool keep = mask[(long)b * NPIX + i] != 0 && (!valid_depth_only || d > 0.0f);
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < WG / 64; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (keep) {
            const int p = base + before + __popcll(bal & ((1ull << lane) - 1ull));      // < NPIX: at most one point per pixel
            P[0 * NPIX + p] = xyz[((long)b * 3 + 0) * NPIX + i];
            P[1 * NPIX + p] = xyz[((long)b * 3 + 1) * NPIX + i];
            P[2 * NPIX + p] = xyz[((long)b * 3 + 2) * NPIX + i];
            P[3 * NPIX + p] = x; P[4 * NPIX + p] = y; P[5 * NPIX + p] = d;
            I[p] = i;
        }
        base += total;
        __syncthreads();                   // s_wave is rewritten in the next round
    }
    for (int p = base + tid; p < NPIX; p += WG) {
#pragma unroll
        for (int c = 0; c < 6; ++c) P[c * NPIX + p] = 0.0f;
        I[p] = -1;
    }
    if (tid == 0) n_points[b] = base;
}

// sum over the workgroup in a fixed order: xor tree over the wave, then (w0 + w1) + (w2 + w3); every thread gets the total.
// Two barriers; `slot` is a [WG / 64] array of LDS that no other value uses between them.
__device__ __forceinline__ double wg_sum(double v, double* slot, int lane, int wave) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}
__device__ __forceinline__ double wg_max(double v, double* slot, int lane, int wave) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    return fmax(fmax(slot[0], slot[1]), fmax(slot[2], slot[3]));
}

// the thread's points into registers (0 past the end: such a point is never counted, the callers test k * WG + tid < n)
#define GPA_LOAD_POINTS(P)                                              \
    float sx[PER_THREAD], sy[PER_THREAD], sz[PER_THREAD], tx[PER_THREAD], ty[PER_THREAD], tz[PER_THREAD]; \
    _Pragma("unroll") for (int k = 0; k < PER_THREAD; ++k) {            \
        const int p = k * WG + tid;                                     \
        sx[k] = (P)[0 * NPIX + p]; sy[k] = (P)[1 * NPIX + p]; sz[k] = (P)[2 * NPIX + p]; \
        tx[k] = (P)[3 * NPIX + p]; ty[k] = (P)[4 * NPIX + p]; tz[k] = (P)[5 * NPIX + p]; \
    }

__global__ __launch_bounds__(WG) void align_hypotheses_kernel(const float* __restrict__ points, const int* __restrict__ n_points,
                                                              const unsigned int* __restrict__ draws, double* __restrict__ hyp,
                                                              int* __restrict__ counts) {
    __shared__ double s_red[WG / 64];
    __shared__ int s_cnt[HYP_PER_WG][WG / 64];
    const int b = blockIdx.x, h0 = blockIdx.y * HYP_PER_WG, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(n_points[b], NPIX);
    if (n <= 0) {                          // uniform over the workgroup
        if (tid < HYP_PER_WG) counts[b * GPA_MAX_ITER + h0 + tid] = 0;
        return;
    }
    const float* P = points + (long)b * 6 * NPIX;
    GPA_LOAD_POINTS(P)
    // InlierT = 2 max |src - mean(src)| / 10 (align_utils.py:53-59)
    double ax = 0.0, ay = 0.0, az = 0.0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const bool in = k * WG + tid < n;
        ax += in ? (double)sx[k] : 0.0; ay += in ? (double)sy[k] : 0.0; az += in ? (double)sz[k] : 0.0;
    }
    const double mx = wg_sum(ax, s_red, lane, wave) / (double)n, my = wg_sum(ay, s_red, lane, wave) / (double)n,
                 mz = wg_sum(az, s_red, lane, wave) / (double)n;
    double far2 = 0.0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const double dx = (double)sx[k] - mx, dy = (double)sy[k] - my, dz = (double)sz[k] - mz;
        const double r2 = fma(dz, dz, fma(dy, dy, dx * dx));
        far2 = fmax(far2, k * WG + tid < n ? r2 : 0.0);
    }
    const double inlier_t = 2.0 * sqrt(wg_max(far2, s_red, lane, wave)) / 10.0;

    // hypothesis h0 + (lane & 15): the four 16-lane rows of a wave, and the four waves, compute the same 16 fits
    const int h = h0 + (lane & (HYP_PER_WG - 1));
    double M[9], t[3], thr2;
    {
        double qs[3][GPA_SAMPLE], qt[3][GPA_SAMPLE];
#pragma unroll
        for (int j = 0; j < GPA_SAMPLE; ++j) {
            const int p = (int)(draws[((long)b * GPA_MAX_ITER + h) * GPA_SAMPLE + j] % (unsigned)n);      // < n <= NPIX
#pragma unroll
            for (int c = 0; c < 3; ++c) { qs[c][j] = (double)P[c * NPIX + p]; qt[c][j] = (double)P[(3 + c) * NPIX + p]; }
        }
        double ms[3], mt[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ms[c] = ((((qs[c][0] + qs[c][1]) + qs[c][2]) + qs[c][3]) + qs[c][4]) / 5.0;
            mt[c] = ((((qt[c][0] + qt[c][1]) + qt[c][2]) + qt[c][3]) + qt[c][4]) / 5.0;
        }
        double C[9], var = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < GPA_SAMPLE; ++k) acc = fma(qt[i][k] - mt[i], qs[j][k] - ms[j], acc);
                C[3 * i + j] = acc / 5.0;
            }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < GPA_SAMPLE; ++k) var = fma(qs[c][k] - ms[c], qs[c][k] - ms[c], var);
        var /= 5.0;
        const gpa::Fit f = gpa::umeyama_from_cov(C, var, GPA_RANK_TOL);
#pragma unroll
        for (int i = 0; i < 9; ++i) M[i] = f.ok ? f.scale * f.R[i] : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            t[i] = f.ok ? mt[i] - fma(M[3 * i + 2], ms[2], fma(M[3 * i + 1], ms[1], M[3 * i] * ms[0])) : 0.0;
        const double thr = f.scale * inlier_t;
        thr2 = f.ok ? thr * thr : -1.0;
        if (tid < HYP_PER_WG) {            // the workspace: align_finish_kernel reads the winner's transform back, bit for bit
            double* o = hyp + ((long)b * GPA_MAX_ITER + h) * GPA_HYP_STRIDE;
#pragma unroll
            for (int i = 0; i < 9; ++i) o[i] = M[i];
            o[9] = t[0]; o[10] = t[1]; o[11] = t[2]; o[12] = thr2; o[13] = 0.0; o[14] = 0.0; o[15] = 0.0;
        }
    }
    for (int j = 0; j < HYP_PER_WG; ++j) {
        double Mj[9], tj[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) Mj[i] = __shfl(M[i], j, 64);
#pragma unroll
        for (int i = 0; i < 3; ++i) tj[i] = __shfl(t[i], j, 64);
        const double thr2j = __shfl(thr2, j, 64);
        int c = 0;
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const bool in = k * WG + tid < n &&
                            gpa::is_inlier(Mj, tj, thr2j, (double)sx[k], (double)sy[k], (double)sz[k], (double)tx[k], (double)ty[k], (double)tz[k]);
            c += __popcll(__ballot(in));
        }
        if (lane == 0) s_cnt[j][wave] = c;
    }
    __syncthreads();
    if (tid < HYP_PER_WG) counts[b * GPA_MAX_ITER + h0 + tid] = (s_cnt[tid][0] + s_cnt[tid][1]) + (s_cnt[tid][2] + s_cnt[tid][3]);
}

// x^e for 0 <= e < 128 by squaring (the reference's `**`: a few ulp apart, and the fixtures keep 1e-9 away from the 0.99 it is compared with)
__device__ __forceinline__ double powi(double x, int e) {
    double r = 1.0;
    for (int bit = 0; bit < 7; ++bit) {
        r = (e >> bit) & 1 ? r * x : r;
        x *= x;
    }
    return r;
}

__global__ __launch_bounds__(WG) void align_finish_kernel(const float* __restrict__ points, const int* __restrict__ n_points,
                                                          const double* __restrict__ hyp, const int* __restrict__ counts,
                                                          unsigned char* __restrict__ inlier, double* __restrict__ fit64,
                                                          double* __restrict__ sRT, int* __restrict__ record, float* __restrict__ fit32) {
    __shared__ double s_red[WG / 64];
    __shared__ int s_dec[4];               // best iteration, its count, iterations run, status so far
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(n_points[b], NPIX);
    if (tid == 0) {
        // the loop of align_utils.py:67-92 on the counts alone
        int best = -1, bestc = 0, iters = 0;
        if (n > 0) {
            for (int i = 0; i < GPA_MAX_ITER; ++i) {
                const int c = counts[b * GPA_MAX_ITER + i];
                if (c > bestc) { bestc = c; best = i; }      // InlierRatio > BestInlierRatio: the same n divides both
                iters = i + 1;
                const double r = (double)bestc / (double)n;
                const double r5 = ((r * r) * (r * r)) * r;
                if (1.0 - powi(1.0 - r5, i) > 0.99) break;
            }
        }
        s_dec[0] = best; s_dec[1] = bestc; s_dec[2] = iters;
        s_dec[3] = n <= 0 ? GPA_NO_POINTS : ((double)bestc / (double)n < 0.1 ? GPA_LOW_INLIERS : GPA_OK);
    }
    __syncthreads();
    const int best = s_dec[0], iters = s_dec[2];
    int status = s_dec[3];
    const float* P = points + (long)b * 6 * NPIX;
    GPA_LOAD_POINTS(P)
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0}, thr2 = -1.0;
    if (best >= 0) {
        const double* o = hyp + ((long)b * GPA_MAX_ITER + best) * GPA_HYP_STRIDE;
#pragma unroll
        for (int i = 0; i < 9; ++i) M[i] = o[i];
        t[0] = o[9]; t[1] = o[10]; t[2] = o[11]; thr2 = o[12];
    }
    unsigned in_mask = 0;                  // bit k: the thread's point k is an inlier of the winner
    double a[6] = {0, 0, 0, 0, 0, 0}, cnt = 0.0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const bool in = k * WG + tid < n &&
                        gpa::is_inlier(M, t, thr2, (double)sx[k], (double)sy[k], (double)sz[k], (double)tx[k], (double)ty[k], (double)tz[k]);
        inlier[(long)b * NPIX + k * WG + tid] = in;
        in_mask |= (unsigned)in << k;
        a[0] += in ? (double)sx[k] : 0.0; a[1] += in ? (double)sy[k] : 0.0; a[2] += in ? (double)sz[k] : 0.0;
        a[3] += in ? (double)tx[k] : 0.0; a[4] += in ? (double)ty[k] : 0.0; a[5] += in ? (double)tz[k] : 0.0;
        cnt += in ? 1.0 : 0.0;
    }
    const double m = wg_sum(cnt, s_red, lane, wave);       // exact: an integer below 2^53
    const double dm = m > 0.0 ? m : 1.0;
    double mean[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) mean[c] = wg_sum(a[c], s_red, lane, wave) / dm;
    double cv[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // the 9 covariance sums and the source variance sum
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const bool in = (in_mask >> k) & 1;
        const double ds0 = (double)sx[k] - mean[0], ds1 = (double)sy[k] - mean[1], ds2 = (double)sz[k] - mean[2];
        const double dt0 = (double)tx[k] - mean[3], dt1 = (double)ty[k] - mean[4], dt2 = (double)tz[k] - mean[5];
        const double w = in ? 1.0 : 0.0;   // a factor, not a branch: the adds below happen for every point, in the same order
        cv[0] = fma(w * dt0, ds0, cv[0]); cv[1] = fma(w * dt0, ds1, cv[1]); cv[2] = fma(w * dt0, ds2, cv[2]);
        cv[3] = fma(w * dt1, ds0, cv[3]); cv[4] = fma(w * dt1, ds1, cv[4]); cv[5] = fma(w * dt1, ds2, cv[5]);
        cv[6] = fma(w * dt2, ds0, cv[6]); cv[7] = fma(w * dt2, ds1, cv[7]); cv[8] = fma(w * dt2, ds2, cv[8]);
        cv[9] = fma(w * ds2, ds2, fma(w * ds1, ds1, fma(w * ds0, ds0, cv[9])));
    }
    double C[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = wg_sum(cv[i], s_red, lane, wave) / dm;
    const double var = wg_sum(cv[9], s_red, lane, wave) / dm;
    const gpa::Fit f = gpa::umeyama_from_cov(C, var, GPA_RANK_TOL);
    if (status == GPA_OK && !f.ok) status = GPA_DEGENERATE;
    if (tid != 0) return;
    const bool ok = status == GPA_OK;
    double out[GPA_FIT_STRIDE];
    out[0] = ok ? f.scale : 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) out[1 + i] = ok ? f.R[i] : (i % 4 == 0 ? 1.0 : 0.0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        // t = mean(tgt) - Scale R mean(src) (align_utils.py:35)
        const double rm = fma(f.R[3 * i + 2], mean[2], fma(f.R[3 * i + 1], mean[1], f.R[3 * i] * mean[0]));
        out[10 + i] = ok ? mean[3 + i] - f.scale * rm : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) out[13 + i] = ok ? f.sigma[i] : 0.0;
#pragma unroll
    for (int i = 0; i < GPA_FIT_STRIDE; ++i) fit64[(long)b * GPA_FIT_STRIDE + i] = out[i];
#pragma unroll
    for (int i = 0; i < GPA_FIT32_STRIDE; ++i) fit32[(long)b * GPA_FIT32_STRIDE + i] = (float)out[i];
    double* S = sRT + (long)b * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) S[4 * i + j] = out[0] * out[1 + 3 * i + j];
        S[4 * i + 3] = out[10 + i];
    }
    S[12] = 0.0; S[13] = 0.0; S[14] = 0.0; S[15] = 1.0;
    int* rec = record + b * GPA_RECORD;
    rec[0] = n; rec[1] = (int)m; rec[2] = best; rec[3] = iters; rec[4] = status;
}

__global__ __launch_bounds__(WG) void crop_depth_kernel(const float* __restrict__ depth, const int* __restrict__ frame_idx,
                                                        const double* __restrict__ inv_out, float* __restrict__ roi_depth,
                                                        float* __restrict__ roi_pix, int H, int W, int R) {
    const int b = blockIdx.y, i = blockIdx.x * WG + threadIdx.x;
    if (i >= R * R) return;
    const int y = i / R, x = i - y * R;
    int X, Y;
    const bool ok = warp_src(inv_out + b * 6, x, y, W, H, X, Y);
    roi_depth[(long)b * R * R + i] = ok ? depth[((long)frame_idx[b] * H + Y) * W + X] : 0.0f;
    roi_pix[((long)b * 2 + 0) * R * R + i] = ok ? (float)X : 0.0f;
    roi_pix[((long)b * 2 + 1) * R * R + i] = ok ? (float)Y : 0.0f;
}

}  // namespace

extern "C" int gpa_backproject(const float* xyz, const float* coor_2d, const float* cam_K, const float* depth, const unsigned char* mask,
                               int valid_depth_only, int B, int R, float* points, int* index, int* n_points, float* pc, void* stream) {
    GP_REQUIRE(xyz && coor_2d && cam_K && depth && mask && points && index && n_points, "gpa_backproject: null pointer");
    GP_REQUIRE(R == GPA_RES, "gpa_backproject: the maps are %d x %d, not %d x %d", GPA_RES, GPA_RES, R, R);
    GP_REQUIRE(B > 0 && B <= 65535, "gpa_backproject: bad batch size %d", B);
    hipStream_t s = (hipStream_t)stream;
    gp_timing_before(s, GP_KC_SMALL, (double)B * NPIX * 6, (double)B * NPIX * (4 * 7 + 1 + 28));
    hipLaunchKernelGGL(align_backproject_kernel, dim3(B), dim3(WG), 0, s, xyz, coor_2d, cam_K, depth, mask, valid_depth_only, points, index,
                       n_points, pc);
    GP_LAUNCH_CHECK("gpa_backproject");
}

extern "C" int gpa_umeyama(const float* points, const int* n_points, const unsigned int* draws, int B, double* hyp, int* counts,
                           unsigned char* inlier, double* fit64, double* sRT, int* record, float* fit32, void* stream) {
    GP_REQUIRE(points && n_points && draws && hyp && counts && inlier && fit64 && sRT && record && fit32, "gpa_umeyama: null pointer");
    GP_REQUIRE(B > 0 && B <= 65535, "gpa_umeyama: bad batch size %d", B);
    hipStream_t s = (hipStream_t)stream;
    gp_timing_before(s, GP_KC_SMALL, (double)B * GPA_MAX_ITER * NPIX * 30, (double)B * NPIX * 24 * (HYP_SLICES + 1));
    hipLaunchKernelGGL(align_hypotheses_kernel, dim3(B, HYP_SLICES), dim3(WG), 0, s, points, n_points, draws, hyp, counts);
    hipLaunchKernelGGL(align_finish_kernel, dim3(B), dim3(WG), 0, s, points, n_points, hyp, counts, inlier, fit64, sRT, record, fit32);
    GP_LAUNCH_CHECK("gpa_umeyama");
}

extern "C" int gpa_crop_depth(const float* depth_frames, const int* frame_idx, const double* inv_out, float* roi_depth, float* roi_pix_2d,
                              int B, int F, int H, int W, int R, void* stream) {
    GP_REQUIRE(depth_frames && frame_idx && inv_out && roi_depth && roi_pix_2d, "gpa_crop_depth: null pointer");
    GP_REQUIRE(B > 0 && B <= 65535 && F > 0 && H > 0 && W > 0 && R > 0 && R <= 4096 && (long)F * H * W < (1l << 40), "gpa_crop_depth: bad shape");
    hipStream_t s = (hipStream_t)stream;
    gp_timing_before(s, GP_KC_SMALL, 0.0, (double)B * R * R * 16);
    hipLaunchKernelGGL(crop_depth_kernel, dim3(cdiv(R * R, WG), B), dim3(WG), 0, s, depth_frames, frame_idx, inv_out, roi_depth, roi_pix_2d, H, W, R);
    GP_LAUNCH_CHECK("gpa_crop_depth");
}
