// The validation-loss family (include/givepose_loss.h): the reference's train-time pose decode and PoseLoss.forward
// (losses/pose_loss.py:30-196) on the device, forward values only.  Three kernels:
//   pose_decode_train_kernel   one thread per crop
//   pose_loss_partials_kernel  grid (GPL_SPLIT, crop): every workgroup repeats the crop's 360-candidate search (a wave holds 6
//                              candidates per lane; all four waves compute the same winner, so nothing is exchanged), then sums
//                              its quarter of the two coordinate maps (16-byte loads, 4 pixels per lane) and of the model points
//   pose_loss_reduce_kernel    one workgroup: crops in a fixed order -> the six weighted terms, mean re / te, the running sums
// float64 from the float32 inputs.  Every sum is store-and-sum: the thread's elements in turn, xor tree over the wave, the 4 waves
// as (w0 + w1) + (w2 + w3), the workgroups of a crop in turn, the crops of a thread in turn -- no floating-point atomics, equal
// inputs give equal bits.  Contraction is off for the whole file: the scalar arithmetic (3x3 products, traces, the Huber and
// SmoothL1 forms) is written in the order of tests/pose_loss_ref.py and gives its bits; only the order of the long sums differs.
#include "common.hpp"
#include "../../include/givepose_loss.h"

#pragma clang fp contract(off)

namespace {

constexpr int WG = 256;
constexpr int NPIX = GPL_RES * GPL_RES;
constexpr int PIX_PER_WG = NPIX / GPL_SPLIT;
constexpr double HUBER = 0.03;            // PoseLoss.threshold
static_assert(PIX_PER_WG == WG * 4 && GPL_SYM <= 6 * 64 && GPL_PART >= 5 && GPL_RECORD >= 8 && GPL_OUT >= 8 && GPL_ACC >= 10, "layout");

// sum over the workgroup in a fixed order; every thread gets the total (the form of align.hip)
__device__ __forceinline__ double wg_sum(double v, double* slot, int lane, int wave) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

struct Mat3 {
    double m[9];
};

// re of pose_error.py / pose_loss.py:451-466 in degrees: trace(A B^T) = sum_ij A_ij B_ij taken row by row
__device__ __forceinline__ double trace_abt(const Mat3& A, const Mat3& B) {
    double t = A.m[0] * B.m[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) t = t + A.m[i] * B.m[i];
    return t;
}
__device__ __forceinline__ double re_deg(const Mat3& A, const Mat3& B) {
    double t = trace_abt(A, B);
    t = t <= 3.0 ? t : 3.0;
    const double c = fmin(1.0, fmax(-1.0, 0.5 * (t - 1.0)));
    return acos(c) * (180.0 / 3.14159265358979323846);
}
// G * S_k, S_k = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
__device__ __forceinline__ Mat3 times_sym_y(const Mat3& G, double c, double s) {
    Mat3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o.m[3 * i + 0] = G.m[3 * i + 0] * c - G.m[3 * i + 2] * s;
        o.m[3 * i + 1] = G.m[3 * i + 1];
        o.m[3 * i + 2] = G.m[3 * i + 0] * s + G.m[3 * i + 2] * c;
    }
    return o;
}
__device__ __forceinline__ double smooth_l1(double a, double b, double beta) {
    const double d = fabs(a - b);
    return d < beta ? 0.5 * d * d / beta : d - 0.5 * beta;
}
__device__ __forceinline__ double pose_term(double a, double b, int smoothl1) { return smoothl1 ? smooth_l1(a, b, 0.5) : fabs(a - b); }

__global__ __launch_bounds__(64) void pose_decode_train_kernel(const float* __restrict__ pred_t, const float* __restrict__ rot_allo,
                                                               const float* __restrict__ camK, const float* __restrict__ center,
                                                               const float* __restrict__ ratio, const float* __restrict__ wh, int t_site,
                                                               int is_allo, double eps, int B, float* __restrict__ rot32,
                                                               float* __restrict__ trans32, double* __restrict__ rot64,
                                                               double* __restrict__ trans64) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double ox = t_site ? (double)pred_t[b * 3 + 0] : (double)pred_t[b * 3 + 0] * 0.0;
    const double oy = t_site ? (double)pred_t[b * 3 + 1] : (double)pred_t[b * 3 + 1] * 0.0;
    const double cx = ox * (double)wh[b * 2 + 0] + (double)center[b * 2 + 0];
    const double cy = oy * (double)wh[b * 2 + 1] + (double)center[b * 2 + 1];
    const double z = (double)pred_t[b * 3 + 2] * (double)ratio[b];
    const double t[3] = {z * (cx - (double)camK[b * 9 + 2]) / (double)camK[b * 9 + 0],
                         z * (cy - (double)camK[b * 9 + 5]) / (double)camK[b * 9 + 4], z};
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (double)rot_allo[b * 9 + i];
    if (is_allo) {
        const double n = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + eps;
        const double rx = t[0] / n, ry = t[1] / n, rz = t[2] / n;
        const double angle = acos(rz);
        // cross((0, 0, 1), obj_ray) = (-ry, rx, 0)
        double ax = 0.0 * rz - ry, ay = rx - 0.0 * rz, az = 0.0 * ry - 0.0 * rx;
        const double an = sqrt((ax * ax + ay * ay) + az * az) + eps;
        ax = ax / an; ay = ay / an; az = az / an;
        const double h = angle / 2.0, sh = sin(h);
        double qw = cos(h), qx = ax * sh, qy = ay * sh, qz = az * sh;
        // quat2mat_torch (pose_utils.py:348-396, eps = 0): the quaternion is normalised there
        const double qn = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
        qw = qw / qn; qx = qx / qn; qy = qy / qn; qz = qz / qn;
        const double X = qx * 2.0, Y = qy * 2.0, Z = qz * 2.0;
        const double wX = qw * X, wY = qw * Y, wZ = qw * Z, xX = qx * X, xY = qx * Y, xZ = qx * Z, yY = qy * Y, yZ = qy * Z, zZ = qz * Z;
        const double M[9] = {1.0 - (yY + zZ), xY - wZ, xZ + wY, xY + wZ, 1.0 - (xX + zZ), yZ - wX, xZ - wY, yZ + wX, 1.0 - (xX + yY)};
        double E[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) E[3 * i + j] = (M[3 * i + 0] * R[0 + j] + M[3 * i + 1] * R[3 + j]) + M[3 * i + 2] * R[6 + j];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = E[i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        rot32[b * 9 + i] = (float)R[i];
        if (rot64) rot64[b * 9 + i] = R[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        trans32[b * 3 + i] = (float)t[i];
        if (trans64) trans64[b * 3 + i] = t[i];
    }
}

struct LossArgs {
    const float *rot, *trans, *size, *nocs, *ivfc, *gt_rot, *gt_trans, *gt_size, *nocs_scale;
    const int* sym0;
    const float *gt_mask, *gt_mask_sp, *gt_nocs, *gt_ivfc, *model_point;
    const double* sym_table;
    int B, P, r_sym, r_angle, smoothl1;
    double *slabs, *record;
};

// one quarter of one coordinate map: sum of mask * huber(pred * mask - gt' * mask) and of the mask over this thread's 4 pixels
__device__ __forceinline__ void coor_quarter(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                                             int b, int p, bool rotate, const Mat3& rs, double& num, double& den) {
    const long base = (long)b * 3 * NPIX + p;
    const f32x4 m4 = *reinterpret_cast<const f32x4*>(mask + (long)b * NPIX + p);
    f32x4 pc[3], gc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pc[c] = *reinterpret_cast<const f32x4*>(pred + base + (long)c * NPIX);
        gc[c] = *reinterpret_cast<const f32x4*>(gt + base + (long)c * NPIX);
    }
    num = 0.0;
    den = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double mk = (double)m4[e];
        const double g0 = (double)gc[0][e], g1 = (double)gc[1][e], g2 = (double)gc[2][e];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double g = rotate ? (rs.m[3 * c + 0] * g0 + rs.m[3 * c + 1] * g1) + rs.m[3 * c + 2] * g2 : (c == 0 ? g0 : c == 1 ? g1 : g2);
            const double d = fabs((double)pc[c][e] * mk - g * mk);
            const double l = d > HUBER ? d - HUBER / 2.0 : d * d / (2.0 * HUBER);
            num = num + mk * l;
        }
        den = den + mk;
    }
}

__global__ __launch_bounds__(WG) void pose_loss_partials_kernel(const LossArgs a) {
    __shared__ double s_slot[WG / 64];
    const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int any = 0;
    for (int i = tid; i < a.B; i += WG) any |= a.sym0[i] == 1;
    const bool search = __syncthreads_or(any) != 0 && !a.r_sym;       // sym_mask.sum() > 0 and 'sym' not in r_type
    const bool is_sym = a.sym0[b] == 1;
    Mat3 Rp, Rg;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        Rp.m[i] = (double)a.rot[b * 9 + i];
        Rg.m[i] = (double)a.gt_rot[b * 9 + i];
    }
    const double re0 = re_deg(Rp, Rg);
    int idx = -1;
    double re_best = re0;
    Mat3 Rc = Rg;                                                     // the closest ground truth, fp32 values
    if (search && is_sym) {
        double best = __builtin_inf();
        int bk = 1 << 30;
        for (int j = 0; j < 6; ++j) {
            const int k = j * 64 + lane;
            if (k < GPL_SYM) {
                const double r = re_deg(Rp, times_sym_y(Rg, a.sym_table[2 * k], a.sym_table[2 * k + 1]));
                if (r < best) { best = r; bk = k; }                   // k grows: a tie keeps the earlier candidate
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ob = __shfl_xor(best, off, 64);
            const int ok = __shfl_xor(bk, off, 64);
            if (ob < best || (ob == best && ok < bk)) { best = ob; bk = ok; }
        }
        if (best < re0 && bk < GPL_SYM) {                             // strict: a tie keeps the unrotated ground truth
            idx = bk;
            re_best = best;
            const Mat3 G = times_sym_y(Rg, a.sym_table[2 * bk], a.sym_table[2 * bk + 1]);
#pragma unroll
            for (int i = 0; i < 9; ++i) Rc.m[i] = (double)(float)G.m[i];   // torch.tensor(..., dtype=gt_rots.dtype)
        }
    }
    Mat3 rs;                                                          // rot_sym = closest^T gt_rot: not exactly I, kept as it is
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) rs.m[3 * i + j] = (Rc.m[0 + i] * Rg.m[0 + j] + Rc.m[3 + i] * Rg.m[3 + j]) + Rc.m[6 + i] * Rg.m[6 + j];

    const int p = s * PIX_PER_WG + tid * 4;
    double n_num, n_den, i_num, i_den;
    coor_quarter(a.nocs, a.gt_nocs, a.gt_mask, b, p, search, rs, n_num, n_den);
    coor_quarter(a.ivfc, a.gt_ivfc, a.gt_mask_sp, b, p, search, rs, i_num, i_den);

    // point matching: point q of the crop belongs to workgroup (q / WG) % GPL_SPLIT
    const bool zero_xz = a.r_sym && is_sym;
    double pm = 0.0;
    for (int q = s * WG + tid; q < a.P; q += GPL_SPLIT * WG) {
        const float* mp = a.model_point + ((long)b * a.P + q) * 3;
        const double x = zero_xz ? 0.0 : (double)mp[0], y = (double)mp[1], z = zero_xz ? 0.0 : (double)mp[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double pp = (Rp.m[3 * c + 0] * x + Rp.m[3 * c + 1] * y) + Rp.m[3 * c + 2] * z;
            const double gp = (Rc.m[3 * c + 0] * x + Rc.m[3 * c + 1] * y) + Rc.m[3 * c + 2] * z;
            pm = pm + pose_term(pp, gp, a.smoothl1);
        }
    }
    pm = wg_sum(pm, s_slot, lane, wave);
    n_num = wg_sum(n_num, s_slot, lane, wave);
    n_den = wg_sum(n_den, s_slot, lane, wave);
    i_num = wg_sum(i_num, s_slot, lane, wave);
    i_den = wg_sum(i_den, s_slot, lane, wave);
    if (tid != 0) return;
    double* slab = a.slabs + ((long)b * GPL_SPLIT + s) * GPL_PART;
    slab[0] = pm; slab[1] = n_num; slab[2] = n_den; slab[3] = i_num; slab[4] = i_den; slab[5] = 0.0; slab[6] = 0.0; slab[7] = 0.0;
    if (s != 0) return;
    // the small terms of the crop
    double rot1 = 0.0;
    if (a.r_angle) {
        const double c = fmin(0.99999, fmax(-0.99999, (trace_abt(Rc, Rp) - 1.0) / 2.0));
        rot1 = smooth_l1(acos(c), 0.0, 0.2);
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const double mk = (zero_xz && (i % 3) != 1) ? 0.0 : 1.0;
            rot1 = rot1 + (a.r_sym ? pose_term(Rp.m[i] * mk, Rc.m[i] * mk, a.smoothl1) : pose_term(Rp.m[i], Rc.m[i], a.smoothl1));
        }
    }
    const double sc = (double)a.nocs_scale[b];
    double tran = 0.0, size = 0.0, te2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double pt = (double)a.trans[b * 3 + i], gt = (double)a.gt_trans[b * 3 + i] / sc;
        tran = tran + pose_term(pt, gt, a.smoothl1);
        size = size + pose_term((double)a.size[b * 3 + i], (double)a.gt_size[b * 3 + i] / sc, a.smoothl1);
        te2 = te2 + (gt - pt) * (gt - pt);
    }
    double* rec = a.record + (long)b * GPL_RECORD;
    rec[0] = (double)idx; rec[1] = re_best; rec[2] = re0; rec[3] = sqrt(te2); rec[4] = rot1; rec[5] = tran; rec[6] = size;
    rec[7] = search ? 1.0 : 0.0;
}

__global__ __launch_bounds__(WG) void pose_loss_reduce_kernel(const double* __restrict__ slabs, const double* __restrict__ record, int B, int P,
                                                              int r_angle, double rot_1_w, double tran_w, double size_w, double prop_pm_w,
                                                              double coor_w, double* __restrict__ out64, float* __restrict__ out32,
                                                              double* __restrict__ acc) {
    __shared__ double s_slot[WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};         // rot1, tran, size, pm, nocs, ivfc, re, te
    for (int b = tid; b < B; b += WG) {
        const double* rec = record + (long)b * GPL_RECORD;
        double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < GPL_SPLIT; ++s) {
            const double* slab = slabs + ((long)b * GPL_SPLIT + s) * GPL_PART;
#pragma unroll
            for (int i = 0; i < 5; ++i) q[i] = q[i] + slab[i];
        }
        v[0] = v[0] + rec[4]; v[1] = v[1] + rec[5]; v[2] = v[2] + rec[6];
        v[3] = v[3] + q[0];
        v[4] = v[4] + q[1] / (q[2] + 1e-5);
        v[5] = v[5] + q[3] / (q[4] + 1e-5);
        v[6] = v[6] + rec[2]; v[7] = v[7] + rec[3];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = wg_sum(v[i], s_slot, lane, wave);
    if (tid != 0) return;
    const double n = (double)B;
    double o[GPL_OUT];
    o[0] = rot_1_w * (v[0] / (r_angle ? n : 9.0 * n));
    o[1] = tran_w * (v[1] / (3.0 * n));
    o[2] = size_w * (v[2] / (3.0 * n));
    o[3] = prop_pm_w * (v[3] / (3.0 * n * (double)P));
    o[4] = coor_w * (v[4] / n);
    o[5] = coor_w * (v[5] / n);
    o[6] = v[6] / n;
    o[7] = v[7] / n;
#pragma unroll
    for (int i = 0; i < GPL_OUT; ++i) {
        out64[i] = o[i];
        out32[i] = (float)o[i];
    }
    if (acc) {
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[i] = acc[i] + n * o[i];
        acc[6] = acc[6] + v[6];
        acc[7] = acc[7] + v[7];
        acc[8] = acc[8] + n;
        acc[9] = acc[9] + 1.0;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int gpl_pose_decode_train(const float* pred_t, const float* rot_allo, const float* cam_K, const float* bbox_center,
                                     const float* resize_ratio, const float* roi_wh, int t_site, int is_allo, double eps, int B,
                                     float* rot32, float* trans32, double* rot64, double* trans64, void* stream) {
    GP_REQUIRE(pred_t && rot_allo && cam_K && bbox_center && resize_ratio && roi_wh && rot32 && trans32, "gpl_pose_decode_train: null pointer");
    GP_REQUIRE(B > 0 && B <= (1 << 20), "gpl_pose_decode_train: bad batch size %d", B);
    hipStream_t s = (hipStream_t)stream;
    gp_timing_before(s, GP_KC_SMALL, (double)B * 120, (double)B * 200);
    hipLaunchKernelGGL(pose_decode_train_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, pred_t, rot_allo, cam_K, bbox_center, resize_ratio, roi_wh,
                       t_site, is_allo, eps, B, rot32, trans32, rot64, trans64);
    GP_LAUNCH_CHECK("gpl_pose_decode_train");
}

extern "C" int gpl_pose_loss_partials(const float* rot, const float* trans, const float* size, const float* nocs_coor, const float* ivfc_coor,
                                      const float* gt_rot, const float* gt_trans, const float* gt_size, const float* nocs_scale,
                                      const int* sym0, const float* gt_mask, const float* gt_mask_sp, const float* gt_nocs,
                                      const float* gt_ivfc, const float* model_point, const double* sym_table, int B, int P, int R, int r_sym,
                                      int r_angle, int smoothl1, double* slabs, double* record, void* stream) {
    GP_REQUIRE(rot && trans && size && nocs_coor && ivfc_coor && gt_rot && gt_trans && gt_size && nocs_scale && sym0 && gt_mask && gt_mask_sp &&
                   gt_nocs && gt_ivfc && model_point && sym_table && slabs && record, "gpl_pose_loss_partials: null pointer");
    GP_REQUIRE(R == GPL_RES, "gpl_pose_loss_partials: the maps are %d x %d, not %d x %d", GPL_RES, GPL_RES, R, R);
    GP_REQUIRE(B > 0 && B <= 65535 && P > 0 && P <= (1 << 24), "gpl_pose_loss_partials: bad shape B %d P %d", B, P);
    GP_REQUIRE(aligned16(nocs_coor) && aligned16(ivfc_coor) && aligned16(gt_nocs) && aligned16(gt_ivfc) && aligned16(gt_mask) && aligned16(gt_mask_sp),
               "gpl_pose_loss_partials: the maps and masks must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    LossArgs a{rot, trans, size, nocs_coor, ivfc_coor, gt_rot, gt_trans, gt_size, nocs_scale, sym0, gt_mask, gt_mask_sp, gt_nocs, gt_ivfc,
               model_point, sym_table, B, P, r_sym, r_angle, smoothl1, slabs, record};
    gp_timing_before(s, GP_KC_SMALL, (double)B * (NPIX * 2 * 40 + (double)P * 40), (double)B * (NPIX * 14 * 4 + (double)P * 12));
    hipLaunchKernelGGL(pose_loss_partials_kernel, dim3(GPL_SPLIT, B), dim3(WG), 0, s, a);
    GP_LAUNCH_CHECK("gpl_pose_loss_partials");
}

extern "C" int gpl_pose_loss_reduce(const double* slabs, const double* record, int B, int P, int r_angle, double rot_1_w, double tran_w,
                                    double size_w, double prop_pm_w, double coor_w, double* out64, float* out32, double* acc, void* stream) {
    GP_REQUIRE(slabs && record && out64 && out32, "gpl_pose_loss_reduce: null pointer");
    GP_REQUIRE(B > 0 && B <= 65535 && P > 0 && P <= (1 << 24), "gpl_pose_loss_reduce: bad shape B %d P %d", B, P);
    hipStream_t s = (hipStream_t)stream;
    gp_timing_before(s, GP_KC_SMALL, (double)B * 40, (double)B * (GPL_SPLIT * GPL_PART + GPL_RECORD) * 8);
    hipLaunchKernelGGL(pose_loss_reduce_kernel, dim3(1), dim3(WG), 0, s, slabs, record, B, P, r_angle, rot_1_w, tran_w, size_w, prop_pm_w, coor_w,
                       out64, out32, acc);
    GP_LAUNCH_CHECK("gpl_pose_loss_reduce");
}
