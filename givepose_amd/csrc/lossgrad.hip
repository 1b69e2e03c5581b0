// The loss-gradient family (include/givepose_grad.h): backward of loss.hip.  Two kernels:
//   pose_loss_grad_kernel           grid (GPL_SPLIT, crop) like the forward: every workgroup rebuilds the crop's closest ground
//                                   truth and rot_sym from the forward's record (no search), then writes its quarter of the two map
//                                   gradients (16-byte loads and stores, 4 pixels per lane); workgroup 0 of the crop also sums the
//                                   point-matching gradient over the P points and writes d rot, d trans, d size
//   pose_decode_train_bwd_kernel    one thread per crop: reverse of pose_decode_train_kernel statement by statement, then of
//                                   rot6d_to_mat_batch
// float64 from the float32 inputs, rounded once on the way out.  The P-sum is store-and-sum like the forward's: the thread's points
// in turn, xor tree over the wave, the 4 waves as (w0 + w1) + (w2 + w3) -- no floating-point atomics, equal inputs give equal bits.
// Contraction is off for the whole file: the scalar arithmetic is written in the order of tests/pose_loss_grad_ref.py.
#include "common.hpp"
#include "../../include/givepose_grad.h"

#pragma clang fp contract(off)

namespace {

constexpr int WG = 256;
constexpr int NPIX = GPL_RES * GPL_RES;
constexpr int PIX_PER_WG = NPIX / GPL_SPLIT;
constexpr double HUBER = 0.03;            // PoseLoss.threshold
static_assert(PIX_PER_WG == WG * 4 && GPL_PART >= 5 && GPL_RECORD >= 8 && GPG_TERMS == 6 && GPG_SMALL == 15 && GPG_DECODE == 18, "layout");

__device__ __forceinline__ double wg_sum(double v, double* slot, int lane, int wave) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

__device__ __forceinline__ double sign0(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }
// d term(a, b) / d a, x = a - b: L1, or SmoothL1(beta 0.5)
__device__ __forceinline__ double pose_term_d(double x, int smoothl1) { return (smoothl1 && fabs(x) < 0.5) ? x / 0.5 : sign0(x); }

struct GradArgs {
    const float *rot, *trans, *size, *nocs, *ivfc, *gt_rot, *gt_trans, *gt_size, *nocs_scale;
    const int* sym0;
    const float *gt_mask, *gt_mask_sp, *gt_nocs, *gt_ivfc, *model_point;
    const double *sym_table, *slabs, *record, *gout;
    int B, P, r_sym, r_angle, smoothl1;
    double rot_1_w, tran_w, size_w, prop_pm_w, coor_w;
    float *g_rot, *g_trans, *g_size, *g_nocs, *g_ivfc;
    double* small64;
};

// one quarter of one map gradient: scale * mask * mask * huber'(|pred mask - gt' mask|) * sign, this thread's 4 pixels
__device__ __forceinline__ void coor_quarter_grad(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                                                  float* __restrict__ out, int b, int p, bool rotate, const double* rs, double scale) {
    const long base = (long)b * 3 * NPIX + p;
    const f32x4 m4 = *reinterpret_cast<const f32x4*>(mask + (long)b * NPIX + p);
    f32x4 pc[3], gc[3], o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pc[c] = *reinterpret_cast<const f32x4*>(pred + base + (long)c * NPIX);
        gc[c] = *reinterpret_cast<const f32x4*>(gt + base + (long)c * NPIX);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double mk = (double)m4[e];
        const double g0 = (double)gc[0][e], g1 = (double)gc[1][e], g2 = (double)gc[2][e];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double g = rotate ? (rs[3 * c + 0] * g0 + rs[3 * c + 1] * g1) + rs[3 * c + 2] * g2 : (c == 0 ? g0 : c == 1 ? g1 : g2);
            const double x = (double)pc[c][e] * mk - g * mk;
            const double d = fabs(x);
            const double dl = d > HUBER ? 1.0 : (2.0 * d) / (2.0 * HUBER);
            o[c][e] = (float)(((scale * mk) * (dl * sign0(x))) * mk);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(out + base + (long)c * NPIX) = o[c];
}

__global__ __launch_bounds__(WG) void pose_loss_grad_kernel(const GradArgs a) {
    __shared__ double s_slot[WG / 64];
    const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* rec = a.record + (long)b * GPL_RECORD;
    const int idx = (int)rec[0];
    const bool branch = rec[7] != 0.0;
    const bool is_sym = a.sym0[b] == 1;
    double w[GPG_TERMS];
#pragma unroll
    for (int k = 0; k < GPG_TERMS; ++k) w[k] = a.gout ? a.gout[k] : 1.0;
    double Rp[9], Rg[9], Rc[9], rs[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        Rp[i] = (double)a.rot[b * 9 + i];
        Rg[i] = (double)a.gt_rot[b * 9 + i];
        Rc[i] = Rg[i];
    }
    if (idx >= 0 && idx < GPL_SYM) {                                  // gt_rot * S_idx rounded once to fp32, the forward's order
        const double c = a.sym_table[2 * idx], sn = a.sym_table[2 * idx + 1];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Rc[3 * i + 0] = (double)(float)(Rg[3 * i + 0] * c - Rg[3 * i + 2] * sn);
            Rc[3 * i + 1] = (double)(float)Rg[3 * i + 1];
            Rc[3 * i + 2] = (double)(float)(Rg[3 * i + 0] * sn + Rg[3 * i + 2] * c);
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) rs[3 * i + j] = (Rc[0 + i] * Rg[0 + j] + Rc[3 + i] * Rg[3 + j]) + Rc[6 + i] * Rg[6 + j];

    // the mask sums, the crop's workgroups in the order gpl_pose_loss_reduce adds them
    double dn = 0.0, di = 0.0;
#pragma unroll
    for (int k = 0; k < GPL_SPLIT; ++k) {
        const double* slab = a.slabs + ((long)b * GPL_SPLIT + k) * GPL_PART;
        dn = dn + slab[2];
        di = di + slab[4];
    }
    const double n = (double)a.B;
    const int p = s * PIX_PER_WG + tid * 4;
    coor_quarter_grad(a.nocs, a.gt_nocs, a.gt_mask, a.g_nocs, b, p, branch, rs, ((w[4] * a.coor_w) / n) / (dn + 1e-5));
    coor_quarter_grad(a.ivfc, a.gt_ivfc, a.gt_mask_sp, a.g_ivfc, b, p, branch, rs, ((w[5] * a.coor_w) / n) / (di + 1e-5));
    if (s != 0) return;

    // point matching: d/d rot[c][j] = sum_q term'(pp_c - gp_c) * point_j
    const bool zero_xz = a.r_sym && is_sym;
    double pm[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = tid; q < a.P; q += WG) {
        const float* mp = a.model_point + ((long)b * a.P + q) * 3;
        const double x = zero_xz ? 0.0 : (double)mp[0], y = (double)mp[1], z = zero_xz ? 0.0 : (double)mp[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double pp = (Rp[3 * c + 0] * x + Rp[3 * c + 1] * y) + Rp[3 * c + 2] * z;
            const double gp = (Rc[3 * c + 0] * x + Rc[3 * c + 1] * y) + Rc[3 * c + 2] * z;
            const double t = pose_term_d(pp - gp, a.smoothl1);
            pm[3 * c + 0] = pm[3 * c + 0] + t * x;
            pm[3 * c + 1] = pm[3 * c + 1] + t * y;
            pm[3 * c + 2] = pm[3 * c + 2] + t * z;
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) pm[i] = wg_sum(pm[i], s_slot, lane, wave);
    if (tid != 0) return;

    double g[GPG_SMALL];
    const double k_pm = (w[3] * a.prop_pm_w) / ((3.0 * n) * (double)a.P);
    if (a.r_angle) {
        double tr = Rc[0] * Rp[0];
#pragma unroll
        for (int i = 1; i < 9; ++i) tr = tr + Rc[i] * Rp[i];
        const double u = (tr - 1.0) / 2.0;
        const double c = fmin(0.99999, fmax(-0.99999, u));
        const double pass = (u >= -0.99999 && u <= 0.99999) ? 1.0 : 0.0;
        const double ang = acos(c);
        const double ds = ang < 0.2 ? ang / 0.2 : sign0(ang);
        const double k = (((((w[0] * a.rot_1_w) / n) * ds) * (-1.0 / sqrt(1.0 - c * c))) * pass) * 0.5;
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] = k * Rc[i] + k_pm * pm[i];
    } else {
        const double k = (w[0] * a.rot_1_w) / (9.0 * n);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const double mk = (zero_xz && (i % 3) != 1) ? 0.0 : 1.0;
            const double x = a.r_sym ? Rp[i] * mk - Rc[i] * mk : Rp[i] - Rc[i];
            g[i] = (k * pose_term_d(x, a.smoothl1)) * mk + k_pm * pm[i];
        }
    }
    const double sc = (double)a.nocs_scale[b];
    const double k_t = (w[1] * a.tran_w) / (3.0 * n), k_s = (w[2] * a.size_w) / (3.0 * n);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g[9 + i] = k_t * pose_term_d((double)a.trans[b * 3 + i] - (double)a.gt_trans[b * 3 + i] / sc, a.smoothl1);
        g[12 + i] = k_s * pose_term_d((double)a.size[b * 3 + i] - (double)a.gt_size[b * 3 + i] / sc, a.smoothl1);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) a.g_rot[b * 9 + i] = (float)g[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a.g_trans[b * 3 + i] = (float)g[9 + i];
        a.g_size[b * 3 + i] = (float)g[12 + i];
    }
    if (a.small64) {
#pragma unroll
        for (int i = 0; i < GPG_SMALL; ++i) a.small64[(long)b * GPG_SMALL + i] = g[i];
    }
}

// v = u / den, den = |u| + eps (or |u| itself): gu = gv / den + gden * u / |u|, gden = -sum(gv u) / den^2; d|u| = 0 at u = 0
__device__ __forceinline__ void div_norm_bwd3(const double* u, const double* gv, double nrm, double den, double* gu) {
    const double gden = -(((gv[0] * u[0] + gv[1] * u[1]) + gv[2] * u[2]) / (den * den));
#pragma unroll
    for (int i = 0; i < 3; ++i) gu[i] = gv[i] / den + (nrm > 0.0 ? gden * (u[i] / nrm) : 0.0);
}
// c = a x b
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

struct DecArgs {
    const float *g_rot_ego, *g_trans, *pred_t, *rot_allo, *camK, *center, *ratio, *wh, *rot6d;
    int t_site, is_allo;
    double eps;
    int B;
    float *g_rot_allo, *g_pred_t, *g_rot6d;
    double* g64;
};

__global__ __launch_bounds__(64) void pose_decode_train_bwd_kernel(const DecArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const double eps = a.eps;
    // the forward, as pose_decode_train_kernel writes it
    const double w0 = (double)a.wh[b * 2 + 0], w1 = (double)a.wh[b * 2 + 1];
    const double ox = a.t_site ? (double)a.pred_t[b * 3 + 0] : (double)a.pred_t[b * 3 + 0] * 0.0;
    const double oy = a.t_site ? (double)a.pred_t[b * 3 + 1] : (double)a.pred_t[b * 3 + 1] * 0.0;
    const double cx = ox * w0 + (double)a.center[b * 2 + 0];
    const double cy = oy * w1 + (double)a.center[b * 2 + 1];
    const double ratio = (double)a.ratio[b];
    const double z = (double)a.pred_t[b * 3 + 2] * ratio;
    const double fx = (double)a.camK[b * 9 + 0], fy = (double)a.camK[b * 9 + 4];
    const double ux = cx - (double)a.camK[b * 9 + 2], uy = cy - (double)a.camK[b * 9 + 5];
    const double t[3] = {z * ux / fx, z * uy / fy, z};
    double R[9], gE[9], gR[9], gt[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        R[i] = (double)a.rot_allo[b * 9 + i];
        gE[i] = (double)a.g_rot_ego[b * 9 + i];
        gR[i] = gE[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) gt[i] = (double)a.g_trans[b * 3 + i];
    // rot6d_to_mat_batch: x = normalize(xr), zr = x x yr, z = normalize(zr), y = z x x, rot[:, 0 / 1 / 2] = x / y / z.  With the raw
    // vector at hand the chain starts from it in float64, as the reference's does: rot_allo's float32 rounding stays out
    double xr[3] = {1.0, 0.0, 0.0}, yr[3] = {0.0, 1.0, 0.0}, x[3], zr[3], zz[3], yy[3];
    if (a.rot6d) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            xr[i] = (double)a.rot6d[b * 6 + i];
            yr[i] = (double)a.rot6d[b * 6 + 3 + i];
        }
    }
    const double xn = sqrt((xr[0] * xr[0] + xr[1] * xr[1]) + xr[2] * xr[2]), xd = fmax(xn, 1e-12);
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = xr[i] / xd;
    cross3(x, yr, zr);
    const double zn = sqrt((zr[0] * zr[0] + zr[1] * zr[1]) + zr[2] * zr[2]), zd = fmax(zn, 1e-12);
#pragma unroll
    for (int i = 0; i < 3; ++i) zz[i] = zr[i] / zd;
    cross3(zz, x, yy);
    if (a.rot6d) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            R[3 * i + 0] = x[i];
            R[3 * i + 1] = yy[i];
            R[3 * i + 2] = zz[i];
        }
    }
    if (a.is_allo) {
        const double tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]), n = tn + eps;
        const double r[3] = {t[0] / n, t[1] / n, t[2] / n};
        const double angle = acos(r[2]);
        const double ar[3] = {0.0 * r[2] - r[1], r[0] - 0.0 * r[2], 0.0 * r[1] - 0.0 * r[0]};
        const double arn = sqrt((ar[0] * ar[0] + ar[1] * ar[1]) + ar[2] * ar[2]), an = arn + eps;
        const double ax[3] = {ar[0] / an, ar[1] / an, ar[2] / an};
        const double h = angle / 2.0, sh = sin(h), ch = cos(h);
        const double u[4] = {ch, ax[0] * sh, ax[1] * sh, ax[2] * sh};
        const double qn = sqrt(((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3]);
        const double qw = u[0] / qn, qx = u[1] / qn, qy = u[2] / qn, qz = u[3] / qn;
        const double X = qx * 2.0, Y = qy * 2.0, Z = qz * 2.0;
        const double wX = qw * X, wY = qw * Y, wZ = qw * Z, xX = qx * X, xY = qx * Y, xZ = qx * Z, yY = qy * Y, yZ = qy * Z, zZ = qz * Z;
        const double M[9] = {1.0 - (yY + zZ), xY - wZ, xZ + wY, xY + wZ, 1.0 - (xX + zZ), yZ - wX, xZ - wY, yZ + wX, 1.0 - (xX + yY)};
        // rot_ego = M rot_allo
        double gM[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                gM[3 * i + k] = (gE[3 * i + 0] * R[3 * k + 0] + gE[3 * i + 1] * R[3 * k + 1]) + gE[3 * i + 2] * R[3 * k + 2];
                gR[3 * i + k] = (M[0 + i] * gE[0 + k] + M[3 + i] * gE[3 + k]) + M[6 + i] * gE[6 + k];
            }
        // quat2mat_torch
        const double g_yY = -gM[0] - gM[8], g_zZ = -gM[0] - gM[4], g_xX = -gM[4] - gM[8];
        const double g_xY = gM[1] + gM[3], g_wZ = gM[3] - gM[1], g_xZ = gM[2] + gM[6], g_wY = gM[2] - gM[6];
        const double g_yZ = gM[5] + gM[7], g_wX = gM[7] - gM[5];
        const double g_X = (g_wX * qw + g_xX * qx), g_Y = (g_wY * qw + g_xY * qx) + g_yY * qy;
        const double g_Z = ((g_wZ * qw + g_xZ * qx) + g_yZ * qy) + g_zZ * qz;
        double gq[4];
        gq[0] = (g_wX * X + g_wY * Y) + g_wZ * Z;
        gq[1] = (((g_xX * X + g_xY * Y) + g_xZ * Z) + g_X * 2.0);
        gq[2] = ((g_yY * Y + g_yZ * Z) + g_Y * 2.0);
        gq[3] = (g_zZ * Z + g_Z * 2.0);
        // q = u / |u|
        const double gqn = -((((gq[0] * u[0] + gq[1] * u[1]) + gq[2] * u[2]) + gq[3] * u[3]) / (qn * qn));
        double gu[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) gu[i] = gq[i] / qn + (qn > 0.0 ? gqn * (u[i] / qn) : 0.0);
        // u = (cos h, axis sin h), h = angle / 2
        const double g_h = ((gu[1] * ax[0] + gu[2] * ax[1]) + gu[3] * ax[2]) * ch - gu[0] * sh;
        const double g_angle = g_h / 2.0;
        const double gax[3] = {gu[1] * sh, gu[2] * sh, gu[3] * sh};
        double gar[3], gr[3];
        div_norm_bwd3(ar, gax, arn, an, gar);
        // axis_raw = (0, 0, 1) x obj_ray = (-ry, rx, 0); angle = acos(rz)
        gr[0] = gar[1];
        gr[1] = -gar[0];
        gr[2] = g_angle * (-1.0 / sqrt(1.0 - r[2] * r[2]));
        double gt2[3];
        div_norm_bwd3(t, gr, tn, n, gt2);
#pragma unroll
        for (int i = 0; i < 3; ++i) gt[i] = gt[i] + gt2[i];
    }
    // t = (z ux / fx, z uy / fy, z)
    const double g_z = (gt[0] * ux / fx + gt[1] * uy / fy) + gt[2];
    const double g_cx = gt[0] * z / fx, g_cy = gt[1] * z / fy;
    double o[GPG_DECODE];
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = gR[i];
    o[9] = a.t_site ? g_cx * w0 : (g_cx * w0) * 0.0;
    o[10] = a.t_site ? g_cy * w1 : (g_cy * w1) * 0.0;
    o[11] = g_z * ratio;
#pragma unroll
    for (int i = 12; i < GPG_DECODE; ++i) o[i] = 0.0;
    if (a.rot6d) {
        double gx[3], gy[3], gz[3], c1[3], c2[3], gzr[3], gxr[3], gyr[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gx[i] = gR[3 * i + 0];
            gy[i] = gR[3 * i + 1];
            gz[i] = gR[3 * i + 2];
        }
        cross3(x, gy, c1);                         // y = z x x: gz += x x gy, gx += gy x z
        cross3(gy, zz, c2);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gz[i] = gz[i] + c1[i];
            gx[i] = gx[i] + c2[i];
        }
        // F.normalize: v / max(|v|, 1e-12); the clamp passes the norm's gradient where |v| >= 1e-12
        div_norm_bwd3(zr, gz, zn >= 1e-12 ? zn : 0.0, zd, gzr);
        cross3(yr, gzr, c1);                       // zr = x x yr: gx += yr x gzr, gyr = gzr x x
        cross3(gzr, x, gyr);
#pragma unroll
        for (int i = 0; i < 3; ++i) gx[i] = gx[i] + c1[i];
        div_norm_bwd3(xr, gx, xn >= 1e-12 ? xn : 0.0, xd, gxr);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            o[12 + i] = gxr[i];
            o[15 + i] = gyr[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) a.g_rot_allo[b * 9 + i] = (float)o[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) a.g_pred_t[b * 3 + i] = (float)o[9 + i];
    if (a.rot6d) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.g_rot6d[b * 6 + i] = (float)o[12 + i];
    }
    if (a.g64) {
#pragma unroll
        for (int i = 0; i < GPG_DECODE; ++i) a.g64[(long)b * GPG_DECODE + i] = o[i];
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int gpg_pose_loss_grad(const float* rot, const float* trans, const float* size, const float* nocs_coor, const float* ivfc_coor,
                                  const float* gt_rot, const float* gt_trans, const float* gt_size, const float* nocs_scale, const int* sym0,
                                  const float* gt_mask, const float* gt_mask_sp, const float* gt_nocs, const float* gt_ivfc,
                                  const float* model_point, const double* sym_table, const double* slabs, const double* record,
                                  const double* gout, int B, int P, int R, int r_sym, int r_angle, int smoothl1, double rot_1_w,
                                  double tran_w, double size_w, double prop_pm_w, double coor_w, float* g_rot, float* g_trans,
                                  float* g_size, float* g_nocs, float* g_ivfc, double* small64, void* stream) {
    GP_REQUIRE(rot && trans && size && nocs_coor && ivfc_coor && gt_rot && gt_trans && gt_size && nocs_scale && sym0 && gt_mask && gt_mask_sp &&
                   gt_nocs && gt_ivfc && model_point && sym_table && slabs && record && g_rot && g_trans && g_size && g_nocs && g_ivfc,
               "gpg_pose_loss_grad: null pointer");
    GP_REQUIRE(R == GPL_RES, "gpg_pose_loss_grad: the maps are %d x %d, not %d x %d", GPL_RES, GPL_RES, R, R);
    GP_REQUIRE(B > 0 && B <= 65535 && P > 0 && P <= (1 << 24), "gpg_pose_loss_grad: bad shape B %d P %d", B, P);
    GP_REQUIRE(aligned16(nocs_coor) && aligned16(ivfc_coor) && aligned16(gt_nocs) && aligned16(gt_ivfc) && aligned16(gt_mask) &&
                   aligned16(gt_mask_sp) && aligned16(g_nocs) && aligned16(g_ivfc),
               "gpg_pose_loss_grad: the maps, the masks and the map gradients must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    GradArgs a{rot, trans, size, nocs_coor, ivfc_coor, gt_rot, gt_trans, gt_size, nocs_scale, sym0, gt_mask, gt_mask_sp, gt_nocs, gt_ivfc,
               model_point, sym_table, slabs, record, gout, B, P, r_sym, r_angle, smoothl1, rot_1_w, tran_w, size_w, prop_pm_w, coor_w,
               g_rot, g_trans, g_size, g_nocs, g_ivfc, small64};
    gp_timing_before(s, GP_KC_SMALL, (double)B * (NPIX * 2 * 40 + (double)P * 60), (double)B * (NPIX * 20 * 4 + (double)P * 12));
    hipLaunchKernelGGL(pose_loss_grad_kernel, dim3(GPL_SPLIT, B), dim3(WG), 0, s, a);
    GP_LAUNCH_CHECK("gpg_pose_loss_grad");
}

extern "C" int gpg_pose_decode_train_backward(const float* g_rot_ego, const float* g_trans, const float* pred_t, const float* rot_allo,
                                              const float* cam_K, const float* bbox_center, const float* resize_ratio, const float* roi_wh,
                                              const float* rot6d, int t_site, int is_allo, double eps, int B, float* g_rot_allo,
                                              float* g_pred_t, float* g_rot6d, double* g64, void* stream) {
    GP_REQUIRE(g_rot_ego && g_trans && pred_t && rot_allo && cam_K && bbox_center && resize_ratio && roi_wh && g_rot_allo && g_pred_t,
               "gpg_pose_decode_train_backward: null pointer");
    GP_REQUIRE(!rot6d || g_rot6d, "gpg_pose_decode_train_backward: rot6d is given without g_rot6d");
    GP_REQUIRE(B > 0 && B <= (1 << 20), "gpg_pose_decode_train_backward: bad batch size %d", B);
    hipStream_t s = (hipStream_t)stream;
    DecArgs a{g_rot_ego, g_trans, pred_t, rot_allo, cam_K, bbox_center, resize_ratio, roi_wh, rot6d, t_site, is_allo, eps, B,
              g_rot_allo, g_pred_t, g_rot6d, g64};
    gp_timing_before(s, GP_KC_SMALL, (double)B * 500, (double)B * 300);
    hipLaunchKernelGGL(pose_decode_train_bwd_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, a);
    GP_LAUNCH_CHECK("gpg_pose_decode_train_backward");
}
