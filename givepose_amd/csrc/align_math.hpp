// Umeyama's similarity fit from a 3x3 covariance, in float64 with static indices only (no per-thread array is indexed at run
// time: no scratch segment).  Plain C++ that also compiles for the host (GPA_HD empty), which is how it is checked on a CPU.
//
// The reference (tools/align_utils.py:24-35) takes U, D, Vh from LAPACK, and where det U det Vh < 0 negates the last singular
// value and the last column of U.  Here the SVD is a one-sided Jacobi iteration (Hestenes): the columns of A = C V are rotated
// in pairs until they are orthogonal; then sigma_k = |a_k| and u_k = a_k / sigma_k.  With the singular values sorted in descending
// order, u_3 := u_1 x u_2 and v_3 := v_1 x v_2 make both factors proper rotations, so R = U V^T is the reference's rotation
// after its sign fix, and d_3 = u_3^T C v_3 is the last singular value WITH the reference's sign (negative exactly in the
// reflection case, det C < 0).  Neither needs a third singular vector from a (near-)null space, so a rank-2 covariance is fine.
#pragma once
#include <math.h>

#ifndef GPA_HD
#define GPA_HD __device__ __forceinline__
#endif

namespace gpa {

struct V3 { double x, y, z; };
GPA_HD double dot3(const V3& a, const V3& b) { return fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)); }
GPA_HD V3 cross3(const V3& a, const V3& b) {
    return V3{fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x))};
}
GPA_HD V3 scale3(const V3& a, double s) { return V3{a.x * s, a.y * s, a.z * s}; }

// one Hestenes rotation of the column pair (p, q) of A and of V
GPA_HD void jacobi_pair(V3& ap, V3& aq, V3& vp, V3& vq) {
    const double alpha = dot3(ap, ap), beta = dot3(aq, aq), gamma = dot3(ap, aq);
    const bool rot = fabs(gamma) > 1e-17 * sqrt(alpha * beta) && gamma != 0.0;
    const double zeta = (beta - alpha) / (2.0 * (rot ? gamma : 1.0));
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
    const double c0 = 1.0 / sqrt(fma(t, t, 1.0));
    const double c = rot ? c0 : 1.0, s = rot ? c0 * t : 0.0;
    const V3 np_{fma(c, ap.x, -(s * aq.x)), fma(c, ap.y, -(s * aq.y)), fma(c, ap.z, -(s * aq.z))};
    const V3 nq{fma(s, ap.x, c * aq.x), fma(s, ap.y, c * aq.y), fma(s, ap.z, c * aq.z)};
    const V3 wp{fma(c, vp.x, -(s * vq.x)), fma(c, vp.y, -(s * vq.y)), fma(c, vp.z, -(s * vq.z))};
    const V3 wq{fma(s, vp.x, c * vq.x), fma(s, vp.y, c * vq.y), fma(s, vp.z, c * vq.z)};
    ap = np_; aq = nq; vp = wp; vq = wq;
}

// conditional swaps written per component: a select between two structs becomes a select between their ADDRESSES, which puts
// them in memory (a scratch segment on the device)
GPA_HD void swap_if(bool sw, double& a, double& b) {
    const double t = sw ? a : b;
    a = sw ? b : a;
    b = t;
}
GPA_HD void swap_if(bool sw, V3& a, V3& b) {
    swap_if(sw, a.x, b.x); swap_if(sw, a.y, b.y); swap_if(sw, a.z, b.z);
}
GPA_HD void swap_if(bool sw, double& sa, double& sb, V3& a, V3& b, V3& va, V3& vb) {
    swap_if(sw, sa, sb); swap_if(sw, a, b); swap_if(sw, va, vb);
}

struct Fit {
    double scale;       // sum D / var
    double R[9];        // row-major
    double sigma[3];    // descending, the last with the reference's sign
    bool ok;            // false: rank < 2 or no source variance (GPA_RANK_TOL): scale and R are not to be used
};

constexpr int JACOBI_SWEEPS = 10;      // converges quadratically; a 3x3 is at working precision after 4-5 sweeps

// C row-major: C[3 i + j] = mean over the set of (tgt - mean tgt)_i (src - mean src)_j; var = mean of |src - mean src|^2
GPA_HD Fit umeyama_from_cov(const double (&C)[9], double var, double rank_tol) {
    V3 a0{C[0], C[3], C[6]}, a1{C[1], C[4], C[7]}, a2{C[2], C[5], C[8]};      // columns of A = C V, V = I
    V3 v0{1, 0, 0}, v1{0, 1, 0}, v2{0, 0, 1};
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        jacobi_pair(a0, a1, v0, v1);
        jacobi_pair(a0, a2, v0, v2);
        jacobi_pair(a1, a2, v1, v2);
    }
    double s0 = sqrt(dot3(a0, a0)), s1 = sqrt(dot3(a1, a1)), s2 = sqrt(dot3(a2, a2));
    swap_if(s0 < s1, s0, s1, a0, a1, v0, v1);
    swap_if(s1 < s2, s1, s2, a1, a2, v1, v2);
    swap_if(s0 < s1, s0, s1, a0, a1, v0, v1);
    Fit f;
    f.ok = s0 > 0.0 && s1 > rank_tol * s0 && var > 0.0 && s0 < 1e300 && var < 1e300;      // (the last two also refuse inf and NaN)
    const double i0 = 1.0 / (f.ok ? s0 : 1.0), i1 = 1.0 / (f.ok ? s1 : 1.0);
    const V3 u0 = scale3(a0, i0);
    V3 u1 = scale3(a1, i1);
    // u1 is orthogonal to u0 to eps relative to |a1|; one Gram-Schmidt step and a renormalisation make U orthonormal to eps
    const double g = dot3(u0, u1);
    u1 = V3{fma(-g, u0.x, u1.x), fma(-g, u0.y, u1.y), fma(-g, u0.z, u1.z)};
    u1 = scale3(u1, 1.0 / sqrt(f.ok ? dot3(u1, u1) : 1.0));
    const V3 u2 = cross3(u0, u1), w2 = cross3(v0, v1);
    // C w2, then d3 = u2 . (C w2)
    const V3 cw{fma(C[2], w2.z, fma(C[1], w2.y, C[0] * w2.x)), fma(C[5], w2.z, fma(C[4], w2.y, C[3] * w2.x)),
                fma(C[8], w2.z, fma(C[7], w2.y, C[6] * w2.x))};
    const double d3 = dot3(u2, cw);
    f.sigma[0] = s0; f.sigma[1] = s1; f.sigma[2] = d3;
    f.scale = ((s0 + s1) + d3) / (f.ok ? var : 1.0);
    f.R[0] = fma(u2.x, w2.x, fma(u1.x, v1.x, u0.x * v0.x)); f.R[1] = fma(u2.x, w2.y, fma(u1.x, v1.y, u0.x * v0.y)); f.R[2] = fma(u2.x, w2.z, fma(u1.x, v1.z, u0.x * v0.z));
    f.R[3] = fma(u2.y, w2.x, fma(u1.y, v1.x, u0.y * v0.x)); f.R[4] = fma(u2.y, w2.y, fma(u1.y, v1.y, u0.y * v0.y)); f.R[5] = fma(u2.y, w2.z, fma(u1.y, v1.z, u0.y * v0.z));
    f.R[6] = fma(u2.z, w2.x, fma(u1.z, v1.x, u0.z * v0.x)); f.R[7] = fma(u2.z, w2.y, fma(u1.z, v1.y, u0.z * v0.y)); f.R[8] = fma(u2.z, w2.z, fma(u1.z, v1.z, u0.z * v0.z));
    return f;
}

// |tgt - (sR src + t)|^2 < thr2 (the reference compares the norm with Scale * InlierT, align_utils.py:73-76; both sides are
// non-negative, so the squares order the same way except within an ulp of the threshold).  Every operation is an explicit fma or
// a single rounding, so each kernel that inlines this gets the same bits.  thr2 < 0 (a degenerate hypothesis) and NaN pass nothing.
GPA_HD bool is_inlier(const double (&M)[9], const double (&t)[3], double thr2, double sx, double sy, double sz, double tx, double ty, double tz) {
    const double dx = tx - fma(M[2], sz, fma(M[1], sy, fma(M[0], sx, t[0])));
    const double dy = ty - fma(M[5], sz, fma(M[4], sy, fma(M[3], sx, t[1])));
    const double dz = tz - fma(M[8], sz, fma(M[7], sy, fma(M[6], sx, t[2])));
    return fma(dz, dz, fma(dy, dy, dx * dx)) < thr2;
}

}  // namespace gpa
