// Degree-cm / 3D-IoU mAP evaluation on the device (evaluation/eval_utils_cass.py:490-820 of the reference; evaluate.py:160, 234
// are its two callers).  Three stages, each one launch over all frames of a run:
//   eval_pair_kernel         per (prediction, ground truth) pair of one frame and class: 3D IoU (float32) and (degree, cm)
//   eval_match_*_kernel      per (frame-class group, threshold cell): the greedy matching, "already matched" as a 64-bit mask
//   eval_ap_kernel           per (class, cell): scan of the match flags in score order, precision / recall, running maximum from the
//                            right, and the sum over the recall steps IN NUMPY'S PAIRWISE ORDER (so equal flags give equal bits)
// Everything is float64 arithmetic in plain C++.  The kernels are latency- and divergence-bound (a few thousand pairs, a few
// million tiny matchings); nothing here is tuned.  No per-thread array is indexed at run time (no scratch segment): the pair values
// of a group are re-read from global memory (the lanes of a wave mostly share the group, so the loads are broadcasts).
#include "common.hpp"

#include <math.h>

namespace {

__device__ __forceinline__ double ld_any(const void* p, long i, int f64) {
    return f64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];
}
// numpy's maximum / minimum / amax / amin: a NaN operand wins (fmax / fmin would drop it)
__device__ __forceinline__ double np_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double np_min(double a, double b) { return (a < b || a != a) ? a : b; }

// axis-aligned extent of the 8 corners (+-s/2) of a box under the homogeneous 4x4 M (get_3d_bbox + transform_coordinates_3d,
// division by the homogeneous row included)
__device__ __forceinline__ void box_extent(const double (&M)[16], const double (&s)[3], double (&lo)[3], double (&hi)[3]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const double x = (c & 2) ? -s[0] / 2 : s[0] / 2, y = (c & 4) ? -s[1] / 2 : s[1] / 2, z = (c & 1) ? -s[2] / 2 : s[2] / 2;
        const double w = M[12] * x + M[13] * y + M[14] * z + M[15];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double v = (M[4 * a] * x + M[4 * a + 1] * y + M[4 * a + 2] * z + M[4 * a + 3]) / w;
            lo[a] = c == 0 ? v : np_min(lo[a], v);
            hi[a] = c == 0 ? v : np_max(hi[a], v);
        }
    }
}

// asymmetric_3d_iou of compute_3d_iou_new (real_iou form) for box 1 under M1 against the extent of box 2
__device__ __forceinline__ double iou_against(const double (&M1)[16], const double (&s1)[3], const double (&lo2)[3], const double (&hi2)[3]) {
    double lo1[3], hi1[3], d[3];
    box_extent(M1, s1, lo1, hi1);
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = np_min(hi1[a], hi2[a]) - np_max(lo1[a], lo2[a]);
    const double dmin = np_min(np_min(d[0], d[1]), d[2]);
    const double inter = dmin < 0 ? 0.0 : d[0] * d[1] * d[2];
    const double v1 = (hi1[0] - lo1[0]) * (hi1[1] - lo1[1]) * (hi1[2] - lo1[2]);
    const double v2 = (hi2[0] - lo2[0]) * (hi2[1] - lo2[1]) * (hi2[2] - lo2[2]);
    return inter / (v1 + v2 - inter);
}

__device__ __forceinline__ double det3(const double (&M)[16]) {
    return M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) + M[2] * (M[4] * M[9] - M[5] * M[8]);
}

__global__ __launch_bounds__(256) void eval_normalise_kernel(const void* __restrict__ rt, int f64, double* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double M[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) M[k] = ld_any(rt, i * 16 + k, f64);
    const double c = cbrt(det3(M));
#pragma unroll
    for (int k = 0; k < 16; ++k) out[i * 16 + k] = k < 12 ? M[k] / c : M[k];
}

// 32 lanes per pair: for a symmetric pair lanes 0..19 each take one of the 20 rotations about y and the maximum meets in lane 0;
// lane 0 also does the (degree, cm) of the pair.
__global__ __launch_bounds__(256) void eval_pair_kernel(const void* __restrict__ pred_rt, const void* __restrict__ pred_size, int pf64,
                                                        const void* __restrict__ gt_rt, const void* __restrict__ gt_size, int gf64,
                                                        const int* __restrict__ pair_pred, const int* __restrict__ pair_gt,
                                                        const unsigned char* __restrict__ pair_sym, const double* __restrict__ cs20,
                                                        float* __restrict__ iou, double* __restrict__ deg_cm, long n_pairs) {
    const long p = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int r = threadIdx.x & 31;
    if (p >= n_pairs) return;      // the 32 lanes of a pair leave together; the exchanges below stay inside them
    const long ip = pair_pred[p], ig = pair_gt[p];
    const int sym = pair_sym[p];
    double A[16], B[16], sa[3], sb[3];
#pragma unroll
    for (int k = 0; k < 16; ++k) { A[k] = ld_any(pred_rt, ip * 16 + k, pf64); B[k] = ld_any(gt_rt, ig * 16 + k, gf64); }
#pragma unroll
    for (int k = 0; k < 3; ++k) { sa[k] = ld_any(pred_size, ip * 3 + k, pf64); sb[k] = ld_any(gt_size, ig * 3 + k, gf64); }
    double lo2[3], hi2[3];
    box_extent(B, sb, lo2, hi2);
    double v;
    if (sym) {
        v = 0.0;                   // max_iou starts from 0 and `max` keeps it against a NaN: fmax
        if (r < 20) {
            const double c = cs20[r], s = cs20[20 + r];
            double Mr[16];
#pragma unroll
            for (int i = 0; i < 4; ++i) {      // RT_1 @ Ry(theta): columns 0 and 2 mix
                Mr[4 * i] = A[4 * i] * c + A[4 * i + 2] * (-s);
                Mr[4 * i + 1] = A[4 * i + 1];
                Mr[4 * i + 2] = A[4 * i] * s + A[4 * i + 2] * c;
                Mr[4 * i + 3] = A[4 * i + 3];
            }
            v = fmax(0.0, iou_against(Mr, sa, lo2, hi2));
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 32));
    } else {
        v = iou_against(A, sa, lo2, hi2);
    }
    if (r != 0) return;
    iou[p] = (float)v;             // the reference keeps the overlaps in a float32 array
    // compute_RT_degree_cm_symmetry
    const double c1 = cbrt(det3(A)), c2 = cbrt(det3(B));
    double R1[9], R2[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { R1[3 * i + j] = A[4 * i + j] / c1; R2[3 * i + j] = B[4 * i + j] / c2; }
    double arg;
    if (sym) {                     // angle between the y axes (column 1)
        const double dot = R1[1] * R2[1] + R1[4] * R2[4] + R1[7] * R2[7];
        const double n1 = sqrt(R1[1] * R1[1] + R1[4] * R1[4] + R1[7] * R1[7]), n2 = sqrt(R2[1] * R2[1] + R2[4] * R2[4] + R2[7] * R2[7]);
        arg = dot / (n1 * n2);
    } else {                       // trace(R1 R2^T)
        const double t0 = R1[0] * R2[0] + R1[1] * R2[1] + R1[2] * R2[2], t1 = R1[3] * R2[3] + R1[4] * R2[4] + R1[5] * R2[5];
        const double t2 = R1[6] * R2[6] + R1[7] * R2[7] + R1[8] * R2[8];
        arg = ((t0 + t1) + t2 - 1) / 2;
    }
    const double theta = acos(arg) * 57.29577951308232;      // 180 / pi; an argument outside [-1, 1] gives NaN, as in the reference
    const double dx = A[3] - B[3], dy = A[7] - B[7], dz = A[11] - B[11];
    deg_cm[2 * p] = theta;
    deg_cm[2 * p + 1] = sqrt(dx * dx + dy * dy + dz * dz) * 100;
}

// One work-item per (group, IoU threshold).  For each prediction in score order: the unmatched ground truths in descending IoU
// order (masked arg-max), stop below the threshold, match above it, pass over an exact tie with the threshold.  A NaN IoU compares
// false both ways in the reference and is passed over.
__global__ __launch_bounds__(256) void eval_match_iou_kernel(const float* __restrict__ iou, const int* __restrict__ pred_off,
                                                             const int* __restrict__ gt_off, const int* __restrict__ pair_off,
                                                             long n_items, const double* __restrict__ thr, int n_thr, long n_pred,
                                                             long n_gt, unsigned char* __restrict__ pred_flag,
                                                             unsigned char* __restrict__ gt_flag, int* __restrict__ status) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_items) return;
    const int cell = (int)(idx % n_thr);
    const long g = idx / n_thr;
    const int p0 = pred_off[g], np = pred_off[g + 1] - p0, g0 = gt_off[g], ng = gt_off[g + 1] - g0;
    if (np > GP_EVAL_MAX_PER_GROUP || ng > GP_EVAL_MAX_PER_GROUP) { *status = 1; return; }
    const float* v = iou + pair_off[g];
    const double t = thr[cell];
    unsigned long long matched = 0;
    for (int i = 0; i < np; ++i) {
        unsigned long long skip = matched;
        bool hit = false;
        for (;;) {
            int best = -1;
            float bv = 0.f;
            for (int j = 0; j < ng; ++j) {
                const float x = v[i * ng + j];
                if (((skip >> j) & 1) || x != x) continue;
                if (best < 0 || x >= bv) { best = j; bv = x; }
            }
            if (best < 0 || (double)bv < t) break;
            if ((double)bv > t) { matched |= 1ull << best; hit = true; break; }
            skip |= 1ull << best;
        }
        pred_flag[(long)cell * n_pred + p0 + i] = hit;
    }
    for (int j = 0; j < ng; ++j) gt_flag[(long)cell * n_gt + g0 + j] = (matched >> j) & 1;
}

// One work-item per (group, degree threshold, shift threshold).  For each prediction that enters (all of them, or those matched in
// the IoU cell `gate`): the unmatched ground truth of smallest degree + cm (NaN sums last) among those not above either threshold.
__global__ __launch_bounds__(256) void eval_match_pose_kernel(const double* __restrict__ deg_cm, const int* __restrict__ pred_off,
                                                              const int* __restrict__ gt_off, const int* __restrict__ pair_off,
                                                              long n_items, const double* __restrict__ deg_thr, int n_deg,
                                                              const double* __restrict__ shift_thr, int n_shift,
                                                              const unsigned char* __restrict__ gate, long n_pred, long n_gt,
                                                              unsigned char* __restrict__ pred_flag, unsigned char* __restrict__ gt_flag) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_items) return;
    const int n_cells = n_deg * n_shift;
    const int cell = (int)(idx % n_cells);
    const long g = idx / n_cells;
    const int p0 = pred_off[g], np = pred_off[g + 1] - p0, g0 = gt_off[g], ng = gt_off[g + 1] - g0;
    if (np > GP_EVAL_MAX_PER_GROUP || ng > GP_EVAL_MAX_PER_GROUP) return;      // the IoU kernel has set the status
    const double* v = deg_cm + 2 * (long)pair_off[g];
    const double dt = deg_thr[cell / n_shift], st = shift_thr[cell % n_shift];
    unsigned long long matched = 0;
    for (int i = 0; i < np; ++i) {
        int best = -1;
        if (!gate || gate[p0 + i]) {
            double bs = 0.0;
            for (int j = 0; j < ng; ++j) {
                const double d = v[2 * (i * ng + j)], c = v[2 * (i * ng + j) + 1];
                if (((matched >> j) & 1) || d > dt || c > st) continue;
                const double s = d + c;
                if (best < 0 || s < bs || (bs != bs && s == s)) { best = j; bs = s; }
            }
            if (best >= 0) matched |= 1ull << best;
        }
        pred_flag[(long)cell * n_pred + p0 + i] = best >= 0;
    }
    for (int j = 0; j < ng; ++j) gt_flag[(long)cell * n_gt + g0 + j] = (matched >> j) & 1;
}

// numpy's pairwise summation (the order np.sum adds a contiguous or strided 1-D float64 array of up to 8192 elements in): below 8 elements one running sum,
// up to 128 eight interleaved accumulators combined as a tree plus the tail, above that two halves, the first a multiple of 8 long.
__device__ __forceinline__ double np_block_sum(const double* a, long stride, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i * stride];
        return res;
    }
    double r0 = a[0], r1 = a[stride], r2 = a[2 * stride], r3 = a[3 * stride], r4 = a[4 * stride], r5 = a[5 * stride], r6 = a[6 * stride], r7 = a[7 * stride];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        const double* b = a + i * stride;
        r0 += b[0]; r1 += b[stride]; r2 += b[2 * stride]; r3 += b[3 * stride];
        r4 += b[4 * stride]; r5 += b[5 * stride]; r6 += b[6 * stride]; r7 += b[7 * stride];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i * stride];
    return res;
}
constexpr int NP_BLOCK = 128;
constexpr int NP_CHUNK = 8192;      // np.sum hands the array to the pairwise loop in pieces of the ufunc buffer size and adds the pieces in turn
__device__ __forceinline__ int np_first_half(int n) { const int h = n / 2; return h - (h % 8); }

// np.sum of a[0..K): pieces of NP_CHUNK added in turn, each piece pairwise.  First every block of at most 128 (a leaf of numpy's
// recursion; at least 64 long unless it is a whole piece, so it holds a multiple of 64 from the piece's start, and the first such
// index owns it) is summed into its first element, by all threads.  Then thread 0 walks each piece's tree depth first, its stack in LDS
// (a few dozen nodes per piece), and returns the total; the other threads return 0.
__device__ __forceinline__ double np_sum_terms(double* a, int K, int tid, int* st_off, int* st_n, int* st_stage, double* st_val) {
    for (int m = tid * 64; m < K; m += 256 * 64) {
        const int base = m & ~(NP_CHUNK - 1);
        int off = 0, n = min(NP_CHUNK, K - base);
        while (n > NP_BLOCK) {
            const int h = np_first_half(n);
            if (m - base < off + h) n = h; else { off += h; n -= h; }
        }
        if (m - base - off < 64) a[base + off] = np_block_sum(a + base + off, 1, n);
    }
    __syncthreads();
    double res = 0.0;
    if (tid == 0) {
        for (int base = 0; base < K; base += NP_CHUNK) {
            int sp = 0;
            double ret = 0.0;
            st_off[0] = 0; st_n[0] = min(NP_CHUNK, K - base); st_stage[0] = 0;
            while (sp >= 0) {
                const int off = st_off[sp], n = st_n[sp], stage = st_stage[sp];
                if (n <= NP_BLOCK) { ret = a[base + off]; --sp; continue; }
                const int h = np_first_half(n);
                if (stage == 0) { st_stage[sp] = 1; ++sp; st_off[sp] = off; st_n[sp] = h; st_stage[sp] = 0; }
                else if (stage == 1) { st_val[sp] = ret; st_stage[sp] = 2; ++sp; st_off[sp] = off + h; st_n[sp] = n - h; st_stage[sp] = 0; }
                else { ret = st_val[sp] + ret; --sp; }
            }
            res = base ? res + ret : ret;
        }
    }
    return res;
}

// One workgroup per (class, cell), looping over the items so that the term buffers stay n_workgroups * work_stride doubles.
//   pass 1  every thread counts the taking-part slots and the matches of its contiguous chunk of the class's score order; block scan
//   pass 2  chunk maxima of the precision cum / (position + 1), exclusive maximum over the chunks to the right
//   pass 3  right to left inside the chunk: running maximum, and at match number t the term (recall[t+1] - recall[t]) * maximum -> work[t]
//           (recall = float64(float32(t) / float32(n_gt)) as the reference computes it; one more term, (1 - recall[M]) * 0, when not every
//           ground truth was matched: it is a zero, but numpy's order of additions depends on the number of terms)
//   pass 4  the terms added in np.sum's order (np_sum_terms)
__global__ __launch_bounds__(256) void eval_ap_kernel(const unsigned char* __restrict__ flags, const unsigned char* __restrict__ valid,
                                                      int n_pred, const int* __restrict__ order, const int* __restrict__ cls_off,
                                                      const int* __restrict__ cls_ngt, int n_items, int n_cells, double* __restrict__ work_all,
                                                      int work_stride, double* __restrict__ ap) {
    __shared__ int s_v[256], s_m[256];
    __shared__ double s_p[256];
    __shared__ int st_off[32], st_n[32], st_stage[32];      // thread 0's stack in the summation tree (depth <= 8; s_p holds its values)
    const int tid = threadIdx.x;
    double* work = work_all + (long)blockIdx.x * work_stride;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int c = item / n_cells, cell = item - c * n_cells;
        const int* ord = order + cls_off[c];
        const int L = cls_off[c + 1] - cls_off[c], n_gt = cls_ngt[c];
        const unsigned char* f = flags + (long)cell * n_pred;
        const int per = (L + 255) / 256, lo = min(tid * per, L), hi = min(lo + per, L);
        // pass 1
        int nv = 0, nm = 0;
        for (int k = lo; k < hi; ++k) {
            const int slot = ord[k];
            const int ok = valid ? valid[slot] != 0 : 1;
            nv += ok;
            nm += ok && f[slot];
        }
        __syncthreads();           // the previous item's readers of the shared arrays are done
        s_v[tid] = nv; s_m[tid] = nm;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int a = tid >= off ? s_v[tid - off] : 0, b = tid >= off ? s_m[tid - off] : 0;
            __syncthreads();
            s_v[tid] += a; s_m[tid] += b;
            __syncthreads();
        }
        const int vbase = s_v[tid] - nv, mbase = s_m[tid] - nm, V = s_v[255], M = s_m[255];
        if (L + 1 > work_stride || n_gt <= 0) {      // no ground truth: the reference divides by zero -- 0 without predictions, NaN with
            if (tid == 0) ap[(long)c * n_cells + cell] = (n_gt <= 0 && V == 0 && L + 1 <= work_stride) ? 0.0 : __builtin_nan("");
            continue;
        }
        // pass 2
        double pm = 0.0;
        {
            int q = vbase, cum = mbase;
            for (int k = lo; k < hi; ++k) {
                const int slot = ord[k];
                if (valid && !valid[slot]) continue;
                cum += f[slot] != 0;
                ++q;
                pm = fmax(pm, (double)cum / (double)q);
            }
        }
        s_p[tid] = pm;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const double a = tid + off < 256 ? s_p[tid + off] : 0.0;
            __syncthreads();
            s_p[tid] = fmax(s_p[tid], a);
            __syncthreads();
        }
        // pass 3
        {
            double run = tid + 1 < 256 ? s_p[tid + 1] : 0.0;
            const float fn = (float)n_gt;
            int q = vbase + nv, cum = mbase + nm;
            for (int k = hi - 1; k >= lo; --k) {
                const int slot = ord[k];
                if (valid && !valid[slot]) continue;
                run = fmax(run, (double)cum / (double)q);
                if (f[slot]) {
                    work[cum - 1] = ((double)((float)cum / fn) - (double)((float)(cum - 1) / fn)) * run;
                    --cum;
                }
                --q;
            }
            if (tid == 0 && M != n_gt) work[M] = (1.0 - (double)((float)M / fn)) * 0.0;
        }
        const int K = M + (M != n_gt);
        __syncthreads();
        // pass 4
        const double total = np_sum_terms(work, K, tid, st_off, st_n, st_stage, s_p);
        if (tid == 0) ap[(long)c * n_cells + cell] = total;
    }
}

// row n_cls of ap = mean over the classes, in numpy's order (np.mean = sum / count)
__global__ __launch_bounds__(256) void eval_mean_kernel(double* __restrict__ ap, int n_cls, int n_cells, int pairwise) {
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= n_cells) return;
    double s;
    if (pairwise) s = np_block_sum(ap + cell, n_cells, n_cls);
    else {
        s = 0.0;
        for (int c = 0; c < n_cls; ++c) s += ap[(long)c * n_cells + cell];
    }
    ap[(long)n_cls * n_cells + cell] = s / (double)n_cls;
}

bool f32_or_f64(int dt) { return dt == GP_F32 || dt == GP_F64; }

}  // namespace

extern "C" int gp_eval_normalise(const void* rt, int dtype, double* out, long n, void* stream) {
    GP_REQUIRE(rt && out && n > 0 && f32_or_f64(dtype), "gp_eval_normalise: bad argument");
    hipStream_t s = (hipStream_t)stream;
    gp_timing_before(s, GP_KC_SMALL, 0.0, (double)n * 16 * 12);
    hipLaunchKernelGGL(eval_normalise_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, rt, dtype == GP_F64, out, n);
    GP_LAUNCH_CHECK("gp_eval_normalise");
}

extern "C" int gp_eval_pair_overlaps(const void* pred_rt, const void* pred_size, int pred_dtype, const void* gt_rt, const void* gt_size,
                                     int gt_dtype, const int* pair_pred, const int* pair_gt, const unsigned char* pair_sym,
                                     const double* cs20, float* iou, double* deg_cm, long n_pairs, void* stream) {
    GP_REQUIRE(pred_rt && pred_size && gt_rt && gt_size && pair_pred && pair_gt && pair_sym && cs20 && iou && deg_cm && n_pairs > 0,
               "gp_eval_pair_overlaps: bad argument");
    GP_REQUIRE(f32_or_f64(pred_dtype) && f32_or_f64(gt_dtype), "gp_eval_pair_overlaps: poses are GP_F32 or GP_F64");
    hipStream_t s = (hipStream_t)stream;
    gp_timing_before(s, GP_KC_SMALL, (double)n_pairs * 20 * 200, (double)n_pairs * 340);
    hipLaunchKernelGGL(eval_pair_kernel, dim3(cdiv(n_pairs, 8)), dim3(256), 0, s, pred_rt, pred_size, pred_dtype == GP_F64, gt_rt, gt_size,
                       gt_dtype == GP_F64, pair_pred, pair_gt, pair_sym, cs20, iou, deg_cm, n_pairs);
    GP_LAUNCH_CHECK("gp_eval_pair_overlaps");
}

extern "C" int gp_eval_match(const float* iou, const double* deg_cm, const int* pred_off, const int* gt_off, const int* pair_off,
                             int n_groups, int max_per_group, const double* iou_thr, int n_iou, const double* deg_thr, int n_deg,
                             const double* shift_thr, int n_shift, int pose_iou_cell, long n_pred, long n_gt,
                             unsigned char* iou_pred_flag, unsigned char* iou_gt_flag, unsigned char* pose_pred_flag,
                             unsigned char* pose_gt_flag, int* status, void* stream) {
    GP_REQUIRE(iou && deg_cm && pred_off && gt_off && pair_off && iou_thr && deg_thr && shift_thr && iou_pred_flag && iou_gt_flag &&
                   pose_pred_flag && pose_gt_flag && status, "gp_eval_match: null pointer");
    GP_REQUIRE(n_groups > 0 && n_iou > 0 && n_deg > 0 && n_shift > 0 && n_pred >= 0 && n_gt >= 0, "gp_eval_match: bad size");
    GP_REQUIRE(max_per_group <= GP_EVAL_MAX_PER_GROUP, "gp_eval_match: %d predictions or ground truths of one class in one frame, at most %d are supported",
               max_per_group, GP_EVAL_MAX_PER_GROUP);
    GP_REQUIRE(pose_iou_cell < n_iou, "gp_eval_match: pose_iou_cell %d of %d IoU cells", pose_iou_cell, n_iou);
    GP_REQUIRE((long)n_deg * n_shift < (1l << 30), "gp_eval_match: too many pose cells");
    hipStream_t s = (hipStream_t)stream;
    const long ni = (long)n_groups * n_iou, np = (long)n_groups * n_deg * n_shift;
    GP_REQUIRE(np / 256 < 0x7fffffffl, "gp_eval_match: too many (group, cell) items");
    gp_timing_before(s, GP_KC_SMALL, 0.0, (double)(n_iou + n_deg * n_shift) * (n_pred + n_gt));
    hipLaunchKernelGGL(eval_match_iou_kernel, dim3(cdiv(ni, 256)), dim3(256), 0, s, iou, pred_off, gt_off, pair_off, ni, iou_thr, n_iou,
                       n_pred, n_gt, iou_pred_flag, iou_gt_flag, status);
    const unsigned char* gate = pose_iou_cell >= 0 ? iou_pred_flag + (long)pose_iou_cell * n_pred : nullptr;
    hipLaunchKernelGGL(eval_match_pose_kernel, dim3(cdiv(np, 256)), dim3(256), 0, s, deg_cm, pred_off, gt_off, pair_off, np, deg_thr, n_deg,
                       shift_thr, n_shift, gate, n_pred, n_gt, pose_pred_flag, pose_gt_flag);
    GP_LAUNCH_CHECK("gp_eval_match");
}

extern "C" int gp_eval_ap(const unsigned char* flags, const unsigned char* valid, long n_pred, const int* order, const int* cls_off,
                          const int* cls_ngt, int n_cls, int n_cells, double* work, long work_stride, int n_workgroups,
                          int pairwise_mean, double* ap, void* stream) {
    GP_REQUIRE(flags && order && cls_off && cls_ngt && work && ap, "gp_eval_ap: null pointer");
    GP_REQUIRE(n_cls > 0 && n_cls <= NP_BLOCK && n_cells > 0 && n_pred >= 0 && work_stride > 0 && n_workgroups > 0, "gp_eval_ap: bad size");
    GP_REQUIRE(n_pred < (1l << 31) && work_stride < (1l << 31) && (long)n_cls * n_cells < (1l << 31), "gp_eval_ap: too large");
    hipStream_t s = (hipStream_t)stream;
    const long items = (long)n_cls * n_cells;
    gp_timing_before(s, GP_KC_SMALL, 0.0, (double)n_cells * n_pred * 15);
    hipLaunchKernelGGL(eval_ap_kernel, dim3((unsigned)(items < n_workgroups ? items : n_workgroups)), dim3(256), 0, s, flags, valid, (int)n_pred,
                       order, cls_off, cls_ngt, (int)items, n_cells, work, (int)work_stride, ap);
    hipLaunchKernelGGL(eval_mean_kernel, dim3(cdiv(n_cells, 256)), dim3(256), 0, s, ap, n_cls, n_cells, pairwise_mean);
    GP_LAUNCH_CHECK("gp_eval_ap");
}
