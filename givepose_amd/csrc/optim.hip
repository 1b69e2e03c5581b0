// The optimiser family (include/givepose_optim.h, gpo_*): gradient-norm clip + Ranger over all tensors of a step in three launches.
//
//   reduce_kernel    a workgroup per chunk: the chunk's sum of squares (clip norm) and, for centralised tensors, the row sums
//   finalize_kernel  one workgroup: the chunks' sums of squares added in a fixed order -> norm and clip coefficient (device scalars)
//   update_kernel    a workgroup per chunk: the element-wise Ranger update, every buffer touched once
//   scale_kernel     gpo_clip_grad_norm only: g *= coef
//
// The chunks, the quad rule, the reductions and finalize_kernel are flat_tensors.hpp's, shared with accum.hip and adam.hip; here element i
// of a chunk is counted from the row's or the segment's first element, and a row that fits a chunk is served by a wave (STRIDE 64).
#include "common.hpp"
#include "../../include/givepose_optim.h"

// The code of this file asks for no contraction; the __f*_rn wrappers of the runtime's headers are plain operators compiled under the
// headers' own mode, though, and may still fuse.  Nothing here depends on it: the one exact result, the 0 of a centralised row of
// length 1, is the single subtraction g - mean, and the sum of squares is flat_tensors.hpp's sq_add, an fma by its spelling.
#pragma clang fp contract(off)

#include "flat_tensors.hpp"

namespace {

struct DevTensor {
    gpo_tensor t;
    long long part_off;      // first row partial of this tensor in the row-partial array
    int segs;                // segments per row (1: the row fits a chunk and is served by a wave)
    int pad;
};
static_assert(sizeof(DevTensor) == 80, "table layout");

__device__ __forceinline__ bool row_mode(const DevTensor& t) { return t.t.rows > 0 && t.segs == 1; }

// thread `id` of STRIDE adds its elements of g[0 .. n) to s and their squares to sq, in index order
template <int STRIDE>
__device__ __forceinline__ void accumulate(const float* __restrict__ g, int n, int id, float& s, float& sq) {
    const bool vec = al16(g);
    const int nq = n >> 2;
    for (int q = id; q < nq; q += STRIDE) {
        const f32x4 x = load_quad(g + 4 * q, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s = __fadd_rn(s, x[j]);
            sq = sq_add(sq, x[j]);
        }
    }
    if (id == nq % STRIDE)
        for (int i = 4 * nq; i < n; ++i) {
            s = __fadd_rn(s, g[i]);
            sq = sq_add(sq, g[i]);
        }
}

__global__ __launch_bounds__(WG) void reduce_kernel(const DevTensor* __restrict__ T, const Chunk* __restrict__ C, float* __restrict__ chunk_sq,
                                                    float* __restrict__ rowpart) {
    __shared__ float sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Chunk c = C[blockIdx.x];
    const DevTensor& t = T[c.tensor];
    float sq = 0.0f, total;
    if (row_mode(t)) {
        const int L = t.t.row_len;
        for (int r = wave; r < c.count; r += 4) {
            const long long row = c.start + r;
            float s = 0.0f;
            accumulate<64>(t.t.g + row * L, L, lane, s, sq);
            s = wave_sum(s);
            if (lane == 0) rowpart[t.part_off + row] = s;
        }
        total = wg_sum(sq, sh, lane, wave);
    } else {
        float s = 0.0f;
        accumulate<WG>(t.t.g + c.start, c.count, threadIdx.x, s, sq);
        total = wg_sum(sq, sh, lane, wave);
        if (t.t.rows > 0) {      // a segment of a long row
            s = wg_sum(s, sh, lane, wave);
            const long long row = c.start / t.t.row_len, seg = (c.start - row * t.t.row_len) / GPO_CHUNK;
            if (threadIdx.x == 0) rowpart[t.part_off + row * t.segs + seg] = s;
        }
    }
    if (threadIdx.x == 0) chunk_sq[blockIdx.x] = total;
}

struct Consts {
    float beta1, beta2, omb1, omb2, eps, alpha, wd;
};

template <bool RECT, bool LOOK>
__device__ __forceinline__ void element(float& p, float g, float& m, float& v, float& slow, float coef, float mean, float step_lr, const Consts& k) {
    const float gp = __fmul_rn(coef, __fsub_rn(g, mean));
    v = __fadd_rn(__fmul_rn(v, k.beta2), __fmul_rn(__fmul_rn(k.omb2, gp), gp));
    m = __fadd_rn(__fmul_rn(m, k.beta1), __fmul_rn(k.omb1, gp));
    float G = m;
    if (RECT) G = __fdiv_rn(m, __fadd_rn(__fsqrt_rn(v), k.eps));
    if (k.wd != 0.0f) {
        G = __fadd_rn(G, __fmul_rn(k.wd, p));
        if (!RECT) m = G;      // ranger2020.py:225-228: on an unrectified step G_grad IS exp_avg, and the decay is added to it in place
    }
    p = __fsub_rn(p, __fmul_rn(step_lr, G));
    if (LOOK) {
        slow = __fadd_rn(slow, __fmul_rn(k.alpha, __fsub_rn(p, slow)));
        p = slow;
    }
}

// the elements [off, off + n) of tensor t: thread `id` of STRIDE takes the quads id, id + STRIDE, ... and the owner of the last,
// partial quad its 1 .. 3 elements
template <int STRIDE, bool RECT, bool LOOK>
__device__ __forceinline__ void update_span(const gpo_tensor& t, long long off, int n, int id, float coef, float mean, const Consts& k) {
    float* __restrict__ p = t.p + off;
    const float* __restrict__ g = t.g + off;
    float* __restrict__ m = t.m + off;
    float* __restrict__ v = t.v + off;
    float* __restrict__ sl = t.slow + off;
    const bool vec = al16(p) && al16(g) && al16(m) && al16(v) && (!LOOK || al16(sl));
    const int nq = n >> 2;
    for (int q = id; q < nq; q += STRIDE) {
        const int i = 4 * q;
        f32x4 xp = load_quad(p + i, vec), xm = load_quad(m + i, vec), xv = load_quad(v + i, vec), xs = {0.0f, 0.0f, 0.0f, 0.0f};
        const f32x4 xg = load_quad(g + i, vec);
        if (LOOK) xs = load_quad(sl + i, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = xp[j], b = xm[j], c = xv[j], d = xs[j];
            element<RECT, LOOK>(a, xg[j], b, c, d, coef, mean, t.step_lr, k);
            xp[j] = a, xm[j] = b, xv[j] = c, xs[j] = d;
        }
        store_quad(p + i, vec, xp), store_quad(m + i, vec, xm), store_quad(v + i, vec, xv);
        if (LOOK) store_quad(sl + i, vec, xs);
    }
    if (id == nq % STRIDE)
        for (int i = 4 * nq; i < n; ++i) {
            float a = p[i], b = m[i], c = v[i], d = LOOK ? sl[i] : 0.0f;
            element<RECT, LOOK>(a, g[i], b, c, d, coef, mean, t.step_lr, k);
            p[i] = a, m[i] = b, v[i] = c;
            if (LOOK) sl[i] = d;
        }
}

template <int STRIDE>
__device__ __forceinline__ void update_any(const gpo_tensor& t, long long off, int n, int id, float coef, float mean, const Consts& k) {
    const bool rect = t.flags & GPO_FLAG_RECTIFIED, look = t.flags & GPO_FLAG_LOOKAHEAD;
    if (rect && look) update_span<STRIDE, true, true>(t, off, n, id, coef, mean, k);
    else if (rect) update_span<STRIDE, true, false>(t, off, n, id, coef, mean, k);
    else if (look) update_span<STRIDE, false, true>(t, off, n, id, coef, mean, k);
    else update_span<STRIDE, false, false>(t, off, n, id, coef, mean, k);
}

__global__ __launch_bounds__(WG) void update_kernel(const DevTensor* __restrict__ T, const Chunk* __restrict__ C, const float* __restrict__ rowpart,
                                                    const float* __restrict__ scal, Consts k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Chunk c = C[blockIdx.x];
    const DevTensor& t = T[c.tensor];
    const float coef = scal[1];
    if (row_mode(t)) {
        const int L = t.t.row_len;
        for (int r = wave; r < c.count; r += 4) {
            const long long row = c.start + r;
            const float mean = __fdiv_rn(rowpart[t.part_off + row], (float)L);
            update_any<64>(t.t, row * L, L, lane, coef, mean, k);
        }
    } else {
        float mean = 0.0f;
        if (t.t.rows > 0) {
            const long long row = c.start / t.t.row_len;
            const float* part = rowpart + t.part_off + row * t.segs;
            float s = part[0];
            for (int i = 1; i < t.segs; ++i) s = __fadd_rn(s, part[i]);
            mean = __fdiv_rn(s, (float)t.t.row_len);
        }
        update_any<WG>(t.t, c.start, c.count, threadIdx.x, coef, mean, k);
    }
}

__global__ __launch_bounds__(WG) void scale_kernel(const DevTensor* __restrict__ T, const Chunk* __restrict__ C, const float* __restrict__ scal) {
    const Chunk c = C[blockIdx.x];
    float* __restrict__ g = T[c.tensor].t.g + c.start;
    const float coef = scal[1];
    const bool vec = al16(g);
    const int nq = c.count >> 2;
    for (int q = threadIdx.x; q < nq; q += WG) {
        f32x4 x = load_quad(g + 4 * q, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = __fmul_rn(x[j], coef);
        store_quad(g + 4 * q, vec, x);
    }
    if (threadIdx.x == nq % WG)
        for (int i = 4 * nq; i < c.count; ++i) g[i] = __fmul_rn(g[i], coef);
}

// ---------------------------------------------------------------------------------- host
// checks the table and lays the workspace out; with `stage` also writes the device tables into it.  clip: only g and n count.
int plan_tables(const gpo_tensor* tensors, int n, bool clip, Plan& pl, std::vector<char>* stage, const char* name) {
    GP_REQUIRE(tensors && n >= 1 && n <= GPO_MAX_TENSORS, "%s: a table of 1 .. %d tensors is expected (n = %d)", name, GPO_MAX_TENSORS, n);
    long long chunks = 0, parts = 0;
    for (int i = 0; i < n; ++i) {
        const gpo_tensor& t = tensors[i];
        GP_REQUIRE(t.n >= 1 && t.n < (1LL << 40), "%s: tensor %d has %lld elements", name, i, t.n);
        GP_REQUIRE(t.g && al4(t.g), "%s: tensor %d: g is null or misaligned", name, i);
        if (clip) {
            chunks += flat_chunks(t.n);
            continue;
        }
        GP_REQUIRE(t.p && t.m && t.v && t.slow && al4(t.p) && al4(t.m) && al4(t.v) && al4(t.slow),
                   "%s: tensor %d: a null or misaligned pointer", name, i);
        GP_REQUIRE(t.rows >= 0 && (t.rows == 0 || (t.row_len >= 1 && (long long)t.rows * t.row_len == t.n)),
                   "%s: tensor %d: rows %d x row_len %d is not its %lld elements", name, i, t.rows, t.row_len, t.n);
        GP_REQUIRE((t.flags & ~(GPO_FLAG_RECTIFIED | GPO_FLAG_LOOKAHEAD)) == 0, "%s: tensor %d: unknown flags %d", name, i, t.flags);
        if (t.rows == 0) {
            chunks += flat_chunks(t.n);
        } else if (t.row_len <= GPO_CHUNK) {
            const int per = GPO_CHUNK / t.row_len;
            chunks += (t.rows + per - 1) / per;
            parts += t.rows;
        } else {
            const long long segs = flat_chunks(t.row_len);
            chunks += segs * t.rows;
            parts += segs * t.rows;
        }
    }
    GP_REQUIRE(chunks < (1LL << 30), "%s: %lld chunks", name, chunks);
    lay_out(pl, n, sizeof(DevTensor), chunks, parts);
    if (!stage) return 0;
    stage->resize((size_t)pl.table_bytes);
    DevTensor* dt = (DevTensor*)stage->data();
    Chunk *const ch0 = (Chunk*)(stage->data() + (size_t)n * sizeof(DevTensor)), *ch = ch0;
    long long part = 0;
    for (int i = 0; i < n; ++i) {
        gpo_tensor t = tensors[i];
        if (clip) t.p = t.m = t.v = t.slow = nullptr, t.rows = t.row_len = t.flags = 0, t.step_lr = 0.0f;
        dt[i] = DevTensor{t, part, 1, 0};
        if (t.rows == 0 || t.row_len > GPO_CHUNK) {
            const long long L = t.rows ? t.row_len : t.n, nrow = t.rows ? t.rows : 1, segs = flat_chunks(L);
            if (t.rows) dt[i].segs = (int)segs, part += segs * nrow;
            for (long long r = 0; r < nrow; ++r) ch = emit_flat(ch, i, r * L, L);
        } else {
            const int per = GPO_CHUNK / t.row_len;
            for (int r = 0; r < t.rows; r += per) *ch++ = Chunk{i, t.rows - r < per ? t.rows - r : per, r};
            part += t.rows;
        }
    }
    GP_REQUIRE(ch - ch0 == chunks && part == parts, "%s: internal chunk count", name);
    return 0;
}

}  // namespace

extern "C" {

long long gpo_ranger_step_workspace(const gpo_tensor* tensors, int n) {
    Plan pl;
    return plan_tables(tensors, n, false, pl, nullptr, "gpo_ranger_step_workspace") == 0 ? pl.total : 0;
}

int gpo_ranger_step(const gpo_tensor* tensors, int n, const gpo_hyper* h, float* scalars, void* ws, long long ws_bytes, void* stream) {
    const char* name = "gpo_ranger_step";
    hipStream_t s = (hipStream_t)stream;
    GP_REQUIRE(h, "%s: null hyper-parameters", name);
    GP_REQUIRE(h->beta1 >= 0 && h->beta1 < 1 && h->beta2 >= 0 && h->beta2 < 1 && h->eps > 0 && h->alpha >= 0 && h->alpha <= 1,
               "%s: bad hyper-parameters (betas %g %g, eps %g, alpha %g)", name, h->beta1, h->beta2, h->eps, h->alpha);
    Plan pl;
    if (int rc = plan_tables(tensors, n, false, pl, &g_stage, name)) return rc;
    if (int rc = send_tables(pl, ws, ws_bytes, s, name)) return rc;
    char* base = (char*)ws;
    const DevTensor* T = (const DevTensor*)base;
    const Chunk* C = (const Chunk*)(base + (size_t)n * sizeof(DevTensor));
    float *sq = (float*)(base + pl.off_sq), *part = (float*)(base + pl.off_part), *scal = (float*)(base + pl.off_scal);
    const Consts k{(float)h->beta1, (float)h->beta2, (float)(1.0 - h->beta1), (float)(1.0 - h->beta2), (float)h->eps, (float)h->alpha,
                   (float)h->weight_decay};
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)pl.n_chunks), dim3(WG), 0, s, T, C, sq, part);
    FLAT_CHECK(name);
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(WG), 0, s, (const float*)sq, (int)pl.n_chunks, (float)h->max_norm, scal, scalars);
    FLAT_CHECK(name);
    hipLaunchKernelGGL(update_kernel, dim3((unsigned)pl.n_chunks), dim3(WG), 0, s, T, C, (const float*)part, (const float*)scal, k);
    FLAT_CHECK(name);
    return 0;
}

long long gpo_clip_grad_norm_workspace(const gpo_tensor* tensors, int n) {
    Plan pl;
    return plan_tables(tensors, n, true, pl, nullptr, "gpo_clip_grad_norm_workspace") == 0 ? pl.total : 0;
}

int gpo_clip_grad_norm(const gpo_tensor* tensors, int n, float max_norm, float* scalars, void* ws, long long ws_bytes, void* stream) {
    const char* name = "gpo_clip_grad_norm";
    hipStream_t s = (hipStream_t)stream;
    GP_REQUIRE(scalars && max_norm > 0.0f, "%s: null scalars or max_norm %g <= 0", name, (double)max_norm);
    Plan pl;
    if (int rc = plan_tables(tensors, n, true, pl, &g_stage, name)) return rc;
    if (int rc = send_tables(pl, ws, ws_bytes, s, name)) return rc;
    char* base = (char*)ws;
    const DevTensor* T = (const DevTensor*)base;
    const Chunk* C = (const Chunk*)(base + (size_t)n * sizeof(DevTensor));
    float *sq = (float*)(base + pl.off_sq), *part = (float*)(base + pl.off_part), *scal = (float*)(base + pl.off_scal);
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)pl.n_chunks), dim3(WG), 0, s, T, C, sq, part);
    FLAT_CHECK(name);
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(WG), 0, s, (const float*)sq, (int)pl.n_chunks, max_norm, scal, scalars);
    FLAT_CHECK(name);
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)pl.n_chunks), dim3(WG), 0, s, T, C, (const float*)scal);
    FLAT_CHECK(name);
    return 0;
}

}  // extern "C"
