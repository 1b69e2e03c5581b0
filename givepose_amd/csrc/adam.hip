// Adam and AdamW (include/givepose_adam.h, gpad_*): gradient-norm clip + the step over all tensors in three launches.
//
//   adam_reduce_kernel  a workgroup per chunk: the chunk's sum of squares of g (clip norm)
//   finalize_kernel     one workgroup: the chunks' sums of squares added in a fixed order -> norm and clip coefficient (device scalars)
//   adam_update_kernel  a workgroup per chunk: the element-wise update, every buffer touched once
//
// The tables, the chunks and the order of the norm are those of optim.hip for a tensor that is not centralised: the chunks, the quad rule,
// the reductions and finalize_kernel are flat_tensors.hpp's, one text for both.
#include "common.hpp"
#include "../../include/givepose_adam.h"

// The update's contract is one rounding per operation.  hipcc contracts a * b + c into an fma by default, and the __f*_rn wrappers of
// the runtime's headers are plain operators compiled under the headers' own mode, so they fuse like any other: the products, sums,
// quotients and the square root live in helpers of plain operators under contract(off).  `/` and sqrtf are the correctly rounded
// sequences (__fsqrt_rn is a bare v_sqrt_f32, 1 ulp).
#pragma clang fp contract(off)

#include "flat_tensors.hpp"

namespace {

static_assert(sizeof(gpad_tensor) == 64 && sizeof(gpad_hyper) == 48, "table layout");

__device__ __forceinline__ float fmul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float fadd(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float fsub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float fdiv(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}
__device__ __forceinline__ float fsqrt(float a) { return sqrtf(a); }

// the chunk's sum of squares of g, a thread's elements in index order (sq_add)
__global__ __launch_bounds__(WG) void adam_reduce_kernel(const gpad_tensor* __restrict__ T, const Chunk* __restrict__ C, float* __restrict__ chunk_sq) {
    __shared__ float sh[4];
    const Chunk c = C[blockIdx.x];
    const float* __restrict__ g = T[c.tensor].g + c.start;
    const bool vec = al16(g);
    const int nq = c.count >> 2, id = threadIdx.x;
    float sq = 0.0f;
    for (int q = id; q < nq; q += WG) {
        const f32x4 x = load_quad(g + 4 * q, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) sq = sq_add(sq, x[j]);
    }
    if (id == nq % WG)
        for (int i = 4 * nq; i < c.count; ++i) sq = sq_add(sq, g[i]);
    const float total = wg_sum(sq, sh, threadIdx.x & 63, threadIdx.x >> 6);
    if (threadIdx.x == 0) chunk_sq[blockIdx.x] = total;
}

struct Consts {
    float beta2, omb1, omb2, eps, wd;
    int mode, amsgrad;
};

constexpr int WD_NONE = 0, WD_GRAD = 1, WD_PARAM = 2;

template <int WD, bool AMS>
__device__ __forceinline__ void element(float& p, float g, float& m, float& v, float& vmax, float coef, const gpad_tensor& t, const Consts& k) {
    float gp = fmul(coef, g);
    if (WD == WD_GRAD) gp = fadd(gp, fmul(k.wd, p));
    if (WD == WD_PARAM) p = fmul(p, t.decay);
    m = fadd(m, fmul(k.omb1, fsub(gp, m)));
    v = fadd(fmul(v, k.beta2), fmul(fmul(k.omb2, gp), gp));
    float u = v;
    if (AMS) u = vmax = fmaxf(vmax, v);
    const float den = fadd(fdiv(fsqrt(u), t.bc2_sqrt), k.eps);
    p = fsub(p, fmul(t.step_size, fdiv(m, den)));
}

// the elements [off, off + n) of tensor t: thread `id` takes the quads id, id + WG, ... and the owner of the last, partial quad its
// 1 .. 3 elements
template <int WD, bool AMS>
__device__ __forceinline__ void update_span(const gpad_tensor& t, long long off, int n, int id, float coef, const Consts& k) {
    float* __restrict__ p = t.p + off;
    const float* __restrict__ g = t.g + off;
    float* __restrict__ m = t.m + off;
    float* __restrict__ v = t.v + off;
    float* __restrict__ vm = AMS ? t.vmax + off : nullptr;
    const bool vec = al16(p) && al16(g) && al16(m) && al16(v) && (!AMS || al16(vm));
    const int nq = n >> 2;
    for (int q = id; q < nq; q += WG) {
        const int i = 4 * q;
        f32x4 xp = load_quad(p + i, vec), xm = load_quad(m + i, vec), xv = load_quad(v + i, vec), xu = {0.0f, 0.0f, 0.0f, 0.0f};
        const f32x4 xg = load_quad(g + i, vec);
        if (AMS) xu = load_quad(vm + i, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = xp[j], b = xm[j], c = xv[j], d = xu[j];
            element<WD, AMS>(a, xg[j], b, c, d, coef, t, k);
            xp[j] = a, xm[j] = b, xv[j] = c, xu[j] = d;
        }
        store_quad(p + i, vec, xp), store_quad(m + i, vec, xm), store_quad(v + i, vec, xv);
        if (AMS) store_quad(vm + i, vec, xu);
    }
    if (id == nq % WG)
        for (int i = 4 * nq; i < n; ++i) {
            float a = p[i], b = m[i], c = v[i], d = AMS ? vm[i] : 0.0f;
            element<WD, AMS>(a, g[i], b, c, d, coef, t, k);
            p[i] = a, m[i] = b, v[i] = c;
            if (AMS) vm[i] = d;
        }
}

template <int WD>
__device__ __forceinline__ void update_ams(const gpad_tensor& t, long long off, int n, int id, float coef, const Consts& k) {
    if (k.amsgrad) update_span<WD, true>(t, off, n, id, coef, k);
    else update_span<WD, false>(t, off, n, id, coef, k);
}

__global__ __launch_bounds__(WG) void adam_update_kernel(const gpad_tensor* __restrict__ T, const Chunk* __restrict__ C, const float* __restrict__ scal,
                                                         Consts k) {
    const Chunk c = C[blockIdx.x];
    const gpad_tensor t = T[c.tensor];
    const float coef = scal[1];
    if (k.wd == 0.0f) update_ams<WD_NONE>(t, c.start, c.count, threadIdx.x, coef, k);
    else if (k.mode == GPAD_MODE_ADAMW) update_ams<WD_PARAM>(t, c.start, c.count, threadIdx.x, coef, k);
    else update_ams<WD_GRAD>(t, c.start, c.count, threadIdx.x, coef, k);
}

// ---------------------------------------------------------------------------------- host
int check_hyper(const gpad_hyper* h, const char* name) {
    GP_REQUIRE(h, "%s: null hyper-parameters", name);
    GP_REQUIRE(h->beta1 >= 0 && h->beta1 < 1 && h->beta2 >= 0 && h->beta2 < 1 && h->eps >= 0 && h->weight_decay >= 0,
               "%s: bad hyper-parameters (betas %g %g, eps %g, weight_decay %g)", name, h->beta1, h->beta2, h->eps, h->weight_decay);
    GP_REQUIRE(h->mode == GPAD_MODE_ADAM || h->mode == GPAD_MODE_ADAMW, "%s: unknown mode %d", name, h->mode);
    GP_REQUIRE(h->amsgrad == 0 || h->amsgrad == 1, "%s: amsgrad %d is neither 0 nor 1", name, h->amsgrad);
    return 0;
}

// checks the table and lays the workspace out; with `stage` also writes the device tables into it
int plan_tables(const gpad_tensor* tensors, int n, const gpad_hyper* h, Plan& pl, std::vector<char>* stage, const char* name) {
    if (int rc = check_hyper(h, name)) return rc;
    GP_REQUIRE(tensors && n >= 1 && n <= GPAD_MAX_TENSORS, "%s: a table of 1 .. %d tensors is expected (n = %d)", name, GPAD_MAX_TENSORS, n);
    long long chunks = 0;
    for (int i = 0; i < n; ++i) {
        const gpad_tensor& t = tensors[i];
        GP_REQUIRE(t.n >= 1 && t.n < (1LL << 40), "%s: tensor %d has %lld elements", name, i, t.n);
        GP_REQUIRE(t.g && al4(t.g), "%s: tensor %d: g is null or misaligned", name, i);
        GP_REQUIRE(t.p && t.m && t.v && (t.vmax || !h->amsgrad) && al4(t.p) && al4(t.m) && al4(t.v) && al4(t.vmax),
                   "%s: tensor %d: a null or misaligned pointer", name, i);
        GP_REQUIRE(t.step_size == t.step_size && t.bc2_sqrt > 0.0f && t.decay == t.decay, "%s: tensor %d: step_size %g, bc2_sqrt %g, decay %g", name, i,
                   (double)t.step_size, (double)t.bc2_sqrt, (double)t.decay);
        chunks += flat_chunks(t.n);
    }
    GP_REQUIRE(chunks < (1LL << 30), "%s: %lld chunks", name, chunks);
    lay_out(pl, n, sizeof(gpad_tensor), chunks);
    if (!stage) return 0;
    stage->resize((size_t)pl.table_bytes);
    gpad_tensor* dt = (gpad_tensor*)stage->data();
    Chunk *const ch0 = (Chunk*)(stage->data() + (size_t)n * sizeof(gpad_tensor)), *ch = ch0;
    for (int i = 0; i < n; ++i) {
        dt[i] = tensors[i];
        ch = emit_flat(ch, i, 0, tensors[i].n);
    }
    GP_REQUIRE(ch - ch0 == chunks, "%s: internal chunk count", name);
    return 0;
}

}  // namespace

extern "C" {

long long gpad_adam_step_workspace(const gpad_tensor* tensors, int n, const gpad_hyper* h) {
    Plan pl;
    return plan_tables(tensors, n, h, pl, nullptr, "gpad_adam_step_workspace") == 0 ? pl.total : 0;
}

int gpad_adam_step(const gpad_tensor* tensors, int n, const gpad_hyper* h, float* scalars, void* ws, long long ws_bytes, void* stream) {
    const char* name = "gpad_adam_step";
    hipStream_t s = (hipStream_t)stream;
    Plan pl;
    if (int rc = plan_tables(tensors, n, h, pl, &g_stage, name)) return rc;
    if (int rc = send_tables(pl, ws, ws_bytes, s, name)) return rc;
    char* base = (char*)ws;
    const gpad_tensor* T = (const gpad_tensor*)base;
    const Chunk* C = (const Chunk*)(base + (size_t)n * sizeof(gpad_tensor));
    float *sq = (float*)(base + pl.off_sq), *scal = (float*)(base + pl.off_scal);
    const Consts k{(float)h->beta2, (float)(1.0 - h->beta1), (float)(1.0 - h->beta2), (float)h->eps, (float)h->weight_decay, h->mode, h->amsgrad};
    hipLaunchKernelGGL(adam_reduce_kernel, dim3((unsigned)pl.n_chunks), dim3(WG), 0, s, T, C, sq);
    FLAT_CHECK(name);
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(WG), 0, s, (const float*)sq, (int)pl.n_chunks, (float)h->max_norm, scal, scalars);
    FLAT_CHECK(name);
    hipLaunchKernelGGL(adam_update_kernel, dim3((unsigned)pl.n_chunks), dim3(WG), 0, s, T, C, (const float*)scal, k);
    FLAT_CHECK(name);
    return 0;
}

}  // extern "C"
