// The gradient-accumulation family (include/givepose_accum.h, gpc_*): add a micro-step's gradients into slices of a flat buffer, norm the
// result and clip it in place, in three launches whatever the number of tensors.
//
//   accum_add_kernel    a workgroup per chunk: a = scale * g, a = a + scale * g or a as it is; the chunk's sum of squares of the new a
//   finalize_kernel     one workgroup: the chunks' sums added in a fixed order -> norm and clip coefficient (device scalars)
//   accum_scale_kernel  a workgroup per chunk: a *= coef (only with clipping)
//
// The element-to-thread map, the summation order and the quad rule are those of optim.hip's reduce / finalize / scale kernels for a tensor
// that is not centralised: the helpers and the finalize kernel are flat_tensors.hpp's, one text for both.
#include "common.hpp"
#include "../../include/givepose_accum.h"

// a + scale * g is a multiply and an add.  The sum of squares goes through the same sq_add as optim.hip's reduce_kernel.
#pragma clang fp contract(off)

#include "flat_tensors.hpp"

namespace {

struct DevTensor {
    float* a;
    const float* g;
    int flags;
    int pad;
};
static_assert(sizeof(DevTensor) == 24, "table layout");

// MODE 0: a stays (no gradient on this micro-step); 1: a = scale * g; 2: a = a + scale * g.  -> the thread's sum of squares of the new a
template <int MODE>
__device__ __forceinline__ float accumulate_span(float* a, const float* g, int n, int id, float scale) {
    const bool vec = al16(a) && (MODE == 0 || al16(g));
    const int nq = n >> 2;
    float sq = 0.0f;
    for (int q = id; q < nq; q += WG) {
        const int i = 4 * q;
        f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
        if (MODE != 1) x = load_quad(a + i, vec);
        if (MODE != 0) {
            const f32x4 xg = load_quad(g + i, vec);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float sg = scale * xg[j];
                x[j] = MODE == 1 ? sg : x[j] + sg;
            }
            store_quad(a + i, vec, x);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) sq = sq_add(sq, x[j]);
    }
    if (id == nq % WG)
        for (int i = 4 * nq; i < n; ++i) {
            float x = MODE != 1 ? a[i] : 0.0f;
            if (MODE != 0) {
                const float sg = scale * g[i];
                x = MODE == 1 ? sg : x + sg;
                a[i] = x;
            }
            sq = sq_add(sq, x);
        }
    return sq;
}

__global__ __launch_bounds__(WG) void accum_add_kernel(const DevTensor* __restrict__ T, const Chunk* __restrict__ C, float scale,
                                                        float* __restrict__ chunk_sq) {
    __shared__ float sh[4];
    const Chunk c = C[blockIdx.x];
    const DevTensor t = T[c.tensor];
    float* a = t.a + c.start;
    float sq;
    if (!t.g) sq = accumulate_span<0>(a, nullptr, c.count, threadIdx.x, scale);
    else if (t.flags & GPC_FLAG_OVERWRITE) sq = accumulate_span<1>(a, t.g + c.start, c.count, threadIdx.x, scale);
    else sq = accumulate_span<2>(a, t.g + c.start, c.count, threadIdx.x, scale);
    const float total = wg_sum(sq, sh, threadIdx.x & 63, threadIdx.x >> 6);
    if (threadIdx.x == 0) chunk_sq[blockIdx.x] = total;
}

__global__ __launch_bounds__(WG) void accum_scale_kernel(const DevTensor* __restrict__ T, const Chunk* __restrict__ C, const float* __restrict__ scal) {
    const Chunk c = C[blockIdx.x];
    float* __restrict__ a = T[c.tensor].a + c.start;
    const float coef = scal[1];
    const bool vec = al16(a);
    const int nq = c.count >> 2;
    for (int q = threadIdx.x; q < nq; q += WG) {
        f32x4 x = load_quad(a + 4 * q, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = __fmul_rn(x[j], coef);
        store_quad(a + 4 * q, vec, x);
    }
    if (threadIdx.x == nq % WG)
        for (int i = 4 * nq; i < c.count; ++i) a[i] = __fmul_rn(a[i], coef);
}

// ---------------------------------------------------------------------------------- host
// checks the table and lays the workspace out; with `stage` also writes the device tables into it
int plan_tables(const gpo_tensor* tensors, int n, Plan& pl, std::vector<char>* stage, const char* name) {
    GP_REQUIRE(tensors && n >= 1 && n <= GPO_MAX_TENSORS, "%s: a table of 1 .. %d tensors is expected (n = %d)", name, GPO_MAX_TENSORS, n);
    long long chunks = 0;
    for (int i = 0; i < n; ++i) {
        const gpo_tensor& t = tensors[i];
        GP_REQUIRE(t.n >= 1 && t.n < (1LL << 40), "%s: tensor %d has %lld elements", name, i, t.n);
        GP_REQUIRE(t.p && al4(t.p), "%s: tensor %d: p (the accumulator) is null or misaligned", name, i);
        GP_REQUIRE(al4(t.g), "%s: tensor %d: g is misaligned", name, i);      // null: no gradient on this micro-step
        GP_REQUIRE((t.flags & ~GPC_FLAG_OVERWRITE) == 0, "%s: tensor %d: unknown flags %d", name, i, t.flags);
        GP_REQUIRE(t.g || !(t.flags & GPC_FLAG_OVERWRITE), "%s: tensor %d: GPC_FLAG_OVERWRITE without a gradient", name, i);
        chunks += flat_chunks(t.n);
    }
    GP_REQUIRE(chunks < (1LL << 30), "%s: %lld chunks", name, chunks);
    lay_out(pl, n, sizeof(DevTensor), chunks);
    if (!stage) return 0;
    stage->resize((size_t)pl.table_bytes);
    DevTensor* dt = (DevTensor*)stage->data();
    Chunk *const ch0 = (Chunk*)(stage->data() + (size_t)n * sizeof(DevTensor)), *ch = ch0;
    for (int i = 0; i < n; ++i) {
        const gpo_tensor& t = tensors[i];
        dt[i] = DevTensor{t.p, t.g, t.flags, 0};
        ch = emit_flat(ch, i, 0, t.n);
    }
    GP_REQUIRE(ch - ch0 == chunks, "%s: internal chunk count", name);
    return 0;
}

}  // namespace

extern "C" {

long long gpc_grad_accumulate_workspace(const gpo_tensor* tensors, int n) {
    Plan pl;
    return plan_tables(tensors, n, pl, nullptr, "gpc_grad_accumulate_workspace") == 0 ? pl.total : 0;
}

int gpc_grad_accumulate(const gpo_tensor* tensors, int n, float scale, float max_norm, float* scalars, void* ws, long long ws_bytes,
                        void* stream) {
    const char* name = "gpc_grad_accumulate";
    hipStream_t s = (hipStream_t)stream;
    GP_REQUIRE(scale == scale && scale - scale == 0.0f && max_norm == max_norm, "%s: scale %g must be finite and max_norm %g a number", name,
               (double)scale, (double)max_norm);
    Plan pl;
    if (int rc = plan_tables(tensors, n, pl, &g_stage, name)) return rc;
    if (int rc = send_tables(pl, ws, ws_bytes, s, name)) return rc;
    char* base = (char*)ws;
    const DevTensor* T = (const DevTensor*)base;
    const Chunk* C = (const Chunk*)(base + (size_t)n * sizeof(DevTensor));
    float *sq = (float*)(base + pl.off_sq), *scal = (float*)(base + pl.off_scal);
    hipLaunchKernelGGL(accum_add_kernel, dim3((unsigned)pl.n_chunks), dim3(WG), 0, s, T, C, scale, sq);
    FLAT_CHECK(name);
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(WG), 0, s, (const float*)sq, (int)pl.n_chunks, max_norm, scal, scalars);
    FLAT_CHECK(name);
    if (max_norm > 0.0f) {
        hipLaunchKernelGGL(accum_scale_kernel, dim3((unsigned)pl.n_chunks), dim3(WG), 0, s, T, C, (const float*)scal);
        FLAT_CHECK(name);
    }
    return 0;
}

}  // extern "C"
