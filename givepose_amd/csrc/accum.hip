// The gradient-accumulation family (include/givepose_accum.h, gpc_*): add a micro-step's gradients into slices of a flat buffer, norm the
// result and clip it in place, in three launches whatever the number of tensors.
//
//   accum_add_kernel  a workgroup per chunk: a = scale * g, a = a + scale * g or a as it is; the chunk's sum of squares of the new a
//   accum_finalize_kernel    one workgroup: the chunks' sums added in a fixed order -> norm and clip coefficient (device scalars)
//   accum_scale_kernel       a workgroup per chunk: a *= coef (only with clipping)
//
// The element-to-thread map, the summation order and the quad rule are those of optim.hip's reduce / finalize / scale kernels for a tensor
// that is not centralised; the helpers are restated here so that optim.hip and its code objects stay as they are.
#include <vector>

#include "common.hpp"
#include "../../include/givepose_accum.h"

// a + scale * g is a multiply and an add.  The sum of squares goes through the same __fadd_rn(sq, __fmul_rn(x, x)) as optim.hip's
// reduce_kernel, so that whatever the runtime's headers make of the pair is made of it here as well.
#pragma clang fp contract(off)

namespace {

constexpr int WG = 256;

struct DevTensor {
    float* a;
    const float* g;
    int flags;
    int pad;
};
struct Chunk {
    int tensor;
    int count;               // elements
    long long start;         // first element
};
static_assert(sizeof(DevTensor) == 24 && sizeof(Chunk) == 16, "table layout");

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ float wave_sum(float v) {      // a fixed butterfly: every lane gets the same total
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the four waves of a workgroup as (w0 + w1) + (w2 + w3); every thread gets the total
__device__ __forceinline__ float wg_sum(float v, float* sh, int lane, int wave) {
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ f32x4 load_quad(const float* p, bool vec) {
    if (vec) return *(const f32x4*)p;
    return f32x4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void store_quad(float* p, bool vec, const f32x4& x) {
    if (vec) {
        *(f32x4*)p = x;
    } else {
        p[0] = x[0], p[1] = x[1], p[2] = x[2], p[3] = x[3];
    }
}

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
        for (int j = 0; j < 4; ++j) sq = __fadd_rn(sq, __fmul_rn(x[j], x[j]));
    }
    if (id == nq % WG)
        for (int i = 4 * nq; i < n; ++i) {
            float x = MODE != 1 ? a[i] : 0.0f;
            if (MODE != 0) {
                const float sg = scale * g[i];
                x = MODE == 1 ? sg : x + sg;
                a[i] = x;
            }
            sq = __fadd_rn(sq, __fmul_rn(x, x));
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

__global__ __launch_bounds__(WG) void accum_finalize_kernel(const float* __restrict__ chunk_sq, int n, float max_norm, float* __restrict__ scal,
                                                      float* __restrict__ out) {
    __shared__ float sh[4];
    float s = 0.0f;
    for (int i = threadIdx.x; i < n; i += WG) s = __fadd_rn(s, chunk_sq[i]);
    s = wg_sum(s, sh, threadIdx.x & 63, threadIdx.x >> 6);
    if (threadIdx.x == 0) {
        const float norm = __fsqrt_rn(s);
        const float coef = max_norm > 0.0f ? fminf(1.0f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f))) : 1.0f;
        scal[0] = norm, scal[1] = coef;
        if (out) out[0] = norm, out[1] = coef;
    }
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
long long up256(long long n) { return (n + 255) / 256 * 256; }
bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

struct Plan {
    long long n_chunks = 0, table_bytes = 0, off_sq = 0, off_scal = 0, total = 0;
};

// checks the table and lays the workspace out; with `stage` also writes the device tables into it
int plan_tables(const gpo_tensor* tensors, int n, Plan& pl, std::vector<char>* stage, const char* name) {
    GP_REQUIRE(tensors && n >= 1 && n <= GPO_MAX_TENSORS, "%s: a table of 1 .. %d tensors is expected (n = %d)", name, GPO_MAX_TENSORS, n);
    long long chunks = 0;
    for (int i = 0; i < n; ++i) {
        const gpo_tensor& t = tensors[i];
        GP_REQUIRE(t.n >= 1 && t.n < (1LL << 40), "%s: tensor %d has %lld elements", name, i, t.n);
        GP_REQUIRE(t.p && al4(t.p), "%s: tensor %d: p (the accumulator) is null or misaligned", name, i);
        GP_REQUIRE(al4(t.g), "%s: tensor %d: g is misaligned", name, i);
        GP_REQUIRE((t.flags & ~GPC_FLAG_OVERWRITE) == 0, "%s: tensor %d: unknown flags %d", name, i, t.flags);
        GP_REQUIRE(t.g || !(t.flags & GPC_FLAG_OVERWRITE), "%s: tensor %d: GPC_FLAG_OVERWRITE without a gradient", name, i);
        chunks += (t.n + GPO_CHUNK - 1) / GPO_CHUNK;
    }
    GP_REQUIRE(chunks < (1LL << 30), "%s: %lld chunks", name, chunks);
    pl.n_chunks = chunks;
    pl.table_bytes = (long long)n * sizeof(DevTensor) + chunks * (long long)sizeof(Chunk);
    pl.off_sq = up256(pl.table_bytes);
    pl.off_scal = pl.off_sq + up256(chunks * 4);
    pl.total = pl.off_scal + 256;
    if (!stage) return 0;
    stage->resize((size_t)pl.table_bytes);
    DevTensor* dt = (DevTensor*)stage->data();
    Chunk* ch = (Chunk*)(stage->data() + (size_t)n * sizeof(DevTensor));
    long long c = 0;
    for (int i = 0; i < n; ++i) {
        const gpo_tensor& t = tensors[i];
        dt[i] = DevTensor{t.p, t.g, t.flags, 0};
        for (long long lo = 0; lo < t.n; lo += GPO_CHUNK) ch[c++] = Chunk{i, (int)(t.n - lo < GPO_CHUNK ? t.n - lo : GPO_CHUNK), lo};
    }
    GP_REQUIRE(c == chunks, "%s: internal chunk count", name);
    return 0;
}

thread_local std::vector<char> g_stage;

#define GPC_CHECK(name)                                                                               \
    do {                                                                                              \
        hipError_t e__ = hipGetLastError();                                                           \
        if (e__ != hipSuccess) return gp_fail(GP_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e__)); \
    } while (0)

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
    GP_REQUIRE(ws && ((uintptr_t)ws & 255) == 0 && ws_bytes >= pl.total, "%s: workspace of %lld bytes (256-byte aligned) needed, %lld given", name,
               pl.total, ws_bytes);
    // pageable source: the runtime has consumed the host buffer when the call returns, so the next call may rewrite it
    const hipError_t e = hipMemcpyAsync(ws, g_stage.data(), (size_t)pl.table_bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return gp_fail(GP_ERR_RUNTIME, "%s: table copy: %s", name, hipGetErrorString(e));
    char* base = (char*)ws;
    const DevTensor* T = (const DevTensor*)base;
    const Chunk* C = (const Chunk*)(base + (size_t)n * sizeof(DevTensor));
    float *sq = (float*)(base + pl.off_sq), *scal = (float*)(base + pl.off_scal);
    hipLaunchKernelGGL(accum_add_kernel, dim3((unsigned)pl.n_chunks), dim3(WG), 0, s, T, C, scale, sq);
    GPC_CHECK(name);
    hipLaunchKernelGGL(accum_finalize_kernel, dim3(1), dim3(WG), 0, s, (const float*)sq, (int)pl.n_chunks, max_norm, scal, scalars);
    GPC_CHECK(name);
    if (max_norm > 0.0f) {
        hipLaunchKernelGGL(accum_scale_kernel, dim3((unsigned)pl.n_chunks), dim3(WG), 0, s, T, C, (const float*)scal);
        GPC_CHECK(name);
    }
    return 0;
}

}  // extern "C"
