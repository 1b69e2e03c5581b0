// What the three flat-tensor families share (optim.hip gpo_*, accum.hip gpc_*, adam.hip gpad_*): a table of fp32 tensors cut into
// chunks of at most GPO_CHUNK elements, a workgroup of 256 threads per chunk.  Included by exactly those three files; everything here
// has internal linkage, so each of them gets its own copy of the kernel, of the staging buffer and of the helpers.
//
// A chunk never crosses a tensor; inside it element i belongs to quad i / 4 and the quad to thread (i / 4) % STRIDE, whatever the
// pointers' alignment.  An aligned quad moves as one 16-byte access, any other as four 4-byte ones: the arithmetic and its order are the
// same, so the bits do not depend on where a buffer lies.  The norm of the three families has the same bits on equal data because its
// pieces -- sq_add, wave_sum, wg_sum, finalize_kernel -- are this one text.
#pragma once
#include <vector>

#include "common.hpp"
#include "../../include/givepose_optim.h"

// No contraction is asked for: the one fused operation of this file is the fma that sq_add spells out.
#pragma clang fp contract(off)

namespace {

constexpr int WG = 256;

struct Chunk {
    int tensor;
    int count;               // elements (optim.hip's row mode: rows of the run)
    long long start;         // first element (row mode: first row)
};
static_assert(sizeof(Chunk) == 16, "table layout");

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

// A thread adds the squares of its elements in index order as sq = fma(x, x, sq).  That is what __fadd_rn(sq, __fmul_rn(x, x)) compiles
// to (the runtime headers' wrappers are plain operators under the headers' own mode, and the pair is contracted to v_fmac_f32); it is
// spelled out so that the norm's bits do not hang on the compiler.
__device__ __forceinline__ float sq_add(float sq, float x) { return __builtin_fmaf(x, x, sq); }

// one workgroup: the chunks' sums of squares added in a fixed order -> norm and clip coefficient (device scalars; max_norm <= 0: no clip)
__global__ __launch_bounds__(WG) void finalize_kernel(const float* __restrict__ chunk_sq, int n, float max_norm, float* __restrict__ scal,
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

// ---------------------------------------------------------------------------------- host
long long up256(long long n) { return (n + 255) / 256 * 256; }
bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }      // alignment only: a call site that refuses null says so itself

long long flat_chunks(long long n) { return (n + GPO_CHUNK - 1) / GPO_CHUNK; }

// the chunks of the elements [first, first + n) of `tensor`; -> the slot after the last one written
Chunk* emit_flat(Chunk* ch, int tensor, long long first, long long n) {
    for (long long lo = 0; lo < n; lo += GPO_CHUNK) *ch++ = Chunk{tensor, (int)(n - lo < GPO_CHUNK ? n - lo : GPO_CHUNK), first + lo};
    return ch;
}

// The workspace: n tensor records and the chunks (the tables, written on the host), then the chunks' sums of squares, the row partials
// (optim.hip's centralised tensors only) and the two scalars, each rounded up to 256 bytes.
struct Plan {
    long long n_chunks = 0, n_parts = 0, table_bytes = 0, off_sq = 0, off_part = 0, off_scal = 0, total = 0;
};

void lay_out(Plan& pl, int n, size_t record_bytes, long long chunks, long long parts = 0) {
    pl.n_chunks = chunks, pl.n_parts = parts;
    pl.table_bytes = (long long)n * (long long)record_bytes + chunks * (long long)sizeof(Chunk);
    pl.off_sq = up256(pl.table_bytes);
    pl.off_part = pl.off_sq + up256(chunks * 4);
    pl.off_scal = pl.off_part + up256(parts * 4);
    pl.total = pl.off_scal + 256;
}

thread_local std::vector<char> g_stage;      // the tables of the call in flight, as plan_tables staged them

int send_tables(const Plan& pl, void* ws, long long ws_bytes, hipStream_t s, const char* name) {
    GP_REQUIRE(ws && ((uintptr_t)ws & 255) == 0 && ws_bytes >= pl.total, "%s: workspace of %lld bytes (256-byte aligned) needed, %lld given", name,
               pl.total, ws_bytes);
    // pageable source: the runtime has consumed the host buffer when the call returns, so the next call may rewrite it
    const hipError_t e = hipMemcpyAsync(ws, g_stage.data(), (size_t)pl.table_bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return gp_fail(GP_ERR_RUNTIME, "%s: table copy: %s", name, hipGetErrorString(e));
    return 0;
}

#define FLAT_CHECK(name)                                                                              \
    do {                                                                                              \
        hipError_t e__ = hipGetLastError();                                                           \
        if (e__ != hipSuccess) return gp_fail(GP_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e__)); \
    } while (0)

}  // namespace
