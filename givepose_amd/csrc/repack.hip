// The weight-repack family (include/givepose_repack.h, gpr_*): PoseNet._pack on the device, in place, in at most four launches.
//
//   bnfold_kernel    eval BatchNorm1d folded into the 1x1 conv in front of it: fp32, the host's expression, every operation correctly rounded
//   matfold_kernel   out = A B (+ add): a thread per output, one fp64 chain over k, rounded once (launched per level)
//   copy_kernel      a workgroup per chunk of the entry table: a strided fp32 view -> dense fp32 / fp16 / split planes
//
// A chunk never crosses an entry.  Every output element is a function of its own source value alone, so neither the chunking nor the
// choice between the 16-byte and the element-wise accesses can change a bit.
#include "common.hpp"
#include "../../include/givepose_repack.h"

// No contraction in this file: the BatchNorm fold's product and sum are rounded separately, as the host's expression rounds them.
#pragma clang fp contract(off)

namespace {

constexpr int WG = 256;

struct DevEntry {
    gpr_entry e;
    int contig;              // the view is one contiguous run of the source
    int pad;
};
struct Chunk {
    int entry;
    int count;               // destination elements
    long long start;         // first element, counted row-major over the entry's view
};
struct MChunk {
    int fold;
    int count;               // outputs
    long long start;         // first output, m N + n
};
static_assert(sizeof(DevEntry) % 8 == 0 && sizeof(Chunk) == 16 && sizeof(MChunk) == 16 && sizeof(gpr_bnfold) % 8 == 0 && sizeof(gpr_matfold) % 8 == 0,
              "table layout");
// what the ctypes mirrors of givepose_amd/_lib.py must measure (tests/test_repack_cpu.py compares)
static_assert(sizeof(gpr_entry) == 112 && sizeof(gpr_bnfold) == 96 && sizeof(gpr_matfold) == 120 && sizeof(gpr_info) == 72, "struct sizes");

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ half_t lo_plane(float v, half_t hi) { return (half_t)((v - (float)hi) * (float)(1 << GP_SPLIT_SHIFT)); }

__device__ __forceinline__ void put_one(const gpr_entry& e, long long pos, float v) {
    if (e.kind == GPR_KIND_F32) {
        reinterpret_cast<float*>(e.dst)[pos] = v;
    } else {
        half_t* d = reinterpret_cast<half_t*>(e.dst);
        const half_t h = (half_t)v;
        d[pos] = h;
        if (e.kind == GPR_KIND_SPLIT) d[e.plane_stride + pos] = lo_plane(v, h);
    }
}

__global__ __launch_bounds__(WG) void copy_kernel(const DevEntry* __restrict__ E, const Chunk* __restrict__ C) {
    const Chunk c = C[blockIdx.x];
    const DevEntry& d = E[c.entry];
    const gpr_entry& e = d.e;
    const long long dpos = e.dst_off + c.start;
    const int tid = threadIdx.x;
    if (d.contig) {
        const float* __restrict__ s = e.src + e.src_off + c.start;
        int done = 0;
        bool vec = al16(s);
        if (e.kind == GPR_KIND_F32) {
            vec = vec && al16(reinterpret_cast<float*>(e.dst) + dpos);
        } else {
            half_t* h = reinterpret_cast<half_t*>(e.dst) + dpos;
            vec = vec && al16(h) && (e.kind != GPR_KIND_SPLIT || al16(h + e.plane_stride));
        }
        if (vec) {
            const int no = c.count >> 3;
            for (int q = tid; q < no; q += WG) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(s + 8 * q), b = *reinterpret_cast<const f32x4*>(s + 8 * q + 4);
                if (e.kind == GPR_KIND_F32) {
                    float* o = reinterpret_cast<float*>(e.dst) + dpos + 8 * q;
                    *reinterpret_cast<f32x4*>(o) = a;
                    *reinterpret_cast<f32x4*>(o + 4) = b;
                } else {
                    half_t* o = reinterpret_cast<half_t*>(e.dst) + dpos + 8 * q;
                    half8 h;
#pragma unroll
                    for (int j = 0; j < 8; ++j) h[j] = (half_t)(j < 4 ? a[j] : b[j - 4]);
                    *reinterpret_cast<half8*>(o) = h;
                    if (e.kind == GPR_KIND_SPLIT) {      // (uniform over the workgroup: the lo' plane is formed for split entries only)
                        half8 l;
#pragma unroll
                        for (int j = 0; j < 8; ++j) l[j] = lo_plane(j < 4 ? a[j] : b[j - 4], h[j]);
                        *reinterpret_cast<half8*>(o + e.plane_stride) = l;
                    }
                }
            }
            done = no << 3;
        }
        for (int i = done + tid; i < c.count; i += WG) put_one(e, dpos + i, s[i]);
        return;
    }
    // any other view: element i of the view is (i0, i1, i2, i3) row-major over dims
    const float* __restrict__ s = e.src + e.src_off;
    const unsigned d1 = e.dims[1], d2 = e.dims[2], d3 = e.dims[3];
    for (int i = tid; i < c.count; i += WG) {
        unsigned r = (unsigned)(c.start + i);
        const unsigned i3 = r % d3;
        r /= d3;
        const unsigned i2 = r % d2;
        r /= d2;
        const unsigned i1 = r % d1, i0 = r / d1;
        put_one(e, dpos + i, s[i0 * e.strides[0] + i1 * e.strides[1] + i2 * e.strides[2] + i3 * e.strides[3]]);
    }
}

__global__ __launch_bounds__(WG) void bnfold_kernel(const gpr_bnfold* __restrict__ F) {
    const gpr_bnfold f = F[blockIdx.y];
    const long long j = (long long)blockIdx.x * WG + threadIdx.x;
    if (j >= (long long)f.C * (f.K + 1)) return;
    const int c = (int)(j / (f.K + 1)), k = (int)(j - (long long)c * (f.K + 1));
    const float sc = f.bn_w[c] / sqrtf(f.var[c] + f.eps);
    if (k < f.K) {
        f.w_out[(long long)c * f.K + k] = f.w[(long long)c * f.K + k] * sc;
    } else {
        const float t = (f.b[c] - f.mean[c]) * sc;
        f.b_out[c] = t + f.bn_b[c];
    }
}

__global__ __launch_bounds__(WG) void matfold_kernel(const gpr_matfold* __restrict__ F, const MChunk* __restrict__ C) {
    const MChunk c = C[blockIdx.x];
    if ((int)threadIdx.x >= c.count) return;
    const gpr_matfold f = F[c.fold];
    const long long o = c.start + threadIdx.x;
    const int m = (int)(o / f.N), n = (int)(o - (long long)m * f.N);
    const float* __restrict__ a = f.A + (long long)m * f.a_rs;
    double acc = 0.0;
    if (f.b_f64) {
        const double* __restrict__ b = reinterpret_cast<const double*>(f.B) + n;
        for (int k = 0; k < f.K; ++k) acc = fma((double)a[k], b[(long long)k * f.b_rs], acc);
    } else {
        const float* __restrict__ b = reinterpret_cast<const float*>(f.B) + n;
        for (int k = 0; k < f.K; ++k) acc = fma((double)a[k], (double)b[(long long)k * f.b_rs], acc);
    }
    if (f.add) acc += (double)f.add[m];
    if (f.out32) f.out32[(long long)m * f.ld32 + n] = (float)acc;
    if (f.out64) f.out64[(long long)m * f.ld64 + n] = acc;
}

// ---------------------------------------------------------------------------------- host
long long up256(long long n) { return (n + 255) / 256 * 256; }
bool al(const void* p, int a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

long long view_count(const gpr_entry& e) {
    long long n = 1;
    for (int i = 0; i < GPR_MAX_DIMS; ++i) n *= e.dims[i];
    return n;
}

// checks the host tables and lays the device tables out; with `stage` also writes them
int plan_tables(const gpr_entry* entries, int n, const gpr_bnfold* bn, int n_bn, const gpr_matfold* mat, int n_mat, gpr_info& info,
                char* stage, long long stage_bytes, const char* name) {
    GP_REQUIRE(entries && n >= 1 && n <= GPR_MAX_ENTRIES, "%s: a table of 1 .. %d entries is expected (n = %d)", name, GPR_MAX_ENTRIES, n);
    GP_REQUIRE(n_bn >= 0 && n_bn <= 1024 && (n_bn == 0 || bn) && n_mat >= 0 && n_mat <= 1024 && (n_mat == 0 || mat), "%s: bad fold tables (%d, %d)", name,
               n_bn, n_mat);
    long long chunks = 0;
    for (int i = 0; i < n; ++i) {
        const gpr_entry& e = entries[i];
        GP_REQUIRE(e.kind == GPR_KIND_F32 || e.kind == GPR_KIND_F16 || e.kind == GPR_KIND_SPLIT, "%s: entry %d: unknown kind %d", name, i, e.kind);
        GP_REQUIRE(al(e.src, 4) && al(e.dst, e.kind == GPR_KIND_F32 ? 4 : 2), "%s: entry %d: a null or misaligned pointer", name, i);
        long long last = e.src_off;
        for (int k = 0; k < GPR_MAX_DIMS; ++k) {
            GP_REQUIRE(e.dims[k] >= 1 && e.strides[k] >= 0, "%s: entry %d: dim %d is %d with stride %lld", name, i, k, e.dims[k], e.strides[k]);
            GP_REQUIRE(e.strides[k] < (1LL << 31), "%s: entry %d: stride %lld", name, i, e.strides[k]);
            last += (long long)(e.dims[k] - 1) * e.strides[k];
        }
        const long long cnt = view_count(e);
        GP_REQUIRE(cnt >= 1 && cnt < (1LL << 31), "%s: entry %d: a view of %lld elements", name, i, cnt);
        GP_REQUIRE(e.src_off >= 0 && last < e.src_numel, "%s: entry %d: the view reaches element %lld of a source of %lld", name, i, last, e.src_numel);
        GP_REQUIRE(e.dst_off >= 0 && e.dst_off + cnt <= e.dst_numel, "%s: entry %d: elements %lld .. %lld of a destination of %lld", name, i, e.dst_off,
                   e.dst_off + cnt, e.dst_numel);
        GP_REQUIRE(e.kind == GPR_KIND_SPLIT ? e.plane_stride >= e.dst_numel : e.plane_stride == 0, "%s: entry %d: plane_stride %lld", name, i, e.plane_stride);
        chunks += (cnt + GPR_CHUNK - 1) / GPR_CHUNK;
    }
    GP_REQUIRE(chunks < (1LL << 30), "%s: %lld chunks", name, chunks);
    long long bn_blocks = 0;
    for (int i = 0; i < n_bn; ++i) {
        const gpr_bnfold& f = bn[i];
        GP_REQUIRE(al(f.w, 4) && al(f.b, 4) && al(f.bn_w, 4) && al(f.bn_b, 4) && al(f.mean, 4) && al(f.var, 4) && al(f.w_out, 4) && al(f.b_out, 4),
                   "%s: BatchNorm fold %d: a null or misaligned pointer", name, i);
        GP_REQUIRE(f.C >= 1 && f.K >= 1 && (long long)f.C * (f.K + 1) < (1LL << 31) && f.eps > 0.0f, "%s: BatchNorm fold %d: C %d, K %d, eps %g", name, i, f.C,
                   f.K, (double)f.eps);
        GP_REQUIRE((long long)f.C * f.K <= f.w_numel && f.C <= f.c_numel, "%s: BatchNorm fold %d: C %d x K %d against tensors of %lld and %lld elements", name,
                   i, f.C, f.K, f.w_numel, f.c_numel);
        const long long b = ((long long)f.C * (f.K + 1) + WG - 1) / WG;
        if (b > bn_blocks) bn_blocks = b;
    }
    long long mch[2] = {0, 0};
    for (int i = 0; i < n_mat; ++i) {
        const gpr_matfold& f = mat[i];
        GP_REQUIRE(al(f.A, 4) && al(f.B, f.b_f64 ? 8 : 4) && (!f.add || al(f.add, 4)) && (f.out32 || f.out64) && (!f.out32 || al(f.out32, 4)) &&
                       (!f.out64 || al(f.out64, 8)),
                   "%s: matrix fold %d: a null or misaligned pointer", name, i);
        GP_REQUIRE(f.M >= 1 && f.N >= 1 && f.K >= 1 && (long long)f.M * f.N < (1LL << 31) && f.a_rs >= f.K && f.b_rs >= f.N && (!f.out32 || f.ld32 >= f.N) &&
                       (!f.out64 || f.ld64 >= f.N),
                   "%s: matrix fold %d: M %d, N %d, K %d, strides %d %d %d %d", name, i, f.M, f.N, f.K, f.a_rs, f.b_rs, f.ld32, f.ld64);
        GP_REQUIRE((f.level == 0 && !f.b_f64) || f.level == 1, "%s: matrix fold %d: level %d, b_f64 %d", name, i, f.level, f.b_f64);
        // the last element each index expression of matfold_kernel reaches
        GP_REQUIRE((long long)(f.M - 1) * f.a_rs + f.K <= f.a_numel && (long long)(f.K - 1) * f.b_rs + f.N <= f.b_numel && (!f.add || f.M <= f.add_numel) &&
                       (!f.out32 || (long long)(f.M - 1) * f.ld32 + f.N <= f.out32_numel) && (!f.out64 || (long long)(f.M - 1) * f.ld64 + f.N <= f.out64_numel),
                   "%s: matrix fold %d: M %d, N %d, K %d reach outside tensors of %lld, %lld, %lld, %lld, %lld elements", name, i, f.M, f.N, f.K, f.a_numel,
                   f.b_numel, f.add_numel, f.out32_numel, f.out64_numel);
        mch[f.level] += ((long long)f.M * f.N + WG - 1) / WG;
    }
    info = gpr_info{};
    info.n_entries = n, info.n_chunks = (int)chunks, info.n_bn = n_bn, info.n_bn_blocks = (int)bn_blocks, info.n_mat = n_mat;
    info.n_mchunks0 = (int)mch[0], info.n_mchunks1 = (int)mch[1];
    info.off_chunks = up256((long long)n * sizeof(DevEntry));
    info.off_bn = info.off_chunks + up256(chunks * (long long)sizeof(Chunk));
    info.off_mat = info.off_bn + up256((long long)n_bn * sizeof(gpr_bnfold));
    info.off_mchunks = info.off_mat + up256((long long)n_mat * sizeof(gpr_matfold));
    info.bytes = info.off_mchunks + up256((mch[0] + mch[1]) * (long long)sizeof(MChunk)) + 256;
    if (!stage) return 0;
    GP_REQUIRE(stage_bytes >= info.bytes, "%s: staging buffer of %lld bytes needed, %lld given", name, info.bytes, stage_bytes);
    memset(stage, 0, (size_t)info.bytes);
    DevEntry* de = (DevEntry*)stage;
    Chunk* ch = (Chunk*)(stage + info.off_chunks);
    long long c = 0;
    for (int i = 0; i < n; ++i) {
        const gpr_entry& e = entries[i];
        long long run = 1;
        int contig = 1;
        for (int k = GPR_MAX_DIMS - 1; k >= 0; --k) {
            if (e.dims[k] == 1) continue;
            if (e.strides[k] != run) contig = 0;
            run *= e.dims[k];
        }
        de[i] = DevEntry{e, contig, 0};
        const long long cnt = view_count(e);
        for (long long s = 0; s < cnt; s += GPR_CHUNK) ch[c++] = Chunk{i, (int)(cnt - s < GPR_CHUNK ? cnt - s : GPR_CHUNK), s};
    }
    GP_REQUIRE(c == chunks, "%s: internal chunk count", name);
    if (n_bn) memcpy(stage + info.off_bn, bn, (size_t)n_bn * sizeof(gpr_bnfold));
    if (n_mat) memcpy(stage + info.off_mat, mat, (size_t)n_mat * sizeof(gpr_matfold));
    MChunk* mc = (MChunk*)(stage + info.off_mchunks);
    long long m = 0;
    for (int level = 0; level < 2; ++level)
        for (int i = 0; i < n_mat; ++i) {
            if (mat[i].level != level) continue;
            const long long cnt = (long long)mat[i].M * mat[i].N;
            for (long long s = 0; s < cnt; s += WG) mc[m++] = MChunk{i, (int)(cnt - s < WG ? cnt - s : WG), s};
        }
    GP_REQUIRE(m == mch[0] + mch[1], "%s: internal fold chunk count", name);
    return 0;
}

#define GPR_CHECK(name)                                                                               \
    do {                                                                                              \
        hipError_t e__ = hipGetLastError();                                                           \
        if (e__ != hipSuccess) return gp_fail(GP_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e__)); \
    } while (0)

}  // namespace

extern "C" {

long long gpr_tables_bytes(const gpr_entry* entries, int n, const gpr_bnfold* bn, int n_bn, const gpr_matfold* mat, int n_mat) {
    gpr_info info;
    return plan_tables(entries, n, bn, n_bn, mat, n_mat, info, nullptr, 0, "gpr_tables_bytes") == 0 ? info.bytes : 0;
}

int gpr_tables_upload(const gpr_entry* entries, int n, const gpr_bnfold* bn, int n_bn, const gpr_matfold* mat, int n_mat, void* stage,
                      void* tables, long long tables_bytes, gpr_info* info, void* stream) {
    const char* name = "gpr_tables_upload";
    GP_REQUIRE(info && stage, "%s: null info or staging buffer", name);
    gpr_info pl;
    GP_REQUIRE(tables && ((uintptr_t)tables & 255) == 0, "%s: null or misaligned tables", name);
    if (int rc = plan_tables(entries, n, bn, n_bn, mat, n_mat, pl, (char*)stage, tables_bytes, name)) return rc;
    GP_REQUIRE(tables_bytes >= pl.bytes, "%s: tables of %lld bytes needed, %lld given", name, pl.bytes, tables_bytes);
    // the caller owns `stage` and keeps it unchanged until this copy has run (include/givepose_repack.h): nothing here is reused
    const hipError_t e = hipMemcpyAsync(tables, stage, (size_t)pl.bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) return gp_fail(GP_ERR_RUNTIME, "%s: table copy: %s", name, hipGetErrorString(e));
    *info = pl;
    return 0;
}

int gpr_repack(const void* tables, const gpr_info* info, void* stream) {
    const char* name = "gpr_repack";
    hipStream_t s = (hipStream_t)stream;
    GP_REQUIRE(tables && ((uintptr_t)tables & 255) == 0 && info, "%s: null or misaligned tables", name);
    const gpr_info& p = *info;
    GP_REQUIRE(p.n_entries >= 1 && p.n_chunks >= p.n_entries && p.n_bn >= 0 && p.n_mat >= 0 && p.n_mchunks0 >= 0 && p.n_mchunks1 >= 0 &&
                   p.off_chunks > 0 && p.off_bn > p.off_chunks && p.off_mat >= p.off_bn && p.off_mchunks >= p.off_mat && p.bytes > p.off_mchunks,
               "%s: info was not filled by gpr_tables_upload", name);
    const char* base = (const char*)tables;
    const DevEntry* E = (const DevEntry*)base;
    const Chunk* C = (const Chunk*)(base + p.off_chunks);
    const gpr_bnfold* BN = (const gpr_bnfold*)(base + p.off_bn);
    const gpr_matfold* MF = (const gpr_matfold*)(base + p.off_mat);
    const MChunk* MC = (const MChunk*)(base + p.off_mchunks);
    if (p.n_bn) {
        hipLaunchKernelGGL(bnfold_kernel, dim3((unsigned)p.n_bn_blocks, (unsigned)p.n_bn), dim3(WG), 0, s, BN);
        GPR_CHECK(name);
    }
    if (p.n_mchunks0) {
        hipLaunchKernelGGL(matfold_kernel, dim3((unsigned)p.n_mchunks0), dim3(WG), 0, s, MF, MC);
        GPR_CHECK(name);
    }
    if (p.n_mchunks1) {
        hipLaunchKernelGGL(matfold_kernel, dim3((unsigned)p.n_mchunks1), dim3(WG), 0, s, MF, MC + p.n_mchunks0);
        GPR_CHECK(name);
    }
    hipLaunchKernelGGL(copy_kernel, dim3((unsigned)p.n_chunks), dim3(WG), 0, s, E, C);
    GPR_CHECK(name);
    return 0;
}

}  // extern "C"
