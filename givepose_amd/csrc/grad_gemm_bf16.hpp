// The bf16-operand form of the functor GEMM (grad_gemm.hpp): the same operand views and store functors, the products on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulators.
//
// Numerical contract.  Every operand element is the fp32 value its view returns, rounded to bf16 (round to nearest even:
// `(__bf16)x` is v_cvt_pk_bf16_f32 on gfx950) after the view's own arithmetic and before the product; in memory the operands stay
// fp32, the rounding lives in the tile staging.  An element outside the tensor is an exact 0.  The accumulators are fp32 and the
// store functor sees the fp32 accumulator.  The split of k depends on the shape alone (gemm_bf16_split), the partial results are
// merged in order by gemm_merge_kernel, and there is no atomic: equal inputs give equal bits, and scaling an operand by a power of
// two scales the result bit for bit (short of overflow and underflow).
//
// Kernel.  A workgroup of four waves owns a 128 x 128 tile, a wave 64 x 64 of it as 2 x 2 MFMA tiles: 32 FLOP per byte of fp32
// operand traffic, twice the 64 x 64 tile's.  k advances in steps of 32 through two LDS buffers, so a step costs one barrier: the
// next step's operands are fetched into registers before the step's MFMAs and stored to the other buffer after them.  Both LDS
// images are [m or n][k] in bf16, rows padded from 64 to 80 bytes, so a lane's eight k-neighbours of a fragment are one 16-byte
// read.  Staging packs four k-neighbours in registers and stores 8 bytes: an operand whose k is adjacent in memory is fetched as
// four consecutive elements per lane (eight lanes cover a 128-byte row segment), one whose m (or n) is adjacent is fetched with the
// lane index on m, four k apart in the lane's own registers -- every load instruction of a wave is contiguous either way.
#ifndef GIVEPOSE_GRAD_GEMM_BF16_HPP
#define GIVEPOSE_GRAD_GEMM_BF16_HPP

#include "grad_gemm.hpp"

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

namespace {

constexpr int HM = 128, HN = 128, HK = 32, HLD = HK + 8;      // tile, k step, LDS row length in bf16 (80 bytes: 16-byte aligned)
constexpr int H_MAX_SPLIT = 16;                               // partial sums of one contraction, merged in k order

// element (mn, k) of an operand: A(m, k), or B(k, n)
template <bool IS_B, class F>
__device__ __forceinline__ float bf16_operand(const F& f, int mn, int k) { return IS_B ? f(k, mn) : f(mn, k); }

// the thread's four groups of four k-neighbours of a 128 x 32 operand tile.  KFAST: consecutive k are adjacent in memory
template <bool KFAST>
__device__ __forceinline__ void bf16_slot(int i, int& mn, int& k) {
    const int t = threadIdx.x;
    if (KFAST) {
        k = (t & 7) * 4;
        mn = (t >> 3) + 32 * i;
    } else {
        mn = t & 127;
        k = (t >> 7) * 4 + 8 * i;
    }
}

// a plain matrix whose k is adjacent in memory -- MatRow as A, MatCol as B: p[mn * ld + k] -- gives its four k-neighbours in one
// 16-byte load (a global load needs 4-byte alignment only)
template <bool IS_B, class F> struct Bf16Plain { static constexpr bool value = false; };
template <> struct Bf16Plain<false, MatRow> { static constexpr bool value = true; };
template <> struct Bf16Plain<true, MatCol> { static constexpr bool value = true; };

// A view whose k is adjacent in memory only inside a stretch (a channel of a crop) may give a group of four k-neighbours in one
// 16-byte load as well: get() fills q and answers true when the whole group lies inside one stretch, and answers false where it does
// not (a crop boundary), in which case the group is fetched element by element through the view.  Which elements are read, and so
// every bit of the result, is the same either way.  (The same for the stride-1 window as B -- a row of a map, at a tap shift -- was
// measured slower than the element-wise fetch and is not kept: DESIGN.md 1k.)  GP_BF16_WIDE_MASK (investigation builds only,
// givepose_amd/build.py GP_EXTRA_HIPCC_FLAGS) switches specialisations off for A/B timing: bit 0 Tr<Nchw> as A, bit 1 the stride-1
// window as A (Bf16Rows below, specialised in xyz_conv_prec.hpp).
#ifndef GP_BF16_WIDE_MASK
#define GP_BF16_WIDE_MASK 3
#endif
template <bool IS_B, class F> struct Bf16Wide { static constexpr bool value = false; };
template <> struct Bf16Wide<false, Tr<Nchw>> {      // A(m, k) = p[(b C + m) HW + px], k = (b, px): four pixels of one channel of one crop
    static constexpr bool value = (GP_BF16_WIDE_MASK & 1) != 0;
    static __device__ __forceinline__ bool get(const Tr<Nchw>& f, int m, int k, f32x4& q) {
        const int HW = f.f.HW, b = k / HW, px = k - b * HW;
        if (px + 3 >= HW) return false;
        __builtin_memcpy(&q, f.f.p + (((long)b * f.f.C + m) * HW + px), 16);
        return true;
    }
};

template <bool IS_B, bool KFAST, class F>
__device__ __forceinline__ void bf16_fetch(const F& f, int mn0, int MN, int k0, int kend, float (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int mn, k;
        bf16_slot<KFAST>(i, mn, k);
        const int gmn = mn0 + mn, gk = k0 + k;
        if (gmn < MN && gk + 3 < kend) {
            if constexpr (KFAST && Bf16Plain<IS_B, F>::value) {
                f32x4 q;
                __builtin_memcpy(&q, f.p + ((long)gmn * f.ld + gk), 16);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[4 * i + j] = q[j];
            } else if constexpr (KFAST && Bf16Wide<IS_B, F>::value) {
                f32x4 q;
                if (Bf16Wide<IS_B, F>::get(f, gmn, gk, q)) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[4 * i + j] = q[j];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[4 * i + j] = bf16_operand<IS_B>(f, gmn, gk + j);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[4 * i + j] = bf16_operand<IS_B>(f, gmn, gk + j);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * i + j] = (gmn < MN && gk + j < kend) ? bf16_operand<IS_B>(f, gmn, gk + j) : 0.0f;
        }
    }
}

// An A operand fetched with m on the lane keeps a thread on ONE row m for the whole contraction, and its k -- (t >> 7) * 4 + 8 i + j on top
// of the step's k0 -- is the same in every lane of a wave.  A view can therefore keep what depends on the row in a per-thread State
// formed once in front of the k loop (init), and form what depends on k in scalar registers (get); the k offset of the wave is read
// through readfirstlane so that the compiler knows it to be uniform.  A row outside the matrix gets a State whose elements are all 0.
template <class F> struct Bf16Rows {
    static constexpr bool value = false;
    struct State {};
    static __device__ __forceinline__ State init(const F&, int, int) { return {}; }
};

template <class F>
__device__ __forceinline__ void bf16_fetch_rows(const F& f, const typename Bf16Rows<F>::State& st, int k0, int kend, float (&v)[16]) {
    const int kq = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 7)) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gk = k0 + kq + 8 * i + j;
            v[4 * i + j] = gk < kend ? Bf16Rows<F>::get(f, st, gk) : 0.0f;
        }
}

template <bool KFAST>
__device__ __forceinline__ void bf16_put(__bf16 (*S)[HLD], const float (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int mn, k;
        bf16_slot<KFAST>(i, mn, k);
        bf16x4_t p;
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = (__bf16)v[4 * i + j];
        *reinterpret_cast<bf16x4_t*>(&S[mn][k]) = p;
    }
}

// C(m, n) = sum_k bf16(A(m, k)) bf16(B(k, n)), k in [z kchunk, min(K, (z + 1) kchunk)).  With one chunk the result goes through the
// store functor, else to part[z][m][n] for gemm_merge_kernel.
template <class AF, class BF, class EP>
__global__ __launch_bounds__(WG) void gemm_bf16_kernel(AF A, BF Bm, EP ep, int M, int N, int K, int kchunk, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) __bf16 As[2][HM][HLD];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[2][HN][HLD];
    constexpr bool AK = AF::FAST_C, BK = !BF::FAST_C, AROWS = !AK && Bf16Rows<AF>::value;
    const int m0 = blockIdx.x * HM, n0 = blockIdx.y * HN;
    const int kbeg = blockIdx.z * kchunk, kend = min(K, kbeg + kchunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int l32 = lane & 31, half = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    float ra[16], rb[16];
    const typename Bf16Rows<AF>::State arow = Bf16Rows<AF>::init(A, blockIdx.x * HM + (threadIdx.x & 127), M);
    auto fetch_a = [&](int k0) {
        if constexpr (AROWS) bf16_fetch_rows(A, arow, k0, kend, ra);
        else bf16_fetch<false, AK>(A, m0, M, k0, kend, ra);
    };
    fetch_a(kbeg);
    bf16_fetch<true, BK>(Bm, n0, N, kbeg, kend, rb);
    bf16_put<AK>(As[0], ra);
    bf16_put<BK>(Bs[0], rb);
    __syncthreads();
    int cur = 0;
    for (int k0 = kbeg; k0 < kend; k0 += HK) {
        const bool more = k0 + HK < kend;
        if (more) {
            fetch_a(k0 + HK);
            bf16_fetch<true, BK>(Bm, n0, N, k0 + HK, kend, rb);
        }
#pragma unroll
        for (int ks = 0; ks < HK; ks += 16) {
            bf16x8_t fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const bf16x8_t*>(&As[cur][wm + 32 * i + l32][ks + 8 * half]);
                fb[i] = *reinterpret_cast<const bf16x8_t*>(&Bs[cur][wn + 32 * i + l32][ks + 8 * half]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    // the MFMA puts its second operand's index on the lane: m when the store wants m adjacent, else n
                    if (EP::M_FAST) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
                    else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
                }
        }
        if (more) {      // the other buffer: its last readers passed the barrier that ended the step before
            bf16_put<AK>(As[cur ^ 1], ra);
            bf16_put<BK>(Bs[cur ^ 1], rb);
        }
        __syncthreads();
        cur ^= 1;
    }
    const bool split = gridDim.z > 1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int q = (r & 3) + 8 * (r >> 2) + 4 * half;      // index of the first operand, l32 that of the second
                const int m = m0 + wm + 32 * i + (EP::M_FAST ? l32 : q), n = n0 + wn + 32 * j + (EP::M_FAST ? q : l32);
                if (m < M && n < N) {
                    if (split) part[((long)blockIdx.z * M + m) * N + n] = acc[i][j][r];
                    else ep(m, n, acc[i][j][r]);
                }
            }
}

// the split of a contraction depends on the shape alone: problems with fewer tiles than the chip has compute units are cut into
// up to H_MAX_SPLIT chunks of k, each a multiple of the k step
void gemm_bf16_split(long M, long N, long K, int& S, int& kchunk) {
    S = 1;
    kchunk = HK;
    if (M <= 0 || N <= 0 || K <= 0) return;      // not a GEMM: the callers refuse it, the size queries answer 0
    const long tiles = (long)cdiv(M, HM) * cdiv(N, HN);
    long s = 1;
    if (tiles < 256) s = 512 / tiles < H_MAX_SPLIT ? 512 / tiles : H_MAX_SPLIT;
    kchunk = cdiv(cdiv(K, s), HK) * HK;
    S = cdiv(K, kchunk);
}
long gemm_bf16_ws_floats(long M, long N, long K) {
    int S, kc;
    gemm_bf16_split(M, N, K, S, kc);
    return S > 1 ? (long)S * M * N : 0;
}

template <class AF, class BF, class EP>
int gemm_bf16(const AF& A, const BF& Bm, const EP& ep, long M, long N, long K, float* ws, long ws_floats, hipStream_t s, const char* name) {
    GP_REQUIRE(M > 0 && N > 0 && K > 0 && M < (1L << 30) && N < (1L << 30) && K < (1L << 30) && cdiv(N, HN) <= 65535,
               "%s: bad GEMM shape %ld x %ld x %ld", name, M, N, K);
    int S, kchunk;
    gemm_bf16_split(M, N, K, S, kchunk);
    GP_REQUIRE(S == 1 || (ws && ws_floats >= (long)S * M * N), "%s: workspace too small (%ld floats, %ld needed)", name, ws_floats,
               (long)S * M * N);
    hipLaunchKernelGGL((gemm_bf16_kernel<AF, BF, EP>), dim3(cdiv(M, HM), cdiv(N, HN), S), dim3(WG), 0, s, A, Bm, ep, (int)M, (int)N, (int)K,
                       kchunk, ws);
    GPH_CHECK(name);
    if (S > 1) {
        hipLaunchKernelGGL((gemm_merge_kernel<EP>), dim3(cdiv(M * N, WG)), dim3(WG), 0, s, (const float*)ws, ep, (int)M, (int)N, S);
        GPH_CHECK(name);
    }
    return 0;
}

}  // namespace

#endif
