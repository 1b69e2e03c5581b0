// The ordered d xp of the map encoder's DCNv3 core (include/givepose_encgrad_ordered.h, GPE_SCATTER_ORDERED): the same terms the
// scatter of encgrad.hip adds with fp32 atomics, added per destination in ascending order of their source id, so that two runs give
// equal bits.
//
// A source is one corner of one tap: id s = (row 9 + q) 4 + (k - 1) for output row `row`, tap q and corner k = 1..4; its group g
// belongs to the destination (b, h, w, g), which holds the 64 channels of that group.  The inverted index is built per call:
//   zero_counts      the (N,H,W,4) counters
//   sources<false>   one thread per (row, g, q): an integer increment per corner inside the image
//   scan_*           exclusive scan of the counters (tile sums, the scan of the tile sums in one workgroup, the tiles' own scans)
//   sources<true>    the same threads hand out the slots of each destination's segment with an integer add and store their ids:
//                    the ORDER inside a segment depends on the run, its SET does not
//   gather           one wavefront per destination, a lane per channel: it takes the ids of its segment in ascending order
//                    (up to 64: held one per lane, ranked by counting; more: repeated selection of the smallest id above the
//                    last one taken), re-forms the wave-uniform corner weight from the offsets and adds
//                    fmul(w_k, fmul(dy, mask)) to a register; every element of d xp is written once, by its own lane.
// The integer atomics decide only how many ids a destination has and where in its segment each lies; neither reaches the sum.
// No floating-point atomic, and no zero-fill of d xp.
#include "common.hpp"
#include "encscatter.hpp"
#include "../../include/givepose_encgrad_ordered.h"

namespace {

constexpr int FEAT = GPE_FEAT, DG = GPE_DCN_GROUPS, DD = GPE_DCN_CHANNELS, TAPS = GPE_TAPS;
constexpr int WG = 256, SCAN_TILE = 4 * WG, CORNERS = 4;
constexpr int NO_ID = 0x7fffffff;
static_assert(FEAT == DG * DD && DD == 64, "a destination is one wavefront: 64 channels of one group");

long up64(long n) { return (n + 63) / 64 * 64; }

// hipcc contracts a * b + c into an fma by default; the contract of the ordered mode is a product rounded on its own, then a sum
__device__ __forceinline__ float fmul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float fadd(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// tap_of of encgrad.hip: the same expressions, so the same corners and the same weights
struct Tap {
    bool valid, o[CORNERS];
    int h_low, w_low;
    float lh, lw, hh, hw;
};
__device__ __forceinline__ Tap tap_of(float w, float h, int H, int W) {
    Tap t;
    t.valid = h > -1.0f && w > -1.0f && h < (float)H && w < (float)W;
    t.h_low = (int)floorf(h);
    t.w_low = (int)floorf(w);
    t.lh = h - (float)t.h_low;
    t.lw = w - (float)t.w_low;
    t.hh = 1.0f - t.lh;
    t.hw = 1.0f - t.lw;
    const bool top = t.h_low >= 0, bot = t.h_low + 1 <= H - 1, lef = t.w_low >= 0, rig = t.w_low + 1 <= W - 1;
    t.o[0] = t.valid && top && lef;
    t.o[1] = t.valid && top && rig;
    t.o[2] = t.valid && bot && lef;
    t.o[3] = t.valid && bot && rig;
    return t;
}
__device__ __forceinline__ Tap tap_at(const float* __restrict__ offset, long rg, int q, int wo, int ho, int H, int W) {
    const float* off = offset + rg * (TAPS * 2);
    const float w = (float)(2 * wo - 1) + ((float)(q / 3) + off[2 * q]);
    const float h = (float)(2 * ho - 1) + ((float)(q % 3) + off[2 * q + 1]);
    return tap_of(w, h, H, W);
}

__global__ __launch_bounds__(WG) void zero_counts_kernel(int* __restrict__ p, long n) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    if (i < n) p[i] = 0;
}

// One thread per (row, g, q).  FILL false: slots = the counters, one increment per corner inside the image.  FILL true: slots = the
// segments' cursors (their starts before this launch, their ends after it); the value an add returns is this id's place.
template <bool FILL>
__global__ __launch_bounds__(WG) void sources_kernel(const float* __restrict__ offset, int H, int W, int Ho, int Wo, long rows, int* slots,
                                                     int* __restrict__ ids) {
    const long idx = (long)blockIdx.x * WG + threadIdx.x;
    if (idx >= rows * (DG * TAPS)) return;
    const int q = (int)(idx % TAPS);
    const long rg = idx / TAPS, row = rg / DG;
    const int g = (int)(rg % DG);
    const int wo = (int)(row % Wo), ho = (int)(row / Wo % Ho), b = (int)(row / ((long)Wo * Ho));
    const Tap t = tap_at(offset, rg, q, wo, ho, H, W);
    if (!t.valid) return;
    const long pix = ((long)b * H + t.h_low) * W + t.w_low;      // corner 1; used only through the corners inside the image
    const int s0 = (int)((row * TAPS + q) * CORNERS);
#pragma unroll
    for (int k = 0; k < CORNERS; ++k) {
        if (!t.o[k]) continue;
        const long d = (pix + (k >> 1) * W + (k & 1)) * DG + g;
        const int place = atomicAdd(slots + d, 1);      // int: a count, or a slot of a list that the gather orders by id
        if (FILL) ids[place] = s0 + k;
    }
}

// ---- exclusive scan of n <= 2^25 counters, tiles of SCAN_TILE (a thread holds 4 consecutive ones)
__device__ __forceinline__ int block_scan_exclusive(int v, int* sh, int& total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < WG; o <<= 1) {
        const int a = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    total = sh[WG - 1];
    const int r = sh[t] - v;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(WG) void scan_tile_sums_kernel(const int* __restrict__ cnt, long n, int* __restrict__ tile_sum) {
    __shared__ int sh[WG];
    const long i0 = (long)blockIdx.x * SCAN_TILE + threadIdx.x * 4;
    int v = 0, total;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i0 + j < n) v += cnt[i0 + j];
    block_scan_exclusive(v, sh, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(WG) void scan_tiles_kernel(int* __restrict__ tile_sum, int tiles) {      // one workgroup, in place
    __shared__ int sh[WG];
    int carry = 0;
    for (int c = 0; c < tiles; c += WG) {
        const int i = c + threadIdx.x;
        int total;
        const int e = block_scan_exclusive(i < tiles ? tile_sum[i] : 0, sh, total);
        if (i < tiles) tile_sum[i] = carry + e;
        carry += total;
    }
}

// cnt holds the counters on entry and each segment's start on exit (the fill's cursor); start keeps a second copy
__global__ __launch_bounds__(WG) void scan_finish_kernel(int* __restrict__ cnt, long n, const int* __restrict__ tile_sum,
                                                         int* __restrict__ start) {
    __shared__ int sh[WG];
    const long i0 = (long)blockIdx.x * SCAN_TILE + threadIdx.x * 4;
    int v[4], sum = 0, total;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = i0 + j < n ? cnt[i0 + j] : 0;
        sum += v[j];
    }
    int e = block_scan_exclusive(sum, sh, total) + tile_sum[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (i0 + j < n) {
            start[i0 + j] = e;
            cnt[i0 + j] = e;
        }
        e += v[j];
    }
}

// ---- the gather
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// acc + fmul(w_k, fmul(dy, mask)) of source s (wave-uniform) for this lane's channel of group g
__device__ __forceinline__ float add_term(float acc, int s, int g, int lane, const float* __restrict__ offset, const float* __restrict__ mask,
                                          const float* __restrict__ dy, int H, int W, int Ho, int Wo) {
    const int k = s & 3, rq = s >> 2, row = rq / TAPS, q = rq - row * TAPS;
    const int wo = row % Wo, ho = row / Wo % Ho;
    const long rg = (long)row * DG + g;
    const Tap t = tap_at(offset, rg, q, wo, ho, H, W);
    const float wk = k == 0 ? fmul(t.hh, t.hw) : k == 1 ? fmul(t.hh, t.lw) : k == 2 ? fmul(t.lh, t.hw) : fmul(t.lh, t.lw);
    const float tg = fmul(dy[rg * DD + lane], mask[rg * TAPS + q]);
    return fadd(acc, fmul(wk, tg));
}

__global__ __launch_bounds__(WG) void gather_kernel(const float* __restrict__ offset, const float* __restrict__ mask,
                                                    const float* __restrict__ dy, const int* __restrict__ start,
                                                    const int* __restrict__ end, const int* __restrict__ ids, int H, int W, int Ho, int Wo,
                                                    long ndest, int nsrc, float* __restrict__ dxp) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long dest = (long)blockIdx.x * (WG / 64) + wave;      // ((b H + h) W + w) 4 + g
    if (dest >= ndest) return;      // wave-uniform
    const int g = (int)(dest % DG);
    const int begin = __builtin_amdgcn_readfirstlane(start[dest]);
    const int n = __builtin_amdgcn_readfirstlane(end[dest]) - begin;
    float acc = 0.0f;
    if (n <= 64) {
        const int mine = lane < n ? ids[begin + lane] : NO_ID;
        int rank = 0;      // the ids of a list differ, so the ranks of its lanes are 0 .. n - 1
        for (int j = 0; j < n; ++j) rank += __builtin_amdgcn_readlane(mine, j) < mine ? 1 : 0;
        for (int i = 0; i < n; ++i) {
            const unsigned long long holder = __ballot(rank == i);
            if (holder == 0) continue;
            const int s = __builtin_amdgcn_readlane(mine, __builtin_amdgcn_readfirstlane(__ffsll(holder) - 1));
            if ((unsigned)s >= (unsigned)nsrc) continue;      // never for a list the two passes above built
            acc = add_term(acc, s, g, lane, offset, mask, dy, H, W, Ho, Wo);
        }
    } else {
        int last = -1;
        for (int i = 0; i < n; ++i) {
            int m = NO_ID;
            for (int j = lane; j < n; j += 64) {
                const int v = ids[begin + j];
                m = v > last && v < m ? v : m;
            }
            const int s = __builtin_amdgcn_readfirstlane(wave_min(m));
            if ((unsigned)s >= (unsigned)nsrc) break;
            acc = add_term(acc, s, g, lane, offset, mask, dy, H, W, Ho, Wo);
            last = s;
        }
    }
    dxp[dest * DD + lane] = acc;
}

#define LAUNCHED(name)                                                                                    \
    do {                                                                                                  \
        hipError_t e__ = hipGetLastError();                                                               \
        if (e__ != hipSuccess) return gp_fail(GP_ERR_LAUNCH, "%s: %s", name, hipGetErrorString(e__));     \
    } while (0)

}  // namespace

namespace encscatter {

long ordered_dxp_ws_floats(long N, long H, long W) {
    const long ndest = N * H * W * DG, rows = N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    return 2 * up64(ndest) + up64(cdiv(ndest, SCAN_TILE)) + up64(rows * (DG * TAPS * CORNERS));
}

int ordered_dxp(const float* offset, const float* mask, const float* dy, int N, int H, int W, float* dxp, float* ws, long ws_floats,
                hipStream_t s, const char* name) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long ndest = (long)N * H * W * DG, rows = (long)N * Ho * Wo, threads = rows * (DG * TAPS);
    const int tiles = cdiv(ndest, SCAN_TILE);
    GP_REQUIRE(ndest < (1L << 25) && rows * (TAPS * CORNERS) < (1L << 31), "%s: too many destinations or sources for 32-bit ids", name);
    GP_REQUIRE(ws && ws_floats >= ordered_dxp_ws_floats(N, H, W), "%s: workspace of the ordered scatter missing or too small", name);
    int* cursor = (int*)ws;
    int* start = cursor + up64(ndest);
    int* tile_sum = start + up64(ndest);
    int* ids = tile_sum + up64(tiles);
    hipLaunchKernelGGL(zero_counts_kernel, dim3(cdiv(ndest, WG)), dim3(WG), 0, s, cursor, ndest);
    LAUNCHED(name);
    hipLaunchKernelGGL(sources_kernel<false>, dim3(cdiv(threads, WG)), dim3(WG), 0, s, offset, H, W, Ho, Wo, rows, cursor, ids);
    LAUNCHED(name);
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3(tiles), dim3(WG), 0, s, (const int*)cursor, ndest, tile_sum);
    LAUNCHED(name);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(WG), 0, s, tile_sum, tiles);
    LAUNCHED(name);
    hipLaunchKernelGGL(scan_finish_kernel, dim3(tiles), dim3(WG), 0, s, cursor, ndest, (const int*)tile_sum, start);
    LAUNCHED(name);
    hipLaunchKernelGGL(sources_kernel<true>, dim3(cdiv(threads, WG)), dim3(WG), 0, s, offset, H, W, Ho, Wo, rows, cursor, ids);
    LAUNCHED(name);
    hipLaunchKernelGGL(gather_kernel, dim3(cdiv(ndest, WG / 64)), dim3(WG), 0, s, offset, mask, dy, (const int*)start, (const int*)cursor,
                       (const int*)ids, H, W, Ho, Wo, ndest, (int)(rows * (TAPS * CORNERS)), dxp);
    LAUNCHED(name);
    return 0;
}

}  // namespace encscatter
