// The colour augmentation on the device (include/givepose_coloraug.h, gpca_*): PIL.ImageEnhance's Sharpness, Contrast, Brightness and
// Color on whole uint8 frames, byte for byte.
//
//   coloraug_luma_kernel    grid (GPCA_PARTIALS, F): the integer sum of L over a range of a Contrast frame's pixels, one value per block
//   coloraug_apply_kernel   grid (blocks, F): one stage of every frame that takes part in it.  The operation is uniform in a block.
//                           Three walks of a frame, all on out_byte's arithmetic:
//                             bytes     any alignment and shape: a thread per byte (odd shapes, and the tail of the next walk)
//                             chunks    source and destination 16-byte aligned: a 16-byte vector per thread and step; Color takes the
//                                       two bytes before and after the vector for the pixels that straddle it
//                             strips    Sharpness, aligned, 3 W a multiple of 16: a thread owns 16 bytes of SR consecutive rows and
//                                       keeps the three live rows (24 bytes each, with the neighbour pixels) in registers
#include <stdint.h>

#include "common.hpp"
#include "../../include/givepose_coloraug.h"

// No contraction in this file: blend's product and sum, and SMOOTH's products and sums, are rounded separately, as Pillow's C rounds them.
// The operators below are plain * and + under this pragma (the idiom of repack.hip): the header's __fmul_rn / __fadd_rn are compiled
// under the command line's contraction mode and fuse.
#pragma clang fp contract(off)

namespace {

constexpr int CT = 256;                  // threads of a workgroup
constexpr int SR = 8;                    // rows of a Sharpness strip
constexpr float K1 = 1.0f / 13.0f, K5 = 5.0f / 13.0f;      // fl32(1/13), fl32(5/13): the compiler folds them correctly rounded

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// t <= 0 -> 0, t >= 255 -> 255, else trunc(t); for 0 <= f <= 1, t lies in [0, 255] and the clip is the identity
__device__ __forceinline__ int clip_trunc(float t) { return (int)fminf(fmaxf(t, 0.0f), 255.0f); }

__device__ __forceinline__ int blend(int d, int x, float f) {
    const float p = f * (float)(x - d);
    return clip_trunc((float)d + p);
}

__device__ __forceinline__ float row3(float a, float b, float c, float kb) {
    const float pa = a * K1, pb = b * kb, pc = c * K1;
    return (pa + pb) + pc;
}

// SMOOTH of an interior byte: the rows below, at and above it, each as (left, centre, right) of the same channel
__device__ __forceinline__ int smooth9(float dl, float dc, float dr, float ml, float mc, float mr, float ul, float uc, float ur) {
    float s = 0.5f;
    s = s + row3(dl, dc, dr, K1);
    s = s + row3(ml, mc, mr, K5);
    s = s + row3(ul, uc, ur, K1);
    return clip_trunc(s);
}

// One output byte from global memory: the definition the vector walks restate.  s: the frame as it enters the stage, i: byte index.
__device__ __forceinline__ int out_byte(const unsigned char* __restrict__ s, int i, int op, float f, int m, int H, int W) {
    const int x = s[i];
    if (op == GPCA_OP_NONE) return x;
    int d = m;                                               // Contrast: the mean; Brightness: the caller passes 0
    if (op == GPCA_OP_COLOR) {
        const unsigned char* p = s + (i - i % 3);
        d = luma(p[0], p[1], p[2]);
    } else if (op == GPCA_OP_SHARPNESS) {
        const int rb = 3 * W, y = i / rb, px = (i - y * rb) / 3;
        if (y == 0 || y == H - 1 || px == 0 || px == W - 1) d = x;
        else {
            const unsigned char *u = s + i - rb, *l = s + i + rb;
            d = smooth9((float)l[-3], (float)l[0], (float)l[3], (float)s[i - 3], (float)x, (float)s[i + 3], (float)u[-3], (float)u[0], (float)u[3]);
        }
    }
    return blend(d, x, f);
}

__device__ __forceinline__ const unsigned char* pick_src(int sel, const unsigned char* frames, const unsigned char* tmp0, const unsigned char* tmp1) {
    return sel == GPCA_BUF_FRAMES ? frames : sel == GPCA_BUF_TMP0 ? tmp0 : tmp1;
}

// byte j (compile-time after unrolling) of a run of dwords
#define BYTE_OF(w, j) ((int)(((w)[(j) >> 2] >> (((j) & 3) * 8)) & 255u))

// The 2 bytes that follow a 16-byte vector at c0, as the low half of a dword; 0 beyond the frame's n bytes.
__device__ __forceinline__ unsigned after16(const unsigned char* __restrict__ s, int c0, int n) {
    if (c0 + 20 <= n) return *reinterpret_cast<const unsigned*>(s + c0 + 16);
    unsigned w = 0;
    if (c0 + 16 < n) w |= s[c0 + 16];
    if (c0 + 17 < n) w |= (unsigned)s[c0 + 17] << 8;
    return w;
}

// ---------------------------------------------------------------------------------- the Contrast reduction
__global__ __launch_bounds__(CT) void coloraug_luma_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ tmp0,
                                                           const unsigned char* __restrict__ tmp1, const int* __restrict__ table,
                                                           unsigned long long* __restrict__ partials, int H, int W) {
    __shared__ unsigned long long wsum[CT / 64];
    const int f = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    const int4 e = reinterpret_cast<const int4*>(table)[f];
    if (e.x != GPCA_OP_CONTRAST) return;
    const int N = H * W, n = 3 * N;
    const unsigned char* __restrict__ s = pick_src(e.z, frames, tmp0, tmp1) + (long)f * n;
    unsigned sum = 0;                                        // a thread sees N / (GPCA_PARTIALS * CT) + 1 pixels of at most 255 each
    if (((uintptr_t)s & 15) == 0) {
        // a pixel belongs to the vector its first byte lies in
        const int nch = n >> 4, cpb = (nch + GPCA_PARTIALS - 1) / GPCA_PARTIALS, k1 = min((b + 1) * cpb, nch);
        for (int k = b * cpb + t; k < k1; k += CT) {
            const int c0 = k << 4;
            const uint4 v = *reinterpret_cast<const uint4*>(s + c0);
            const unsigned w[5] = {v.x, v.y, v.z, v.w, after16(s, c0, n)};
            const int ph = c0 % 3;                           // the channel of byte 0
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                int c = ph + j % 3;
                c = c >= 3 ? c - 3 : c;
                if (c == 0) sum += luma(BYTE_OF(w, j), BYTE_OF(w, j + 1), BYTE_OF(w, j + 2));
            }
        }
        if (b == GPCA_PARTIALS - 1)
            for (int i = (nch << 4) + t; i < n; i += CT)
                if (i % 3 == 0) sum += luma(s[i], s[i + 1], s[i + 2]);
    } else {
        const int ppb = (N + GPCA_PARTIALS - 1) / GPCA_PARTIALS, p1 = min((b + 1) * ppb, N);
        for (int p = b * ppb + t; p < p1; p += CT) sum += luma(s[3 * p], s[3 * p + 1], s[3 * p + 2]);
    }
    unsigned long long v = sum;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((t & 63) == 0) wsum[t >> 6] = v;
    __syncthreads();
    if (t == 0) {
        unsigned long long tot = 0;
#pragma unroll
        for (int w = 0; w < CT / 64; ++w) tot += wsum[w];
        partials[(long)f * GPCA_PARTIALS + b] = tot;
    }
}

// ---------------------------------------------------------------------------------- a stage
// 24 bytes of row `row` around the 16 at byte offset c: c - 4 .. c + 19, zero where they would leave the row (those feed border pixels only)
__device__ __forceinline__ void load_row24(const unsigned char* __restrict__ row, int c, bool first, bool last, unsigned (&w)[6]) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + c);
    w[0] = first ? 0u : *reinterpret_cast<const unsigned*>(row + c - 4);
    w[1] = v.x, w[2] = v.y, w[3] = v.z, w[4] = v.w;
    w[5] = last ? 0u : *reinterpret_cast<const unsigned*>(row + c + 16);
}

__global__ __launch_bounds__(CT) void coloraug_apply_kernel(const unsigned char* __restrict__ frames, unsigned char* tmp0, unsigned char* tmp1,
                                                            unsigned char* out, const int* __restrict__ table,
                                                            const unsigned long long* __restrict__ partials, int H, int W) {
    __shared__ int s_m;
    const int f = blockIdx.y, t = threadIdx.x;
    const int4 e = reinterpret_cast<const int4*>(table)[f];
    const int op = e.x;
    if (op < 0) return;
    const float fac = __int_as_float(e.y);
    const int N = H * W, n = 3 * N;
    const unsigned char* __restrict__ s = pick_src(e.z, frames, tmp0, tmp1) + (long)f * n;
    unsigned char* __restrict__ d = (e.w == GPCA_BUF_TMP0 ? tmp0 : e.w == GPCA_BUF_TMP1 ? tmp1 : out) + (long)f * n;
    int m = 0;
    if (op == GPCA_OP_CONTRAST) {                            // uniform in the block
        if (t < 64) {
            unsigned long long v = partials[(long)f * GPCA_PARTIALS + t];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (t == 0) {
                // (2 sum + N) / (2 N) <= 255, bit by bit: a 64-bit division would expand to float code with fused multiply-adds,
                // which the conformance test of this file's kernels (tests/test_color_aug_cpu.py) looks for
                const unsigned long long num = 2ull * v + (unsigned long long)N, den = 2ull * (unsigned long long)N;
                int q = 0;
#pragma unroll
                for (int bit = 128; bit > 0; bit >>= 1)
                    if ((unsigned long long)(q + bit) * den <= num) q += bit;
                s_m = q;
            }
        }
        __syncthreads();
        m = s_m;
    }
    const int first = blockIdx.x * CT + t, stride = gridDim.x * CT;
    const bool aligned = ((((uintptr_t)s) | ((uintptr_t)d)) & 15) == 0;
    const int rb = 3 * W;
    if (!aligned || (op == GPCA_OP_SHARPNESS && (rb & 15) != 0)) {
        for (int i = first; i < n; i += stride) d[i] = (unsigned char)out_byte(s, i, op, fac, m, H, W);
        return;
    }
    const int nch = n >> 4;
    for (int i = (nch << 4) + first; i < n; i += stride) d[i] = (unsigned char)out_byte(s, i, op, fac, m, H, W);      // n % 16 bytes

    if (op == GPCA_OP_SHARPNESS) {
        const int cpr = rb >> 4, nstrip = (H + SR - 1) / SR;
        for (int wk = first; wk < nstrip * cpr; wk += stride) {
            const int strip = wk / cpr, cx = wk - strip * cpr, c = cx << 4;
            const bool cf = cx == 0, cl = cx == cpr - 1;
            const int y0 = strip * SR, y1 = min(y0 + SR, H);
            unsigned up[6] = {0, 0, 0, 0, 0, 0}, mid[6], dn[6] = {0, 0, 0, 0, 0, 0};
            if (y0 > 0) load_row24(s + (long)(y0 - 1) * rb, c, cf, cl, up);
            load_row24(s + (long)y0 * rb, c, cf, cl, mid);
            for (int y = y0; y < y1; ++y) {
                if (y + 1 < H) load_row24(s + (long)(y + 1) * rb, c, cf, cl, dn);
                unsigned o[4] = {mid[1], mid[2], mid[3], mid[4]};
                if (y > 0 && y < H - 1) {
                    o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int j = q + 4, x = BYTE_OF(mid, j);
                        int sm = smooth9((float)BYTE_OF(dn, j - 3), (float)BYTE_OF(dn, j), (float)BYTE_OF(dn, j + 3),
                                         (float)BYTE_OF(mid, j - 3), (float)x, (float)BYTE_OF(mid, j + 3),
                                         (float)BYTE_OF(up, j - 3), (float)BYTE_OF(up, j), (float)BYTE_OF(up, j + 3));
                        if ((q < 3 && cf) || (q >= 13 && cl)) sm = x;            // the first and the last pixel of the row
                        o[q >> 2] |= (unsigned)blend(sm, x, fac) << ((q & 3) * 8);
                    }
                }
                *reinterpret_cast<uint4*>(d + (long)y * rb + c) = make_uint4(o[0], o[1], o[2], o[3]);
#pragma unroll
                for (int i = 0; i < 6; ++i) up[i] = mid[i], mid[i] = dn[i];
            }
        }
        return;
    }

    for (int k = first; k < nch; k += stride) {
        const int c0 = k << 4;
        const uint4 v = *reinterpret_cast<const uint4*>(s + c0);
        unsigned o[4] = {v.x, v.y, v.z, v.w};
        if (op == GPCA_OP_COLOR) {
            // w: bytes c0 - 4 .. c0 + 19; L of the pixel that would start at byte j, for j = c0 - 2 .. c0 + 15; a byte takes the one
            // its channel points back to
            const unsigned w[6] = {k > 0 ? *reinterpret_cast<const unsigned*>(s + c0 - 4) : 0u, v.x, v.y, v.z, v.w, after16(s, c0, n)};
            const int ph = c0 % 3;                           // the channel of byte 0
            int L[18];
#pragma unroll
            for (int j = 0; j < 18; ++j) L[j] = luma(BYTE_OF(w, j + 2), BYTE_OF(w, j + 3), BYTE_OF(w, j + 4));
            o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                int c = ph + q % 3;
                c = c >= 3 ? c - 3 : c;
                const int dd = c == 0 ? L[q + 2] : c == 1 ? L[q + 1] : L[q];
                o[q >> 2] |= (unsigned)blend(dd, BYTE_OF(w, q + 4), fac) << ((q & 3) * 8);
            }
        } else if (op != GPCA_OP_NONE) {                     // Brightness (m = 0) and Contrast
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
            o[0] = o[1] = o[2] = o[3] = 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) o[q >> 2] |= (unsigned)blend(m, BYTE_OF(w, q), fac) << ((q & 3) * 8);
        }
        *reinterpret_cast<uint4*>(d + c0) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

int check_shape(const char* who, int F, int H, int W) {
    GP_REQUIRE(F > 0 && F <= GPCA_MAX_FRAMES && H >= 3 && W >= 3 && 3l * H * W < (1l << 30),
               "%s: bad shape (1 <= F <= %d, H, W >= 3, 3 H W < 2^30)", who, GPCA_MAX_FRAMES);
    return 0;
}

}  // namespace

extern "C" int gpca_luma_partials(const unsigned char* frames, const unsigned char* tmp0, const unsigned char* tmp1, const int* table,
                                  unsigned long long* partials, int F, int H, int W, void* stream) {
    GP_REQUIRE(frames && table && partials, "gpca_luma_partials: null pointer");
    GP_REQUIRE(((uintptr_t)table & 15) == 0 && ((uintptr_t)partials & 7) == 0, "gpca_luma_partials: table must be 16-byte aligned, partials 8-byte");
    if (int rc = check_shape("gpca_luma_partials", F, H, W)) return rc;
    hipStream_t s = (hipStream_t)stream;
    gp_timing_before(s, GP_KC_SMALL, 0.0, (double)F * 3.0 * H * W);
    coloraug_luma_kernel<<<dim3(GPCA_PARTIALS, F), CT, 0, s>>>(frames, tmp0, tmp1, table, partials, H, W);
    GP_LAUNCH_CHECK("gpca_luma_partials");
}

extern "C" int gpca_apply(const unsigned char* frames, unsigned char* tmp0, unsigned char* tmp1, unsigned char* out, const int* table,
                          const unsigned long long* partials, int F, int H, int W, void* stream) {
    GP_REQUIRE(frames && out && table, "gpca_apply: null pointer");
    GP_REQUIRE(((uintptr_t)table & 15) == 0, "gpca_apply: table must be 16-byte aligned");
    if (int rc = check_shape("gpca_apply", F, H, W)) return rc;
    const long n = 3l * H * W;
    GP_REQUIRE(out + n * F <= frames || frames + n * F <= out, "gpca_apply: out overlaps frames");
    GP_REQUIRE(!tmp0 || !tmp1 || tmp0 != tmp1, "gpca_apply: tmp0 and tmp1 must be two buffers");
    hipStream_t s = (hipStream_t)stream;
    // two 16-byte vectors per thread where the frames fill the chip anyway; one otherwise
    const long nch = cdiv(n, 16);
    const int per = (long)F * nch >= 2l * 2048 * CT ? 2 : 1;
    gp_timing_before(s, GP_KC_SMALL, 0.0, (double)F * 2.0 * n);
    coloraug_apply_kernel<<<dim3(cdiv(nch, (long)CT * per), F), CT, 0, s>>>(frames, tmp0, tmp1, out, table, partials, H, W);
    GP_LAUNCH_CHECK("gpca_apply");
}
