// The training batch on the device (include/givepose_traindata.h, gpt_*): the train-time crops and defor_2D.
//
//   crop_train_kernel    a thread per destination pixel of the S x S crops (image, instance mask) and of the R x R crops (the
//                        coordinate grid, the two output masks, the NOCS and IVFC maps): crop_rois_kernel of misc.hip with the
//                        train-time maps, on the same warp_src
//   mask_deform_kernel   a workgroup per sample: mask and band bitmaps in LDS, radix select of the floor(l/2)-th (key, pixel) of
//                        the band, ties in pixel order
#include "common.hpp"
#include "../../include/givepose_traindata.h"

namespace {

// the counter hash of sizegrad.hip (givepose_sizegrad.h states it): the murmur3 finaliser over the seed and the unit's index
__device__ __forceinline__ unsigned keep_hash(unsigned lo, unsigned hi, unsigned idx) {
    unsigned x = lo ^ (idx * 0x9E3779B9u) ^ ((hi << 16) | (hi >> 16));
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// ---------------------------------------------------------------------------------- crops
__global__ __launch_bounds__(256) void crop_train_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ inst_masks,
                                                         const unsigned char* __restrict__ nocs_png, const unsigned char* __restrict__ ivfc_png,
                                                         const int* __restrict__ frame_idx, const int* __restrict__ ivfc_idx,
                                                         const int* __restrict__ inst_id, const double* __restrict__ inv_img,
                                                         const double* __restrict__ inv_out, const float* __restrict__ img_lut,
                                                         const float* __restrict__ xlut, const float* __restrict__ ylut,
                                                         const float* __restrict__ nocs_tab, const float* __restrict__ ivfc_tab,
                                                         float* __restrict__ roi_img, float* __restrict__ roi_mask,
                                                         float* __restrict__ roi_mask_output, float* __restrict__ roi_ivfc_mask_output,
                                                         float* __restrict__ roi_coord, float* __restrict__ nocs_coord,
                                                         float* __restrict__ ivfc_coord, int H, int W, int S, int R) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const long fr = (long)frame_idx[b] * H * W;
    const int id = inst_id[b];
    int X, Y;
    if (i < S * S) {
        const int y = i / S, x = i - y * S;
        const bool ok = warp_src(inv_img + b * 6, x, y, W, H, X, Y);
        const long p = fr + (ok ? (long)Y * W + X : 0);
        const unsigned char* px = frames + p * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) roi_img[((long)b * 3 + c) * S * S + i] = img_lut[c * 256 + (ok ? px[c] : 0)];
        roi_mask[(long)b * S * S + i] = (ok && (int)inst_masks[p] == id) ? 1.0f : 0.0f;
    }
    if (i < R * R) {
        const int y = i / R, x = i - y * R;
        const bool ok = warp_src(inv_out + b * 6, x, y, W, H, X, Y);
        const long q = ok ? (long)Y * W + X : 0;
        const bool m = ok && (int)inst_masks[fr + q] == id;
        const unsigned char* np = nocs_png + (fr + q) * 3;
        const unsigned char* ip = ivfc_png + ((long)ivfc_idx[b] * H * W + q) * 3;
        const bool im = ok && ip[0] != 0;
        const long RR = (long)R * R;
        roi_coord[((long)b * 2 + 0) * RR + i] = ok ? xlut[X] : 0.0f;
        roi_coord[((long)b * 2 + 1) * RR + i] = ok ? ylut[Y] : 0.0f;
        roi_mask_output[(long)b * RR + i] = m ? 1.0f : 0.0f;
        roi_ivfc_mask_output[(long)b * RR + i] = im ? 1.0f : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            nocs_coord[((long)b * 3 + c) * RR + i] = m ? nocs_tab[(b * 3 + c) * 256 + np[c]] : 0.0f;
            ivfc_coord[((long)b * 3 + c) * RR + i] = im ? ivfc_tab[(b * 3 + c) * 256 + ip[c]] : 0.0f;
        }
    }
}

// ---------------------------------------------------------------------------------- mask deformation
constexpr int DT = 1024, DW = DT / 64;             // threads and waves of a workgroup
constexpr int DG = GPT_MAX_PIXELS / 64;            // 64-pixel groups of a sample at most: one bitmap word and one scan slot each
static_assert(DG <= DT, "the tie scan holds one group per thread");

__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    return v;
}

// Pixel i of the sample belongs to group i >> 6, whose 64 pixels one wave handles in one step: `base` runs over the groups of this
// wave, the same for all its lanes, so every ballot below is taken by a whole wave.
__global__ __launch_bounds__(DT) void mask_deform_kernel(const float* __restrict__ roi_mask, const unsigned char* __restrict__ deform,
                                                         const unsigned* __restrict__ keys, unsigned seed_lo, unsigned seed_hi,
                                                         float* __restrict__ out, int S) {
    __shared__ unsigned long long mbits[DG], bbits[DG];      // the mask and the band, a bit per pixel
    __shared__ int tpre[DG];                                 // ties per group, then their exclusive prefix
    __shared__ int hist[256], wtot[DW];
    __shared__ int s_l, s_krem;
    __shared__ unsigned s_prefix;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
    const int N = S * S, NG = (N + 63) >> 6;
    const float* __restrict__ src = roi_mask + (long)b * N;
    float* __restrict__ dst = out + (long)b * N;
    if (!deform[b]) {
        for (int i = t; i < N; i += DT) dst[i] = src[i];
        return;
    }
    if (t == 0) s_l = 0;
    for (int base = wave * 64; base < NG * 64; base += DT) {
        const int i = base + lane;
        const unsigned long long w = __ballot(i < N && src[i] != 0.0f);
        if (lane == 0) mbits[base >> 6] = w;
    }
    __syncthreads();
    auto mbit = [&](int i) { return (int)((mbits[i >> 6] >> (i & 63)) & 1ull); };
    int cnt = 0;
    for (int base = wave * 64; base < NG * 64; base += DT) {
        const int i = base + lane;
        bool band = false;
        if (i < N) {
            const int y = i / S, x = i - y * S, m = mbit(i);
            band = (y > 0 && mbit(i - S) != m) || (x > 0 && mbit(i - 1) != m);      // erode != dilate: a neighbour differs from the pixel
        }
        const unsigned long long w = __ballot(band);
        if (lane == 0) bbits[base >> 6] = w, cnt += __popcll(w);
    }
    if (lane == 0 && cnt) atomicAdd(&s_l, cnt);
    __syncthreads();
    const int l = s_l, k = l >> 1;
    auto key_of = [&](int i) { return keys ? keys[(long)b * N + i] : keep_hash(seed_lo, seed_hi, (unsigned)b * (unsigned)N + (unsigned)i); };
    // radix select, most significant byte first: after pass p the first p + 1 bytes of the key of rank k (1-based, keys in ascending
    // order) are known, and krem is that rank among the band keys that share them
    unsigned prefix = 0;
    int krem = k;
    if (k > 0) {
        for (int p = 0; p < 4; ++p) {
            const int shift = 24 - 8 * p;
            if (t < 256) hist[t] = 0;
            __syncthreads();
            for (int base = wave * 64; base < NG * 64; base += DT) {
                const int i = base + lane;
                if (i < N && ((bbits[base >> 6] >> lane) & 1ull)) {
                    const unsigned key = key_of(i);
                    if (p == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
                }
            }
            __syncthreads();
            if (wave == 0) {
                int h[4], s = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) h[j] = hist[lane * 4 + j], s += h[j];
                const int incl = wave_scan_incl(s, lane);
                int before = incl - s;
                if (before < krem && krem <= incl) {          // exactly one lane: 1 <= krem <= the sum of all bins
                    int bin = 3;
                    bool found = false;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (!found) {
                            if (before + h[j] >= krem) bin = j, found = true;
                            else before += h[j];
                        }
                    s_prefix = (prefix << 8) | (unsigned)(lane * 4 + bin);
                    s_krem = krem - before;
                }
            }
            __syncthreads();
            prefix = s_prefix, krem = s_krem;
        }
    }
    // band keys below `prefix` belong to the subset, and the first krem of its ties in pixel order: count the ties per group and scan
    const unsigned kv = prefix;
    for (int base = wave * 64; base < NG * 64; base += DT) {
        const int i = base + lane;
        const bool tie = k > 0 && i < N && ((bbits[base >> 6] >> lane) & 1ull) && key_of(i) == kv;
        const unsigned long long w = __ballot(tie);
        if (lane == 0) tpre[base >> 6] = __popcll(w);
    }
    __syncthreads();
    {
        const int v = t < NG ? tpre[t] : 0;
        const int incl = wave_scan_incl(v, lane);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int off = 0;
        for (int w = 0; w < wave; ++w) off += wtot[w];
        if (t < NG) tpre[t] = off + incl - v;
    }
    __syncthreads();
    for (int base = wave * 64; base < NG * 64; base += DT) {
        const int i = base + lane;
        const bool band = i < N && ((bbits[base >> 6] >> lane) & 1ull);
        const unsigned key = (band && k > 0) ? key_of(i) : 0u;
        const bool tie = band && k > 0 && key == kv;
        const unsigned long long w = __ballot(tie);
        if (i < N) {
            float v = mbit(i) ? 1.0f : 0.0f;
            if (band) {
                const int rank = tpre[base >> 6] + __popcll(w & ((1ull << lane) - 1ull));
                const bool zero = k > 0 && (key < kv || (tie && rank < krem));
                v = zero ? 0.0f : 1.0f;
            }
            dst[i] = v;
        }
    }
}

}  // namespace

extern "C" int gpt_crop_train(const unsigned char* frames, const unsigned char* inst_masks, const unsigned char* nocs_png,
                              const unsigned char* ivfc_png, const int* frame_idx, const int* ivfc_idx, const int* inst_id,
                              const double* inv_img, const double* inv_out, const float* img_lut, const float* xlut, const float* ylut,
                              const float* nocs_tab, const float* ivfc_tab, float* roi_img, float* roi_mask, float* roi_mask_output,
                              float* roi_ivfc_mask_output, float* roi_coord_2d, float* nocs_coord, float* ivfc_coord,
                              int B, int F, int NI, int H, int W, int S, int R, void* stream) {
    GP_REQUIRE(frames && inst_masks && nocs_png && ivfc_png && frame_idx && ivfc_idx && inst_id && inv_img && inv_out && img_lut && xlut &&
               ylut && nocs_tab && ivfc_tab && roi_img && roi_mask && roi_mask_output && roi_ivfc_mask_output && roi_coord_2d &&
               nocs_coord && ivfc_coord, "gpt_crop_train: null pointer");
    GP_REQUIRE(B > 0 && B <= 65535 && F > 0 && NI > 0 && H > 0 && W > 0 && S > 0 && S <= 4096 && R > 0 && R <= S && (long)H * W < (1l << 31),
               "gpt_crop_train: bad shape");
    hipStream_t s = (hipStream_t)stream;
    gp_timing_before(s, GP_KC_SMALL, 0.0, (double)B * (S * S * 4.0 * 4 + S * S * 4.0 + R * R * (10.0 * 4 + 8.0)));
    crop_train_kernel<<<dim3(cdiv((long)S * S, 256), B), 256, 0, s>>>(frames, inst_masks, nocs_png, ivfc_png, frame_idx, ivfc_idx, inst_id,
                                                                      inv_img, inv_out, img_lut, xlut, ylut, nocs_tab, ivfc_tab, roi_img,
                                                                      roi_mask, roi_mask_output, roi_ivfc_mask_output, roi_coord_2d,
                                                                      nocs_coord, ivfc_coord, H, W, S, R);
    GP_LAUNCH_CHECK("gpt_crop_train");
}

extern "C" int gpt_mask_deform(const float* roi_mask, const unsigned char* deform, const unsigned int* keys, unsigned long long seed,
                               float* roi_mask_deform, int B, int S, void* stream) {
    GP_REQUIRE(roi_mask && deform && roi_mask_deform, "gpt_mask_deform: null pointer");
    GP_REQUIRE(roi_mask != roi_mask_deform, "gpt_mask_deform: in place");
    GP_REQUIRE(B > 0 && B <= 65535 && S > 0 && (long)S * S <= GPT_MAX_PIXELS, "gpt_mask_deform: bad shape (S * S <= %d)", GPT_MAX_PIXELS);
    hipStream_t s = (hipStream_t)stream;
    gp_timing_before(s, GP_KC_SMALL, 0.0, (double)B * S * S * (8.0 + (keys ? 6 * 4.0 : 0.0)));
    mask_deform_kernel<<<B, DT, 0, s>>>(roi_mask, deform, keys, (unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), roi_mask_deform, S);
    GP_LAUNCH_CHECK("gpt_mask_deform");
}
