/* givepose_traindata.h -- the training batch on the device, of libgivepose_hip.so (gfx950 / MI355X).
 *
 * The reference builds a training sample on the host (datasets/load_data_nocs.py:180-386): float conversions of three full frames,
 * seven cv2.warpAffine(..., INTER_NEAREST) calls and defor_2D (datasets/data_augmentation.py:11-33).  Here the frames travel as uint8
 * and two launches, whatever the batch size, write every map of the `data` dict that forward(do_loss=True), PoseLoss and train_step
 * read.  gp_crop_rois (givepose_hip.h) is the inference form of the first launch; both walk warp_src of csrc/common.hpp and agree.
 *
 * The family has its own header and prefix (gpt_) next to givepose_sizegrad.h (gps_), whose conventions apply: device pointers to
 * caller-owned buffers, no allocation on the device, no synchronisation, no copy to the host, a hipStream_t `stream`, 0 or a negative
 * gp_status, gp_last_error().
 *
 * gpt_crop_train, one launch.  Sample b reads frame frame_idx[b] of frames (F,H,W,3), inst_masks (F,H,W) and nocs_png (F,H,W,3) and
 * map ivfc_idx[b] of ivfc_png (NI,H,W,3), all uint8.  inv_img / inv_out are the (B,6) double inverse maps of the S x S and R x R
 * crops.  A destination pixel takes the NEAREST source pixel of cv::warpAffine's fixed-point walk (AB_BITS = 10); `in` below says
 * that this pixel lies in the frame, and every output is 0 where it does not, except roi_img, which takes the table value of byte 0
 * (as gp_crop_rois does).
 *   roi_img (B,3,S,S)               img_lut[c][frame byte]                                   img_lut (3,256)
 *   roi_mask (B,1,S,S)              in and instance byte == inst_id[b] ? 1 : 0
 *   roi_mask_output (B,1,R,R)       the same on the R x R grid
 *   roi_coord_2d (B,2,R,R)          xlut[X], ylut[Y]                                         xlut (W,), ylut (H,)
 *   nocs_coord (B,3,R,R)            nocs_tab[b][c][nocs byte c] where roi_mask_output is 1   nocs_tab (B,3,256)
 *   ivfc_coord (B,3,R,R)            ivfc_tab[b][c][ivfc byte c] where the ivfc R byte != 0   ivfc_tab (B,3,256)
 *   roi_ivfc_mask_output (B,1,R,R)  in and ivfc R byte != 0 ? 1 : 0                          (the instance mask is not applied to ivfc)
 * The tables are the host's: every value of the reference's float arithmetic is a function of (sample, channel, byte).
 *
 * gpt_mask_deform, one launch, one workgroup per sample: defor_2D.  deform[b] == 0: roi_mask_deform[b] = roi_mask[b].  Otherwise, with
 * m = (roi_mask != 0), erode / dilate are the minimum / maximum of m over (x,y), (x,y-1), (x-1,y) -- cv2's 2 x 2 MORPH_ELLIPSE element
 * [[0,1],[1,1]] with anchor (1,1), ONE iteration (the reference passes its radius in the position of `dst`), neighbours outside the image
 * ignored -- and the band is where they differ, l pixels.  The floor(l/2) band pixels that come first in the order (key, pixel index)
 * become 0, the other band pixels 1, the rest keep m.  That is a uniform random floor(l/2)-subset for independent uniform keys, the
 * distribution of np.random.choice(l, l // 2, replace=False); numpy's stream itself cannot be reproduced.
 *   keys (B,S,S) uint32, explicit; or keys null: key of pixel i of sample b is the counter hash of givepose_sizegrad.h (the murmur3
 *   finaliser over seed_lo ^ idx * 0x9E3779B9 ^ rotl32(seed_hi, 16)) at idx = b S S + i, seed = seed_hi : seed_lo.
 * The selection is an exact rank select: a radix select over the key's four bytes on a 256-bin LDS histogram finds the key value of
 * rank floor(l/2) and how many of its ties belong to the subset; the ties are then taken in pixel order by a prefix count.  The mask
 * and band bitmaps live in LDS (S S / 8 bytes each, hence S S <= GPT_MAX_PIXELS); keys are read from global memory or re-hashed per
 * pass.  Only integer LDS atomics (the histogram and the band count: their result does not depend on the order) and no global atomic:
 * equal inputs give equal bits on every run.
 */
#ifndef GIVEPOSE_TRAINDATA_H
#define GIVEPOSE_TRAINDATA_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPT_MAX_PIXELS 65536            /* S * S of gpt_mask_deform: two bitmaps of 8 KB in LDS at S = 256 */
#define GPT_TRAIN_BATCH_LAUNCHES 2      /* gpt_crop_train + gpt_mask_deform, whatever B */

int gpt_crop_train(const unsigned char* frames, const unsigned char* inst_masks, const unsigned char* nocs_png,
                   const unsigned char* ivfc_png, const int* frame_idx, const int* ivfc_idx, const int* inst_id,
                   const double* inv_img, const double* inv_out, const float* img_lut, const float* xlut, const float* ylut,
                   const float* nocs_tab, const float* ivfc_tab, float* roi_img, float* roi_mask, float* roi_mask_output,
                   float* roi_ivfc_mask_output, float* roi_coord_2d, float* nocs_coord, float* ivfc_coord,
                   int B, int F, int NI, int H, int W, int S, int R, void* stream);

int gpt_mask_deform(const float* roi_mask, const unsigned char* deform, const unsigned int* keys, unsigned long long seed,
                    float* roi_mask_deform, int B, int S, void* stream);

#ifdef __cplusplus
}
#endif
#endif
