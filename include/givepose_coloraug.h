/* givepose_coloraug.h -- the colour augmentation on the device, of libgivepose_hip.so (gfx950 / MI355X).
 *
 * The reference's loader augments the whole 480 x 640 RGB frame before any crop (datasets/load_data_nocs.py:231-237, 559-574): for
 * color_aug_type 'new' a random-order sequence of imgaug.pillike.EnhanceSharpness / Contrast / Brightness / Color, which wrap
 * PIL.ImageEnhance.  PIL's operations are integer and float32 arithmetic with a closed definition, restated here; the kernels give
 * Pillow's bytes (tests/golden/color_aug_pil.npz is Pillow's output; tests/color_aug_ref.py is the numpy restatement).
 *
 * The family has its own header and prefix (gpca_) next to givepose_traindata.h (gpt_), whose conventions apply: device pointers to
 * caller-owned buffers, no allocation on the device, no synchronisation, no copy to the host, a hipStream_t `stream`, 0 or a negative
 * gp_status, gp_last_error().
 *
 * The arithmetic.  A frame is (H,W,3) uint8; a stage applies one operation to it and rounds to uint8 before the next stage reads it.
 *   blend(d, x, f), per channel byte, f a float32:
 *       t = fl32(fl32(d) + fl32(f * fl32(x - d)))      x - d is an exact integer; the product and the sum are rounded separately
 *                                                      (never one fused multiply-add)
 *       0 <= f <= 1: trunc(t).  Otherwise 0 for t <= 0, 255 for t >= 255, else trunc(t).  (For 0 <= f <= 1, t lies between d and x, so
 *       the kernels clip always.)  This is libImaging/Blend.c as ImageEnhance._Enhance.enhance calls it.
 *   L(r,g,b) = (19595 r + 38470 g + 7471 b + 32768) >> 16                                   (Image.convert("L"))
 *   GPCA_OP_BRIGHTNESS   blend(0, x, f)
 *   GPCA_OP_COLOR        blend(L(pixel), x, f) on each channel
 *   GPCA_OP_CONTRAST     blend(m, x, f), m = (2 sum L + N) / (2 N) in integers over the N = H W pixels of the frame as it enters the
 *                        stage: PIL's int(mean + 0.5)
 *   GPCA_OP_SHARPNESS    blend(SMOOTH(frame), x, f)
 *   GPCA_OP_NONE         x
 *   SMOOTH is ImageFilter.SMOOTH, the 3 x 3 kernel (1,1,1,1,5,1,1,1,1) / 13.  A pixel of the first or last row or column is the input
 *   pixel.  An interior pixel is, per channel, s = 0.5 + row(y+1) + row(y) + row(y-1), each row fl32(fl32(k0 a + k1 b) + k2 c) over its
 *   three pixels from left to right with the float32 coefficients fl32(1/13) and fl32(5/13), every product and sum rounded to float32;
 *   the result is 0 for s <= 0, 255 for s >= 255, else trunc(s).  THE ROW ORDER chosen is lower row first (y+1, y, y-1).  No input
 *   tells it from (y-1, y, y+1): with n = the eight neighbours + 5 x the centre, the exact value 0.5 + n / 13 = (13 + 2 n) / 26 has an
 *   odd numerator, so it lies at least 1/26 from every integer, and the float32 rounding of ten operations on values below 256 moves s
 *   by less than 2^-12; both orders truncate to the same byte (tests/test_color_aug_cpu.py checks both against Pillow).
 *
 * A call of the augmentation is a sequence of stages; the host walks the (F,S) plan and launches, per stage that some frame uses,
 * gpca_luma_partials (only when a frame of the stage is a Contrast) and gpca_apply: at most two launches per stage, whatever F.
 *
 * The stage table, (F,4) int32 on the device, 16-byte aligned, one row per frame: { op, the bits of the float32 factor, src, dst }.
 *   op    GPCA_OP_*; GPCA_OP_SKIP: the frame is not read or written in this stage
 *   src   GPCA_BUF_FRAMES | GPCA_BUF_TMP0 | GPCA_BUF_TMP1     where the frame stands as it enters the stage
 *   dst   GPCA_BUF_TMP0 | GPCA_BUF_TMP1 | GPCA_BUF_OUT         where the stage writes it; never the buffer it reads
 * All four buffers are (F,H,W,3) uint8 and frame f lies at byte f * 3 H W of each.  `frames` is never written.  The kernels trust the
 * table: the host checks codes and factors before any launch (givepose_amd/color_aug.py).  A frame whose plan holds k operations goes
 * frames -> tmp0 -> tmp1 -> tmp0 ... -> out in k stages and is skipped in every other stage; a frame with none is copied to out by
 * a GPCA_OP_NONE row of the first stage launched.  tmp0 / tmp1 may be null when no row names them.
 *
 * gpca_luma_partials: for every frame whose op is GPCA_OP_CONTRAST, partials[f][b] = the sum of L over the b-th of GPCA_PARTIALS
 * contiguous ranges of the frame's pixels.  Integer sums, written (not accumulated) by their one owner: no atomic, no zero fill, equal
 * bits on every run.  gpca_apply adds the GPCA_PARTIALS values of a Contrast frame and applies the stage.
 *
 * Rows are 3 W bytes and frames 3 H W bytes; neither need be a multiple of 16.  A frame whose source and destination are both
 * 16-byte aligned is walked in 16-byte vectors (Sharpness: when 3 W is a multiple of 16 as well, eight rows per thread with the three
 * live rows in registers); any other frame is walked byte by byte by the same arithmetic.
 */
#ifndef GIVEPOSE_COLORAUG_H
#define GIVEPOSE_COLORAUG_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPCA_OP_SKIP (-1)
#define GPCA_OP_NONE 0
#define GPCA_OP_SHARPNESS 1
#define GPCA_OP_CONTRAST 2
#define GPCA_OP_BRIGHTNESS 3
#define GPCA_OP_COLOR 4

#define GPCA_BUF_FRAMES 0
#define GPCA_BUF_TMP0 1
#define GPCA_BUF_TMP1 2
#define GPCA_BUF_OUT 3

#define GPCA_PARTIALS 64                /* partial sums of L per frame */
#define GPCA_STAGE_LAUNCHES 2           /* gpca_luma_partials + gpca_apply at most, whatever F */
#define GPCA_MAX_FRAMES 65535

int gpca_luma_partials(const unsigned char* frames, const unsigned char* tmp0, const unsigned char* tmp1, const int* table,
                       unsigned long long* partials, int F, int H, int W, void* stream);

int gpca_apply(const unsigned char* frames, unsigned char* tmp0, unsigned char* tmp1, unsigned char* out, const int* table,
               const unsigned long long* partials, int F, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
