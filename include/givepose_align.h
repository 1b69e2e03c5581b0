/* givepose_align.h -- the alignment family of libgivepose_hip.so (gfx950 / MI355X): pose from the NOCS map and depth.
 *
 * Device form of the reference's `pose_from_umeyama` (tools/umeyama.py:17-60; arithmetic: tools/align_utils.py:10-104): the
 * camera-space points of a crop, back-projected from its depth, are aligned to the crop's NOCS coordinates by a similarity
 * transform -- RANSAC over 5-point Umeyama fits, then one fit on the inliers of the winner.
 *
 * The family has its own header and its own prefix (gpa_) next to givepose_hip.h; the symbols live in the same library, follow
 * the same conventions (device pointers, caller-owned buffers, no allocation, no synchronisation, no copy to the host, a
 * hipStream_t `stream`, 0 or a negative gp_status, gp_last_error()) and are covered by the same GP_ABI_VERSION.
 *
 * The maps are GPA_RES x GPA_RES; any other size is GP_ERR_INVALID.  Everything after the back-projection is float64.
 */
#ifndef GIVEPOSE_ALIGN_H
#define GIVEPOSE_ALIGN_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPA_RES 64            /* side of the maps */
#define GPA_MAX_POINTS 4096   /* GPA_RES * GPA_RES: every pixel of a crop */
#define GPA_MAX_ITER 128      /* maxIter of estimateSimilarityTransform (align_utils.py:60) */
#define GPA_SAMPLE 5          /* points per hypothesis (align_utils.py:71) */
#define GPA_HYP_STRIDE 16     /* doubles per hypothesis in the workspace: s*R (9), t (3), (Scale * InlierT)^2 or -1 (1), pad (3) */
#define GPA_FIT_STRIDE 16     /* doubles per crop in fit64: scale, R (9, row-major), t (3), singular values of the final covariance (3) */
#define GPA_FIT32_STRIDE 13   /* floats per crop in fit32: scale, R (9), t (3): fit64 rounded once */
#define GPA_RECORD 5          /* int32 per crop: n_points, n_inliers, best_iteration, iterations_run, status */
/* A sample or an inlier set whose covariance has sigma_2 <= GPA_RANK_TOL * sigma_1, or whose source variance is 0, has no
 * defined fit (the reference's answer there is LAPACK's choice of null-space vectors): such a hypothesis counts 0 inliers,
 * such a final set fails with GPA_DEGENERATE.  The one documented departure from the reference. */
#define GPA_RANK_TOL 1e-12
enum gpa_status {
    GPA_OK = 0,
    GPA_NO_POINTS = 1,     /* no masked point: the reference returns None (align_utils.py:56-57) */
    GPA_LOW_INLIERS = 2,   /* best inlier ratio < 0.1: the reference returns None (align_utils.py:90-92) */
    GPA_DEGENERATE = 3     /* the final inlier set has rank < 2 (see GPA_RANK_TOL) */
};

/* Back-projection and ordered compaction (get_PC_nocs, tools/umeyama.py:42-60, and the mask selection of :27-28).
 *   xyz (B,3,R,R) fp32 NOCS map, coor_2d (B,2,R,R) fp32 pixel x / y, cam_K (B,3,3) fp32, depth (B,R,R) fp32, mask (B,R,R) uint8
 *   x = (x_label - ux) * depth / fx (y alike), z = depth, in float32 in exactly this order: the reference's bits.
 *   The pixels with mask != 0 (and depth > 0 when valid_depth_only: backproject, align_utils.py:116-117) are kept in row-major
 *   pixel order (wave ballot + prefix counts, no atomics):
 *   -> points (B,6,GPA_MAX_POINTS) fp32: rows 0-2 the source (NOCS) x,y,z, rows 3-5 the target (camera) x,y,z of point k; 0 past the end
 *      index  (B,GPA_MAX_POINTS) int32: the pixel of point k, -1 past the end;  n_points (B) int32
 *      pc     (B,R*R,3) fp32 or null: the back-projection of EVERY pixel (the reference's PC). */
int gpa_backproject(const float* xyz, const float* coor_2d, const float* cam_K, const float* depth, const unsigned char* mask,
                    int valid_depth_only, int B, int R, float* points, int* index, int* n_points, float* pc, void* stream);

/* RANSAC Umeyama alignment of the compacted points (estimateSimilarityTransform, align_utils.py:44-104).
 *   draws (B,GPA_MAX_ITER,GPA_SAMPLE) uint32: hypothesis i of crop b fits the points draws[b,i,:] mod n_points[b].
 *   All GPA_MAX_ITER hypotheses are evaluated; one thread per crop then replays the reference's sequential rule on the counts
 *   (best changes on a strictly larger count; stop after the first i with 1 - (1 - r^5)^i > 0.99; fail below 0.1), so the
 *   result, iterations_run included, is the sequential loop's.  The final fit runs over the inliers of the winner in a fixed
 *   reduction order (no floating-point atomics): equal inputs give equal bits.
 *   workspace: hyp (B,GPA_MAX_ITER,GPA_HYP_STRIDE) float64
 *   -> counts (B,GPA_MAX_ITER) int32: inliers of every hypothesis (the reference ran the first iterations_run of them)
 *      inlier (B,GPA_MAX_POINTS) uint8: flags of the winner over the compacted points (0 when there is no winner)
 *      fit64 (B,GPA_FIT_STRIDE) float64, sRT (B,4,4) float64 = [[s R | t], [0 0 0 1]], record (B,GPA_RECORD) int32,
 *      fit32 (B,GPA_FIT32_STRIDE) fp32 (what the reference returns).  A failed crop gets scale 1, R = I, t = 0
 *      (tools/umeyama.py:30-33) and its gpa_status in the record. */
int gpa_umeyama(const float* points, const int* n_points, const unsigned int* draws, int B, double* hyp, int* counts,
                unsigned char* inlier, double* fit64, double* sRT, int* record, float* fit32, void* stream);

/* Depth crop on the grid of roi_coord_2d: per crop and output pixel the NEAREST source pixel under the inv_out map of
 * gp_crop_rois (the same fixed-point walk).
 *   depth_frames (F,H,W) fp32, frame_idx (B) int32, inv_out (B,6) float64
 *   -> roi_depth (B,1,R,R) fp32 and roi_pix_2d (B,2,R,R) fp32 = the source pixel's x and y; both 0 outside the frame
 *      (the constant border of warpAffine). */
int gpa_crop_depth(const float* depth_frames, const int* frame_idx, const double* inv_out, float* roi_depth, float* roi_pix_2d,
                   int B, int F, int H, int W, int R, void* stream);

#ifdef __cplusplus
}
#endif
#endif
