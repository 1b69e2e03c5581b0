/* givepose_grad.h -- the loss-gradient family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * Backward of the validation-loss family (givepose_loss.h): the gradient of the reference's total loss
 * (losses/pose_loss.py:30-196, the line `total_loss.backward()` of engine/train.py) with respect to the five tensors PoseLoss
 * reads from the network, and the backward of the train-time pose decode (pose_from_predictions_train with
 * allo_to_ego_mat_torch, and rot6d_to_mat_batch, network/pose_utils/rot_reps.py:34-55) down to the network's raw outputs.
 * The backward pass through the network itself is not here.
 *
 * The family has its own header and prefix (gpg_) next to givepose_hip.h, givepose_align.h and givepose_loss.h; the symbols
 * live in the same library and follow the same conventions (device pointers, caller-owned buffers, no allocation, no
 * synchronisation, no copy to the host, a hipStream_t `stream`, 0 or a negative gp_status, gp_last_error()).
 *
 * Every gradient is computed in float64 from the float32 inputs and rounded once to float32; every sum has a fixed order (no
 * floating-point atomics), so equal inputs give equal bits.  The derivative conventions are torch's: d|x| = sign(x) with
 * sign(0) = 0; SmoothL1(beta)' = x / beta where |x| < beta, else sign(x); clamp passes the gradient on [min, max]; the norm of a
 * zero vector has gradient 0.
 */
#ifndef GIVEPOSE_GRAD_H
#define GIVEPOSE_GRAD_H

#include "givepose_loss.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPG_TERMS 6       /* length of gout: Rot1, Tran, Size, Point_matching, nocs_coor, sp2d_coor */
#define GPG_SMALL 15      /* doubles per crop of the float64 record of gpg_pose_loss_grad: d rot (9), d trans (3), d size (3) */
#define GPG_DECODE 18     /* doubles per crop of the float64 record of the decode backward: d rot_allo (9), d pred_t (3), d rot6d (6) */

/* d(sum_k gout[k] * term_k) / d(rot, trans, size, nocs_coor, ivfc_coor), term_k the six weighted terms of gpl_pose_loss_reduce.
 *   the first sixteen pointers, B, P, R and the three flags: as for gpl_pose_loss_partials
 *   slabs, record: what gpl_pose_loss_partials wrote for these inputs.  The chosen candidate, the branch flag and the mask sums
 *          are read from them (the mask sums of a crop's workgroups added in the order of gpl_pose_loss_reduce); the search is
 *          not repeated.  The closest ground truth and rot_sym are recomputed from the candidate index in the forward's order.
 *   gout (GPG_TERMS) float64 on the device, or null for ones
 *   the five weights: as for gpl_pose_loss_reduce
 * The closest ground-truth rotation and the rotated ground-truth maps are constants.  Point matching reaches rot only.  The
 * coordinate maps carry mask^2 (the prediction is masked before the difference, the loss matrix after it).
 * Grid (GPL_SPLIT, B): each workgroup writes its quarter of the two map gradients; workgroup 0 of a crop also sums the P points
 * (each thread its points in turn, xor tree over the wave, the four waves as (w0 + w1) + (w2 + w3)) and writes the small ones.
 *   -> g_rot (B,3,3), g_trans (B,3), g_size (B,3), g_nocs (B,3,R,R), g_ivfc (B,3,R,R) fp32 (the maps 16-byte aligned);
 *      small64 (B,GPG_SMALL) float64 or null */
int gpg_pose_loss_grad(const float* rot, const float* trans, const float* size, const float* nocs_coor, const float* ivfc_coor,
                       const float* gt_rot, const float* gt_trans, const float* gt_size, const float* nocs_scale, const int* sym0,
                       const float* gt_mask, const float* gt_mask_sp, const float* gt_nocs, const float* gt_ivfc,
                       const float* model_point, const double* sym_table, const double* slabs, const double* record,
                       const double* gout, int B, int P, int R, int r_sym, int r_angle, int smoothl1, double rot_1_w, double tran_w,
                       double size_w, double prop_pm_w, double coor_w, float* g_rot, float* g_trans, float* g_size, float* g_nocs,
                       float* g_ivfc, double* small64, void* stream);

/* Backward of gpl_pose_decode_train, and of rot6d_to_mat_batch when rot6d is given.
 *   g_rot_ego (B,3,3), g_trans (B,3) fp32: the upstream gradients of the decode's two results
 *   pred_t, rot_allo, cam_K, bbox_center, resize_ratio, roi_wh, t_site, is_allo, eps: the forward's inputs
 *   rot6d (B,6) fp32 or null: the raw vector rot_allo was decoded from (normalise, cross, normalise, cross; F.normalize's 1e-12).
 *          When it is given the chain starts from it in float64, as the reference's does, and rot_allo's values are not read.
 * The translation's gradient is g_trans plus what allo_to_ego_mat_torch passes back from g_rot_ego; t_site == 0 multiplies the
 * centroid's gradient by 0; is_allo == 0 passes g_rot_ego through.  The `+ eps` normalisations are differentiated as written.
 *   -> g_rot_allo (B,3,3), g_pred_t (B,3) fp32; g_rot6d (B,6) fp32, required when rot6d is given; g64 (B,GPG_DECODE) float64
 *      or null (its last six columns are 0 without rot6d) */
int gpg_pose_decode_train_backward(const float* g_rot_ego, const float* g_trans, const float* pred_t, const float* rot_allo,
                                   const float* cam_K, const float* bbox_center, const float* resize_ratio, const float* roi_wh,
                                   const float* rot6d, int t_site, int is_allo, double eps, int B, float* g_rot_allo,
                                   float* g_pred_t, float* g_rot6d, double* g64, void* stream);

#ifdef __cplusplus
}
#endif
#endif
