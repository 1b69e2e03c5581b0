/* givepose_loss.h -- the validation-loss family of libgivepose_hip.so (gfx950 / MI355X).
 *
 * Device form of the reference's train-time pose decode (pose_from_predictions_train,
 * network/pose_utils/pose_from_pred_centroid_z.py:160-249, rotation-matrix branch) and of PoseLoss.forward
 * (losses/pose_loss.py:30-196) with its per-crop search of the closest symmetric ground truth (:329-353, :401-428, :451-466).
 * Forward values only: nothing here carries a gradient.
 *
 * The family has its own header and its own prefix (gpl_) next to givepose_hip.h and givepose_align.h; the symbols live in the
 * same library, follow the same conventions (device pointers, caller-owned buffers, no allocation, no synchronisation, no copy
 * to the host, a hipStream_t `stream`, 0 or a negative gp_status, gp_last_error()) and are covered by the same GP_ABI_VERSION.
 *
 * Every value is computed in float64 from the float32 inputs; every sum has a fixed order (no floating-point atomics), so equal
 * inputs give equal bits.  The maps are GPL_RES x GPL_RES and must be 16-byte aligned.
 */
#ifndef GIVEPOSE_LOSS_H
#define GIVEPOSE_LOSS_H

#include "givepose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPL_RES 64        /* side of the coordinate maps and masks */
#define GPL_SYM 360       /* y-rotations searched for a symmetric crop: symmetry_rotation_matrix_y(360) */
#define GPL_SPLIT 4       /* workgroups per crop of gpl_pose_loss_partials: each owns GPL_RES * GPL_RES / GPL_SPLIT pixels */
#define GPL_PART 8        /* doubles per (crop, workgroup) slab: point-matching sum, NOCS numerator, NOCS mask sum, IVFC numerator,
                             IVFC mask sum, 3 unused */
#define GPL_RECORD 8      /* doubles per crop: chosen candidate (-1 = the unrotated ground truth), its re [deg], re [deg] and te of
                             the crop against the unrotated ground truth, Rot1 sum, Tran sum, Size sum, 1 when the symmetric branch ran */
#define GPL_OUT 8         /* Rot1, Tran, Size, Point_matching, nocs_coor, sp2d_coor (weighted), mean re, mean te */
#define GPL_ACC 10        /* running sums: B x each of the 6 terms, sum of re, sum of te, crops, calls */

/* pose_from_predictions_train on a (B,3,3) rotation.
 *   pred_t (B,3), rot_allo (B,3,3), cam_K (B,3,3), bbox_center (B,2), resize_ratio (B), roi_wh (B,2): fp32
 *   t_site: FLAGS.t_type == 'site' (otherwise the centroid offset is multiplied by 0);  is_allo: 'allo' in the rotation type
 *   translation = (z (cx - px) / fx, z (cy - py) / fy, z), z = pred_t[2] * resize_ratio (no wild6d rescaling in the train variant);
 *   rot_ego = allo_to_ego_mat_torch(translation, rot_allo, eps), the `+ eps` of both normalisations as written.
 *   -> rot32 (B,3,3) / trans32 (B,3) fp32, rounded once from rot64 / trans64 (float64, either may be null). */
int gpl_pose_decode_train(const float* pred_t, const float* rot_allo, const float* cam_K, const float* bbox_center,
                          const float* resize_ratio, const float* roi_wh, int t_site, int is_allo, double eps, int B,
                          float* rot32, float* trans32, double* rot64, double* trans64, void* stream);

/* Per-crop partial sums of every term of PoseLoss.forward.  Grid (GPL_SPLIT, B).
 *   predictions: rot (B,3,3), trans (B,3), size (B,3), nocs_coor (B,3,R,R), ivfc_coor (B,3,R,R)
 *   ground truth: gt_rot (B,3,3), gt_trans (B,3), gt_size (B,3), nocs_scale (B), sym0 (B) int32 = sym_info[:,0],
 *                 gt_mask / gt_mask_sp (B,1,R,R) float (need not be binary), gt_nocs / gt_ivfc (B,3,R,R), model_point (B,P,3)
 *   sym_table (GPL_SYM,2) float64: cos and sin of 2 pi / 360 * k, as the host's NumPy gives them
 *   r_sym: 'sym' in r_type -- no search; the x and z columns of Rot1 and the x and z coordinates of the model points of a
 *          symmetric crop are zeroed instead (model_point itself is only read)
 *   r_angle: r_loss == 'angle' (clip at +-0.99999, SmoothL1 beta 0.2);  smoothl1: pose_loss_type == 'smoothl1' (beta 0.5)
 *   The search branch runs when some crop has sym0 == 1 and !r_sym: a symmetric crop takes the first candidate with the smallest
 *   re that is strictly below the unrotated one, gt_rot * S_k rounded once to fp32, and EVERY crop's ground-truth maps are
 *   multiplied by closest^T * gt_rot.  Each of a crop's workgroups repeats the search; there is no cross-workgroup dependency.
 *   -> slabs (B,GPL_SPLIT,GPL_PART) float64, record (B,GPL_RECORD) float64 */
int gpl_pose_loss_partials(const float* rot, const float* trans, const float* size, const float* nocs_coor, const float* ivfc_coor,
                           const float* gt_rot, const float* gt_trans, const float* gt_size, const float* nocs_scale, const int* sym0,
                           const float* gt_mask, const float* gt_mask_sp, const float* gt_nocs, const float* gt_ivfc,
                           const float* model_point, const double* sym_table, int B, int P, int R, int r_sym, int r_angle, int smoothl1,
                           double* slabs, double* record, void* stream);

/* The partial sums of B crops -> out64 (GPL_OUT) float64 and out32 (GPL_OUT) fp32 = out64 rounded once: the six terms times their
 * weights (nocs_coor and sp2d_coor both times coor_w), mean re, mean te.  One workgroup sums the crops in a fixed order.
 * acc (GPL_ACC) float64 or null: += B x each term, the re and te sums, B and 1, so that a sweep copies one vector to the host. */
int gpl_pose_loss_reduce(const double* slabs, const double* record, int B, int P, int r_angle, double rot_1_w, double tran_w,
                         double size_w, double prop_pm_w, double coor_w, double* out64, float* out32, double* acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
