"""ctypes binding of libgivepose_hip.so (the C ABI declared in include/givepose_hip.h).

There is NO fallback: if the HIP library is missing or does not load, importing the product ops
raises.  Nothing here imports oracle/.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_long, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# GP_LIB_PATH: A/B runs of two builds on one box (scripts/race_probe.py); the default is the in-tree library
LIB_PATH = os.environ.get("GP_LIB_PATH") or os.path.join(_HERE, "libgivepose_hip.so")

ABI_VERSION = 328       # include/givepose_hip.h GP_ABI_VERSION: gp_gemm_desc layout (checked against gp_version() at load)
GP_F32, GP_F16, GP_F64 = 0, 1, 2
ACT_NONE, ACT_GELU, ACT_RELU, ACT_LRELU = 0, 1, 2, 3
EPI_NONE, EPI_GELU, EPI_RELU, EPI_LRELU, EPI_SCALE_RES, EPI_RES_RELU, EPI_LNFOLD_GELU = 0, 1, 2, 3, 4, 5, 6
ROT_6D, ROT_6D_Y, ROT_6D_Z, ROT_QUAT, ROT_EULER = 0, 1, 2, 3, 4   # enum gp_rot_kind
KC_GEMM, KC_DCNV3, KC_DWCONV_LN, KC_NORM, KC_ELEMENTWISE, KC_SMALL, KC_COUNT = 0, 1, 2, 3, 4, 5, 6
KC_NAMES = ["gemm", "dcnv3", "dwconv_ln", "norm", "elementwise", "small"]


class GemmDesc(Structure):
    _fields_ = [("X", c_void_p), ("W", c_void_p), ("bias", c_void_p), ("gamma", c_void_p), ("residual", c_void_p),
                ("C", c_void_p), ("workspace", c_void_p),
                ("M", c_int), ("N", c_int), ("K", c_int), ("ldx", c_int), ("ldc", c_int), ("ldres", c_int),
                ("epilogue", c_int), ("out_f32", c_int), ("splitk", c_int),
                ("B", c_int), ("H", c_int), ("Win", c_int), ("Cin", c_int), ("KH", c_int), ("KW", c_int),
                ("stride", c_int), ("pad", c_int), ("Ho", c_int), ("Wo", c_int), ("dtype", c_int),
                ("gn_partial", c_void_p), ("gn_groups", c_int), ("gn_hw", c_int), ("variant", c_int),
                ("ln_stats", c_void_p), ("ln_colsum", c_void_p), ("ln_nslab", c_int), ("ln_eps", c_float),
                ("co_scheduled", c_int), ("prefetch", c_void_p), ("prefetch_bytes", c_long),
                ("split_shift", c_int), ("x_plane_stride", c_long), ("w_plane_stride", c_long),
                ("out_planes", c_int), ("c_plane_stride", c_long),
                ("residual_f32", c_int), ("c16", c_void_p), ("ldc16", c_int), ("gn_rows", c_int), ("W_cm", c_void_p)]


# name -> argtypes; every symbol include/givepose_hip.h declares (tests/test_abi.py checks both ways)
_P = c_void_p
PROTOTYPES = {
    "gp_last_error": ([], c_char_p),
    "gp_version": ([], c_int),
    "gp_device_info": ([POINTER(c_int), c_char_p, c_int], c_int),
    "gp_dcnv3_forward": ([_P, _P, _P, _P] + [c_int] * 9 + [c_float] + [c_int] * 7 + [_P], c_int),
    "gp_dcnv3_forward_any": ([_P] * 4 + [c_int] * 13 + [c_float] + [c_int] * 3 + [_P], c_int),
    "gp_dcnv3_backward": ([_P] * 7 + [c_long, c_long] + [c_int] * 13 + [c_float] + [c_int] * 3 + [_P], c_int),
    "gp_gemm": ([POINTER(GemmDesc), _P], c_int),
    "gp_gemm_gn_rows": ([c_int] * 4, c_int),
    "gp_split_planes": ([_P, _P, c_long, c_int, c_long, c_long, c_int, _P], c_int),
    "gp_convnext_mlp_pack_w2": ([_P, _P, c_int, _P], c_int),
    "gp_convnext_mlp_pack_w2_s32": ([_P, _P, c_int, _P], c_int),
    "gp_convnext_mlp": ([_P] * 8 + [c_long, c_int, c_int, _P], c_int),
    "gp_convnext_stem": ([_P] * 6 + [c_int] * 4 + [c_float, c_int, _P], c_int),
    "gp_dwconv_ln": ([_P] * 6 + [c_int] * 5 + [c_float, c_int, c_long, c_int, _P], c_int),
    "gp_dwconv_ln_groups": ([_P] * 6 + [c_int] * 5 + [c_float, c_int, _P, c_int, _P], c_int),
    "gp_dwconv7_raw_stats": ([_P] * 5 + [c_int] * 5 + [_P], c_int),
    "gp_layernorm": ([_P] * 4 + [c_long, c_int, c_float, c_int, c_int, _P], c_int),
    "gp_groupnorm_chunks": ([c_int, c_int], c_int),
    "gp_groupnorm_stats": ([_P] * 2 + [c_int] * 5 + [_P], c_int),
    "gp_groupnorm_apply": ([_P] * 5 + [c_int] * 4 + [c_float] + [c_int] * 4 + [_P], c_int),
    "gp_groupnorm_upsample2x": ([_P] * 5 + [c_int] * 5 + [c_float] + [c_int] * 3 + [_P], c_int),
    "gp_groupnorm_apply_xyz": ([_P] * 8 + [c_int] * 4 + [c_float] + [c_int] * 3 + [_P], c_int),
    "gp_upsample_bilinear2x": ([_P, _P] + [c_int] * 5 + [_P], c_int),
    "gp_deconv_col2im": ([_P, _P] + [c_int] * 5 + [_P], c_int),
    "gp_xyz_out_layer": ([_P] * 5 + [c_int] * 4 + [_P], c_int),
    "gp_pointwise_k3": ([_P] * 4 + [c_long, c_int, c_int, _P], c_int),
    "gp_dcnv3_xyz_project": ([_P] * 6 + [c_long] + [c_int] * 14 + [_P], c_int),
    "gp_pnp_conv1": ([_P] * 4 + [c_int] * 4 + [_P], c_int),
    "gp_xyz_conv3x3_s2": ([_P] * 3 + [c_int] * 4 + [_P], c_int),
    "gp_size_head": ([_P] * 8 + [c_int] * 5 + [_P], c_int),
    "gp_pose_tail": ([_P, _P, c_int] + [_P] * 10 + [c_int, c_int] + [_P] * 5 + [c_int, _P], c_int),
    "gp_pose_tail_rt": ([_P, _P, c_int] + [_P] * 10 + [c_int] * 5 + [_P] * 5 + [c_int, _P], c_int),
    "gp_pnp_conv1_masked": ([_P] * 5 + [c_int] * 4 + [_P], c_int),
    "gp_pool_mmm": ([_P, _P] + [c_int] * 5 + [_P], c_int),
    "gp_patchify_xyz": ([_P, _P, c_int, c_int, c_int, c_int, _P], c_int),
    "gp_attention64": ([_P, _P, c_int, c_int, c_int, _P], c_int),
    "gp_attention64_hd": ([_P, _P] + [c_int] * 4 + [_P], c_int),
    "gp_patchify_pnp": ([_P, _P, _P] + [c_int] * 4 + [_P], c_int),
    "gp_resnet_stem": ([_P] * 4 + [c_int] * 4 + [_P], c_int),
    "gp_maxpool3x3s2": ([_P, _P] + [c_int] * 5 + [_P], c_int),
    "gp_mask_resize_nearest": ([_P, _P, c_int, c_int, c_int, _P], c_int),
    "gp_crop_rois": ([_P] * 12 + [c_int] * 7 + [_P], c_int),
    "gp_pred_rt": ([_P] * 6 + [c_int, _P], c_int),
    "gp_pack_poses": ([_P] * 4 + [c_int, _P], c_int),
    "gp_sn_stem": ([_P] * 4 + [c_int] * 3 + [_P], c_int),
    "gp_sn_pointwise": ([_P] * 6 + [c_long] + [c_int] * 4 + [_P], c_int),
    "gp_sn_depthwise": ([_P] * 4 + [c_int] * 7 + [_P], c_int),
    "gp_sn_avgpool": ([_P] * 2 + [c_int] * 3 + [_P], c_int),
    "gp_sn_se": ([_P] * 6 + [c_int] * 3 + [_P], c_int),
    "gp_sn_head": ([_P] * 12 + [c_int] * 5 + [_P], c_int),
    "gp_eval_normalise": ([_P, c_int, _P, c_long, _P], c_int),
    "gp_eval_pair_overlaps": ([_P, _P, c_int, _P, _P, c_int] + [_P] * 6 + [c_long, _P], c_int),
    "gp_eval_match": ([_P] * 5 + [c_int, c_int, _P, c_int, _P, c_int, _P, c_int, c_int, c_long, c_long] + [_P] * 6, c_int),
    "gp_eval_ap": ([_P, _P, c_long, _P, _P, _P, c_int, c_int, _P, c_long, c_int, c_int, _P, _P], c_int),
    "gp_graph_begin": ([_P], c_int),
    "gp_graph_end": ([_P, POINTER(c_void_p)], c_int),
    "gp_graph_launch": ([_P, _P], c_int),
    "gp_graph_destroy": ([_P], c_int),
    "gp_timing_begin": ([_P], c_int),
    "gp_timing_end": ([], c_int),
    "gp_timing_report": ([c_int, POINTER(c_long), POINTER(c_double), POINTER(c_double), POINTER(c_double)], c_int),
    "gp_timing_top": ([c_int, c_char_p, c_int, POINTER(c_int), POINTER(c_long), POINTER(c_double), POINTER(c_double), POINTER(c_double)], c_int),
}

# the alignment family (include/givepose_align.h, prefix gpa_; tests/test_umeyama_cpu.py checks both ways)
ALIGN_PROTOTYPES = {
    "gpa_backproject": ([_P] * 5 + [c_int] * 3 + [_P] * 5, c_int),
    "gpa_umeyama": ([_P] * 3 + [c_int] + [_P] * 8, c_int),
    "gpa_crop_depth": ([_P] * 5 + [c_int] * 5 + [_P], c_int),
}
GPA_RES, GPA_MAX_POINTS, GPA_MAX_ITER, GPA_SAMPLE = 64, 4096, 128, 5
GPA_HYP_STRIDE, GPA_FIT_STRIDE, GPA_FIT32_STRIDE, GPA_RECORD = 16, 16, 13, 5
GPA_OK, GPA_NO_POINTS, GPA_LOW_INLIERS, GPA_DEGENERATE = 0, 1, 2, 3      # enum gpa_status

# the validation-loss family (include/givepose_loss.h, prefix gpl_; tests/test_pose_loss_cpu.py checks both ways)
LOSS_PROTOTYPES = {
    "gpl_pose_decode_train": ([_P] * 6 + [c_int, c_int, c_double, c_int] + [_P] * 5, c_int),
    "gpl_pose_loss_partials": ([_P] * 16 + [c_int] * 6 + [_P] * 3, c_int),
    "gpl_pose_loss_reduce": ([_P, _P, c_int, c_int, c_int] + [c_double] * 5 + [_P] * 4, c_int),
}
GPL_RES, GPL_SYM, GPL_SPLIT, GPL_PART, GPL_RECORD, GPL_OUT, GPL_ACC = 64, 360, 4, 8, 8, 8, 10

# the loss-gradient family (include/givepose_grad.h, prefix gpg_; tests/test_pose_loss_grad_cpu.py checks both ways)
GRAD_PROTOTYPES = {
    "gpg_pose_loss_grad": ([_P] * 19 + [c_int] * 6 + [c_double] * 5 + [_P] * 7, c_int),
    "gpg_pose_decode_train_backward": ([_P] * 9 + [c_int, c_int, c_double, c_int] + [_P] * 5, c_int),
}
GPG_TERMS, GPG_SMALL, GPG_DECODE = 6, 15, 18


# the pose-head backward family (include/givepose_headgrad.h, prefix gph_; tests/test_pnp_backward_cpu.py checks both ways)
class PnpParams(Structure):      # gph_pnp_params: the 23 tensors of pnp_net, weights or their gradients
    FIELDS = (["conv_w"] * 3 + ["gn_w"] * 3 + ["gn_b"] * 3 + ["fc1_w", "fc1_b", "fc1z_w", "fc1z_b", "fc2_w", "fc2_b", "fc2z_w", "fc2z_b",
                                                             "fcr_w", "fcr_b", "fct_w", "fct_b", "fcz_w", "fcz_b"])
    _fields_ = [("conv_w", c_void_p * 3), ("gn_w", c_void_p * 3), ("gn_b", c_void_p * 3)] + [(n, c_void_p) for n in FIELDS[9:]]


class PnpSaved(Structure):       # gph_pnp_saved
    _fields_ = [("x0", c_void_p), ("conv", c_void_p * 3), ("mean", c_void_p * 3), ("rstd", c_void_p * 3), ("act", c_void_p * 3),
                ("h1", c_void_p), ("h2", c_void_p), ("h2z", c_void_p), ("pred_rot", c_void_p), ("pred_t", c_void_p)]


c_longlong = ctypes.c_longlong
HEADGRAD_PROTOTYPES = {
    "gph_linear_backward_workspace": ([c_int] * 3, c_longlong),
    "gph_linear_backward": ([_P, c_int, _P, c_int, _P, _P] + [c_int] * 5 + [_P, c_int, _P, _P, _P, c_longlong, _P], c_int),
    "gph_gn_relu_backward_workspace": ([c_int] * 2, c_longlong),
    "gph_gn_relu_backward": ([_P] * 6 + [c_int] * 3 + [_P] * 4 + [c_longlong, _P], c_int),
    "gph_conv3x3s2_backward_workspace": ([c_int] * 5, c_longlong),
    "gph_conv3x3s2_backward": ([_P] * 4 + [c_int] * 5 + [_P] * 3 + [c_longlong, _P], c_int),
    "gph_pnp_forward_workspace": ([c_int] * 2, c_longlong),
    "gph_pnp_forward_save": ([_P] * 3 + [POINTER(PnpParams), c_int, c_int, POINTER(PnpSaved), _P, c_longlong, _P], c_int),
    "gph_pnp_backward_workspace": ([c_int] * 2, c_longlong),
    "gph_pnp_backward": ([POINTER(PnpParams), POINTER(PnpSaved)] + [_P] * 3 + [c_int, c_int, POINTER(PnpParams), _P, _P, c_longlong, _P], c_int),
}
GPH_MAX_SPLIT, GPH_FEAT, GPH_GROUPS, GPH_RES = 8, 128, 32, 64


# the coordinate-head backward family (include/givepose_xyzgrad.h, prefix gpx_; tests/test_xyz_backward_cpu.py checks both ways)
class XyzParams(Structure):      # gpx_xyz_params: the 23 tensors of a TopDownXyzHead, weights or their gradients
    _fields_ = [("deconv_w", c_void_p), ("conv_w", c_void_p * 6), ("gn_w", c_void_p * 7), ("gn_b", c_void_p * 7), ("out_w", c_void_p),
                ("out_b", c_void_p)]


class XyzSaved(Structure):       # gpx_xyz_saved
    _fields_ = [("pre", c_void_p * 7), ("mean", c_void_p * 7), ("rstd", c_void_p * 7), ("act", c_void_p * 7), ("up", c_void_p * 2),
                ("coor", c_void_p)]


XYZGRAD_PROTOTYPES = {
    "gpx_conv3x3s1_workspace": ([c_int] * 4, c_longlong),
    "gpx_conv3x3s1_forward": ([_P, _P] + [c_int] * 4 + [_P, _P, c_longlong, _P], c_int),
    "gpx_conv3x3s1_backward": ([_P] * 3 + [c_int] * 4 + [_P] * 3 + [c_longlong, _P], c_int),
    "gpx_deconv3x3s2_workspace": ([c_int] * 4, c_longlong),
    "gpx_deconv3x3s2_forward": ([_P, _P] + [c_int] * 4 + [_P, _P, c_longlong, _P], c_int),
    "gpx_deconv3x3s2_backward": ([_P] * 3 + [c_int] * 4 + [_P] * 3 + [c_longlong, _P], c_int),
    "gpx_gn_gelu_backward_workspace": ([c_int] * 2, c_longlong),
    "gpx_gn_gelu_backward": ([_P] * 6 + [c_int] * 4 + [_P] * 4 + [c_longlong, _P], c_int),
    "gpx_upsample_bilinear2x_forward": ([_P] + [c_int] * 3 + [_P, _P], c_int),
    "gpx_upsample_bilinear2x_backward": ([_P] + [c_int] * 3 + [_P, _P], c_int),
    "gpx_conv1x1_backward_workspace": ([c_int] * 4, c_longlong),
    "gpx_conv1x1_backward": ([_P] * 3 + [c_int] * 4 + [_P] * 4 + [c_longlong, _P], c_int),
    "gpx_xyz_forward_workspace": ([c_int] * 3, c_longlong),
    "gpx_xyz_forward_save": ([_P, POINTER(XyzParams)] + [c_int] * 3 + [POINTER(XyzSaved), _P, c_longlong, _P], c_int),
    "gpx_xyz_backward_workspace": ([c_int] * 3, c_longlong),
    "gpx_xyz_backward": ([POINTER(XyzParams), POINTER(XyzSaved), _P, _P] + [c_int] * 3 + [POINTER(XyzParams), _P, _P, c_longlong, _P], c_int),
}
GPX_FEAT, GPX_GROUPS, GPX_LAYERS = 256, 32, 7

# its mixed-precision forms (include/givepose_xyzgrad_bf16.h, prefix gpxm_; tests/test_xyz_bf16_cpu.py checks both ways): a trailing
# `precision` on the conv, transposed-conv and head entry points and their size queries
GPX_PREC_F32, GPX_PREC_BF16 = 0, 1
XYZGRAD_BF16_PROTOTYPES = {
    "gpxm_" + name[len("gpx_"):]: (XYZGRAD_PROTOTYPES[name][0] + [c_int], XYZGRAD_PROTOTYPES[name][1])
    for name in ("gpx_conv3x3s1_workspace", "gpx_conv3x3s1_forward", "gpx_conv3x3s1_backward", "gpx_deconv3x3s2_workspace",
                 "gpx_deconv3x3s2_forward", "gpx_deconv3x3s2_backward", "gpx_xyz_forward_workspace", "gpx_xyz_forward_save",
                 "gpx_xyz_backward_workspace", "gpx_xyz_backward")
}


# the map-encoder backward family (include/givepose_encgrad.h, prefix gpe_; tests/test_enc_backward_cpu.py checks both ways)
class EncLayerParams(Structure):      # gpe_layer_params: the 16 tensors of one encoder layer, weights or their gradients
    FIELDS = ("conv_w", "conv_b", "dw_w", "dw_b", "ln_w", "ln_b", "off_w", "off_b", "mask_w", "mask_b", "in_w", "in_b", "out_w", "out_b",
              "gn_w", "gn_b")
    _fields_ = [(n, c_void_p) for n in FIELDS]


class EncParams(Structure):           # gpe_enc_params
    _fields_ = [("layer", EncLayerParams * 3)]


class EncLayerSaved(Structure):       # gpe_layer_saved
    FIELDS = ("x", "xp", "dwout", "ln_mean", "ln_rstd", "x1", "offset", "mask", "y", "pre", "gn_mean", "gn_rstd", "act")
    _fields_ = [(n, c_void_p) for n in FIELDS]


class EncSaved(Structure):            # gpe_enc_saved
    _fields_ = [("layer", EncLayerSaved * 3)]


ENCGRAD_PROTOTYPES = {
    "gpe_linear_workspace": ([c_int] * 3, c_longlong),
    "gpe_linear_forward": ([_P] * 3 + [c_int] * 3 + [_P, _P, c_longlong, _P], c_int),
    "gpe_linear_backward": ([_P] * 3 + [c_int] * 3 + [_P] * 4 + [c_longlong, _P], c_int),
    "gpe_dwln_forward_save": ([_P] * 5 + [c_int] * 5 + [_P] * 5, c_int),
    "gpe_dwln_backward_workspace": ([c_int] * 5, c_longlong),
    "gpe_dwln_backward": ([_P] * 8 + [c_int] * 5 + [_P] * 6 + [c_longlong, _P], c_int),
    "gpe_dcnv3_core_forward": ([_P] * 3 + [c_int] * 3 + [_P] * 3, c_int),
    "gpe_dcnv3_core_backward": ([_P] * 4 + [c_int] * 3 + [_P] * 4, c_int),
    "gpe_gn_relu_forward": ([_P] * 3 + [c_int] * 4 + [_P] * 4, c_int),
    "gpe_gn_relu_backward_workspace": ([c_int] * 2, c_longlong),
    "gpe_gn_relu_backward": ([_P] * 6 + [c_int] * 4 + [_P] * 4 + [c_longlong, _P], c_int),
    "gpe_conv1x1_backward_workspace": ([c_int] * 4, c_longlong),
    "gpe_conv1x1_backward": ([_P] * 3 + [c_int] * 4 + [_P] * 4 + [c_longlong, _P], c_int),
    "gpe_map_encoder_forward_workspace": ([c_int] * 2, c_longlong),
    "gpe_map_encoder_forward_save": ([_P, POINTER(EncParams), c_int, c_int, POINTER(EncSaved), _P, c_longlong, _P], c_int),
    "gpe_map_encoder_backward_workspace": ([c_int] * 2, c_longlong),
    "gpe_map_encoder_backward": ([POINTER(EncParams), POINTER(EncSaved), _P, _P, c_int, c_int, POINTER(EncParams), _P, _P, c_longlong, _P], c_int),
}
GPE_FEAT, GPE_DCN_GROUPS, GPE_DCN_CHANNELS, GPE_TAPS, GPE_GN_GROUPS, GPE_LAYERS = 256, 4, 64, 9, 32, 3

# its forms with a selectable d xp scatter (include/givepose_encgrad_ordered.h, prefix gpeo_; tests/test_enc_ordered_cpu.py checks both
# ways): a trailing `scatter`, and for the core a workspace
GPE_SCATTER_ATOMIC, GPE_SCATTER_ORDERED = 0, 1
ENCGRAD_ORDERED_PROTOTYPES = {
    "gpeo_dcnv3_core_backward_workspace": ([c_int] * 4, c_longlong),
    "gpeo_dcnv3_core_backward": (ENCGRAD_PROTOTYPES["gpe_dcnv3_core_backward"][0] + [c_int, _P, c_longlong], c_int),
    "gpeo_map_encoder_backward_workspace": ([c_int] * 3, c_longlong),
    "gpeo_map_encoder_backward": (ENCGRAD_PROTOTYPES["gpe_map_encoder_backward"][0] + [c_int], c_int),
}


# the backbone backward family (include/givepose_bbgrad.h, prefix gpb_; tests/test_bb_backward_cpu.py checks both ways)
class BbBlockParams(Structure):       # gpb_block_params: the 9 tensors of one ConvNeXt block in state_dict order
    FIELDS = ("gamma", "dw_w", "dw_b", "ln_w", "ln_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
    _fields_ = [(n, c_void_p) for n in FIELDS]


_PP, _PI = POINTER(c_void_p), POINTER(c_int)
BBGRAD_PROTOTYPES = {
    "gpb_dw7_forward": ([_P] * 3 + [c_int] * 4 + [_P, _P], c_int),
    "gpb_dw7_backward_workspace": ([c_int] * 4, c_longlong),
    "gpb_dw7_backward": ([_P] * 3 + [c_int] * 4 + [_P] * 4 + [c_longlong, _P], c_int),
    "gpb_layernorm_forward_save": ([_P] * 3 + [c_int] * 2 + [_P] * 4, c_int),
    "gpb_layernorm_backward_workspace": ([c_int] * 2, c_longlong),
    "gpb_layernorm_backward": ([_P] * 5 + [c_int] * 2 + [_P] * 4 + [c_longlong, _P], c_int),
    "gpb_patch_conv_workspace": ([c_int] * 7, c_longlong),
    "gpb_patch_conv_forward": ([_P] * 3 + [c_int] * 7 + [_P, _P, c_longlong, _P], c_int),
    "gpb_patch_conv_backward": ([_P] * 3 + [c_int] * 7 + [_P] * 4 + [c_longlong, _P], c_int),
    "gpb_block_workspace": ([c_int] * 4, c_longlong),
    "gpb_block_forward_save": ([_P, POINTER(BbBlockParams)] + [c_int] * 4 + [_P] * 7 + [c_longlong, _P], c_int),
    "gpb_block_backward": ([_P, _P, POINTER(BbBlockParams)] + [_P] * 5 + [c_int] * 4 + [POINTER(BbBlockParams), _P, _P, c_longlong, _P], c_int),
    "gpb_param_count": ([_PI, c_int], c_int),
    "gpb_backbone_forward_workspace": ([_PI, _PI] + [c_int] * 3, c_longlong),
    "gpb_backbone_forward_save": ([_P, _PP, _PI, _PI] + [c_int] * 3 + [_PP, _P, _P, c_longlong, _P], c_int),
    "gpb_backbone_backward_workspace": ([_PI, _PI] + [c_int] * 3, c_longlong),
    "gpb_backbone_backward": ([_PP, _PP, _P, _P, _PI, _PI] + [c_int] * 3 + [_PP, _P, _P, c_longlong, _P], c_int),
}
GPB_MAX_STAGES, GPB_STEM_PATCH, GPB_DOWN_PATCH = 8, 4, 2

# its mixed-precision forms (include/givepose_bbgrad_bf16.h, prefix gpbm_; tests/test_bb_bf16_cpu.py checks both ways): a trailing
# `precision` on the block and backbone entry points and their size queries, and the bf16 contraction as a piece of its own
GPB_PREC_F32, GPB_PREC_BF16 = 0, 1
BBGRAD_BF16_PROTOTYPES = {
    "gpbm_matmul_bf16_workspace": ([c_int] * 3, c_longlong),
    "gpbm_matmul_bf16": ([_P, _P] + [c_int] * 5 + [_P, _P, c_longlong, _P], c_int),
    "gpbm_block_workspace": ([c_int] * 5, c_longlong),
    "gpbm_block_forward_save": (BBGRAD_PROTOTYPES["gpb_block_forward_save"][0] + [c_int], c_int),
    "gpbm_block_backward": (BBGRAD_PROTOTYPES["gpb_block_backward"][0] + [c_int], c_int),
    "gpbm_backbone_forward_workspace": (BBGRAD_PROTOTYPES["gpb_backbone_forward_workspace"][0] + [c_int], c_longlong),
    "gpbm_backbone_forward_save": (BBGRAD_PROTOTYPES["gpb_backbone_forward_save"][0] + [c_int], c_int),
    "gpbm_backbone_backward_workspace": (BBGRAD_PROTOTYPES["gpb_backbone_backward_workspace"][0] + [c_int], c_longlong),
    "gpbm_backbone_backward": (BBGRAD_PROTOTYPES["gpb_backbone_backward"][0] + [c_int], c_int),
}


# the optimiser family (include/givepose_optim.h, prefix gpo_; tests/test_optim_cpu.py checks both ways)
class OptTensor(Structure):           # gpo_tensor: one parameter of a step (device pointers, host table)
    _fields_ = [(n, c_void_p) for n in ("p", "g", "m", "v", "slow")] + [("n", c_longlong), ("rows", c_int), ("row_len", c_int),
                                                                         ("flags", c_int), ("step_lr", c_float)]


class OptHyper(Structure):            # gpo_hyper
    _fields_ = [(n, c_double) for n in ("beta1", "beta2", "eps", "alpha", "weight_decay", "max_norm")]


OPTIM_PROTOTYPES = {
    "gpo_ranger_step_workspace": ([POINTER(OptTensor), c_int], c_longlong),
    "gpo_ranger_step": ([POINTER(OptTensor), c_int, POINTER(OptHyper), _P, _P, c_longlong, _P], c_int),
    "gpo_clip_grad_norm_workspace": ([POINTER(OptTensor), c_int], c_longlong),
    "gpo_clip_grad_norm": ([POINTER(OptTensor), c_int, c_float, _P, _P, c_longlong, _P], c_int),
}
GPO_CHUNK, GPO_STEP_LAUNCHES, GPO_CLIP_LAUNCHES, GPO_MAX_TENSORS, GPO_FLAG_RECTIFIED, GPO_FLAG_LOOKAHEAD = 4096, 3, 3, 65536, 1, 2

# the gradient-accumulation family (include/givepose_accum.h, prefix gpc_; tests/test_grad_accum_cpu.py checks both ways)
ACCUM_PROTOTYPES = {
    "gpc_grad_accumulate_workspace": ([POINTER(OptTensor), c_int], c_longlong),
    "gpc_grad_accumulate": ([POINTER(OptTensor), c_int, c_float, c_float, _P, _P, c_longlong, _P], c_int),
}
GPC_ACCUM_LAUNCHES, GPC_FLAG_OVERWRITE = 3, 4


# Adam / AdamW (include/givepose_adam.h, prefix gpad_; tests/test_adam_cpu.py checks both ways)
class AdamTensor(Structure):          # gpad_tensor: one parameter of a step (device pointers, host table)
    _fields_ = [(n, c_void_p) for n in ("p", "g", "m", "v", "vmax")] + [("n", c_longlong), ("step_size", c_float), ("bc2_sqrt", c_float),
                                                                         ("decay", c_float), ("pad", c_int)]


class AdamHyper(Structure):           # gpad_hyper
    _fields_ = [(n, c_double) for n in ("beta1", "beta2", "eps", "weight_decay", "max_norm")] + [("mode", c_int), ("amsgrad", c_int)]


ADAM_PROTOTYPES = {
    "gpad_adam_step_workspace": ([POINTER(AdamTensor), c_int, POINTER(AdamHyper)], c_longlong),
    "gpad_adam_step": ([POINTER(AdamTensor), c_int, POINTER(AdamHyper), _P, _P, c_longlong, _P], c_int),
}
GPAD_STEP_LAUNCHES, GPAD_MAX_TENSORS, GPAD_MODE_ADAM, GPAD_MODE_ADAMW = 3, 65536, 0, 1



# the train-mode size head (include/givepose_sizegrad.h, prefix gps_; tests/test_size_train_cpu.py checks both ways)
class SizeParams(Structure):          # gps_params: size_head's six tensors, weights or their gradients
    FIELDS = ("w1", "b1", "w2", "b2", "gamma", "beta")
    _fields_ = [(n, c_void_p) for n in FIELDS]


class SizeSaved(Structure):           # gps_saved
    FIELDS = ("pooled", "arg", "h", "mean", "mean_lo", "rstd", "rstd_lo", "d", "keep", "out", "var_unbiased")
    _fields_ = [(n, c_void_p) for n in FIELDS]


c_ulonglong = ctypes.c_ulonglong
SIZEGRAD_PROTOTYPES = {
    "gps_size_forward_save": ([_P, c_int, c_int, POINTER(SizeParams), _P, c_ulonglong, _P] + [c_int] * 4 + [POINTER(SizeSaved), _P, _P], c_int),
    "gps_size_backward_workspace": ([c_int] * 4, c_longlong),
    "gps_size_backward": ([POINTER(SizeParams), POINTER(SizeSaved), _P] + [c_int] * 4 + [POINTER(SizeParams), _P, _P, c_longlong, _P], c_int),
    "gps_bn_running_update": ([_P] * 5 + [c_int, c_double, _P], c_int),
}
GPS_CHUNK, GPS_MAX_C, GPS_FORWARD_LAUNCHES, GPS_BACKWARD_LAUNCHES, GPS_DROP_THRESHOLD = 4, 4096, 3, 3, 858993459


# the weight-repack family (include/givepose_repack.h, prefix gpr_; tests/test_repack_cpu.py checks both ways)
class RepackEntry(Structure):         # gpr_entry: one strided fp32 view -> a dense run of a packed tensor
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("src_numel", c_longlong), ("dst_numel", c_longlong), ("src_off", c_longlong),
                ("dst_off", c_longlong), ("plane_stride", c_longlong), ("strides", c_longlong * 4), ("dims", c_int * 4), ("kind", c_int),
                ("pad", c_int)]


class RepackBnFold(Structure):        # gpr_bnfold
    _fields_ = [(n, c_void_p) for n in ("w", "b", "bn_w", "bn_b", "mean", "var", "w_out", "b_out")] + [
        ("w_numel", c_longlong), ("c_numel", c_longlong), ("C", c_int), ("K", c_int), ("eps", c_float), ("pad", c_int)]


class RepackMatFold(Structure):       # gpr_matfold
    _fields_ = [(n, c_void_p) for n in ("A", "B", "add", "out32", "out64")] + [
        (n, c_longlong) for n in ("a_numel", "b_numel", "add_numel", "out32_numel", "out64_numel")] + [
        (n, c_int) for n in ("M", "N", "K", "a_rs", "b_rs", "ld32", "ld64", "b_f64", "level", "pad")]


class RepackInfo(Structure):          # gpr_info
    _fields_ = [(n, c_longlong) for n in ("bytes", "off_chunks", "off_bn", "off_mat", "off_mchunks")] + [
        (n, c_int) for n in ("n_entries", "n_chunks", "n_bn", "n_bn_blocks", "n_mat", "n_mchunks0", "n_mchunks1", "pad")]


REPACK_PROTOTYPES = {
    "gpr_tables_bytes": ([POINTER(RepackEntry), c_int, POINTER(RepackBnFold), c_int, POINTER(RepackMatFold), c_int], c_longlong),
    "gpr_tables_upload": ([POINTER(RepackEntry), c_int, POINTER(RepackBnFold), c_int, POINTER(RepackMatFold), c_int, _P, _P, c_longlong,
                           POINTER(RepackInfo), _P], c_int),
    "gpr_repack": ([_P, POINTER(RepackInfo), _P], c_int),
}
GPR_CHUNK, GPR_REPACK_LAUNCHES, GPR_REPACK_LAUNCHES_F32, GPR_MAX_ENTRIES, GPR_MAX_DIMS = 4096, 4, 3, 65536, 4
GPR_KIND_F32, GPR_KIND_F16, GPR_KIND_SPLIT = 0, 1, 2

# the training-batch family (include/givepose_traindata.h, prefix gpt_; tests/test_train_batch_cpu.py checks both ways)
TRAINDATA_PROTOTYPES = {
    "gpt_crop_train": ([_P] * 21 + [c_int] * 7 + [_P], c_int),
    "gpt_mask_deform": ([_P] * 3 + [c_ulonglong, _P, c_int, c_int, _P], c_int),
}
GPT_MAX_PIXELS, GPT_TRAIN_BATCH_LAUNCHES = 65536, 2

# the weight-pack family (include/givepose_wpack.h, prefix gpw_; tests/test_conv3_pp128_cpu.py checks both ways)
WPACK_PROTOTYPES = {
    "gpw_conv3_pack_wcm": ([_P, _P, c_int, c_int, _P], c_int),
    "gpw_gemm_desc_bytes": ([], c_int),
}

# the colour-augmentation family (include/givepose_coloraug.h, prefix gpca_; tests/test_color_aug_cpu.py checks both ways)
COLORAUG_PROTOTYPES = {
    "gpca_luma_partials": ([_P] * 5 + [c_int] * 3 + [_P], c_int),
    "gpca_apply": ([_P] * 6 + [c_int] * 3 + [_P], c_int),
}
GPCA_OP_SKIP, GPCA_OP_NONE, GPCA_OP_SHARPNESS, GPCA_OP_CONTRAST, GPCA_OP_BRIGHTNESS, GPCA_OP_COLOR = -1, 0, 1, 2, 3, 4
GPCA_BUF_FRAMES, GPCA_BUF_TMP0, GPCA_BUF_TMP1, GPCA_BUF_OUT = 0, 1, 2, 3
GPCA_PARTIALS, GPCA_STAGE_LAUNCHES, GPCA_MAX_FRAMES = 64, 2, 65535

_lib = None


class GivePoseHipError(RuntimeError):
    pass


def load():
    """Load the HIP library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GivePoseHipError(
            f"{LIB_PATH} not found: build it with `python -m givepose_amd.build` (hipcc --offload-arch=gfx950). "
            "There is no CPU or PyTorch fallback for the product path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (argtypes, restype) in (list(PROTOTYPES.items()) + list(ALIGN_PROTOTYPES.items()) + list(LOSS_PROTOTYPES.items())
                                      + list(GRAD_PROTOTYPES.items()) + list(HEADGRAD_PROTOTYPES.items())
                                      + list(XYZGRAD_PROTOTYPES.items()) + list(XYZGRAD_BF16_PROTOTYPES.items()) + list(ENCGRAD_PROTOTYPES.items())
                                      + list(ENCGRAD_ORDERED_PROTOTYPES.items())
                                      + list(BBGRAD_PROTOTYPES.items()) + list(BBGRAD_BF16_PROTOTYPES.items()) + list(OPTIM_PROTOTYPES.items())
                                      + list(SIZEGRAD_PROTOTYPES.items()) + list(ACCUM_PROTOTYPES.items())
                                      + list(REPACK_PROTOTYPES.items()) + list(TRAINDATA_PROTOTYPES.items())
                                      + list(ADAM_PROTOTYPES.items()) + list(WPACK_PROTOTYPES.items())
                                      + list(COLORAUG_PROTOTYPES.items())):
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.argtypes = argtypes
        fn.restype = restype
    if lib.gp_version() != ABI_VERSION:      # a stale build would read gp_gemm_desc with another layout
        raise GivePoseHipError(f"{LIB_PATH}: ABI version {lib.gp_version()}, this package needs {ABI_VERSION}: rebuild with "
                               "`python -m givepose_amd.build`")
    if lib.gpw_gemm_desc_bytes() != ctypes.sizeof(GemmDesc):      # gp_gemm_desc.W_cm came without a new ABI number: the size tells the layouts apart
        raise GivePoseHipError(f"{LIB_PATH}: gp_gemm_desc is {lib.gpw_gemm_desc_bytes()} bytes there, {ctypes.sizeof(GemmDesc)} here: rebuild with "
                               "`python -m givepose_amd.build`")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().gp_last_error()
        raise GivePoseHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


_capturing = 0


def capturing():
    """True between gp_graph_begin and gp_graph_end of this process (raw hipStreamBeginCapture: torch does not see it)."""
    return _capturing > 0
