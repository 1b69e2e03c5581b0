"""givepose_amd -- MI355X-native (gfx950) inference path for GIVEPose's PoseNet.

Public surface mirrors the reference for this path:
  PoseNet            network/PoseNet.py:134-231 (forward(data, device, do_loss=False, pred_scale=None) -> dict)
  dcnv3_forward      the pybind op DCNv3.dcnv3_forward (network/ops_dcnv3/src/dcnv3.h:20-38)
  dcnv3_backward     the pybind op DCNv3.dcnv3_backward (dcnv3.h:40-59);  DCNv3Function: functions/dcnv3_func.py:25-98
  Scale_net          network/scale_net.py:22-65 (forward(data, device, mode) -> scale (B,)), run before PoseNet by evaluate.py
  PoseNetConfig      the absl FLAGS the path reads (config/config.py)
  compute_degree_cm_mAP, MapAccumulator, paper_table
                     evaluation/eval_utils_cass.py:490-820 and the tables evaluate.py:160-280 logs, on the device (evalmap.py)
  pose_from_umeyama, pose_from_umeyama_device
                     tools/umeyama.py:17-60 (RANSAC Umeyama alignment of the NOCS map to the depth), on the device (umeyama.py)
  PoseLoss, LossConfig, LossAccumulator
                     losses/pose_loss.py:13-196 (the six validation-loss terms of a batch, forward values only), on the device
                     (loss.py); PoseNet.forward(..., do_loss=True) returns the predictions it reads
  PoseLoss.value_and_grad, PoseLoss.with_grad, pose_decode_train, pose_decode_train_backward, PoseNet.head_grads
                     the gradient of the total loss at the network's raw outputs (the loss half of `total_loss.backward()`,
                     engine/train.py:115-121), on the device (loss.py)
  PoseNet.pnp_backward, PoseNet.head_grads_pnp, pnp_grad
                     the backward pass through the pose head ConvPnPNet (network/conv_pnp_net.py:18-201): from d pred_rot, d pred_t to
                     the gradient of every pnp_net.* parameter and the head's part of d ivfc_coor, in fp32 on the device
                     (pnp_grad.py, include/givepose_headgrad.h)
  PoseNet.xyz_head_backward, PoseNet.head_grads_xyz, xyz_grad
                     the backward pass through a coordinate head TopDownXyzHead (network/xyz_head.py:195-366; xyz_nocs_head or
                     xyz_deform_head): from d coor to the gradient of every parameter of the head and of its input feature, in fp32
                     on the device (xyz_grad.py, include/givepose_xyzgrad.h); head_grads_xyz carries head_grads_pnp on through
                     xyz_deform_head
  PoseNet.map_encoder_backward, PoseNet.feat_reducer_backward, PoseNet.head_grads_feat, enc_grad
                     the backward pass through the map encoder MAPEncoder with DCNv3 layers (network/conv_pnp_net.py:254-332): from
                     d nocs_feat to the gradient of its 48 parameters and of the coordinate map, per coupling batch, in fp32 on the
                     device (enc_grad.py, include/givepose_encgrad.h), and through feat_reducer; head_grads_feat carries
                     head_grads_xyz on through both and xyz_nocs_head to the gradient at the backbone's output
  PoseNet.backbone_backward, PoseNet.head_grads_backbone, bb_grad
                     the backward pass through the ConvNeXt backbone (timm convnext_base as called by network/backbone.py:36-46):
                     from d feat to the gradient of its 340 parameters and of the image crop, in fp32 on the device, without an
                     atomic (bb_grad.py, include/givepose_bbgrad.h); head_grads_backbone carries head_grads_feat on through it.
                     The backward of the resnet34 backbone and of the 'att' / plain-conv encoders is not part of this library
  PoseNet.size_head_backward, size_grad, and size_head={"seed": s} | {"keep": mask} of head_grads_feat / head_grads_backbone / train_step
                     the size head as the training loop runs it (network/pose_head.py:17-42 under network.train()): BatchNorm1d on
                     the statistics of the batch, Dropout(0.2) with an explicit or seeded mask, its backward to the six size_head.*
                     parameters and to d feat, and the update of bn1's running statistics, in fp32 on the device without an atomic
                     (size_grad.py, include/givepose_sizegrad.h)
  Ranger, clip_grad_norm_, flat_and_anneal_lr, PoseNet.train_step, PoseNet.params_updated, optim
                     what the training loop does after backward() (engine/train.py:117-129): clip_grad_norm_ with the 2-norm, one
                     step of Ranger (tools/torch_utils/solver/ranger2020.py: RAdam + Lookahead + gradient centralisation) over all
                     tensors in three launches, and the factor of the flat_and_anneal schedule
                     (tools/torch_utils/solver/lr_scheduler.py:177-263), on the device (optim.py, include/givepose_optim.h);
                     train_step runs head_grads_backbone and then the step
  Adam, AdamW, build_optimizer
                     the loop's other two FLAGS.optimizer_type choices (engine/train.py:66-72): torch.optim.Adam / AdamW after
                     clip_grad_norm_, over all tensors in three launches, bit for bit the fp32 restatement of
                     torch.optim.adam._single_tensor_adam; the interface is Ranger's (step, train_step, GradAccumulator), the
                     state dict torch's own, so last_optimizer.pth moves both ways (optim.py, include/givepose_adam.h);
                     build_optimizer(model, optimizer_type, lr) is the loop's choice between the three
  PoseNet.set_repack("host" | "device"), PoseNet.repack_count, repack
                     how the forward's packed weights follow the parameters.  "host" (the default): PoseNet._pack on the host, and
                     params_updated() drops the packed weights and every plan.  "device": the same tensors are written in place on
                     the device in at most four launches (permutations, concatenations, fp16 / split-plane roundings, the BatchNorm
                     fold in fp32, the matrix folds in float64), so params_updated() costs no host copy, no synchronise and no graph
                     recapture (repack.py, include/givepose_repack.h); for the configurations train_step accepts
  PoseNet.set_backward_precision("fp32" | "bf16"), PoseNet.backward_precision, bb_grad.matmul_bf16, precision= of bb_grad's block and backbone calls
                     the backbone's recompute and backward in mixed precision: under "bf16" the six dense contractions of every
                     ConvNeXt block multiply bf16-rounded operands on v_mfma_f32_32x32x16_bf16 and add in fp32, everything else
                     stays the fp32 code; "fp32" (the default) is bit for bit what it was (csrc/grad_gemm_bf16.hpp,
                     include/givepose_bbgrad_bf16.h)
  PoseNet.set_backward_precision(mode, xyz_heads="fp32" | "bf16"), PoseNet.xyz_backward_precision, precision= of xyz_grad's conv, transposed-conv and head calls
                     the same for the two coordinate heads: under "bf16" the 21 contractions of a head's 3x3 layers (forward, dX, dW)
                     take bf16-rounded operands in the recompute and in the backward; GroupNorm + GELU, the bilinear x2 and the 1x1
                     output conv stay fp32 (csrc/xyz_conv_prec.hpp, include/givepose_xyzgrad_bf16.h)
  GradAccumulator, train_step(accumulator=, accumulate=, micro_step=, group=)
                     FLAGS.accumulate and the gradient all-reduce across ranks (engine/train.py:117-131): the micro-steps' gradients
                     added, scaled and clipped in place in one flat device buffer in three launches, exchanged between ranks by one
                     all_reduce, and stepped from by Ranger (optim.py, include/givepose_accum.h)
  TrainBatchBuilder, fs_net_scale, sym_info
                     the training batch of datasets/load_data_nocs.py:180-386 from uint8 frames and labels: the DZI-augmented crops
                     (tools/dataset_utils.py:32-82), the NOCS / IVFC coordinate targets and their masks, and defor_2D
                     (datasets/data_augmentation.py:11-33) with explicit or seeded draws, in two launches on the device
                     (train_batch.py, include/givepose_traindata.h)
  ColorAugmenter, color_aug_draws, color_aug
                     the colour augmentation of a training frame (datasets/load_data_nocs.py:231-237, 559-574, color_aug_type 'new'):
                     PIL.ImageEnhance's Sharpness, Contrast, Brightness and Color in a drawn order, byte for byte what Pillow gives,
                     on whole uint8 frames on the device before TrainBatchBuilder crops them, with explicit or seeded plans
                     (color_aug.py, include/givepose_coloraug.h)
"""
from .config import PoseNetConfig  # noqa: F401
from .posenet import PoseNet  # noqa: F401
from . import bb_grad, color_aug, enc_grad, optim, pnp_grad, repack, size_grad, xyz_grad  # noqa: F401  (ctypes wrappers only: the library is loaded at the first call)
from .color_aug import ColorAugmenter, color_aug_draws  # noqa: F401
from .optim import Adam, AdamW, GradAccumulator, Ranger, build_optimizer, clip_grad_norm_, flat_and_anneal_lr  # noqa: F401


def dcnv3_forward(*args, **kwargs):
    from .ops import dcnv3_forward as f
    return f(*args, **kwargs)


def dcnv3_backward(*args, **kwargs):
    """The pybind op DCNv3.dcnv3_backward (network/ops_dcnv3/src/dcnv3.h:40-59)."""
    from .ops import dcnv3_backward as f
    return f(*args, **kwargs)


def __getattr__(name):
    if name == "DCNv3Function":          # functions/dcnv3_func.py:25-98
        from .dcnv3_function import DCNv3Function
        return DCNv3Function
    if name == "Scale_net":              # network/scale_net.py:22-65
        from .scale_net import Scale_net
        return Scale_net
    if name in ("compute_degree_cm_mAP", "MapAccumulator", "paper_table"):      # evaluation/eval_utils_cass.py:490
        from . import evalmap
        return getattr(evalmap, name)
    if name in ("pose_from_umeyama", "pose_from_umeyama_device"):                # tools/umeyama.py:17
        from . import umeyama
        return getattr(umeyama, name)
    if name in ("PoseLoss", "LossConfig", "LossAccumulator", "pose_decode_train", "pose_decode_train_backward"):   # losses/pose_loss.py:13
        from . import loss
        return getattr(loss, name)
    if name in ("TrainBatchBuilder", "fs_net_scale", "sym_info"):                # datasets/load_data_nocs.py:180
        from . import train_batch
        return getattr(train_batch, name)
    raise AttributeError(name)
