"""CPU restatement of the AttentionPnPNet pose head (network/attention_pnp_net.py:36-124) and of PoseNet.forward with that head in
ConvPnPNet's seat (network/PoseNet.py:173-231), composed from oracle.posenet_ref -- test infrastructure, not product code.

AttentionPnPNet.forward_feature is MAPTransformerEncoer.forward_feature at embed_dim 192 (8 heads of 24, in_chans 5), so
oracle.posenet_ref.map_transformer_ref computes it; its (B, C, 8, 8) result read back token-major is the (B, 64, 192) token tensor
whose flatten(1) feeds fc1 / fc1_z (forward_head, flat_op 'flatten').  The fc tail uses exact GELU (act_layer=nn.GELU) throughout.
tests/test_att_pnp_cpu.py pins this file against scripts/gen_golden_att_pnp.py's goldens from the reference classes.
"""
import torch
import torch.nn.functional as F

from oracle import posenet_ref as O


def att_pnp_ref(P, x, prefix="pnp_net."):
    """AttentionPnPNet(in_chans=5).forward on x (B,5,64,64) -> (rot (B,6), t (B,3), flat (B,12288))."""
    g = lambda k: P[prefix + k]
    feat = O.map_transformer_ref(P, x, prefix)                      # (B, 192, 8, 8) = tokens permuted (0, 2, 1)
    B, C = feat.shape[:2]
    flat = feat.reshape(B, C, 64).permute(0, 2, 1).reshape(B, 64 * C)
    h = F.gelu(F.linear(flat, g("fc1.weight"), g("fc1.bias")))
    h = F.gelu(F.linear(h, g("fc2.weight"), g("fc2.bias")))
    rot = F.linear(h, g("fc_r.weight"), g("fc_r.bias"))
    t = F.linear(h, g("fc_t.weight"), g("fc_t.bias"))
    hz = F.gelu(F.linear(flat, g("fc1_z.weight"), g("fc1_z.bias")))
    hz = F.gelu(F.linear(hz, g("fc2_z.weight"), g("fc2_z.bias")))
    z = F.linear(hz, g("fc_z.weight"), g("fc_z.bias"))
    return rot, torch.cat([t, z], dim=1), flat


def posenet_att_forward_ref(P, data, cfg):
    """oracle.posenet_ref.posenet_forward_ref with AttentionPnPNet as pnp_net: the same trunk, size / xyz heads, encoder and
    pose_decode_ref.  Rotation: the rot6d types of kind 0 (allo_rot6d, ego_rot6d, ...); is_allo = 'allo' in r_type (PoseNet.py:224).
    Returns the reference's dict plus pred_rot / pred_t."""
    from givepose_amd.config import ROT_TYPES
    rot_dim, kind, is_allo = ROT_TYPES[cfg.r_type]
    if kind != 0:
        raise NotImplementedError(f"att_pnp_ref: r_type {cfg.r_type} (kind {kind}) is not restated here")
    dt = next(iter(P.values())).dtype
    f = lambda k: data[k].to(dt)
    img = f("roi_img")
    mask_out = data["roi_mask"][..., :: cfg.img_size // cfg.out_res, :: cfg.img_size // cfg.out_res]
    feat = O.convnext_ref(P, img, cfg) if cfg.main_backbone == "convnext" else O.resnet34_ref(P, img)
    pred_size = O.size_head_ref(P, feat[0])
    nocs = O.xyz_head_ref(P, feat[0], "xyz_nocs_head.")
    nocs_feat = O.map_transformer_ref(P, nocs) if cfg.nocsmap_encoder == "att" else O.map_encoder_ref(P, nocs, cfg)
    red = F.conv2d(feat[0], P["feat_reducer.weight"], P["feat_reducer.bias"])
    ivfc = O.xyz_head_ref(P, torch.cat([red, nocs_feat], dim=1), "xyz_deform_head.")
    pred_rot, pred_t, _ = att_pnp_ref(P, torch.cat([ivfc, f("roi_coord_2d")], dim=1))
    ms = f("mean_size")
    pred_size = pred_size + ms / ms.norm(dim=1).unsqueeze(-1)
    rot_m = O.rot6d_to_mat_ref(pred_rot)
    rot, trans = O.pose_decode_ref(rot_m, pred_t, f("cam_K"), f("bbox_center"), f("resize_ratio"), f("roi_wh"), cfg.dataset, cfg.t_type)
    if not is_allo:
        rot = rot_m.detach().cpu()
    return {"rot": rot, "trans": trans, "size": pred_size, "mask": mask_out, "nocs_coor": nocs, "ivfc_coor": ivfc,
            "pred_rot": pred_rot, "pred_t": pred_t}
