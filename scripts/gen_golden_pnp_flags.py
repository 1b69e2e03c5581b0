#!/usr/bin/env python3
"""Generate tests/golden/pnp_flags_*.npz: ConvPnPNet's flat_op / mask_attention_type and every r_type, from the REFERENCE's own
classes (build container only; scripts/ref_shim.py stubs the third-party packages it imports, as for scripts/gen_golden.py).

Run:  python scripts/gen_golden_pnp_flags.py            (needs the reference checkout; never runs on the GPU box)

Fixtures (weights are the seeded synthetic tensors of givepose_amd.synth, loaded by name; nothing large is stored):
  * pnp_flags_inputs.npz         the module input x (2,5,64,64) by seed + checksum, and its NEAREST-resized binary mask (2,1,64,64)
  * pnp_flags_conv_<flat>_<mask>.npz  ConvPnPNet(5, rot_dim=6, flat_op, mask_attention_type) on that input: rot (2,6), t (2,3)
  * pnp_flags_pose_decode_<ds>.npz    get_rot_mat + pose_from_pred_centroid_z for every r_type: "<r_type>__<key>" arrays
  * pnp_flags_e2e_<tag>.npz           network.PoseNet.forward at B = 4 (the batch of posenet_e2e_B4): rot, trans, size, pred_rot, pred_t
  * pnp_flags_manifest.json           the reference's non-backbone state-dict name -> shape of each e2e configuration
"""
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import ref_shim  # noqa: E402

FLAGS = ref_shim.install()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from givepose_amd.config import PoseNetConfig, ROT_TYPES  # noqa: E402
from givepose_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)
SEED = 0
X_SEED = 78            # module input x: Philox(key=[SEED, X_SEED]).uniform(-0.8, 0.8, (2, 5, 64, 64)) float32
FLAT_OPS = ("flatten", "avg", "avg-max", "avg-max-min")
# e2e configurations: tag -> PoseNetConfig fields (the reference FLAGS of the same names)
E2E = {
    "avgmaxmin": dict(flat_op="avg-max-min"),
    "mul": dict(mask_attention_type="mul"),
    "ego_rot6d": dict(r_type="ego_rot6d"),
    "allo_quat": dict(r_type="allo_quat"),
    "euler": dict(r_type="euler"),
    "avg_mul_ego_quat": dict(flat_op="avg", mask_attention_type="mul", r_type="ego_quat"),
}


def crc(a):
    return int(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def module_input():
    r = np.random.Generator(np.random.Philox(key=[SEED, X_SEED]))
    return r.uniform(-0.8, 0.8, (2, 5, 64, 64)).astype(np.float32)


def save(name, **arrs):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    size = os.path.getsize(path)
    print(f"  wrote {name}.npz ({size / 1024:.0f} KB)")
    assert size < 200 * 1024


def load_synth_into(module, prefix, rename=None):
    sd = module.state_dict()
    new = {}
    for k, v in sd.items():
        canon = rename(k) if rename else k
        new[k] = v if canon is None else torch.from_numpy(synth.synth_tensor(prefix + canon, tuple(v.shape), SEED)).to(v.dtype)
    module.load_state_dict(new, strict=True)
    return module


def set_flags(**kw):
    base = {f: getattr(PoseNetConfig(), f) for f in ("flat_op", "mask_attention_type", "r_type")}
    base.update(kw)
    for k, v in base.items():
        setattr(FLAGS, k, v)


def gen_modules():
    from network.conv_pnp_net import ConvPnPNet
    print("ConvPnPNet flat_op x mask_attention_type")
    x = module_input()
    # binary mask with both values: an ellipse per crop on the 256 x 256 crop, resized as PoseNet does (Resize(64, NEAREST))
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float32)
    m256 = np.stack([((xx - 120) / 90) ** 2 + ((yy - 130) / 70) ** 2 < 1, ((xx - 140) / 60) ** 2 + ((yy - 110) / 100) ** 2 < 1])
    m256 = torch.from_numpy(m256.astype(np.float32))[:, None]
    mask = F.interpolate(m256, size=(64, 64), mode="nearest")
    assert 0 < float(mask.mean()) < 1
    save("pnp_flags_inputs", x_seed=X_SEED, x_crc=crc(x), mask=mask)
    xt = torch.from_numpy(x)
    for flat in FLAT_OPS:
        for mat in ("none", "mul"):
            set_flags(flat_op=flat, mask_attention_type=mat)
            m = load_synth_into(ConvPnPNet(5, featdim=128, mask_attention_type=mat, rot_dim=6, flat_op=flat).eval(), "pnp_net.")
            ours = synth.param_manifest(PoseNetConfig(flat_op=flat, mask_attention_type=mat))
            assert all(tuple(v.shape) == tuple(ours["pnp_net." + k]) for k, v in m.state_dict().items())
            rot, t, _ = m(coor_feat=xt, mask_attention=mask)
            print(f"  {flat:12s} {mat:4s} rot[0] {rot[0].numpy().round(3)} t[0] {t[0].numpy().round(3)}")
            save(f"pnp_flags_conv_{flat.replace('-', '_')}_{mat}", rot=rot, t=t)
    set_flags()


def gen_pose_decode():
    from network.PoseNet import get_rot_mat
    from network.pose_utils.pose_from_pred_centroid_z import pose_from_pred_centroid_z
    print("pose decode, every r_type")
    for ds in ("CAMERA+Real", "wild6d"):
        B = 6
        r = np.random.Generator(np.random.Philox(key=[SEED, 79]))
        batch = {k: torch.from_numpy(v) for k, v in synth.synth_batch(B, seed=5).items()}
        pt = torch.from_numpy(np.concatenate([0.2 * r.standard_normal((B, 2)), 1.0 + 0.3 * r.random((B, 1))], 1).astype(np.float32))
        out = {"pred_t": pt, **{k: batch[k] for k in ("cam_K", "bbox_center", "resize_ratio", "roi_wh")}}
        for rt, (rot_dim, _, is_allo) in ROT_TYPES.items():
            pred_rot = torch.from_numpy(r.standard_normal((B, rot_dim)).astype(np.float32))
            Rm = get_rot_mat(pred_rot, rt)
            assert is_allo == ("allo" in rt)
            rot, trans = pose_from_pred_centroid_z(Rm, pred_centroids=pt[:, :2], pred_z_vals=pt[:, 2:3], roi_cams=batch["cam_K"].clone(),
                                                   roi_centers=batch["bbox_center"], resize_ratios=batch["resize_ratio"],
                                                   roi_whs=batch["roi_wh"], eps=1e-4, is_allo="allo" in rt, z_type="REL",
                                                   is_train=False, dataset_name=ds)
            out.update({f"{rt}__pred_rot": pred_rot, f"{rt}__rot_allo": Rm, f"{rt}__rot": rot, f"{rt}__trans": trans})
        save("pnp_flags_pose_decode_" + ds.replace("+", "_"), **out)


def gen_e2e():
    from network.PoseNet import PoseNet
    print("PoseNet e2e, B = 4")

    def rename(k):
        if k.startswith("backbone."):
            t = synth.hf_to_timm(k[len("backbone."):])
            return None if t is None else "backbone." + t
        return k

    manifests = {}
    B = 4
    npb = synth.synth_batch(B, seed=100 + B)        # the batch of posenet_e2e_B4
    data = {k: torch.from_numpy(v) for k, v in npb.items()}
    for tag, kw in E2E.items():
        set_flags(**kw)
        cfg = PoseNetConfig(**kw)
        net = load_synth_into(PoseNet().eval(), "", rename=rename)
        manifest = {k: list(v.shape) for k, v in net.state_dict().items() if not k.startswith("backbone.")}
        ours = synth.param_manifest(cfg)
        assert [k for k in ours if not k.startswith("backbone.")] == list(manifest), (tag, "manifest order/name mismatch")
        assert all(tuple(manifest[k]) == tuple(ours[k]) for k in manifest), tag
        manifests[tag] = {"config": kw, "non_backbone": manifest}
        mid = {}
        net.pnp_net.register_forward_hook(lambda mod, a, o: mid.update(pred_rot=o[0], pred_t=o[1]))
        out = net(data, "cpu", do_loss=False)
        print(f"  {tag:18s} pred_rot[0] {mid['pred_rot'][0].numpy().round(3)} t[0] {out['trans'][0].numpy().round(3)}")
        save(f"pnp_flags_e2e_{tag}", batch_seed=100 + B, roi_img_crc=crc(npb["roi_img"]), rot=out["rot"], trans=out["trans"],
             size=out["size"], pred_rot=mid["pred_rot"], pred_t=mid["pred_t"])
    set_flags()
    with open(os.path.join(GOLD, "pnp_flags_manifest.json"), "w") as f:
        json.dump(manifests, f, indent=0)
    print("  wrote pnp_flags_manifest.json")


if __name__ == "__main__":
    which = sys.argv[1:] or ["modules", "decode", "e2e"]
    if "modules" in which:
        gen_modules()
    if "decode" in which:
        gen_pose_decode()
    if "e2e" in which:
        gen_e2e()
    print("done")
