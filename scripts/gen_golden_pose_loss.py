#!/usr/bin/env python3
"""Generate tests/golden/pose_loss_*.npz and pose_loss_manifest.json from the REFERENCE's own losses.pose_loss.PoseLoss,
pose_from_predictions_train and network.PoseNet.forward(do_loss=True) (build container only; scripts/ref_shim.py stubs the
third-party packages the reference imports, as for scripts/gen_golden_pnp_flags.py).

Run:  python scripts/gen_golden_pose_loss.py [loss] [decode] [e2e]      (needs the reference checkout; never runs on the GPU box)

Only the reference's OUTPUTS are stored.  The inputs are the seeded arrays of tests/pose_loss_ref.py (make_inputs,
make_decode_inputs) and givepose_amd.synth, recorded by a CRC:
  * pose_loss_<case>.npz     PoseLoss()(pred, data) under the case's flags: `terms` (6) float32 in the reference's key order, and
                             per crop the candidate the reference's get_closest_rot took (`index`, -1 = the unrotated ground truth),
                             its `closest` rotation and the `gap` between the best and the second-best candidate re [deg]
  * pose_loss_decode.npz     pose_from_predictions_train for allo / ego x site / center: "<case>__rot", "<case>__trans"
  * pose_loss_e2e.npz        PoseNet.forward(data, 'cpu', do_loss=True) at B = 4 with the seed-0 synthetic weights, the batch of
                             posenet_e2e_B4 and a seeded roi_mask_deform: rot, trans, size, mask
  * pose_loss_manifest.json  per fixture the largest relative |reference - restatement| over the six terms (decode: absolute)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_shim  # noqa: E402

FLAGS = ref_shim.install()
import torch  # noqa: E402

import pose_loss_ref as R  # noqa: E402
from givepose_amd import synth  # noqa: E402
from givepose_amd.config import ROT_TYPES, PoseNetConfig  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MANIFEST = os.path.join(GOLD, "pose_loss_manifest.json")
torch.set_grad_enabled(False)
MIN_GAP = 1e-9             # degrees between the best and the second-best candidate of every searched fixture crop
E2E_SEED, E2E_MASK_SEED = 104, 0xDEF0


def save(name, **arrs):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    size = os.path.getsize(path)
    print(f"  wrote {name}.npz ({size / 1024:.1f} KB)")
    assert size < 200 * 1024


def update_manifest(section, value):
    m = {}
    if os.path.exists(MANIFEST):
        with open(MANIFEST) as f:
            m = json.load(f)
    m[section] = value
    with open(MANIFEST, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)


def set_flags(cfg):
    for k, v in cfg.items():
        setattr(FLAGS, k, v)
    FLAGS.out_res = 64


def gen_loss():
    from losses import pose_loss as PL
    print("PoseLoss")
    gaps = {}
    for name in R.CASES:
        cfg = R.case_cfg(name)
        set_flags(cfg)
        pred, data = R.case_inputs(name)
        crc = R.crc_of({**pred, **data})
        tp = {k: torch.from_numpy(v.copy()) for k, v in pred.items()}
        td = {k: torch.from_numpy(v.copy()) for k, v in data.items()}
        out = PL.PoseLoss()(tp, td)
        assert tuple(out) == R.KEYS, tuple(out)
        terms = np.array([float(out[k]) for k in R.KEYS], np.float32)
        assert all(out[k].dtype == torch.float32 for k in R.KEYS)
        # the candidate the reference's own search takes, crop by crop (get_closest_rot, pose_loss.py:329-353)
        B = pred["rot"].shape[0]
        sym1 = data["sym_info"][:, 0] == 1
        branch = bool(sym1.any()) and "sym" not in cfg["r_type"]
        index, gap, closest = np.full(B, -1), np.full(B, np.inf), data["rotation"].astype(np.float64)
        if branch:
            S = PL.symmetry_rotation_matrix_y(360)
            for b in np.nonzero(sym1)[0]:
                got = PL.get_closest_rot(pred["rot"][b], data["rotation"][b], S)
                res = np.array([PL.re(pred["rot"][b], data["rotation"][b].dot(S[k])) for k in range(360)])
                u = np.unique(res)
                gap[b] = u[1] - u[0]
                assert gap[b] >= MIN_GAP, (name, b, gap[b])
                closest[b] = got
                hit = [k for k in range(360) if np.array_equal(got, data["rotation"][b].dot(S[k]))]
                index[b] = -1 if got is data["rotation"][b] or np.array_equal(got, data["rotation"][b]) else hit[0]
        ref = R.pose_loss_ref(pred, data, **cfg)
        rel = float(np.max(np.abs(ref["terms"] - terms) / np.maximum(np.abs(terms), 1e-30) * (terms != 0)))
        assert np.array_equal(ref["index"], index), (name, ref["index"], index)
        gaps[name] = {"max_rel_reference_minus_restatement": rel, "min_candidate_gap_deg": float(gap.min()) if np.isfinite(gap.min()) else None}
        print(f"  {name:9s} terms {terms.round(5)} index {index} |ref - restatement| rel {rel:.2e} min gap {gap.min():.2e}")
        save("pose_loss_" + name, input_crc=crc, terms=terms, index=index, gap=gap, closest=closest.astype(np.float32), branch=branch)
    update_manifest("loss", gaps)


def gen_decode():
    from network.pose_utils.pose_from_pred_centroid_z import pose_from_predictions_train
    print("pose_from_predictions_train")
    inp = R.make_decode_inputs()
    t = {k: torch.from_numpy(v.copy()) for k, v in inp.items()}
    out, gaps = {"input_crc": R.crc_of(inp)}, {}
    for name, (r_type, t_type) in R.DECODE_CASES.items():
        is_allo = "allo" in r_type
        assert is_allo == ROT_TYPES[r_type][2]
        cen = t["pred_t"][:, :2] if t_type == "site" else t["pred_t"][:, :2] * 0          # network/PoseNet.py:217
        rot, trans = pose_from_predictions_train(t["rot_allo"], pred_centroids=cen, pred_z_vals=t["pred_t"][:, 2:3], roi_cams=t["cam_K"].clone(),
                                                 roi_centers=t["bbox_center"], resize_ratios=t["resize_ratio"], roi_whs=t["roi_wh"],
                                                 eps=1e-4, is_allo=is_allo, z_type="REL")
        er, et = R.decode_train_ref(t_site=t_type == "site", is_allo=is_allo, **inp)
        gaps[name] = {"rot_abs": float(np.abs(er - rot.numpy()).max()), "trans_abs": float(np.abs(et - trans.numpy()).max())}
        print(f"  {name:12s} {gaps[name]}")
        out[name + "__rot"], out[name + "__trans"] = rot, trans
    save("pose_loss_decode", **out)
    update_manifest("decode", gaps)


def e2e_batch():
    npb = synth.synth_batch(4, seed=E2E_SEED)
    r = np.random.Generator(np.random.Philox(key=[E2E_MASK_SEED, 4]))
    npb["roi_mask_deform"] = (r.random(npb["roi_mask"].shape) > 0.4).astype(np.float32)
    return npb


def gen_e2e():
    from network.PoseNet import PoseNet
    from gen_golden_pnp_flags import crc, load_synth_into
    print("PoseNet.forward(do_loss=True), B = 4")

    def rename(k):
        if k.startswith("backbone."):
            t = synth.hf_to_timm(k[len("backbone."):])
            return None if t is None else "backbone." + t
        return k

    base = PoseNetConfig()
    for f in ("flat_op", "mask_attention_type", "r_type"):
        setattr(FLAGS, f, getattr(base, f))
    npb = e2e_batch()
    assert not np.array_equal(npb["roi_mask"], npb["roi_mask_deform"])
    net = load_synth_into(PoseNet().eval(), "", rename=rename)
    out = net({k: torch.from_numpy(v) for k, v in npb.items()}, "cpu", do_loss=True)
    assert tuple(out) == ("rot", "trans", "size", "mask", "nocs_coor", "ivfc_coor")
    print("  rot[0]", out["rot"][0].numpy().round(3), "trans[0]", out["trans"][0].numpy().round(3))
    save("pose_loss_e2e", batch_seed=E2E_SEED, mask_seed=E2E_MASK_SEED, roi_img_crc=crc(npb["roi_img"]), mask_crc=crc(npb["roi_mask_deform"]),
         rot=out["rot"], trans=out["trans"], size=out["size"], mask=out["mask"].to(torch.uint8))
    update_manifest("e2e", {"keys": list(out)})


if __name__ == "__main__":
    which = sys.argv[1:] or ["loss", "decode", "e2e"]
    if "loss" in which:
        gen_loss()
    if "decode" in which:
        gen_decode()
    if "e2e" in which:
        gen_e2e()
    print("done")
