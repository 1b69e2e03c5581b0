#!/usr/bin/env python3
"""Generate tests/golden/pose_loss_grad_*.npz and pose_loss_grad_manifest.json from the REFERENCE's own losses.pose_loss.PoseLoss,
rot6d_to_mat_batch and pose_from_predictions_train under torch autograd (build container only; scripts/ref_shim.py stubs the
third-party packages the reference imports, as for scripts/gen_golden_pose_loss.py).

Run:  python scripts/gen_golden_pose_loss_grad.py [loss] [decode]      (needs the reference checkout; never runs on the GPU box)

Only the reference's OUTPUTS are stored.  The inputs are the seeded arrays of tests/pose_loss_ref.py (case_inputs,
make_decode_inputs) and the seeded extras of tests/pose_loss_grad_ref.py (make_gout, make_decode_grad_inputs, sample_pixels),
recorded by CRCs.
  * pose_loss_grad_<case>.npz   for the unweighted sum ("ones") and for the non-uniform gout ("gout"), the float64 run (the
                                yardstick): "<v>__rot" / "__trans" / "__size" in full; per map "<v>__<map>_s" (B,3,256), the
                                gradient at the sampled pixels, and "<v>__<map>_sum" / "_abs" (B,3), its sum and sum of |.| per
                                (crop, channel).  The float32 run: "f32_<v>__rot" / "__trans" / "__size", and for "ones" the
                                sampled map values "f32_ones__<map>_s" (float32).
  * pose_loss_grad_decode.npz   rot6d_to_mat_batch -> pose_from_predictions_train in float64 for allo / ego x site / center:
                                "<case>__rot6d" (B,6), "<case>__pred_t" (B,3): d(sum(g_rot_ego * rot) + sum(g_trans * trans))
  * pose_loss_grad_manifest.json  per fixture the largest |reference - restatement| / max|reference| per tensor

The float64 run keeps the reference's one float32 rounding: with its float32 ground truth, get_closest_rot_batch returns
torch.tensor(..., dtype=gt_rots.dtype) (pose_loss.py:427), a float32 rotation; run on float64 tensors it would not round, so the
generator passes its result through float32 -- the constant the float32 reference (and the device's forward) differentiates around.
The generator asserts that the float32 and the float64 gradients never disagree in sign where the float64 one is non-zero.
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

import pose_loss_grad_ref as G  # noqa: E402
import pose_loss_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MANIFEST = os.path.join(GOLD, "pose_loss_grad_manifest.json")
MAPS = ("nocs_coor", "ivfc_coor")


def save(name, **arrs):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
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


def rel(got, ref):
    ref = np.asarray(ref, np.float64)
    m = float(np.abs(ref).max())
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (m if m > 0 else 1.0))


def reference_grads(PL, pred, data, cfg, gout, dtype):
    for k, v in cfg.items():
        setattr(FLAGS, k, v)
    FLAGS.out_res = 64
    cast = lambda v: torch.from_numpy(v.copy()).to(dtype) if v.dtype == np.float32 else torch.from_numpy(v.copy())
    tp = {k: cast(v).requires_grad_(True) for k, v in pred.items()}
    td = {k: cast(v) for k, v in data.items()}
    out = PL.PoseLoss()(tp, td)
    assert tuple(out) == R.KEYS
    total = sum(float(w) * out[k] for w, k in zip(gout, R.KEYS))
    total.backward()
    return {k: tp[k].grad.numpy() for k in G.GRAD_KEYS}


def gen_loss():
    from losses import pose_loss as PL
    closest = PL.get_closest_rot_batch
    PL.get_closest_rot_batch = lambda p, g, s: closest(p, g, s).float().to(g.dtype)       # the reference's float32 constant
    print("PoseLoss under autograd")
    gout, man = G.make_gout(), {}
    assert np.count_nonzero(gout == 0) == 1
    for name in R.CASES:
        cfg = R.case_cfg(name)
        pred, data = R.case_inputs(name)
        B = pred["rot"].shape[0]
        pix = G.sample_pixels(name, B)
        arrs = {"input_crc": R.crc_of({**pred, **data}), "extra_crc": R.crc_of({"gout": gout, "pix": pix})}
        man[name] = {}
        for v, w in (("ones", np.ones(6)), ("gout", gout)):
            g64 = reference_grads(PL, pred, data, cfg, w, torch.float64)
            g32 = reference_grads(PL, pred, data, cfg, w, torch.float32)
            ref = G.pose_loss_grad_ref(pred, data, gout=w, **cfg)
            for k in G.GRAD_KEYS:
                assert g64[k].dtype == np.float64 and g32[k].dtype == np.float32 and np.all(np.isfinite(g64[k]))
                nz = g64[k] != 0
                assert np.array_equal(np.sign(g32[k][nz]), np.sign(g64[k][nz])), (name, v, k, "float32 / float64 sign disagreement")
                man[name][f"{v}__{k}"] = {"f64_minus_restatement": rel(ref[k], g64[k]), "f32_minus_restatement": rel(g32[k], ref[k])}
            for k in ("rot", "trans", "size"):
                arrs[f"{v}__{k}"], arrs[f"f32_{v}__{k}"] = g64[k], g32[k]
            for k in MAPS:
                arrs[f"{v}__{k}_s"], arrs[f"{v}__{k}_sum"], arrs[f"{v}__{k}_abs"] = G.sampled(g64[k], pix)
                if v == "ones":
                    arrs[f"f32_{v}__{k}_s"] = G.sampled(g32[k], pix)[0]
        worst = {t: max(x[t] for x in man[name].values()) for t in ("f64_minus_restatement", "f32_minus_restatement")}
        print(f"  {name:9s} worst |f64 - restatement| {worst['f64_minus_restatement']:.2e}  |f32 - restatement| {worst['f32_minus_restatement']:.2e}")
        save("pose_loss_grad_" + name, **arrs)
    update_manifest("loss", man)


def gen_decode():
    from network.pose_utils.pose_from_pred_centroid_z import pose_from_predictions_train
    from network.pose_utils.rot_reps import rot6d_to_mat_batch
    print("rot6d_to_mat_batch -> pose_from_predictions_train under autograd")
    inp, extra = R.make_decode_inputs(), G.make_decode_grad_inputs()
    assert inp["pred_t"].shape[0] == 4          # B = 3 would make the reference's torch.cross without `dim` another function
    T = lambda v: torch.from_numpy(v.copy()).double()
    out, man = {"input_crc": R.crc_of(inp), "extra_crc": R.crc_of(extra)}, {}
    for name, (r_type, t_type) in R.DECODE_CASES.items():
        is_allo = "allo" in r_type
        d6, pt = T(extra["rot6d"]).requires_grad_(True), T(inp["pred_t"]).requires_grad_(True)
        cen = pt[:, :2] if t_type == "site" else pt[:, :2] * 0          # network/PoseNet.py:217
        rot, trans = pose_from_predictions_train(rot6d_to_mat_batch(d6), pred_centroids=cen, pred_z_vals=pt[:, 2:3], roi_cams=T(inp["cam_K"]),
                                                 roi_centers=T(inp["bbox_center"]), resize_ratios=T(inp["resize_ratio"]), roi_whs=T(inp["roi_wh"]),
                                                 eps=1e-4, is_allo=is_allo, z_type="REL")
        ((rot * T(extra["g_rot_ego"])).sum() + (trans * T(extra["g_trans"])).sum()).backward()
        g6, gt = d6.grad.numpy(), pt.grad.numpy()
        assert np.all(np.isfinite(g6)) and np.all(np.isfinite(gt))
        ref = G.decode_train_backward_ref(extra["g_rot_ego"], extra["g_trans"], rot6d=extra["rot6d"], t_site=t_type == "site", is_allo=is_allo,
                                          **{**inp, "rot_allo": G.rot6d_to_mat_ref(extra["rot6d"])})
        man[name] = {"rot6d": rel(ref["rot6d"], g6), "pred_t_on_axis": rel(ref["pred_t"][:1], gt[:1]), "pred_t_off_axis": rel(ref["pred_t"][1:], gt[1:]),
                     "max_abs_pred_t_on_axis": float(np.abs(gt[0]).max()), "max_abs_pred_t_off_axis": float(np.abs(gt[1:]).max())}
        print(f"  {name:12s} {man[name]}")
        out[name + "__rot6d"], out[name + "__pred_t"] = g6, gt
    save("pose_loss_grad_decode", **out)
    update_manifest("decode", man)


if __name__ == "__main__":
    which = sys.argv[1:] or ["loss", "decode"]
    if "loss" in which:
        gen_loss()
    if "decode" in which:
        gen_decode()
    print("done")
