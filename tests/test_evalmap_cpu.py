"""CPU: the NumPy restatement of the degree-cm / 3D-IoU mAP (tests/evalmap_ref.py, the checker of the GPU tests) against fixtures
recorded from the reference's own functions (tests/golden/evalmap_*.npz, scripts/gen_golden_evalmap.py); the refusals of
givepose_amd.evalmap; paper_table against the lines recorded in the manifest.

Per-pair values: the restatement does the reference's float64 operations in batched form (np.matmul over stacks instead of one BLAS call
per box, an explicit dot instead of np.linalg.norm), so a few ulp are expected and the bounds of evalmap_ref (B_IOU one float32 ulp,
B_DEG 4.8e-6 degree, B_CM 3.6e-12 cm; derivation there) are asserted.  Measured worst case over the three fixtures (printed by
test_pair_values_against_reference; profiles/evalmap.txt): IoU 0 (bit-equal), 1.81e-11 degree, 1.14e-13 cm.  Match flags and AP arrays: exactly equal."""
import json
import os

import numpy as np
import pytest

import evalmap_ref as R

SETS = ("coarse", "precise", "nogt")


def _view(frames, cfg):
    return R.normalised_results(frames) if cfg["view"] == "norm" else frames


@pytest.mark.parametrize("name", SETS)
def test_fixture_conditions(name):
    """What the generator promises: under 2 % of the frames drawn again, every kind of frame present, scores distinct inside a class."""
    frames, z, entry, manifest = R.load_golden(name)
    assert len(frames) == entry["n_frames"] and len(entry["redrawn"]) < 0.02 * entry["n_frames"]
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", f"evalmap_{name}.npz")) < 1_000_000
    n_p, n_g = z["frame_npred"], z["frame_ngt"]
    assert ((n_p == 0) & (n_g == 0)).any() and ((n_p == 0) & (n_g > 0)).any() and ((n_p > 0) & (n_g == 0)).any() or name != "coarse"
    for c in range(1, 7):
        s = z["pred_scores"][z["pred_class_ids"] == c]
        assert len(np.unique(s)) == len(s)
    if name == "coarse":
        assert set(z["gt_class_ids"]) == set(range(1, 7))
        mug = z["gt_handle_visibility"][z["gt_class_ids"] == 6]
        assert (mug == 0).any() and (mug == 1).any()
        lacking = sum(bool(set(f["pred_class_ids"]) - set(f["gt_class_ids"])) for f in frames)      # predictions of a class the frame's ground truth lacks
        assert lacking > 10
    if name == "precise":
        assert 5 not in set(z["gt_class_ids"]) | set(z["pred_class_ids"])
    if name == "nogt":
        assert 3 not in set(z["gt_class_ids"]) and 3 in set(z["pred_class_ids"])


@pytest.mark.parametrize("name", SETS)
def test_pair_values_against_reference(name):
    frames, z, entry, manifest = R.load_golden(name)
    for view in sorted({c["view"] for c in entry["configs"]}):
        rs = R.normalised_results(frames) if view == "norm" else frames
        groups = R.groups_of(rs, manifest["synset_names"])
        R.all_pair_values(rs, groups)
        iou = np.concatenate([g["iou"].reshape(-1) for g in groups])
        dc = np.concatenate([g["deg_cm"].reshape(-1, 2) for g in groups])
        gi, gd = z[f"pair_iou_{view}"], z[f"pair_deg_cm_{view}"]
        assert iou.shape == gi.shape and iou.dtype == gi.dtype == np.float32 and not np.isnan(gd).any()
        e_iou, e_deg, e_cm = np.abs(iou.astype(np.float64) - gi).max(), np.abs(dc[:, 0] - gd[:, 0]).max(), np.abs(dc[:, 1] - gd[:, 1]).max()
        print(f"evalmap restatement vs reference, {name}/{view}: {len(gi)} pairs, max |d iou| {e_iou:.3e}, |d degree| {e_deg:.3e}, |d cm| {e_cm:.3e}")
        assert e_iou <= R.B_IOU and e_deg <= R.B_DEG and e_cm <= R.B_CM
        assert (gi == 0).sum() > 0.2 * len(gi) and np.array_equal(iou == 0, gi == 0)      # disjoint boxes: 0.0 bit for bit on both sides
        # thresholds have pairs on both sides
        for cfg in entry["configs"]:
            if cfg["view"] == view and len(cfg["degree"]) < 5:
                assert all(0 < (gd[:, 0] < t).mean() < 1 for t in cfg["degree"] if t < 360)
                assert all(0 < (gd[:, 1] < t).mean() < 1 for t in cfg["shift"] if t < 1e4)
                assert all(0 < (gi > t).mean() < 1 for t in cfg["iou"])


@pytest.mark.parametrize("name", SETS)
def test_restatement_equals_reference(name):
    """Match flags of the recorded frames and both AP arrays, for every recorded configuration: exactly the reference's (NaN in the same places)."""
    frames, z, entry, manifest = R.load_golden(name)
    for k, cfg in enumerate(entry["configs"]):
        rs = _view(frames, cfg)
        iou_aps, pose_aps, groups = R.compute_degree_cm_mAP(rs, manifest["synset_names"], cfg["degree"], cfg["shift"], cfg["iou"], 0.1, cfg["use_matches"], details=True)
        for g in groups:
            assert R.indecisive(g["iou"], g["deg_cm"], cfg["iou"], cfg["degree"], cfg["shift"]) is None
        gold = R.golden_match_flags(z, k, cfg, groups, manifest["match_frames"])
        assert len(gold) > 10
        for g, (ip, ig, pp, pg) in zip(groups, gold):
            assert np.array_equal(g["iou_pred"], ip) and np.array_equal(g["iou_gt"], ig), (g["frame"], g["cls"])
            assert np.array_equal(g["pose_pred"], pp) and np.array_equal(g["pose_gt"], pg), (g["frame"], g["cls"])
        assert np.array_equal(iou_aps, z[f"iou_aps_{k}"], equal_nan=True), (name, k)
        assert np.array_equal(pose_aps, z[f"pose_aps_{k}"], equal_nan=True), (name, k)
    if name == "nogt":      # a class without any ground truth but with predictions: the reference divides by zero
        assert np.isnan(z["iou_aps_0"][3]).all() and np.isnan(z["iou_aps_0"][-1]).all() and not np.isnan(z["iou_aps_0"][[1, 2, 4, 5, 6]]).any()
    if name == "precise":   # a class without ground truths and without predictions: AP 0, and it counts in the mean
        assert (z["iou_aps_0"][5] == 0).all() and (z["pose_aps_0"][5] == 0).all() and z["iou_aps_0"][-1].max() > 0


def test_sum_order_model_is_numpys():
    """csrc/evalmap.hip adds the recall steps in the order spelt out by evalmap_ref.np_sum_order; that IS np.sum's order."""
    rng = np.random.default_rng(5)
    for n in list(range(0, 40)) + [127, 128, 129, 130, 143, 144, 255, 256, 257, 1000, 2754, 5000, 8191, 8192, 8193, 8200, 16385, 20001, 30000]:
        a = rng.random(n) * 10.0 ** rng.integers(-6, 3, n)
        assert R.np_sum_order(a) == np.sum(a), n
        assert R.np_sum_order(a[::1]) == np.sum(np.tile(a[:, None], (1, 3))[:, 1]), n      # strided 1-D: the same order


def test_refusals_and_signature():
    import inspect
    import givepose_amd
    from givepose_amd import evalmap
    assert givepose_amd.compute_degree_cm_mAP is evalmap.compute_degree_cm_mAP and givepose_amd.MapAccumulator is evalmap.MapAccumulator
    sig = inspect.signature(evalmap.compute_degree_cm_mAP)
    assert list(sig.parameters)[:8] == ["final_results", "synset_names", "log_dir", "degree_thresholds", "shift_thresholds", "iou_3d_thresholds",
                                        "iou_pose_thres", "use_matches_for_pose"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["degree_thresholds"], d["shift_thresholds"], d["iou_3d_thresholds"], d["iou_pose_thres"], d["use_matches_for_pose"]) == ([360], [100], [0.1], 0.1, False)
    names = ["BG", "bottle", "bowl", "camera", "can", "laptop", "mug"]
    for flag in ("eval_recon", "plot_figure", "eval_size"):
        with pytest.raises(NotImplementedError):
            evalmap.compute_degree_cm_mAP([], names, None, **{flag: True})
    with pytest.raises(NotImplementedError):
        evalmap.MapAccumulator(["BG", "bottle", "phone"], "cuda")
    with pytest.raises(RuntimeError):      # no CPU path, no fallback
        evalmap.MapAccumulator(names, "cpu")


def test_paper_table_lines():
    from givepose_amd.evalmap import paper_table
    frames, z, entry, manifest = R.load_golden("coarse")
    seen = 0
    for k, cfg in enumerate(entry["configs"]):
        if "table" in cfg:
            got = paper_table(z[f"iou_aps_{k}"], z[f"pose_aps_{k}"], manifest["synset_names"], cfg["iou"], cfg["degree"], cfg["shift"], normalised=cfg["view"] == "norm")
            assert got == cfg["table"], (k, [x for x in zip(got, cfg["table"]) if x[0] != x[1]][:3])
            seen += 1
    assert seen == 3
    cfg = entry["configs"][0]
    one = paper_table(z["iou_aps_0"], z["pose_aps_0"], manifest["synset_names"], cfg["iou"], cfg["degree"], cfg["shift"], per_obj="mug")
    assert one[0] == "mAP:" and len(one) == 9 and one[1] == cfg["table"][cfg["table"].index("category mug") + 2]
