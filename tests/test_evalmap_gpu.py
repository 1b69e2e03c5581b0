"""GPU: the degree-cm / 3D-IoU mAP kernels (csrc/evalmap.hip through givepose_amd.evalmap) against the fixtures recorded from the reference
(tests/golden/evalmap_*.npz) and, on fresh seeded sets, against the NumPy restatement tests/evalmap_ref.py.

Acceptance is equality of DECISIONS: match flags and both AP arrays exactly equal (np.array_equal, NaN in the same places).  Per-pair
values may differ in the last bits (the kernel does the same float64 operations in another order, with its own acos / cbrt / det), within
  IoU (float32)  1.19e-7 absolute  (one float32 ulp at 1: a few float64 ulp can move the rounding to the neighbouring float32)
  degree         4.83e-6 degree    (arccos argument good to 16 eps; at the endpoints that is sqrt(32 eps) rad)
  cm             3.6e-12 cm        (16 eps of the magnitude 1e3 of scale-normalised translations times 100)
(evalmap_ref.B_IOU / B_DEG / B_CM, derived there from the number formats, not from any implementation's output).  The restatement itself
measures 0 / 1.8e-11 degree / 1.1e-13 cm against the reference's recorded values, the kernels on an MI355X 0 / 1.8e-11 degree / 5.1e-13 cm
(every float32 IoU bit-equal; 4.4e-11 degree against the restatement on the fresh sets); the tests print their figures, profiles/evalmap.txt
keeps them.  The fixtures hold no pair within these bounds of a threshold or of a tie (the generator
checked that on the reference's own values); on fresh sets the same filter, judged on the restatement's values, drops such frames, at
most 2 % of them."""
import numpy as np
import pytest
import torch

import evalmap_ref as R

pytestmark = pytest.mark.gpu
NAMES = ["BG", "bottle", "bowl", "camera", "can", "laptop", "mug"]
COARSE = dict(degree=[5, 10, 360], shift=[5, 10, 1e4], iou=[0.1, 0.25, 0.5, 0.75])


def _accumulate(frames, f32=False):
    """The frames through MapAccumulator; f32: the predictions as float32 DEVICE tensors (what FramePipeline returns)."""
    from givepose_amd.evalmap import MapAccumulator
    acc = MapAccumulator(NAMES, "cuda")
    for r in frames:
        rt, size = r["pred_RTs"], r["pred_scales"]
        if f32:
            rt, size = torch.from_numpy(np.asarray(rt, np.float32)).cuda(), torch.from_numpy(np.asarray(size, np.float32)).cuda()
        acc.add_frame(rt, size, r["pred_class_ids"], r["pred_scores"], r["gt_RTs"], r["gt_scales"], r["gt_class_ids"], r["gt_handle_visibility"])
    return acc


def _check_against_groups(det, groups, what):
    """Kernel details against restatement / fixture groups (same order: frame, class): pair values within the bounds, flags equal."""
    assert len(det["group_frame"]) == len(groups)
    iou = np.concatenate([g["iou"].reshape(-1) for g in groups]) if groups else np.zeros(0, np.float32)
    dc = np.concatenate([g["deg_cm"].reshape(-1, 2) for g in groups]) if groups else np.zeros((0, 2))
    assert det["iou"].shape == iou.shape and det["iou"].dtype == np.float32
    e = (np.abs(det["iou"].astype(np.float64) - iou).max(), np.abs(det["deg_cm"][:, 0] - dc[:, 0]).max(), np.abs(det["deg_cm"][:, 1] - dc[:, 1]).max())
    print(f"evalmap kernel vs {what}: {len(iou)} pairs, max |d iou| {e[0]:.3e}, |d degree| {e[1]:.3e}, |d cm| {e[2]:.3e}")
    assert e[0] <= R.B_IOU and e[1] <= R.B_DEG and e[2] <= R.B_CM, e
    assert np.array_equal(det["iou"] == 0, iou == 0)
    for k, g in enumerate(groups):
        assert (det["group_frame"][k], det["group_class"][k]) == (g["frame"], g["cls"])
        if "iou_pred" not in g:
            continue
        ps, gs = slice(det["pred_off"][k], det["pred_off"][k + 1]), slice(det["gt_off"][k], det["gt_off"][k + 1])
        assert np.array_equal(det["iou_pred_flag"][:, ps].astype(bool), g["iou_pred"]) and np.array_equal(det["iou_gt_flag"][:, gs].astype(bool), g["iou_gt"]), k
        assert np.array_equal(det["pose_pred_flag"][:, :, ps].astype(bool), g["pose_pred"]) and np.array_equal(det["pose_gt_flag"][:, :, gs].astype(bool), g["pose_gt"]), k


@pytest.mark.parametrize("name", ["coarse", "precise", "nogt"])
def test_kernels_against_reference_fixtures(name):
    """Every recorded configuration: per-pair values within the bounds of the reference's, the recorded match flags and both AP arrays
    exactly the reference's.  The normalised configurations go through MapAccumulator.normalised() (the kernel's own cbrt(det))."""
    from givepose_amd import compute_degree_cm_mAP
    frames, z, entry, manifest = R.load_golden(name)
    assert manifest["synset_names"] == NAMES
    raw = _accumulate(frames)
    for k, cfg in enumerate(entry["configs"]):
        norm = cfg["view"] == "norm"
        acc = raw.normalised() if norm else raw
        iou_aps, pose_aps, det = acc.compute(cfg["degree"], cfg["shift"], cfg["iou"], 0.1, cfg["use_matches"], return_details=True)
        groups = R.groups_of(frames, NAMES)
        at = 0
        for g in groups:      # the recorded pair values, cut along the groups
            n = len(g["pred"]) * len(g["gt"])
            g["iou"] = z[f"pair_iou_{cfg['view']}"][at:at + n].reshape(len(g["pred"]), len(g["gt"]))
            g["deg_cm"] = z[f"pair_deg_cm_{cfg['view']}"][at:at + n].reshape(len(g["pred"]), len(g["gt"]), 2)
            at += n
        for g, (ip, ig, pp, pg) in zip(groups, R.golden_match_flags(z, k, cfg, groups, manifest["match_frames"])):
            g["iou_pred"], g["iou_gt"], g["pose_pred"], g["pose_gt"] = ip, ig, pp, pg
        _check_against_groups(det, groups, f"reference fixture {name}/{k}")
        assert np.array_equal(iou_aps, z[f"iou_aps_{k}"], equal_nan=True), (name, k)
        assert np.array_equal(pose_aps, z[f"pose_aps_{k}"], equal_nan=True), (name, k)
        assert iou_aps.dtype == pose_aps.dtype == np.float64
        # the drop-in's list-of-dicts path (for the normalised view: the host-normalised copy evaluate.py builds)
        a, b = compute_degree_cm_mAP(R.normalised_results(frames) if norm else frames, NAMES, None, cfg["degree"], cfg["shift"], cfg["iou"], 0.1, cfg["use_matches"])
        assert np.array_equal(a, iou_aps, equal_nan=True) and np.array_equal(b, pose_aps, equal_nan=True)


@pytest.mark.parametrize("seed,f32,use_matches", [(11, False, True), (12, True, True), (13, False, False)])
def test_fresh_sets_against_restatement(seed, f32, use_matches):
    """300 fresh seeded frames, coarse lists: after the decisiveness filter (restatement as judge, at most 2 % of the frames dropped)
    the kernels' flags and APs are exactly the restatement's.  f32: predictions enter as float32 device tensors through
    MapAccumulator.add_frame and must give what the list-of-dicts path gives for the same (widened) values."""
    from givepose_amd import compute_degree_cm_mAP, synth
    frames = synth.synth_eval_results(300, seed)
    if f32:
        for r in frames:
            r["pred_RTs"], r["pred_scales"] = r["pred_RTs"].astype(np.float32).astype(np.float64), r["pred_scales"].astype(np.float32).astype(np.float64)
    groups = R.groups_of(frames, NAMES)
    R.all_pair_values(frames, groups)
    bad = {g["frame"] for g in groups if R.indecisive(g["iou"], g["deg_cm"], COARSE["iou"], COARSE["degree"], COARSE["shift"])}
    assert len(bad) <= 0.02 * len(frames), bad
    frames = [r for f, r in enumerate(frames) if f not in bad]
    ref_iou, ref_pose, groups = R.compute_degree_cm_mAP(frames, NAMES, COARSE["degree"], COARSE["shift"], COARSE["iou"], 0.1, use_matches, details=True)
    iou_aps, pose_aps, det = _accumulate(frames, f32).compute(COARSE["degree"], COARSE["shift"], COARSE["iou"], 0.1, use_matches, return_details=True)
    _check_against_groups(det, groups, f"restatement, seed {seed}")
    assert np.array_equal(iou_aps, ref_iou, equal_nan=True) and np.array_equal(pose_aps, ref_pose, equal_nan=True)
    assert 0 < iou_aps[-1, 1] < 1 and 0 < pose_aps[-1, 0, 0] < 1
    a, b = compute_degree_cm_mAP(frames, NAMES, None, COARSE["degree"], COARSE["shift"], COARSE["iou"], 0.1, use_matches)
    assert np.array_equal(a, iou_aps) and np.array_equal(b, pose_aps)


def test_two_runs_give_identical_bits():
    frames, z, entry, manifest = R.load_golden("precise")
    cfg = entry["configs"][0]
    runs = [_accumulate(frames).compute(cfg["degree"], cfg["shift"], cfg["iou"], 0.1, True, return_details=True) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    for k in ("iou", "deg_cm", "iou_pred_flag", "iou_gt_flag", "pose_pred_flag", "pose_gt_flag"):
        assert runs[0][2][k].tobytes() == runs[1][2][k].tobytes(), k


def test_long_class_sums_like_numpy():
    """A class with more than 8192 matched predictions: np.sum adds the recall steps in pieces of 8192, each pairwise, and so must the kernel."""
    from givepose_amd import synth
    rng = np.random.default_rng(3)
    frames = []
    for f in range(450):      # 24 cameras per frame, far apart, each predicted a few degrees and millimetres off: ~9 000 matches in one class
        n = 24
        rt = np.tile(np.eye(4), (n, 1, 1))
        rt[:, :3, :3] *= 0.2
        rt[:, 0, 3], rt[:, 1, 3], rt[:, 2, 3] = np.arange(n) % 6, np.arange(n) // 6, 3.0
        size = np.tile(synth.MEAN_SIZES[2] / np.linalg.norm(synth.MEAN_SIZES[2]), (n, 1)).astype(np.float64)
        keep = rng.random(n) < 0.93
        prt = rt[keep].copy()
        for k in range(len(prt)):      # angles well inside the cells of the thresholds 5 and 10
            prt[k, :3, :3] = prt[k, :3, :3] @ synth._rot_axis_angle(rng.standard_normal(3), np.deg2rad(rng.choice([2.0, 3.5, 7.0, 12.0]) + rng.uniform(-0.3, 0.3)))
        prt[:, :3, 3] += rng.uniform(0.002, 0.01, (len(prt), 3))
        far = rng.random(len(prt)) < 0.1
        prt[far, 0, 3] += 0.5
        frames.append(dict(gt_class_ids=np.full(n, 3, np.int32), gt_RTs=rt, gt_scales=size, gt_handle_visibility=np.ones(n, np.int32),
                           pred_class_ids=np.full(len(prt), 3, np.int32), pred_scales=size[keep], pred_RTs=prt,
                           pred_scores=(rng.permutation(len(prt)) + rng.uniform(0.1, 0.9, len(prt)) + 32 * ((f * 7919) % 450)) / (32 * 450)))
    ref_iou, ref_pose = R.compute_degree_cm_mAP(frames, NAMES, [5, 10], [0.5, 1, 2], [0.1, 0.5], 0.1, True)
    iou_aps, pose_aps, det = _accumulate(frames).compute([5, 10], [0.5, 1, 2], [0.1, 0.5], 0.1, True, return_details=True)
    assert det["iou_pred_flag"][0].sum() > 8192 + 128 and det["pose_pred_flag"][-1, -1].sum() > 8192 + 128
    assert np.array_equal(iou_aps, ref_iou) and np.array_equal(pose_aps, ref_pose)
    assert 0.5 < iou_aps[3, 0] < 1 and len(np.unique(pose_aps[3])) > 3


def test_more_than_64_of_a_class_in_a_frame_is_refused():
    from givepose_amd import _lib
    from givepose_amd.evalmap import MapAccumulator
    n = 65
    rt = np.tile(np.eye(4), (n, 1, 1))
    acc = MapAccumulator(NAMES, "cuda")
    acc.add_frame(rt, np.ones((n, 3)), np.full(n, 1), np.linspace(0.1, 0.9, n), rt[:2], np.ones((2, 3)), np.full(2, 1), np.ones(2))
    with pytest.raises(ValueError, match="at most 64"):
        acc.compute()
    L = _lib.load()
    z = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = z.data_ptr()
    rc = L.gp_eval_match(p, p, p, p, p, 1, 65, p, 1, p, 1, p, 1, -1, 1, 1, p, p, p, p, p, 0)
    assert rc == -1 and b"at most 64" in L.gp_last_error()
    # a caller that understates its largest group: the kernel skips the group and raises the status word instead of shifting past 64 bits
    off = torch.tensor([0, 65], dtype=torch.int32, device="cuda")
    zero = torch.zeros(2, dtype=torch.int32, device="cuda")
    vals, flags, status = torch.zeros(65 * 2, dtype=torch.float64, device="cuda"), torch.zeros(4 * 65, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    thr = torch.tensor([0.5], dtype=torch.float64, device="cuda")
    rc = L.gp_eval_match(vals.data_ptr(), vals.data_ptr(), off.data_ptr(), zero.data_ptr(), zero.data_ptr(), 1, 64, thr.data_ptr(), 1, thr.data_ptr(), 1,
                         thr.data_ptr(), 1, -1, 65, 1, flags.data_ptr(), flags.data_ptr(), flags.data_ptr(), flags.data_ptr(), status.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and int(status.cpu()[0]) == 1 and int(flags.sum()) == 0


def test_pipeline_outputs_feed_the_accumulator():
    """End to end: FramePipeline.run_frames on synthetic frames (as tests/test_pipeline_gpu.py builds them); its DEVICE outputs go into
    MapAccumulator.add_frame frame by frame, without a copy of the poses to the host on that path.  Ground truths are the predictions
    perturbed; the checker is the restatement on the host copy of the same float32 poses."""
    from givepose_amd import PoseNet, PoseNetConfig, Scale_net, synth
    from givepose_amd.evalmap import MapAccumulator
    from givepose_amd.pipeline import FramePipeline
    rng = np.random.default_rng(21)
    H, W, sizes = 480, 640, (3, 1, 6, 2)
    F = len(sizes)
    frames_u8 = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    masks = [(rng.random((n, H, W)) > 0.5).astype(np.uint8) for n in sizes]
    boxes = []
    for n in sizes:
        y1, x1 = rng.integers(0, 200, n), rng.integers(0, 300, n)
        boxes.append(np.stack([y1, x1, y1 + rng.integers(60, 260, n), x1 + rng.integers(60, 320, n)], 1))
    cats = [rng.integers(0, 6, n) for n in sizes]
    shapes = [synth.MEAN_SIZES[c] for c in cats]
    full = rng.standard_normal((F, 3, 256, 256)).astype(np.float32)
    net = PoseNet(PoseNetConfig(), dtype=torch.float32, seed=0).cuda()
    pipe = FramePipeline(net, Scale_net(feat_dim=24, seed=0).cuda())
    rt, size, out, got = pipe.run_frames(frames_u8, masks, boxes, cats, synth.REAL_INTRINSICS, shapes, full)
    assert rt.is_cuda and rt.dtype == torch.float32 and rt.shape == (sum(sizes), 4, 4)
    rt_h, size_h = rt.cpu().numpy().astype(np.float64), size.cpu().numpy().astype(np.float64)      # for the checker only
    assert np.isfinite(rt_h).all() and (np.abs(np.linalg.det(rt_h[:, :3, :3])) > 1e-9).all()
    acc, results, i = MapAccumulator(NAMES, "cuda"), [], 0
    for f, n in enumerate(sizes):
        g_rt = rt_h[i:i + n].copy()
        for k in range(n):
            g_rt[k, :3, :3] = g_rt[k, :3, :3] @ synth._rot_axis_angle(rng.standard_normal(3), np.deg2rad(rng.uniform(1, 14)))
        g_rt[:, :3, 3] += rng.standard_normal((n, 3)) * 0.04 * np.abs(rt_h[i:i + n, :3, 3]).max()
        r = dict(gt_class_ids=(cats[f] + 1).astype(np.int32), gt_RTs=g_rt, gt_scales=size_h[i:i + n] * rng.uniform(0.9, 1.1, (n, 3)),
                 gt_handle_visibility=rng.integers(0, 2, n).astype(np.int32), pred_class_ids=(cats[f] + 1).astype(np.int32),
                 pred_scores=rng.permutation(n) / n + 0.01 * f, pred_RTs=rt_h[i:i + n], pred_scales=size_h[i:i + n])
        results.append(r)
        acc.add_frame(rt[i:i + n], size[i:i + n], r["pred_class_ids"], r["pred_scores"], r["gt_RTs"], r["gt_scales"], r["gt_class_ids"], r["gt_handle_visibility"])
        i += n
    ref_iou, ref_pose, groups = R.compute_degree_cm_mAP(results, NAMES, COARSE["degree"], COARSE["shift"], COARSE["iou"], 0.1, True, details=True)
    assert all(R.indecisive(g["iou"], g["deg_cm"], COARSE["iou"], COARSE["degree"], COARSE["shift"]) is None for g in groups)
    iou_aps, pose_aps, det = acc.compute(COARSE["degree"], COARSE["shift"], COARSE["iou"], 0.1, True, return_details=True)
    _check_against_groups(det, groups, "restatement, pipeline outputs")
    assert np.array_equal(iou_aps, ref_iou, equal_nan=True) and np.array_equal(pose_aps, ref_pose, equal_nan=True)
