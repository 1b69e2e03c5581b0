"""GPU: the alignment kernels (csrc/align.hip through givepose_amd.umeyama / RoiCropper.crop_depth) against the fixtures recorded from
the reference (tests/golden/umeyama_*.npz) and, on fresh seeded crops, against the NumPy restatement tests/umeyama_ref.py.

DECISIONS are compared exactly: the back-projection bit for bit, the compaction order, the inlier count of every iteration the
reference ran, the iterations run, the best iteration, the final inlier set, the status.  The float64 VALUES (scale, R, t, sRT) are held
to the bounds derived in tests/umeyama_ref.py from the number formats (B_s, B_R, B_t there; the rotation bound is 1e-13 .. 3e-13 on the
fixtures); the float32 outputs must be the float64 ones rounded once.  The tests print their largest deviations beside the bounds
(profiles/umeyama.txt keeps them)."""
import numpy as np
import pytest
import torch

import umeyama_ref as R

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _run(inputs, draws, flag=False, **kw):
    from givepose_amd.umeyama import pose_from_umeyama_device
    dev = torch.device("cuda:0")
    args = [T(np.ascontiguousarray(inputs[k])).to(dev) for k in ("xyz_coor", "coor_2d", "camK", "Depth", "obj_mask")]
    s, rot, t, det = pose_from_umeyama_device(*args, draws=draws, valid_depth_only=flag, return_details=True, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), rot.cpu().numpy(), t.cpu().numpy(), {k: v.cpu().numpy() for k, v in det.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _got(det, b):
    n = int(det["n_points"][b])
    return {"index": det["index"][b][:n], "counts": det["counts"][b], "iterations_run": int(det["iterations_run"][b]),
            "best_iteration": int(det["best_iteration"][b]), "n_inliers": int(det["n_inliers"][b]),
            "inlier_idx": np.nonzero(det["inlier"][b][:n])[0], "status": int(det["status"][b]), "scale": float(det["scale"][b]),
            "R": det["R"][b], "t": det["t"][b], "sRT": det["sRT"][b]}


def _check_common(s, rot, t, det):
    """What holds for every crop of every call: float32 = float64 rounded once, sRT = [[s R | t], [0 0 0 1]], failures give (1, I, 0),
    nothing is NaN, the padding of the compacted arrays is in place."""
    B = len(s)
    assert s.dtype == rot.dtype == t.dtype == np.float32 and s.shape == (B,) and rot.shape == (B, 3, 3) and t.shape == (B, 3)
    assert np.array_equal(s, det["scale"].astype(np.float32)) and np.array_equal(rot, det["R"].astype(np.float32))
    assert np.array_equal(t, det["t"].astype(np.float32))
    for k in ("scale", "R", "t", "sRT", "sigma"):
        assert np.isfinite(det[k]).all(), k
    srt = np.tile(np.eye(4), (B, 1, 1))
    srt[:, :3, :3] = det["scale"][:, None, None] * det["R"]
    srt[:, :3, 3] = det["t"]
    assert np.array_equal(det["sRT"], srt)
    for b in range(B):
        n = det["n_points"][b]
        assert (det["index"][b][n:] == -1).all() and not det["points"][b][:, n:].any() and not det["inlier"][b][n:].any()
        assert det["n_inliers"][b] == det["inlier"][b].sum() or det["best_iteration"][b] < 0
        if det["status"][b] != R.OK:
            assert det["scale"][b] == 1 and np.array_equal(det["R"][b], np.eye(3)) and not det["t"][b].any()
        else:
            assert abs(np.linalg.det(det["R"][b]) - 1) < 1e-13 and np.abs(det["R"][b] @ det["R"][b].T - np.eye(3)).max() < 1e-13


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixtures_decisions_and_values(name):
    """gpa_backproject + gpa_umeyama (pose_from_umeyama_device) against what the reference did on the same inputs and draws."""
    inputs, draws, PC, flag, crops = R.load_fixture(name)
    s, rot, t, det = _run(inputs, draws, flag)
    assert det["PC"].dtype == np.float32 and np.array_equal(det["PC"].view(np.uint32), PC.view(np.uint32))      # bit for bit
    _check_common(s, rot, t, det)
    worst = {}
    for b, c in enumerate(crops):
        assert det["n_points"][b] == c["n_points"]
        got = _got(det, b)
        # the compacted points are the map's and the back-projection's values at the kept pixels, in order
        nocs = inputs["xyz_coor"][b].reshape(3, -1)[:, c["index"]]
        assert np.array_equal(det["points"][b][:3, :c["n_points"]], nocs) and np.array_equal(det["points"][b][3:, :c["n_points"]], PC[b][c["index"]].T)
        for k, v in R.check_crop_against_fixture(c, got, f"kernel vs fixture {name}[{b}]").items():
            worst[k] = max(worst.get(k, 0.0), v)
        if c["expect"] == "tiny":
            # the documented departure: every sample of a 1- or 2-point crop has rank < 2 and counts nothing
            assert got["status"] == R.LOW_INLIERS and got["iterations_run"] == R.MAX_ITER and not det["counts"][b].any()
            assert got["best_iteration"] == -1 and got["n_inliers"] == 0
    print(f"kernel vs fixture {name}: largest deviation / bound", {k: f"{v:.3f}" for k, v in worst.items()})


def test_fresh_crops_against_the_restatement():
    """64 seeded crops in ONE call, mixed point counts and outlier shares, against tests/umeyama_ref.py.  A crop that is not decisive
    on the restatement's values is dropped; at most 1 of the 64 may be (the margins make a drop a 1e-4 event)."""
    rng = np.random.RandomState(2024)
    sizes = [5, 17, 63, 64, 65, 129, 300, 700, 1500, 2500, 4095, 4096]
    crops = [R.synth_crop(rng, sizes[i % len(sizes)], [0.0, 0.2, 0.45, 0.3][(i // 3) % 4], flat=i % 16 == 7, mirror=i % 16 == 7) for i in range(64)]
    inputs = R.stack_crops(crops)
    draws = rng.randint(0, 2 ** 32, size=(64, R.MAX_ITER, R.SAMPLE), dtype=np.uint64).astype(np.uint32)
    ref, PC = R.pose_from_umeyama_ref(draws=draws, **inputs)
    s, rot, t, det = _run(inputs, draws)
    assert np.array_equal(det["PC"].view(np.uint32), PC.view(np.uint32))
    _check_common(s, rot, t, det)
    dropped, worst, n_ok = [], {"scale": 0.0, "R": 0.0, "t": 0.0}, 0
    for b, r in enumerate(ref):
        assert np.array_equal(det["index"][b][:r["n_points"]], r["index"]) and det["n_points"][b] == r["n_points"]
        if not R.decisive(r):
            dropped.append(b)
            continue
        got = _got(det, b)
        assert got["status"] == r["status"] and got["iterations_run"] == r["iterations_run"], (b, got["status"], r["status"])
        assert np.array_equal(got["counts"][:r["iterations_run"]], r["counts"]), b
        assert got["best_iteration"] == r["best_iteration"] and np.array_equal(got["inlier_idx"], r["inlier_idx"]), b
        if r["status"] != R.OK:
            continue
        n_ok += 1
        f = r["fit"]
        b_s, b_R, b_t, b_srt = R.fit_bounds(f)
        dev = {"scale": abs(got["scale"] - f["scale"]) / b_s, "R": np.abs(got["R"] - f["R"]).max() / b_R, "t": np.abs(got["t"] - f["t"]).max() / b_t}
        for k, v in dev.items():
            worst[k] = max(worst[k], v)
            assert v <= 1, (b, k, v)
        assert (np.abs(got["sRT"] - f["sRT"]) <= b_srt).all(), b
    print(f"kernel vs restatement: {n_ok} fitted crops, dropped {dropped}, largest deviation / bound", {k: f"{v:.3f}" for k, v in worst.items()})
    assert len(dropped) <= 1 and n_ok >= 50


def test_two_runs_give_identical_bits_and_fp16_map_equals_its_widening():
    inputs, draws, PC, flag, crops = R.load_fixture("waves")
    a = _run(inputs, draws)
    b = _run(inputs, draws)
    for k in ("scale", "R", "t", "sRT", "sigma", "record", "counts", "inlier", "index", "points"):
        assert np.array_equal(_bits(a[3][k]), _bits(b[3][k])), k
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[:3], b[:3]))
    h = dict(inputs, xyz_coor=inputs["xyz_coor"].astype(np.float16))
    c = _run(h, draws)
    d = _run(dict(inputs, xyz_coor=h["xyz_coor"].astype(np.float32)), draws)
    for k in ("scale", "R", "t", "sRT", "record", "counts", "inlier", "points"):
        assert np.array_equal(_bits(c[3][k]), _bits(d[3][k])), k


def test_default_draws_are_the_seeded_table_and_the_cpu_signature_returns_host_tensors():
    from givepose_amd import pose_from_umeyama, umeyama as Um
    inputs, draws, PC, flag, crops = R.load_fixture("b1")
    a = _run(inputs, None, seed=5)
    b = _run(inputs, Um.make_draws(1, seed=5))
    assert np.array_equal(a[3]["counts"], b[3]["counts"]) and np.array_equal(a[3]["sRT"], b[3]["sRT"])
    args = [T(inputs[k]) for k in ("xyz_coor", "coor_2d", "camK", "Depth", "obj_mask")]
    s, rot, t = pose_from_umeyama(*args, seed=5)                     # the reference's signature, CPU tensors in and out
    assert s.device.type == rot.device.type == t.device.type == "cpu" and s.dtype == torch.float32
    assert np.array_equal(s.numpy(), a[0]) and np.array_equal(rot.numpy(), a[1]) and np.array_equal(t.numpy(), a[2])


def test_rank_deficient_final_set_reports_degenerate():
    """A crop whose points are all ONE point pair repeated: every sample and the final set have no variance."""
    rng = np.random.RandomState(3)
    c = R.synth_crop(rng, 40, 0.0)
    keep = c["obj_mask"].reshape(-1) != 0
    first = np.nonzero(keep)[0][0]
    for k, ch in (("xyz_coor", 3), ("coor_2d", 2), ("Depth", 1)):
        v = c[k].reshape(ch, -1)
        v[:, keep] = v[:, first:first + 1]
    # ... and a crop whose NOCS points lie exactly on ONE LINE (small dyadic coordinates: no rounding bends it): rank 1 in every sample
    c2 = R.synth_crop(rng, 40, 0.0)
    keep2 = np.nonzero(c2["obj_mask"].reshape(-1))[0]
    x = c2["xyz_coor"].reshape(3, -1)
    x[:, keep2] = (np.array([[-20.0], [3.0], [8.0]]) + np.array([[1.0], [2.0], [-1.0]]) * np.arange(40)[None]).astype(np.float32) / 64
    inputs = R.stack_crops([c, c2])
    draws = rng.randint(0, 2 ** 32, size=(2, R.MAX_ITER, R.SAMPLE), dtype=np.uint64).astype(np.uint32)
    s, rot, t, det = _run(inputs, draws)
    _check_common(s, rot, t, det)
    assert det["status"][0] == R.LOW_INLIERS and not det["counts"][0].any()      # nothing is ever counted: no winner
    # the collinear source points have rank 1 in every sample as well: the same outcome, never a NaN
    assert det["status"][1] == R.LOW_INLIERS and not det["counts"][1].any() and det["scale"][1] == 1


def test_bad_shapes_are_refused_before_any_launch():
    from givepose_amd import _lib
    from givepose_amd.umeyama import pose_from_umeyama_device
    dev = torch.device("cuda:0")
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(_lib.GivePoseHipError, match="64 x 64"):      # an error code from the library, not a launch
        pose_from_umeyama_device(z(2, 3, 32, 32), z(2, 2, 32, 32), z(2, 3, 3), z(2, 1, 32, 32), z(2, 1, 32, 32))
    with pytest.raises(ValueError):
        pose_from_umeyama_device(z(2, 3, 64, 64), z(2, 2, 64, 64), z(1, 3, 3), z(2, 1, 64, 64), z(2, 1, 64, 64))
    with pytest.raises(ValueError):
        pose_from_umeyama_device(z(2, 3, 64, 64), z(2, 3, 64, 64), z(2, 3, 3), z(2, 1, 64, 64), z(2, 1, 64, 64))
    with pytest.raises(ValueError):
        pose_from_umeyama_device(z(2, 3, 64, 64), z(2, 2, 64, 64), z(2, 3, 3), z(2, 1, 64, 64), z(2, 1, 64, 64), draws=np.zeros((2, 64, 5), np.uint32))
    L = _lib.load()
    p = z(16).data_ptr()
    assert L.gpa_backproject(p, p, p, p, p, 0, 1, 32, p, p, p, 0, 0) == -1 and b"64" in L.gp_last_error()
    assert L.gpa_backproject(p, p, p, p, p, 0, 0, 64, p, p, p, 0, 0) == -1
    assert L.gpa_backproject(0, p, p, p, p, 0, 1, 64, p, p, p, 0, 0) == -1
    assert L.gpa_umeyama(p, p, p, 0, p, p, p, p, p, p, p, 0) == -1 and L.gpa_umeyama(p, p, 0, 1, p, p, p, p, p, p, p, 0) == -1
    assert L.gpa_crop_depth(p, p, p, p, p, 0, 1, 4, 4, 2, 0) == -1 and L.gpa_crop_depth(p, p, p, 0, p, 1, 1, 4, 4, 2, 0) == -1
    torch.cuda.synchronize()


def _scene_boxes(seed, n, H=480, W=640):
    """The bounding boxes tests/test_preprocess.py uses (its _scene), boxes that leave the frame included."""
    rng = np.random.default_rng(seed)
    rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rng.random((H, W, n))
    b = []
    for _ in range(n):
        y1, x1 = rng.integers(-30, H - 60), rng.integers(-30, W - 60)
        b.append([y1, x1, y1 + rng.integers(24, 300), x1 + rng.integers(24, 300)])
    b[-1] = [0, 0, H, W]
    return np.array(b)


@pytest.mark.parametrize("seed,n", [(5, 1), (6, 7)])
def test_crop_depth_bit_exact(seed, n):
    """gpa_crop_depth (RoiCropper.crop_depth) against oracle.preprocess_ref.warp_affine_nearest_ref applied to the depth frame and to
    the pixel-coordinate planes, several frames in one call."""
    from givepose_amd import preprocess as P
    from oracle import preprocess_ref as O
    H, W = 480, 640
    rng = np.random.default_rng(seed)
    F = 2
    depth = rng.uniform(0.3, 3.0, (F, H, W)).astype(np.float32)
    depth[rng.random((F, H, W)) < 0.05] = 0
    boxes = np.concatenate([_scene_boxes(seed * 100 + f, n) for f in range(F)])
    boxes[0] = [-200, -300, -100, -150]       # a crop that lies outside the frame altogether: all border
    fidx = [f for f in range(F) for _ in range(n)]
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    out = P.RoiCropper(H, W, torch.device("cuda:0")).crop_depth(depth, fidx, boxes)
    torch.cuda.synchronize()
    rd, rp = out["roi_depth"].cpu().numpy(), out["roi_pix_2d"].cpu().numpy()
    assert rd.shape == (F * n, 1, 64, 64) and rp.shape == (F * n, 2, 64, 64)
    for j, (y1, x1, y2, x2) in enumerate(boxes.astype(np.float64)):
        center = np.array([0.5 * (x1 + x2), 0.5 * (y1 + y2)])
        scale = min(max(y2 - y1, x2 - x1) * 1.5, max(H, W)) * 1.0
        M = O.get_affine_transform_ref(center, scale, 64)
        assert np.array_equal(rd[j, 0], O.warp_affine_nearest_ref(depth[fidx[j]], M, 64)), j
        assert np.array_equal(rp[j, 0], O.warp_affine_nearest_ref(gx, M, 64)) and np.array_equal(rp[j, 1], O.warp_affine_nearest_ref(gy, M, 64)), j
    assert not rd[0].any() and not rp[0].any()
    with pytest.raises(ValueError):
        P.RoiCropper(H, W, torch.device("cuda:0")).crop_depth(depth, [0, 2], boxes[:2])      # frame 2 does not exist


def test_alignment_recovers_a_known_similarity_from_a_rendered_depth_frame():
    """Depth frame -> crop_depth -> alignment, fed the synthetic NOCS map directly: the known transform comes back."""
    from givepose_amd import preprocess as P, synth
    from givepose_amd.umeyama import pose_from_umeyama_device
    H, W, dev = 480, 640, torch.device("cuda:0")
    K3 = np.asarray(synth.REAL_INTRINSICS, np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = (1.2 + 0.15 * np.sin(u / 40) * np.cos(v / 55) + 0.1 * np.cos(u / 23)).astype(np.float32)
    d = depth.astype(np.float64)
    Pc = np.stack([(u - K3[0, 2]) * d / K3[0, 0], (v - K3[1, 2]) * d / K3[1, 1], d], -1)
    q = np.linalg.qr(np.random.RandomState(1).normal(size=(3, 3)))[0]
    q *= np.sign(np.linalg.det(q))
    s, t = 0.37, np.array([0.05, -0.08, 1.25])
    nocs = ((Pc - t) @ q / s).astype(np.float32)                      # x = R^T (P - t) / s per pixel
    boxes = np.array([[100, 150, 300, 380], [200, 300, 420, 560], [-20, -20, 200, 180]])
    crop = P.RoiCropper(H, W, dev).crop_depth(depth[None], [0, 0, 0], boxes)
    pix = crop["roi_pix_2d"].cpu().numpy().astype(np.int64)
    inside = crop["roi_depth"].cpu().numpy() > 0
    xyz = np.stack([nocs[pix[b, 1], pix[b, 0]].transpose(2, 0, 1) for b in range(3)])
    Kb = T(np.broadcast_to(K3.astype(np.float32), (3, 3, 3)).copy()).to(dev)
    sc, rot, tr, det = pose_from_umeyama_device(T(xyz).to(dev), crop["roi_pix_2d"], Kb, crop["roi_depth"], T(inside).to(dev),
                                                valid_depth_only=True, return_details=True)
    assert (det["status"].cpu().numpy() == R.OK).all() and (det["iterations_run"].cpu().numpy() == 2).all()
    assert np.abs(sc.cpu().numpy() - s).max() < 1e-4 and np.abs(rot.cpu().numpy() - q).max() < 1e-4 and np.abs(tr.cpu().numpy() - t).max() < 1e-4
    assert not inside[2].all() and inside[0].all()                   # the third box leaves the frame: border pixels are masked out


def test_frame_pipeline_depth_adds_the_geometric_pose_and_changes_nothing_else():
    from givepose_amd import PoseNet, PoseNetConfig, Scale_net, synth
    from givepose_amd.pipeline import FramePipeline
    rng = np.random.default_rng(12)
    H, W, n = 480, 640, 3
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    masks = (rng.random((n, H, W)) > 0.5).astype(np.uint8)
    boxes = np.array([[100, 150, 300, 380], [200, 300, 420, 560], [-20, -20, 200, 180]])
    cats = rng.integers(0, 6, n)
    full = rng.standard_normal((3, 256, 256)).astype(np.float32)
    depth = rng.uniform(0.5, 2.0, (H, W)).astype(np.float32)
    net = PoseNet(PoseNetConfig(), dtype=torch.float32, seed=0).cuda()
    pipe = FramePipeline(net, Scale_net(feat_dim=24, seed=0).cuda())
    args = (frame, masks, boxes, cats, synth.REAL_INTRINSICS, synth.MEAN_SIZES[cats], full)
    rt0, size0, out0 = pipe(*args)
    rt0, size0, keys0 = rt0.clone(), size0.clone(), set(out0)
    held = {k: v.clone() for k, v in out0.items() if torch.is_tensor(v)}
    rt1, size1, out1 = pipe(*args, depth=depth)
    torch.cuda.synchronize()
    assert not any(k.startswith("umeyama") for k in keys0)
    assert set(out1) == keys0 | {"umeyama_RT", "umeyama_scale", "umeyama_status"}
    assert torch.equal(rt0, rt1) and torch.equal(size0, size1)         # bit for bit
    for k, v in held.items():
        assert torch.equal(v, out1[k]), k
    assert out1["umeyama_RT"].shape == (n, 4, 4) and out1["umeyama_RT"].dtype == torch.float32 and out1["umeyama_scale"].shape == (n,)
    assert out1["umeyama_status"].shape == (n,) and out1["umeyama_status"].dtype == torch.int32
    assert torch.isfinite(out1["umeyama_RT"]).all() and torch.isfinite(out1["umeyama_scale"]).all()
    assert torch.equal(out1["umeyama_RT"][:, 3], torch.tensor([0, 0, 0, 1.0], device=rt1.device).expand(n, 4))
    rt2, size2, out2, sizes = pipe.run_frames(frame[None], [masks], [boxes], [cats], synth.REAL_INTRINSICS, [synth.MEAN_SIZES[cats]], full[None], depths=depth[None])
    # (the multi-frame plan agrees with the one-frame plan to 1e-4, not bit for bit, and an alignment of random-weight maps is not
    #  continuous in its input: only the presence and the shapes are compared here)
    assert sizes == [n] and out2["umeyama_RT"].shape == (n, 4, 4) and out2["umeyama_status"].shape == (n,) and out2["umeyama_scale"].shape == (n,)
    assert torch.isfinite(out2["umeyama_RT"]).all()
    rt2 = rt2.clone()
    rt3, size3, out3, _ = pipe.run_frames(frame[None], [masks], [boxes], [cats], synth.REAL_INTRINSICS, [synth.MEAN_SIZES[cats]], full[None])
    assert torch.equal(rt2, rt3) and not any(k.startswith("umeyama") for k in out3)
