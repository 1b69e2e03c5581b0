"""GPU: givepose_amd.TrainBatchBuilder (gpt_crop_train + gpt_mask_deform, include/givepose_traindata.h) against the numpy restatement of
the reference's train-time sample in tests/train_batch_ref.py.  Every comparison is bit equality: each output value is a table lookup
or an integer decision.  The references are computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

import train_batch_ref as R

pytestmark = pytest.mark.gpu
T = torch.from_numpy
MAPS = ("roi_img", "roi_mask", "roi_mask_deform", "roi_mask_output", "roi_ivfc_mask_output", "roi_coord_2d", "nocs_coord", "ivfc_coord")
SMALL = ("roi_wh", "bbox_center", "resize_ratio")
MUG_META = (np.array([0.013, -0.0625, 0.2071], dtype=np.float64), 0.9137)


def labels_for(B, seed=60):
    import pose_loss_ref as PR
    from givepose_amd import synth
    _, gt = PR.make_inputs(B=B, P=256, seed=seed)
    lab = {k: gt[k] for k in ("rotation", "translation", "real_size", "sym_info", "nocs_scale", "model_point")}
    lab["mean_size"] = synth.MEAN_SIZES[np.arange(B) % 6]
    lab["cam_K"] = np.broadcast_to(synth.REAL_INTRINSICS, (B, 3, 3)).copy()
    return lab


def frames_for(r, F, NI, H, W):
    """Random frames; instance ids in 8 x 8 blocks with a few stray pixels; an IVFC red channel that is 0 on a third of the blocks."""
    up = lambda a: np.repeat(np.repeat(a, 8, 1), 8, 2)[:, :H, :W]
    gh, gw = (H + 7) // 8, (W + 7) // 8
    inst = up(r.integers(0, 4, (F, gh, gw), dtype=np.uint8))
    stray = r.random((F, H, W)) < 0.03
    inst = np.where(stray, r.integers(0, 4, (F, H, W), dtype=np.uint8), inst).astype(np.uint8)
    ivfc = r.integers(0, 256, (NI, H, W, 3), dtype=np.uint8)
    ivfc[..., 0] = np.where(up(r.random((NI, gh, gw)) < 0.33), 0, ivfc[..., 0])
    return {"frames": r.integers(0, 256, (F, H, W, 3), dtype=np.uint8), "inst_masks": np.ascontiguousarray(inst),
            "nocs_png": r.integers(0, 256, (F, H, W, 3), dtype=np.uint8), "ivfc_png": ivfc}


@functools.lru_cache(maxsize=None)
def full_case():
    """480 x 640, S = 256, R = 64, B = 5: sample 1 is a mug, samples 1 and 2 share frame 1, sample 3's crop hangs over the bottom and
    the right edge of the frame, sample 4 is not deformed."""
    H, W, S, B = 480, 640, 256, 5
    r = np.random.Generator(np.random.Philox(key=[11, 0x7B47]))
    c = frames_for(r, 3, 5, H, W)
    c.update(frame_idx=[0, 1, 1, 2, 0], ivfc_idx=[4, 0, 1, 2, 3], inst_id=[1, 2, 3, 1, 2], cat_id=[0, 5, 3, 2, 4],
             mug_meta=[None, MUG_META, None, None, None],
             bbox=np.array([[100, 200, 220, 300], [150.5, 60.25, 400, 250], [30, 330, 90, 480], [370, 510, 478, 638], [5, 8, 470, 600]], dtype=np.float64))
    draws = {"dzi": r.random((B, 3)), "deform": np.array([True, True, True, True, False]),
             "keys": r.integers(0, 1 << 32, (B, S, S), dtype=np.uint64).astype(np.uint32)}
    draws["dzi"][3] = (0.9, 0.95, 0.9)            # larger, shifted right and down: over both edges
    ref = R.batch_ref(c["frames"], c["inst_masks"], c["nocs_png"], c["ivfc_png"], c["frame_idx"], c["ivfc_idx"], c["inst_id"], c["bbox"],
                      c["cat_id"], c["mug_meta"], draws)
    for v in ref.values():
        v.setflags(write=False)
    return c, draws, labels_for(B), ref


def run(builder, c, labels, n=None, **kw):
    sl = (lambda v: v[:n]) if n else (lambda v: v)
    return builder(c["frames"], c["inst_masks"], c["nocs_png"], c["ivfc_png"], sl(c["frame_idx"]), sl(c["ivfc_idx"]), sl(c["inst_id"]),
                   sl(c["bbox"]), sl(c["cat_id"]), sl(c["mug_meta"]), {k: v[:n] if n else v for k, v in labels.items()}, **kw)


def check(got, ref, labels, what):
    for k in MAPS + SMALL:
        g = got[k]
        assert g.dtype == torch.float32 and g.is_cuda and g.is_contiguous() and tuple(g.shape) == ref[k].shape, (what, k)
        assert np.array_equal(g.cpu().numpy().view(np.uint32), ref[k].view(np.uint32)), (what, k)
    for k, v in labels.items():
        assert np.array_equal(got[k].cpu().numpy(), np.asarray(v, dtype=np.float32)) and got[k].dtype == torch.float32, (what, k)
    assert set(got) == set(MAPS + SMALL) | set(labels)


def test_full_size_every_key_bit_equal():
    from givepose_amd import TrainBatchBuilder
    c, draws, labels, ref = full_case()
    got = run(TrainBatchBuilder(480, 640, "cuda"), c, labels, draws=draws)
    check(got, ref, labels, "full size")
    # the case is what it claims: a crop over two edges, a live deformation, a mug whose table differs, an IVFC mask of its own
    assert (ref["roi_coord_2d"][3][:, -1, -1] == 0).all() and (ref["roi_coord_2d"][3][:, 0, 0] != 0).all()
    assert all((ref["roi_mask_deform"][b] != ref["roi_mask"][b]).any() for b in range(4)) and np.array_equal(ref["roi_mask_deform"][4], ref["roi_mask"][4])
    assert np.abs(ref["nocs_coord"][1]).max() > 0.5 >= np.abs(ref["nocs_coord"][0]).max() > 0
    assert (ref["roi_ivfc_mask_output"] != ref["roi_mask_output"]).any() and ((ref["ivfc_coord"] != 0).any(1, keepdims=True) <= (ref["roi_ivfc_mask_output"] != 0)).all()


# ------------------------------------------------------------------------------------------------ the deformation cases
@functools.lru_cache(maxsize=None)
def small_case(S, R_):
    """40 x 50 frames, B = 6, a frame per sample.  With pad_scale 1 and the centre draws an S x S box maps 1 : 1, so roi_mask is the
    window [4:4+S, 9:9+S] of the frame's mask, which is drawn here: all 0, all 1, a single pixel, a blob with an odd band, a
    chequerboard with a few flips (nearly every pixel in the band), and noise whose keys are drawn from 0..3."""
    H, W, B = 40, 50, 6
    r = np.random.Generator(np.random.Philox(key=[S, 0x7B48]))
    c = frames_for(r, B, B, H, W)
    win = np.zeros((B, S, S), np.uint8)
    win[1] = 1
    win[2, S // 2, S // 3] = 1
    win[3, 3:12, 2:10] = 1
    win[3, 7, 2] = 0                                   # a notch in the left edge, and a stray pixel: l = 34 + 3
    win[3, 15, 15] = 1
    win[4] = (np.add.outer(np.arange(S), np.arange(S)) % 2 == 1) ^ (r.random((S, S)) < 0.05)      # a chequerboard with a few flips
    win[5] = r.random((S, S)) > 0.5
    inst = np.full((B, H, W), 9, np.uint8)
    inst[1] = 7
    inst[:, 4:4 + S, 9:9 + S] = np.where(win != 0, 7, 9)
    c["inst_masks"] = inst
    c.update(frame_idx=list(range(B)), ivfc_idx=list(range(B)), inst_id=[7] * B, cat_id=[0, 1, 5, 2, 3, 4], mug_meta=[None, None, MUG_META, None, None, None],
             bbox=np.array([[4, 9, 4 + S, 9 + S]] * B, dtype=np.float64))
    keys = r.integers(0, 1 << 32, (B, S, S), dtype=np.uint64).astype(np.uint32)
    keys[5] = r.integers(0, 4, (S, S))
    draws = {"dzi": np.full((B, 3), 0.5), "deform": np.ones(B, bool), "keys": keys}
    kw = dict(img_size=S, out_res=R_, pad_scale=1.0)
    args = (c["frames"], c["inst_masks"], c["nocs_png"], c["ivfc_png"], c["frame_idx"], c["ivfc_idx"], c["inst_id"], c["bbox"], c["cat_id"], c["mug_meta"])
    ref = R.batch_ref(*args, draws, **kw)
    off = {**draws, "deform": np.zeros(B, bool)}
    return c, draws, off, labels_for(B), ref, R.batch_ref(*args, off, **kw), win


@pytest.mark.parametrize("S,R_", [(32, 8), (20, 5)])        # 16 whole 64-pixel groups; 6 groups and a quarter
def test_small_grid_deformation_cases(S, R_):
    from givepose_amd import TrainBatchBuilder
    from test_train_batch_cpu import _band
    c, draws, off, labels, ref, ref_off, win = small_case(S, R_)
    builder = TrainBatchBuilder(40, 50, "cuda", img_size=S, out_res=R_, pad_scale=1.0)
    got = run(builder, c, labels, draws=draws)
    check(got, ref, labels, f"small grid {S}")
    # the cases are what they claim (read off the reference, not the product)
    m, d = ref["roi_mask"][:, 0], ref["roi_mask_deform"][:, 0]
    assert np.array_equal(m, win.astype(np.float32))
    l = [int(_band(x).sum()) for x in m]
    assert l[0] == 0 and l[1] == 0 and not d[0].any() and d[1].all()
    assert m[2].sum() == 1 and l[2] == 3 and d[2].sum() == 2
    assert l[3] == 37
    assert l[4] > 0.8 * S * S and l[5] > 0.6 * S * S             # nearly every pixel; three quarters for plain noise
    for b in range(6):
        assert int((d[b][_band(m[b])] == 0).sum()) == l[b] // 2, b
    # duplicate keys: among equal keys the lower pixel index is taken, so the zeros of a key class are a prefix of it
    band, k5 = _band(m[5]), draws["keys"][5]
    classes = [np.flatnonzero(d[5][band][k5[band] == v] == 0) for v in range(4)]
    assert all(np.array_equal(z, np.arange(len(z))) for z in classes) and sum(len(z) for z in classes) == l[5] // 2
    # deform = 0: a copy
    got0 = run(builder, c, labels, draws=off)
    check(got0, ref_off, labels, f"small grid {S}, no deformation")
    assert torch.equal(got0["roi_mask_deform"], got0["roi_mask"]) and np.array_equal(ref_off["roi_mask_deform"], ref_off["roi_mask"])


# ------------------------------------------------------------------------------------------------ the seeded form
def test_seeded_form():
    from givepose_amd import TrainBatchBuilder, train_batch as TB
    c, _, _, labels, _, _, _ = small_case(32, 8)
    B, S = 6, 32
    builder = TrainBatchBuilder(40, 50, "cuda", img_size=S, out_res=8, mask_pro=0.7)
    seed = 0x1234567890ABCDEF
    dzi, deform = TB.host_draws(seed, B, 0.7)
    assert deform.any() and not deform.all() and dzi.shape == (B, 3)
    r = np.random.Generator(np.random.Philox(key=[seed, TB.DRAW_TAG]))
    assert np.array_equal(dzi, r.random((B, 3))) and np.array_equal(deform, r.random(B) <= 0.7)
    a = run(builder, c, labels, seed=seed)
    explicit = run(builder, c, labels, draws={"dzi": dzi, "deform": deform, "keys": R.hash_keys(seed, B, S)})
    again = run(builder, c, labels, seed=seed)
    other = run(builder, c, labels, seed=seed + 1)
    for k in a:
        assert torch.equal(a[k], explicit[k]), k
        assert torch.equal(a[k], again[k]), k
    assert not torch.equal(a["roi_img"], other["roi_img"]) and not torch.equal(a["roi_mask_deform"], other["roi_mask_deform"])
    assert any(not torch.equal(a["roi_mask_deform"][b], a["roi_mask"][b]) for b in range(B))
    # the same draws, other keys: only the deformation moves
    rekeyed = run(builder, c, labels, draws={"dzi": dzi, "deform": deform, "keys": R.hash_keys(seed + 1, B, S)})
    assert not torch.equal(a["roi_mask_deform"], rekeyed["roi_mask_deform"])
    assert all(torch.equal(a[k], rekeyed[k]) for k in a if k != "roi_mask_deform")
    with pytest.raises(ValueError, match="exactly one of draws and seed"):
        run(builder, c, labels)
    with pytest.raises(ValueError, match="exactly one of draws and seed"):
        run(builder, c, labels, seed=1, draws={"dzi": dzi, "deform": deform, "keys": R.hash_keys(1, B, S)})
    with pytest.raises(ValueError, match="2\\^64"):
        run(builder, c, labels, seed=1 << 64)


# ------------------------------------------------------------------------------------------------ the inference path
def test_agrees_with_roi_cropper():
    from givepose_amd import TrainBatchBuilder
    from givepose_amd.preprocess import RoiCropper
    c, draws, labels, _ = full_case()
    B = 5
    got = run(TrainBatchBuilder(480, 640, "cuda"), c, labels, draws={**draws, "dzi": np.full((B, 3), 0.5)})
    masks = np.stack([(c["inst_masks"][f] == i) for f, i in zip(c["frame_idx"], c["inst_id"])]).astype(np.uint8)
    inf = RoiCropper(480, 640, "cuda")(c["frames"], masks, c["frame_idx"], list(range(B)), c["bbox"])
    for k in ("roi_img", "roi_coord_2d", "roi_wh", "bbox_center", "resize_ratio", "roi_mask"):
        assert torch.equal(got[k].view(torch.int32), inf[k].view(torch.int32)), k


# ------------------------------------------------------------------------------------------------ the dict is accepted
def test_dict_feeds_head_grads_and_train_step():
    """head_grads on the builder's dict and on the reference dict uploaded with .to(device): the six loss terms are equal.  Should the
    parent's head_grads not repeat its own bits on two runs of the uploaded dict, the builder's run is held to the difference of those
    two runs instead (the inputs are bit-equal either way: test_full_size_every_key_bit_equal)."""
    import bb_backward_ref as BB
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, Ranger, TrainBatchBuilder
    c, draws, labels, ref = full_case()
    n = 2
    lab = {k: v[:n] for k, v in labels.items()}
    built = run(TrainBatchBuilder(480, 640, "cuda"), c, labels, n=n, draws={k: v[:n] for k, v in draws.items()})
    uploaded = {**{k: T(v[:n].copy()).to("cuda") for k, v in ref.items()},
                **{k: T(np.ascontiguousarray(v, dtype=np.float32)).to("cuda") for k, v in lab.items()}}
    assert set(built) == set(uploaded)
    net = PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1)), dtype=torch.float32, seed=BB.WEIGHT_SEED).cuda()
    terms = lambda d: {k: v.detach().double().cpu().clone() for k, v in net.head_grads(d, PoseLoss(), "cuda")["loss"].items()}
    u1, u2, b1 = terms(uploaded), terms(uploaded), terms(built)
    assert len(u1) >= 6
    for k in u1:
        slack = (u1[k] - u2[k]).abs()
        print(f"{k}: uploaded {u1[k].tolist()} built {b1[k].tolist()} run-to-run {slack.tolist()}")
        assert torch.isfinite(b1[k]).all() and ((b1[k] - u1[k]).abs() <= slack).all(), k
    res = net.train_step(built, PoseLoss(), Ranger(net), "cuda")
    assert all(torch.isfinite(v).all() for v in res["loss"].values()) and len(res["loss"]) >= 6


# ------------------------------------------------------------------------------------------------ out= and refusals
def test_out_buffers_and_refusals():
    from givepose_amd import TrainBatchBuilder
    c, draws, _, labels, ref, _, _ = small_case(32, 8)
    B, S, R_ = 6, 32, 8
    builder = TrainBatchBuilder(40, 50, "cuda", img_size=S, out_res=R_, pad_scale=1.0)
    fresh = lambda: {**{k: torch.full(ref[k].shape, -7.0, device="cuda") for k in MAPS + SMALL},
                     **{k: torch.full(np.shape(v), -7.0, device="cuda") for k, v in labels.items()}}
    out = fresh()
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    got = run(builder, c, labels, draws=draws, out=out)
    assert got is out and {k: v.data_ptr() for k, v in out.items()} == ptrs
    check(out, ref, labels, "out=")
    partial = {"roi_img": torch.full(ref["roi_img"].shape, -7.0, device="cuda")}      # the rest is allocated
    check(run(builder, c, labels, draws=draws, out=partial), ref, labels, "partial out=")
    for k, bad in (("nocs_coord", torch.zeros(B, 3, R_, R_ + 1, device="cuda")), ("roi_mask_deform", torch.zeros(B, 1, S, S, device="cuda", dtype=torch.float16)),
                   ("roi_wh", torch.zeros(B, 3, device="cuda")), ("roi_img", torch.zeros(B, 3, S, S)), ("rotation", torch.zeros(B, 9, device="cuda"))):
        o = fresh()
        o[k] = bad
        with pytest.raises(ValueError, match=k):
            run(builder, c, labels, draws=draws, out=o)
        assert all((v == -7.0).all() for n_, v in o.items() if n_ != k), k          # a refused call writes nothing
    o = fresh()
    o["roi_mask_deform"] = o["roi_mask"]
    with pytest.raises(ValueError, match="two buffers"):
        run(builder, c, labels, draws=draws, out=o)
    for field, bad in (("frame_idx", [0, 1, 2, 3, 4, 6]), ("frame_idx", [0, 1, 2, 3, 4, -1]), ("ivfc_idx", [0, 1, 2, 3, 4, 6]),
                       ("inst_id", [7, 7, 7, 7, 7, 256]), ("cat_id", [0, 1, 5, 2, 3, 6]), ("frame_idx", [0, 1, 2])):
        with pytest.raises(ValueError, match="out of range|must lie in|one entry per sample"):
            run(builder, {**c, field: bad}, labels, draws=draws)
    with pytest.raises(ValueError, match="mug"):
        run(builder, {**c, "mug_meta": [None] * B}, labels, draws=draws)
    with pytest.raises(ValueError, match="degenerate"):
        run(builder, {**c, "bbox": np.array([[4, 9, 4, 9]] * B, dtype=np.float64)}, labels, draws=draws)
    with pytest.raises(ValueError, match="keys"):
        run(builder, c, labels, draws={**draws, "keys": draws["keys"].astype(np.int64)})
    with pytest.raises(ValueError, match="dzi"):
        run(builder, c, labels, draws={**draws, "dzi": np.full((B, 3), 1.0)})
    with pytest.raises(ValueError, match="labels"):
        run(builder, c, {k: v for k, v in labels.items() if k != "cam_K"}, draws=draws)
    with pytest.raises(ValueError, match="does not match"):
        run(builder, {**c, "nocs_png": c["nocs_png"][:, :-1]}, labels, draws=draws)
    with pytest.raises(RuntimeError, match="HIP device only"):
        TrainBatchBuilder(40, 50, "cpu")
