"""GPU: the validation-loss path -- gpl_pose_loss_partials / gpl_pose_loss_reduce (givepose_amd.PoseLoss, LossAccumulator),
gpl_pose_decode_train and PoseNet.forward(do_loss=True) -- against the float64 restatement tests/pose_loss_ref.py and the fixtures
scripts/gen_golden_pose_loss.py recorded from the reference's own PoseLoss, pose_from_predictions_train and PoseNet.forward.

Bounds.  Float64 terms against the restatement: 1e-11 relative (a term sums at most 12 288 summands whose elements the kernel
reproduces bit for bit; only the order of the sum differs, a handful of 2^-53 roundings each).  Against the reference's float32
fixture: 16 * 2^-24 relative, the bound of tests/test_pose_loss_cpu.py.  Decode: 1e-12 against the restatement, and against the
reference's float32 fixture the bounds of tests/test_pnp_flags_gpu.py::test_pose_tail_rt_golden (2e-6 rotation, 1e-5 translation).
forward(do_loss=True): the bounds of tests/test_pnp_flags_gpu.py::test_e2e_golden per mode."""
import functools
import zlib

import numpy as np
import pytest
import torch

import pose_loss_ref as R

pytestmark = pytest.mark.gpu
T = torch.from_numpy
REF_BOUND = 16 * 2.0 ** -24
SPLIT = "split"
MODES = {torch.float32: dict(dtype=torch.float32), SPLIT: dict(dtype=torch.float32, split_gemm=True), torch.float16: dict(dtype=torch.float16)}


def tensors(d, device=None):
    return {k: (T(v).to(device) if device else T(v)) for k, v in d.items()}


def cfg_of(cfg):
    from givepose_amd import LossConfig
    return LossConfig(**cfg)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.where(b != 0, np.abs(b), 1.0)))


def run(pred, data, cfg, host_data=True):
    """PoseLoss on the device: predictions on the device, ground truth on the host (or the device) -> (loss dict, details on the host)."""
    from givepose_amd import PoseLoss
    loss, det = PoseLoss(cfg_of(cfg))(tensors(pred, "cuda"), tensors(data, None if host_data else "cuda"), return_details=True)
    torch.cuda.synchronize()
    return loss, {k: v.cpu().numpy() for k, v in det.items()}


def check_against_restatement(pred, data, cfg, what):
    ref = R.pose_loss_ref(pred, data, **cfg)
    loss, det = run(pred, data, cfg)
    err = rel(det["terms"], ref["terms"])
    err_re = float(np.abs(det["re"] - ref["re"]).max()), float(np.abs(det["re_best"] - ref["re_best"]).max())
    err_te = rel(det["te"], ref["te"])
    print(f"{what}: float64 terms vs restatement max rel {err:.2e}; re abs {err_re[0]:.2e} / {err_re[1]:.2e} deg; te rel {err_te:.2e}")
    assert det["terms"].dtype == np.float64 and err < 1e-11, (what, det["terms"], ref["terms"])
    assert np.array_equal(det["index"], ref["index"].astype(np.float64)), (what, det["index"], ref["index"])       # exactly
    assert np.array_equal(det["branch"], np.full(len(ref["index"]), float(ref["branch"])))
    # re: the traces are bit-identical, acos differs by a few ulp of its result; near re = 0 an ulp of the cosine is 1e-6 deg
    assert max(err_re) < 1e-9 + 1e-12 * float(np.abs(ref["re"]).max()) and err_te < 1e-12
    assert rel(det["mean_re"], ref["mean_re"]) < 1e-11 and rel(det["mean_te"], ref["mean_te"]) < 1e-11
    # float32 outputs: the float64 ones rounded once
    assert list(loss) == list(R.KEYS)
    got32 = np.array([loss[k].cpu().numpy() for k in R.KEYS])
    assert all(loss[k].dtype == torch.float32 and loss[k].dim() == 0 and loss[k].is_cuda for k in R.KEYS)
    assert np.array_equal(got32.view(np.uint32), det["terms"].astype(np.float32).view(np.uint32))
    assert np.array_equal(det["out32"][:6].view(np.uint32), got32.view(np.uint32))
    return ref, det


@pytest.mark.parametrize("name", list(R.CASES))
def test_terms_against_the_restatement_and_the_reference_fixture(name):
    pred, data, cfg, z = R.load_fixture(name)
    ref, det = check_against_restatement(pred, data, cfg, name)
    err = rel(det["terms"], z["terms"])
    print(f"{name}: float64 terms vs the reference's float32 fixture, max rel {err:.2e}")
    assert err < REF_BOUND
    assert np.array_equal(det["index"], z["index"].astype(np.float64))


def test_masks_zero_one_pixel_full_and_soft():
    """Every crop of a batch with the same kind of mask, so that a whole term is made of it: all-zero -> 0, not NaN."""
    for kind in ("zero", "one", "full", "soft"):
        pred, data = R.make_inputs(B=3, P=7, seed=40, masks=(kind,))
        ref, det = check_against_restatement(pred, data, R.DEFAULTS, "mask " + kind)
        if kind == "zero":
            assert det["terms"][4] == 0.0 and det["terms"][5] == 0.0
        else:
            assert det["terms"][4] > 0 and det["terms"][5] > 0


def test_prediction_equal_to_ground_truth_keeps_the_unrotated_rotation():
    """A symmetric crop whose prediction IS the ground truth: candidate 0 ties with the unrotated rotation, the strict `<` keeps
    index -1; its rotation and point-matching sums are exactly 0.  With r_loss='angle' the same crop sits at trace = 3 (the clip)."""
    pred, data = R.make_inputs(B=3, P=1024, seed=41, sym="all", equal=1)
    ref, det = check_against_restatement(pred, data, R.DEFAULTS, "pred == gt")
    assert det["index"][1] == -1 and det["rot1_sum"][1] == 0.0 and det["re"][1] == det["re_best"][1] < 0.1
    assert det["index"][0] > 0 and det["index"][2] > 0 and np.all(det["re_best"] <= det["re"])
    cfg = {**R.DEFAULTS, "r_loss": "angle"}
    ref, det = check_against_restatement(pred, data, cfg, "pred == gt, angle")
    assert abs(det["rot1_sum"][1] - 0.5 * np.arccos(0.99999) ** 2 / 0.2) < 1e-15       # acos(0.99999) = 4.5e-3 rad, not 0


def test_sym_r_type_leaves_model_point_untouched():
    pred, data, cfg, z = R.load_fixture("symtype")
    from givepose_amd import PoseLoss
    for dev in ("cpu", "cuda"):
        td = tensors(data, dev)
        before = td["model_point"].clone()
        PoseLoss(cfg_of(cfg))(tensors(pred, "cuda"), td)
        torch.cuda.synchronize()
        assert torch.equal(td["model_point"].view(torch.int32), before.view(torch.int32))


def test_bitwise_repeatable_and_host_equals_device_inputs():
    pred, data, cfg, z = R.load_fixture("b5")
    a, da = run(pred, data, cfg, host_data=True)
    b, db = run(pred, data, cfg, host_data=True)
    c, dc = run(pred, data, cfg, host_data=False)
    for k in ("terms", "record", "out32", "mean_re", "mean_te"):
        assert da[k].tobytes() == db[k].tobytes() == dc[k].tobytes(), k


def test_accumulator_is_the_crop_weighted_mean():
    from givepose_amd import LossAccumulator, LossConfig
    acc, exp, n = LossAccumulator(LossConfig()), np.zeros(8), 0
    for i, B in enumerate((3, 1, 5)):
        pred, data = R.make_inputs(B=B, P=64, seed=50 + i)
        acc.add(tensors(pred, "cuda"), tensors(data))
        _, det = run(pred, data, R.DEFAULTS)
        exp[:6] += B * det["terms"]
        exp[6] += B * det["mean_re"]
        exp[7] += B * det["mean_te"]
        n += B
    got = acc.result()
    exp /= n
    assert got["crops"] == 9 and got["batches"] == 3
    for i, k in enumerate(R.KEYS + ("mean_re", "mean_te")):
        assert abs(got[k] - exp[i]) <= 1e-12 * abs(exp[i]), (k, got[k], exp[i])
    assert abs(got["total"] - exp[:6].sum()) <= 1e-12 * exp[:6].sum()


# ------------------------------------------------------------------------------------------------ the train-time decode
@pytest.mark.parametrize("name", list(R.DECODE_CASES))
def test_pose_decode_train(name):
    from givepose_amd import loss
    inp, z = R.load_decode_fixture()
    r_type, t_type = R.DECODE_CASES[name]
    kw = dict(t_site=t_type == "site", is_allo="allo" in r_type)
    er, et = R.decode_train_ref(**kw, **inp)
    rot32, trans32, det = loss.pose_decode_train(**tensors(inp, "cuda"), return_details=True, **kw)
    r64, t64 = det["rot"].cpu().numpy(), det["trans"].cpu().numpy()
    d = float(np.abs(r64 - er).max()), float(np.abs(t64 - et).max())
    f = float(np.abs(rot32.cpu().numpy() - z[name + "__rot"]).max()), float(np.abs(trans32.cpu().numpy() - z[name + "__trans"]).max())
    print(f"decode {name}: float64 vs restatement rot {d[0]:.2e} trans {d[1]:.2e}; float32 vs the reference rot {f[0]:.2e} trans {f[1]:.2e}")
    assert d[0] < 1e-12 and d[1] < 1e-12 * max(1.0, float(np.abs(et).max()))
    assert t64[0, 0] == 0.0 and t64[0, 1] == 0.0 and np.all(R.off_axis_angle(t64[1:]) >= 0.05)
    assert np.array_equal(rot32.cpu().numpy(), r64.astype(np.float32)) and np.array_equal(trans32.cpu().numpy(), t64.astype(np.float32))
    assert f[0] < 2e-6 and f[1] < 1e-5 * max(1.0, float(np.abs(z[name + "__trans"]).max()))


# ------------------------------------------------------------------------------------------------ forward(do_loss=True)
@functools.lru_cache(maxsize=1)
def _e2e():
    from givepose_amd import synth
    z = np.load(R.GOLDEN + "/pose_loss_e2e.npz")
    npb = synth.synth_batch(4, seed=int(z["batch_seed"]))
    r = np.random.Generator(np.random.Philox(key=[int(z["mask_seed"]), 4]))
    npb["roi_mask_deform"] = (r.random(npb["roi_mask"].shape) > 0.4).astype(np.float32)
    assert zlib.crc32(np.ascontiguousarray(npb["roi_img"]).tobytes()) == int(z["roi_img_crc"])
    assert zlib.crc32(np.ascontiguousarray(npb["roi_mask_deform"]).tobytes()) == int(z["mask_crc"])
    return {k: T(v) for k, v in npb.items()}, z


@pytest.mark.parametrize("mode", [torch.float32, SPLIT, torch.float16])
def test_forward_do_loss(mode):
    from givepose_amd import PoseNet, PoseNetConfig
    data, z = _e2e()
    net = PoseNet(PoseNetConfig(), seed=0, **MODES[mode]).cuda()
    eval_data = {k: v for k, v in data.items() if k != "roi_mask_deform"}
    keys = ("rot", "trans", "size", "mask", "nocs_coor", "ivfc_coor")
    direct = {k: v.clone() for k, v in net.forward_device(eval_data, "cuda").items() if k in keys}
    before = net(eval_data, "cuda")
    out = net(data, "cuda", do_loss=True)
    after = net(eval_data, "cuda")
    torch.cuda.synchronize()
    assert list(out) == list(keys) and all(v.is_cuda for v in out.values())
    err = {k: float(np.abs(out[k].float().cpu().numpy() - z[k]).max()) for k in ("rot", "trans", "size")}
    print(f"forward(do_loss=True) {mode}", err)
    if mode == torch.float16:
        assert err["rot"] < 3e-2 and err["size"] < 3e-2 and err["trans"] < 3e-2 * max(1.0, float(np.abs(z["trans"]).max()))
    else:
        assert err["rot"] < 1e-4 and err["trans"] < 1e-4 and err["size"] < 1e-4, err
    nearest = torch.nn.functional.interpolate(data["roi_mask_deform"], size=(64, 64), mode="nearest")
    assert torch.equal(out["mask"].float().cpu(), nearest) and np.array_equal(nearest.numpy(), z["mask"].astype(np.float32))
    assert not torch.equal(out["mask"].float().cpu(), direct["mask"].float().cpu())       # the deformed mask, not roi_mask
    for k in keys:                                                                          # do_loss=False: the bits of forward_device
        assert torch.equal(before[k].cpu(), direct[k].cpu()) and torch.equal(after[k].cpu(), direct[k].cpu()), k
    assert not before["rot"].is_cuda                                                        # and rot on the host, as the reference


def test_forward_do_loss_feeds_pose_loss():
    """The validation step end to end: forward(do_loss=True) -> PoseLoss, everything on the device, finite terms."""
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig
    data, z = _e2e()
    _, gt = R.make_inputs(B=4, P=256, seed=60)
    net = PoseNet(PoseNetConfig(), seed=0, dtype=torch.float32).cuda()
    pred = net(data, "cuda", do_loss=True)
    loss, det = PoseLoss()(pred, tensors(gt), return_details=True)
    ref = R.pose_loss_ref({k: v.float().cpu().numpy() for k, v in pred.items() if k != "mask"}, gt)
    err = rel(det["terms"].cpu().numpy(), ref["terms"])
    print(f"forward(do_loss=True) -> PoseLoss vs restatement on the same predictions: {err:.2e}")
    assert err < 1e-11 and all(torch.isfinite(v) for v in loss.values())
