"""GPU: the loss-gradient family -- gpg_pose_loss_grad (PoseLoss.value_and_grad, PoseLoss.with_grad), gpg_pose_decode_train_backward
(pose_decode_train_backward) and PoseNet.head_grads -- against the float64 restatement tests/pose_loss_grad_ref.py and the fixtures
scripts/gen_golden_pose_loss_grad.py recorded from the reference under torch autograd.

Bounds.  The small float64 gradients against the restatement: 1e-11 of max|g| (the argument of tests/test_pose_loss_gpu.py: the
kernel reproduces every element, only the order of the P-point sum differs).  Every float32 element: 2^-24 |ref| + 1e-12 max|ref|,
one rounding of the float64 value.  Against the reference's float64 fixture the restatement's own bound (G.F64_BOUND, derived in
tests/test_pose_loss_grad_cpu.py) is added.  The decode backward against its float64 fixture: G.DECODE_BOUND times the conditioning,
off and on the optical axis, as in the CPU test."""
import functools

import numpy as np
import pytest
import torch

import pose_loss_grad_ref as G
import pose_loss_ref as R

pytestmark = pytest.mark.gpu
T = torch.from_numpy
MAPS = ("nocs_coor", "ivfc_coor")
SENTINEL = -7.25
EXTRA = {"p65": dict(B=2, P=65, seed=80, sym="cycle", masks=("soft", "binary")), "p257": dict(B=2, P=257, seed=81, sym="all", masks=("binary", "full"))}


def tensors(d, device=None):
    return {k: (T(np.ascontiguousarray(v)).to(device) if device else T(np.ascontiguousarray(v))) for k, v in d.items()}


def cfg_of(cfg):
    from givepose_amd import LossConfig
    return LossConfig(**cfg)


@functools.lru_cache(maxsize=None)
def case(name):
    """(pred, data, cfg) of a fixture case or of one of the two extra shapes whose P ends in a partial wave."""
    if name in EXTRA:
        return (*R.make_inputs(**EXTRA[name]), dict(R.DEFAULTS))
    return (*R.case_inputs(name), R.case_cfg(name))


@functools.lru_cache(maxsize=None)
def restatement(name, variant):
    pred, data, cfg = case(name)
    return G.pose_loss_grad_ref(pred, data, gout=None if variant == "ones" else G.make_gout(), **cfg)


def run(name, gout=None, host_data=True):
    """value_and_grad on the device -> (loss dict, the five gradients and small64 on the host)."""
    from givepose_amd import PoseLoss
    pred, data, cfg = case(name)
    loss, g, det = PoseLoss(cfg_of(cfg)).value_and_grad(tensors(pred, "cuda"), tensors(data, None if host_data else "cuda"),
                                                       gout=None if gout is None else T(np.asarray(gout, np.float64)), return_details=True)
    torch.cuda.synchronize()
    assert list(g) == list(G.GRAD_KEYS) and all(v.dtype == torch.float32 and v.is_cuda for v in g.values())
    out = {k: v.cpu().numpy() for k, v in g.items()}
    out["small64"] = det["small64"].cpu().numpy()
    return loss, out


def one_rounding(got32, ref, extra=0.0):
    """Every float32 element within 2^-24 |ref| + (1e-12 + extra) max|ref|; -> the worst excess ratio, for the printout."""
    ref = np.asarray(ref, np.float64)
    tol = 2.0 ** -24 * np.abs(ref) + (1e-12 + extra) * np.abs(ref).max()
    err = np.abs(np.float64(got32) - ref)
    assert np.all(err <= tol), float((err - tol).max())
    return float(np.max(err / np.maximum(tol, 1e-300)))


def check_against(g, ref, what, extra=0.0):
    B = ref["rot"].shape[0]
    small_ref = np.concatenate([ref["rot"].reshape(B, 9), ref["trans"], ref["size"]], 1)
    figs = {}
    for k, sl in (("rot", slice(0, 9)), ("trans", slice(9, 12)), ("size", slice(12, 15))):
        r = small_ref[:, sl]
        m = np.abs(r).max()
        figs[k] = float(np.abs(g["small64"][:, sl] - r).max() / (m if m > 0 else 1.0))
        assert figs[k] < 1e-11 + extra, (what, k, figs[k])
        assert np.array_equal(g[k].reshape(B, -1).view(np.uint32), g["small64"][:, sl].astype(np.float32).view(np.uint32)), (what, k)   # rounded once
    for k in G.GRAD_KEYS:
        figs[k + "32"] = one_rounding(g[k], ref[k], extra)
        assert np.all(g[k][ref[k] == 0] == 0), (what, k)                     # exact zeros where the restatement has them
        assert np.all(np.isfinite(g[k]))
    print(f"{what}: small float64 |diff| / max|g| " + " ".join(f"{k} {figs[k]:.2e}" for k in ("rot", "trans", "size")) +
          "; float32 worst error / allowance " + " ".join(f"{k} {figs[k + '32']:.2f}" for k in G.GRAD_KEYS))


@pytest.mark.parametrize("name", list(R.CASES) + list(EXTRA))
def test_gradients_against_the_restatement(name):
    from givepose_amd import PoseLoss
    pred, data, cfg = case(name)
    loss, g = run(name)
    check_against(g, restatement(name, "ones"), name)
    plain = PoseLoss(cfg_of(cfg))(tensors(pred, "cuda"), tensors(data))          # the loss dict is the one __call__ returns
    assert list(loss) == list(R.KEYS) and all(torch.equal(loss[k], plain[k]) and loss[k].dim() == 0 for k in R.KEYS)
    ref = restatement(name, "ones")
    for k, mk in (("nocs_coor", "roi_mask_output"), ("ivfc_coor", "roi_ivfc_mask_output")):
        assert np.all(g[k][np.broadcast_to(data[mk] == 0, g[k].shape)] == 0)      # masked-out pixels, the all-zero crops
    eq = R.CASES.get(name, {}).get("equal")
    if eq is not None:                                                             # pred == gt (sign(0) = 0), or the clipped angle crop
        assert np.all(g["rot"][eq] == 0) and np.all(ref["rot"][eq] == 0)


@pytest.mark.parametrize("name", list(R.CASES))
def test_gradients_against_the_reference_fixture(name):
    """Both the unweighted sum and the non-uniform gout against the reference's float64 autograd."""
    pred, data, cfg, z = G.load_grad_fixture(name)
    pix = G.sample_pixels(name, pred["rot"].shape[0])
    for v, w in (("ones", None), ("gout", G.make_gout())):
        loss, g = run(name, gout=w)
        check_against(g, restatement(name, v), f"{name} {v}")
        for k in ("rot", "trans", "size"):
            one_rounding(g[k], z[f"{v}__{k}"], G.F64_BOUND)
        for k in MAPS:
            s, tot, ab = G.sampled(np.float64(g[k]), pix)
            one_rounding(s, z[f"{v}__{k}_s"], G.F64_BOUND)
            # the whole map: float32 roundings of every element and the restatement's bound, against the sum of |g|
            tol = (2.0 ** -24 + G.F64_BOUND + 1e-12) * z[f"{v}__{k}_abs"]
            assert np.all(np.abs(tot - z[f"{v}__{k}_sum"]) <= tol) and np.all(np.abs(ab - z[f"{v}__{k}_abs"]) <= tol), (name, v, k)
        if v == "gout":
            assert np.all(g["size"] == 0) and np.all(z["gout__size"] == 0)


def test_a_zero_in_gout_leaves_that_term_exactly_out():
    _, ones = run("b5")
    _, no_size = run("b5", gout=[1, 1, 0, 1, 1, 1])
    assert np.all(no_size["size"] == 0)
    for k in ("rot", "trans", "nocs_coor", "ivfc_coor"):
        assert ones[k].tobytes() == no_size[k].tobytes(), k                       # gout of ones is the null pointer's result
    _, r1 = run("b5", gout=[1, 0, 0, 0, 0, 0])
    _, no_pm = run("b5", gout=[1, 1, 1, 0, 1, 1])
    assert r1["rot"].tobytes() == no_pm["rot"].tobytes() and not np.array_equal(r1["rot"], ones["rot"])
    assert np.all(r1["nocs_coor"] == 0) and np.all(r1["ivfc_coor"] == 0) and np.all(r1["trans"] == 0)


def test_bitwise_repeatable_and_host_equals_device_inputs():
    a, b, c = run("b5", gout=G.make_gout())[1], run("b5", gout=G.make_gout())[1], run("b5", gout=G.make_gout(), host_data=False)[1]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


def _guarded(shape, dtype=torch.float32):
    """A buffer of `shape` with 64 sentinel elements on either side, 16-byte aligned -> (whole, view)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 128,), SENTINEL, device="cuda", dtype=dtype)
    return whole, whole[64:64 + n].view(shape)


def test_sentinels_around_every_output_buffer():
    from givepose_amd import PoseLoss, _lib
    for name in ("b5", "p65"):
        pred, data, cfg = case(name)
        pl = PoseLoss(cfg_of(cfg))
        a, dims = pl._inputs(tensors(pred, "cuda"), tensors(data))
        out64, out32, record, slabs = pl._forward(a, dims)
        B, P, dev = dims
        bufs = {"rot": _guarded((B, 3, 3)), "trans": _guarded((B, 3)), "size": _guarded((B, 3)), "nocs_coor": _guarded((B, 3, 64, 64)),
                "ivfc_coor": _guarded((B, 3, 64, 64)), "small": _guarded((B, _lib.GPG_SMALL), torch.float64)}
        assert all(v.data_ptr() % 16 == 0 for _, v in bufs.values())
        c = cfg_of(cfg)
        _lib.check(_lib.load().gpg_pose_loss_grad(*[t.data_ptr() for t in a], slabs.data_ptr(), record.data_ptr(), 0, B, P, 64, int("sym" in c.r_type),
                                                  int(c.r_loss == "angle"), int(c.pose_loss_type == "smoothl1"), c.rot_1_w, c.tran_w, c.size_w,
                                                  c.prop_pm_w, c.coor_w, *[bufs[k][1].data_ptr() for k in G.GRAD_KEYS], bufs["small"][1].data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream), "gpg_pose_loss_grad")
        torch.cuda.synchronize()
        _, g = run(name)
        for k, (whole, view) in bufs.items():
            assert torch.all(whole[:64] == SENTINEL) and torch.all(whole[-64:] == SENTINEL), (name, k)
            assert not torch.any(view == SENTINEL), (name, k)                     # and every element was written
            assert view.cpu().numpy().tobytes() == g["small64" if k == "small" else k].tobytes(), (name, k)


# ------------------------------------------------------------------------------------------------ the decode backward
@pytest.mark.parametrize("name", list(R.DECODE_CASES))
def test_pose_decode_train_backward(name):
    from givepose_amd import _lib, loss
    inp, extra, z = G.load_decode_grad_fixture()
    r_type, t_type = R.DECODE_CASES[name]
    kw = dict(t_site=t_type == "site", is_allo="allo" in r_type)
    Ra = np.float32(G.rot6d_to_mat_ref(extra["rot6d"]))
    dev = tensors({**inp, "rot_allo": Ra, **extra}, "cuda")
    out, g64 = loss.pose_decode_train_backward(**dev, return_details=True, **kw)
    g64 = g64.cpu().numpy()
    got = {"rot_allo": g64[:, :9].reshape(4, 3, 3), "pred_t": g64[:, 9:12], "rot6d": g64[:, 12:]}
    ref = G.decode_train_backward_ref(extra["g_rot_ego"], extra["g_trans"], rot6d=extra["rot6d"], **kw, **{**inp, "rot_allo": Ra})
    off, on = G.DECODE_BOUND * G.DECODE_COND_OFF, G.DECODE_BOUND * G.DECODE_COND_ON
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    figs = {"rot6d": rel(got["rot6d"], z[name + "__rot6d"]), "on": rel(got["pred_t"][:1], z[name + "__pred_t"][:1]),
            "off": rel(got["pred_t"][1:], z[name + "__pred_t"][1:]), "rot_allo": rel(got["rot_allo"], ref["rot_allo"])}
    print(f"decode backward {name}: float64 vs the reference's float64 fixture {figs}")
    assert figs["rot6d"] < off and figs["off"] < off and figs["on"] < on and figs["rot_allo"] < off
    for k in G.DECODE_KEYS:                                # float32 outputs: the float64 ones rounded once
        assert np.array_equal(out[k].cpu().numpy().view(np.uint32), got[k].astype(np.float32).view(np.uint32)), k
    if not kw["t_site"]:
        assert np.all(got["pred_t"][:, :2] == 0)
    if not kw["is_allo"]:
        assert np.array_equal(got["rot_allo"], np.float64(extra["g_rot_ego"]))
    # without rot6d: rot_allo's float32 values are the input, the raw vector's gradient is left out
    out2, g2 = loss.pose_decode_train_backward(**{k: v for k, v in dev.items() if k != "rot6d"}, return_details=True, **kw)
    ref2 = G.decode_train_backward_ref(extra["g_rot_ego"], extra["g_trans"], **kw, **{**inp, "rot_allo": Ra})
    assert list(out2) == ["rot_allo", "pred_t"] and np.all(g2[:, 12:].cpu().numpy() == 0)
    assert rel(g2[1:, 9:12].cpu().numpy(), ref2["pred_t"][1:]) < off and rel(g2[:1, 9:12].cpu().numpy(), ref2["pred_t"][:1]) < on
    # sentinels: the three float32 outputs and the float64 record
    bufs = {"rot_allo": _guarded((4, 3, 3)), "pred_t": _guarded((4, 3)), "rot6d": _guarded((4, 6)), "g64": _guarded((4, _lib.GPG_DECODE), torch.float64)}
    p = lambda k: dev[k].contiguous().data_ptr()
    _lib.check(_lib.load().gpg_pose_decode_train_backward(p("g_rot_ego"), p("g_trans"), p("pred_t"), p("rot_allo"), p("cam_K"), p("bbox_center"),
                                                          p("resize_ratio"), p("roi_wh"), p("rot6d"), int(kw["t_site"]), int(kw["is_allo"]), 1e-4, 4,
                                                          *[bufs[k][1].data_ptr() for k in ("rot_allo", "pred_t", "rot6d", "g64")],
                                                          torch.cuda.current_stream().cuda_stream), "gpg_pose_decode_train_backward")
    torch.cuda.synchronize()
    for k, (whole, view) in bufs.items():
        assert torch.all(whole[:64] == SENTINEL) and torch.all(whole[-64:] == SENTINEL) and not torch.any(view == SENTINEL), k
    assert bufs["g64"][1].cpu().numpy().tobytes() == g64.tobytes()                 # two calls, equal bits


# ------------------------------------------------------------------------------------------------ autograd
def test_with_grad_fills_grad_bitwise_equal_to_value_and_grad():
    from givepose_amd import PoseLoss
    pred, data, cfg = case("b5")
    pl = PoseLoss(cfg_of(cfg))
    combos = ((lambda d: sum(d.values()), [1, 1, 1, 1, 1, 1]), (lambda d: sum(d.values()) / 4, [0.25] * 6),
              (lambda d: 2 * d["Rot1"] + d["nocs_coor"], [2, 0, 0, 0, 1, 0]))
    for fn, gout in combos:
        leaves = {k: v.requires_grad_(True) for k, v in tensors(pred, "cuda").items()}
        d = pl.with_grad(leaves, tensors(data))
        assert list(d) == list(R.KEYS) and all(v.dim() == 0 and v.requires_grad and v.dtype == torch.float32 for v in d.values())
        fn(d).backward()
        _, want = pl.value_and_grad(tensors(pred, "cuda"), tensors(data), gout=T(np.asarray(gout, np.float64)))
        plain = pl(tensors(pred, "cuda"), tensors(data))
        torch.cuda.synchronize()
        for k in G.GRAD_KEYS:
            assert leaves[k].grad is not None and torch.equal(leaves[k].grad.view(torch.int32), want[k].view(torch.int32)), (gout, k)
        assert all(torch.equal(d[k].detach(), plain[k]) for k in R.KEYS)
        assert not plain["Rot1"].requires_grad                                    # __call__ keeps its no_grad behaviour


# ------------------------------------------------------------------------------------------------ PoseNet.head_grads
@functools.lru_cache(maxsize=1)
def _e2e():
    import zlib

    from givepose_amd import synth
    z = np.load(R.GOLDEN + "/pose_loss_e2e.npz")
    npb = synth.synth_batch(4, seed=int(z["batch_seed"]))
    r = np.random.Generator(np.random.Philox(key=[int(z["mask_seed"]), 4]))
    npb["roi_mask_deform"] = (r.random(npb["roi_mask"].shape) > 0.4).astype(np.float32)
    assert zlib.crc32(np.ascontiguousarray(npb["roi_img"]).tobytes()) == int(z["roi_img_crc"])
    _, gt = R.make_inputs(B=4, P=256, seed=60)
    assert not set(npb) & set(gt)
    return npb, gt


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_head_grads(dtype):
    """Bitwise equal to composing the public pieces on the forward's own outputs, and within the bounds of the restatement evaluated
    on those outputs.  No comparison with a reference end-to-end gradient: L1 gradients are sign functions of quantities the fp16
    forward perturbs."""
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, loss
    from givepose_amd.config import ROT_TYPES
    npb, gt = _e2e()
    data = {**tensors(npb), **tensors(gt)}
    net = PoseNet(PoseNetConfig(), seed=0, dtype=dtype).cuda()
    cfg, pl, w = net.cfg, PoseLoss(), G.make_gout()
    assert ROT_TYPES[cfg.r_type][1] == 0
    res = net.head_grads(data, pl, "cuda", gout=T(w))
    assert list(res) == ["loss", "output", "grads"] and list(res["grads"]) == ["rot6d", "pred_t", "size", "nocs_coor", "ivfc_coor"]
    # the public pieces
    out = net(data, "cuda", do_loss=True)
    raw = {k: v.clone() for k, v in net.forward_device({**data, "roi_mask": data["roi_mask_deform"]}, "cuda").items() if k in ("pred_rot", "pred_t", "rot_allo")}
    terms, g = pl.value_and_grad(out, data, gout=T(w))
    kw = dict(t_site=cfg.t_type == "site", is_allo=ROT_TYPES[cfg.r_type][2], eps=1e-4)
    geo = {k: data[k] for k in ("cam_K", "bbox_center", "resize_ratio", "roi_wh")}
    dec = loss.pose_decode_train_backward(g["rot"], g["trans"], raw["pred_t"], raw["rot_allo"], rot6d=raw["pred_rot"], **geo, **kw)
    torch.cuda.synchronize()
    want = {"rot6d": dec["rot6d"], "pred_t": dec["pred_t"], "size": g["size"], "nocs_coor": g["nocs_coor"], "ivfc_coor": g["ivfc_coor"]}
    for k, v in want.items():
        assert res["grads"][k].dtype == torch.float32 and torch.equal(res["grads"][k].view(torch.int32), v.view(torch.int32)), k
    for k in out:
        assert torch.equal(res["output"][k], out[k]), k
    assert all(torch.equal(res["loss"][k], terms[k]) for k in R.KEYS)
    # the restatement on those outputs
    pred_np = {k: out[k].float().cpu().numpy() for k in G.GRAD_KEYS}
    ref = G.pose_loss_grad_ref(pred_np, gt, gout=w)
    got = {k: v.cpu().numpy() for k, v in res["grads"].items()}
    for k in ("size", "nocs_coor", "ivfc_coor"):
        one_rounding(got[k], ref[k])
    one_rounding(g["rot"].cpu().numpy(), ref["rot"])
    one_rounding(g["trans"].cpu().numpy(), ref["trans"])
    dref = G.decode_train_backward_ref(g["rot"].cpu().numpy(), g["trans"].cpu().numpy(), raw["pred_t"].cpu().numpy(), raw["rot_allo"].cpu().numpy().reshape(4, 3, 3),
                                       rot6d=raw["pred_rot"].float().cpu().numpy(), **{k: v.numpy() for k, v in geo.items()}, **kw)
    cond = G.DECODE_BOUND * G.DECODE_COND_ON               # the synthetic crops may sit anywhere: the on-axis conditioning covers them
    print(f"head_grads {dtype}: rot6d", one_rounding(got["rot6d"], dref["rot6d"], cond), "pred_t", one_rounding(got["pred_t"], dref["pred_t"], cond))
    assert all(np.all(np.isfinite(v)) for v in got.values()) and np.any(got["rot6d"] != 0) and np.any(got["pred_t"] != 0)
