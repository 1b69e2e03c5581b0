"""GPU: ConvPnPNet's flat_op (avg / avg-max / avg-max-min pooling), mask_attention_type='mul' and every r_type, against the
goldens scripts/gen_golden_pnp_flags.py captured from the reference's own classes (ConvPnPNet, get_rot_mat +
pose_from_pred_centroid_z, PoseNet.forward).  Reads tests/golden only; tolerances as tests/test_hip_modules.py,
tests/test_hip_ops.py::test_pose_tail_golden, tests/test_hip_posenet.py and tests/test_grouped_launch.py."""
import functools
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SPLIT = "split"
MODES = {torch.float32: dict(dtype=torch.float32), SPLIT: dict(dtype=torch.float32, split_gemm=True), torch.float16: dict(dtype=torch.float16)}
E2E = {
    "avgmaxmin": dict(flat_op="avg-max-min"),
    "mul": dict(mask_attention_type="mul"),
    "ego_rot6d": dict(r_type="ego_rot6d"),
    "allo_quat": dict(r_type="allo_quat"),
    "euler": dict(r_type="euler"),
    "avg_mul_ego_quat": dict(flat_op="avg", mask_attention_type="mul", r_type="ego_quat"),
}


@functools.lru_cache(maxsize=1)
def _base_sd():
    from givepose_amd import PoseNetConfig, synth
    return {k: T(v) for k, v in synth.synth_state_dict(PoseNetConfig(), 0).items()}


def _net(mode, use_graph=False, **kw):
    """PoseNet(cfg) with the seed-0 synthetic weights: the default configuration's tensors where the shapes agree (every one
    but fc1 / fc1_z / fc_r), the rest drawn for this configuration -- what PoseNet(cfg, seed=0) holds, without redrawing the trunk."""
    from givepose_amd import PoseNet, PoseNetConfig, synth
    cfg = PoseNetConfig(**kw)
    base = _base_sd()
    sd = {k: base[k] if k in base and tuple(base[k].shape) == tuple(s) else T(synth.synth_tensor(k, s, 0))
          for k, s in synth.param_manifest(cfg).items()}
    net = PoseNet(cfg, use_graph=use_graph, **MODES[mode])
    net.load_state_dict(sd, strict=True)
    return net.cuda()


def _check(got, exp, dt, tol32, rel16, what):
    err = float(np.abs(got - exp).max())
    scale = float(np.abs(exp).max())
    print(f"{what} {dt}: max abs err {err:.3e} (output scale {scale:.3e})")
    if dt != torch.float16:
        assert err < tol32, (what, err)
    else:
        assert err < rel16 * max(scale, 1.0), (what, err)


# ------------------------------------------------------------------------------------------------ ConvPnPNet module
@pytest.fixture(scope="module")
def pnp_inputs(golden):
    z = golden("pnp_flags_inputs")
    r = np.random.Generator(np.random.Philox(key=[0, int(z["x_seed"])]))
    x = r.uniform(-0.8, 0.8, (2, 5, 64, 64)).astype(np.float32)
    assert zlib.crc32(x.tobytes()) == int(z["x_crc"])
    return T(x).cuda(), T(z["mask"]).cuda()


@pytest.mark.parametrize("dt", [torch.float32, SPLIT, torch.float16])
@pytest.mark.parametrize("mask_type", ["none", "mul"])
@pytest.mark.parametrize("flat_op", ["flatten", "avg", "avg-max", "avg-max-min"])
def test_conv_pnp_golden(golden, pnp_inputs, flat_op, mask_type, dt):
    from givepose_amd import synth
    z = golden(f"pnp_flags_conv_{flat_op.replace('-', '_')}_{mask_type}")
    x, mask = pnp_inputs
    net = _net(dt, flat_op=flat_op, mask_attention_type=mask_type)
    data = {k: T(v).cuda() for k, v in synth.synth_batch(2, seed=5).items()}
    rot, t = net.run_pnp(x, data, mask=mask if mask_type == "mul" else None)
    _check(rot.cpu().numpy(), z["rot"], dt, 1e-4, 2e-2, f"pnp {flat_op} {mask_type} rot")
    _check(t.cpu().numpy(), z["t"], dt, 1e-4, 2e-2, f"pnp {flat_op} {mask_type} t")


def test_run_pnp_mul_needs_mask(pnp_inputs):
    from givepose_amd import synth
    net = _net(torch.float32, mask_attention_type="mul")
    data = {k: T(v).cuda() for k, v in synth.synth_batch(2, seed=5).items()}
    with pytest.raises(ValueError):
        net.run_pnp(pnp_inputs[0], data)


# ------------------------------------------------------------------------------------------------ pose tail, every r_type
@pytest.mark.parametrize("ds", ["CAMERA_Real", "wild6d"])
@pytest.mark.parametrize("r_type", ["allo_rot6d", "ego_rot6d", "allo_rot6d_sym", "allo_rot6d_sym_y", "allo_rot6d_y", "allo_rot6d_z",
                                    "allo_rot6d_x", "allo_quat", "ego_quat", "euler"])
def test_pose_tail_rt_golden(golden, r_type, ds):
    from givepose_amd import ops
    from givepose_amd.config import ROT_TYPES
    z = golden("pnp_flags_pose_decode_" + ds)
    rd, kind, is_allo = ROT_TYPES[r_type]
    pr, pt = z[r_type + "__pred_rot"], z["pred_t"]
    B = pr.shape[0]
    # identity-like heads: the tail's fc outputs are the golden pred_rot / pred_t
    h, hz = torch.zeros(B, 256), torch.zeros(B, 256)
    h[:, :rd] = T(pr)
    h[:, rd:rd + 2] = T(pt[:, :2])
    hz[:, 0] = T(pt[:, 2])
    wr, wt_, wz = torch.zeros(rd, 256), torch.zeros(2, 256), torch.zeros(1, 256)
    for i in range(rd):
        wr[i, i] = 1
    wt_[0, rd] = wt_[1, rd + 1] = 1
    wz[0, 0] = 1
    W = {"fc_r.w": wr.cuda(), "fc_r.b": torch.zeros(rd).cuda(), "fc_t.w": wt_.cuda(), "fc_t.b": torch.zeros(2).cuda(),
         "fc_z.w": wz.cuda(), "fc_z.b": torch.zeros(1).cuda()}
    outs = {k: torch.empty(B, n, device="cuda") for k, n in (("pred_rot", rd), ("pred_t", 3), ("rot_allo", 9), ("rot_ego", 9), ("trans", 3))}
    cu = lambda k: T(z[k]).cuda()
    ops.pose_tail_rt(h.cuda(), hz.cuda(), 256, W, cu("cam_K"), cu("bbox_center"), cu("resize_ratio"), cu("roi_wh"), ds == "wild6d", True,
                     rd, kind, is_allo, outs, B)
    assert np.array_equal(outs["pred_rot"].cpu().numpy(), pr)
    assert np.abs(outs["rot_allo"].cpu().numpy().reshape(B, 3, 3) - z[r_type + "__rot_allo"]).max() < 2e-6
    assert np.abs(outs["rot_ego"].cpu().numpy().reshape(B, 3, 3) - z[r_type + "__rot"]).max() < 2e-6
    tr = z[r_type + "__trans"]
    assert np.abs(outs["trans"].cpu().numpy() - tr).max() < 1e-5 * max(1.0, np.abs(tr).max())


# ------------------------------------------------------------------------------------------------ bitwise identities
def test_pose_tail_is_the_allo_rot6d_call():
    from givepose_amd import ops
    from givepose_amd._lib import ROT_6D
    g = torch.Generator().manual_seed(11)
    B = 37
    rn = lambda *s: torch.randn(*s, generator=g).cuda()
    h, hz = rn(B, 256) * 0.3, rn(B, 256) * 0.3
    W = {"fc_r.w": rn(6, 256) * 0.1, "fc_r.b": rn(6), "fc_t.w": rn(2, 256) * 0.01, "fc_t.b": rn(2) * 0.1, "fc_z.w": rn(1, 256) * 0.01,
         "fc_z.b": rn(1).abs() + 1}
    cam = torch.tensor([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]]).expand(B, 3, 3).contiguous().cuda()
    bc, rr, wh = rn(B, 2) * 50 + 300, rn(B).abs() + 0.5, rn(B, 2).abs() * 100 + 50
    for wild in (False, True):
        a = {k: torch.full((B, n), float("nan"), device="cuda") for k, n in (("rot6d", 6), ("pred_t", 3), ("rot_allo", 9), ("rot_ego", 9), ("trans", 3))}
        b = {k: torch.full((B, n), float("nan"), device="cuda") for k, n in (("pred_rot", 6), ("pred_t", 3), ("rot_allo", 9), ("rot_ego", 9), ("trans", 3))}
        ops.pose_tail(h, hz, 256, W, cam, bc, rr, wh, wild, True, a, B)
        ops.pose_tail_rt(h, hz, 256, W, cam, bc, rr, wh, wild, True, 6, ROT_6D, True, b, B)
        a["pred_rot"] = a.pop("rot6d")
        for k in a:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype,cout", [(torch.float16, 128), (torch.float16, 256), (torch.float16, 64), (torch.float32, 128)])
def test_pnp_conv1_masked_bitwise(dtype, cout):
    """An all-ones mask gives gp_pnp_conv1's bits; a binary mask gives the bits of gp_pnp_conv1 on the input premultiplied on the host
    (the mask is applied in fp32 before anything else).  fp16 Cout 128 / 256: the MFMA form; fp16 Cout 64 and fp32: the generic form."""
    from givepose_amd import ops
    g = torch.Generator().manual_seed(12)
    B, R = 3, 64
    xyz4 = torch.randn(B * R * R, 4, generator=g).cuda()
    c2 = torch.randn(B, 2, R, R, generator=g).cuda()
    w = (torch.randn(45, cout, generator=g) * 0.2).cuda()
    mask = (torch.rand(B, 1, R, R, generator=g) > 0.4).float().cuda()
    y0, y1, y2, y3 = (torch.empty(B, R // 2, R // 2, cout, dtype=dtype, device="cuda") for _ in range(4))
    ops.pnp_conv1(xyz4, c2, w, y0, B, R)
    ops.pnp_conv1_masked(xyz4, c2, torch.ones_like(mask), w, y1, B, R)
    assert torch.equal(y0, y1)
    ops.pnp_conv1_masked(xyz4, c2, mask, w, y2, B, R)
    ops.pnp_conv1((xyz4 * mask.reshape(-1, 1)).contiguous(), (c2 * mask).contiguous(), w, y3, B, R)
    assert torch.equal(y2, y3)
    assert not torch.equal(y0, y2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_pool_mmm(dtype, k):
    from givepose_amd import ops
    g = torch.Generator().manual_seed(13)
    B = 7
    x = torch.randn(B, 64, 128, generator=g).to(dtype)
    out = torch.empty(B, 128 * k, dtype=dtype, device="cuda")
    ops.pool_mmm(x.cuda(), out, k)
    xf = x.float()
    ref = torch.cat([xf.mean(1), xf.amax(1), xf.amin(1)], 1)[:, :128 * k]
    got = out.float().cpu()
    tol = 1e-3 if dtype == torch.float16 else 1e-6
    assert float((got - ref.to(dtype).float()).abs().max()) <= tol
    assert torch.equal(got[:, 128:], ref[:, 128:].to(dtype).float())      # max / min are exact


# ------------------------------------------------------------------------------------------------ fc1 dispatch at K = 128 k
@pytest.mark.parametrize("mode", [torch.float16, torch.float32, SPLIT])
@pytest.mark.parametrize("flat_op", ["avg", "avg-max", "avg-max-min"])
def test_fc1_pooled_dispatch(flat_op, mode):
    """fc1 || fc1_z at K = 128 / 256 / 384 for 1, 4 and 64 crops: the automatic choice must pass over the M <= 8 row-vector kernel
    (variant 23 needs K % 512 == 0) and every kernel it takes must give the product."""
    from givepose_amd import ops
    from givepose_amd._lib import EPI_NONE
    net = _net(mode, flat_op=flat_op)
    W = net._pack(torch.device("cuda"))
    K = {"avg": 128, "avg-max": 256, "avg-max-min": 384}[flat_op]
    sd = {k: v.cpu() for k, v in net.state_dict().items() if k.startswith("pnp_net.fc1")}
    w = torch.cat([sd["pnp_net.fc1.weight"], sd["pnp_net.fc1_z.weight"]], 0)
    dt = torch.float16 if mode == torch.float16 else torch.float32
    g = torch.Generator().manual_seed(14)
    for B in (1, 4, 64):
        x = torch.rand(B, K, generator=g).to(dt)
        out = torch.empty(B, 2048, dtype=dt, device="cuda")
        ops.gemm(x.cuda(), W["pnp.fc1_w"], out, bias=W["pnp.fc1_b"], epilogue=EPI_NONE)
        torch.cuda.synchronize()
        ref = x.double() @ w.to(dt).double().t() + torch.cat([sd["pnp_net.fc1.bias"], sd["pnp_net.fc1_z.bias"]]).double()
        err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
        print(f"fc1 {flat_op} {mode} B{B}: rel err {err:.2e}")
        assert err < (5e-3 if dt == torch.float16 else 1e-5), (B, err)


# ------------------------------------------------------------------------------------------------ end to end
def _e2e_batch(z):
    from givepose_amd import synth
    npb = synth.synth_batch(4, seed=int(z["batch_seed"]))
    assert zlib.crc32(np.ascontiguousarray(npb["roi_img"]).tobytes()) == int(z["roi_img_crc"])
    return {k: T(v) for k, v in npb.items()}


@pytest.mark.parametrize("mode", [torch.float32, SPLIT, torch.float16])
@pytest.mark.parametrize("tag", list(E2E))
def test_e2e_golden(golden, tag, mode):
    z = golden("pnp_flags_e2e_" + tag)
    net = _net(mode, **E2E[tag])
    out = net.forward_device(_e2e_batch(z), "cuda")
    err = {k: float(np.abs(out[k].float().cpu().numpy() - z[k]).max()) for k in ("rot", "trans", "size", "pred_rot", "pred_t")}
    print(f"e2e {tag} {mode}", err)
    assert out["pred_rot"].shape == z["pred_rot"].shape
    assert (out["rot6d"] is None) == (z["pred_rot"].shape[1] == 4)
    if mode == torch.float16:
        assert err["rot"] < 3e-2 and err["size"] < 3e-2
        assert err["trans"] < 3e-2 * max(1.0, float(np.abs(z["trans"]).max()))
    else:
        assert err["rot"] < 1e-4 and err["trans"] < 1e-4 and err["size"] < 1e-4, err
        assert err["pred_rot"] < 1e-4 and err["pred_t"] < 1e-4, err


def test_forward_keys_unchanged(golden):
    z = golden("pnp_flags_e2e_allo_quat")
    out = _net(torch.float32, **E2E["allo_quat"])(_e2e_batch(z), "cuda")
    assert set(out) == {"rot", "trans", "size", "mask", "nocs_coor", "ivfc_coor"}
    assert np.abs(out["rot"].numpy() - z["rot"]).max() < 1e-4


# ------------------------------------------------------------------------------------------------ hipGraph + ragged groups
def test_graph_groups_pooled_mul():
    """avg-max-min + mul under use_graph=True with groups [2, 1, 3] against three separate forwards (fp32 mode: 5e-5, as
    tests/test_grouped_launch.py bounds two schedules of the same frames)."""
    from givepose_amd import synth
    kw = dict(flat_op="avg-max-min", mask_attention_type="mul")
    groups = [2, 1, 3]
    frames = [{k: T(v) for k, v in synth.synth_batch(n, seed=300 + i).items()} for i, n in enumerate(groups)]
    both = {k: torch.cat([f[k] for f in frames], 0) for k in frames[0]}
    keys = ("rot", "trans", "size", "nocs_coor", "ivfc_coor", "pred_rot", "pred_t")
    graph = _net(torch.float32, use_graph=True, **kw)
    for _ in range(3):          # eager warm-up, capture + replay, replay
        og = {k: v.clone() for k, v in graph.forward_device(both, groups=groups).items() if k in keys}
    alone = _net(torch.float32, **kw)
    i = 0
    for f, n in zip(frames, groups):
        oa = alone.forward_device(f)
        d = {k: float((og[k][i:i + n] - oa[k]).abs().max()) for k in keys}
        print(f"graph+groups vs alone, frame of {n}:", d)
        assert all(v < 5e-5 for v in d.values()), d
        i += n
