"""GPU: the AttentionPnPNet pose head (PoseNetConfig.pnp_head='att') -- its kernels (row LayerNorm at C = 192, gp_attention64_hd,
gp_patchify_pnp), the module against att_pnp_module, PoseNet end to end against the goldens scripts/gen_golden_att_pnp.py captured
from the reference's own classes, the configs[3] combination at bs 32 under hipGraph against tests/att_pnp_ref.py, ragged groups, and
the dispatch of the head's fc launches.  Tolerances as tests/test_hip_ops.py::test_layernorm, tests/test_pnp_flags_gpu.py and
tests/test_hip_posenet.py::test_attention_encoder_variant_bs32_matches_oracle."""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SPLIT = "split"
MODES = {torch.float32: dict(dtype=torch.float32), SPLIT: dict(dtype=torch.float32, split_gemm=True), torch.float16: dict(dtype=torch.float16)}
E2E = {
    "att": dict(pnp_head="att"),
    "att_attenc": dict(pnp_head="att", nocsmap_encoder="att"),
    "att_ego_center": dict(pnp_head="att", r_type="ego_rot6d", t_type="center"),
}
TOL = {torch.float32: 2e-5, torch.float16: 4e-3}       # tests/test_hip_ops.py (relative to the output's largest magnitude)


def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))


@functools.lru_cache(maxsize=1)
def _base_sd():
    from givepose_amd import PoseNetConfig, synth
    return {k: T(v) for k, v in synth.synth_state_dict(PoseNetConfig(), 0).items()}


def _sd(cfg):
    """Seed-0 synthetic weights of cfg: the default configuration's tensors where names and shapes agree, the rest drawn by name --
    what PoseNet(cfg, seed=0) holds, without redrawing the trunk."""
    from givepose_amd import synth
    base = _base_sd()
    return {k: base[k] if k in base and tuple(base[k].shape) == tuple(s) else T(synth.synth_tensor(k, s, 0))
            for k, s in synth.param_manifest(cfg).items()}


def _net(mode, use_graph=False, **kw):
    from givepose_amd import PoseNet, PoseNetConfig
    cfg = PoseNetConfig(**kw)
    net = PoseNet(cfg, use_graph=use_graph, **MODES[mode])
    net.load_state_dict(_sd(cfg), strict=True)
    return net.cuda()


def _check(got, exp, dt, tol32, rel16, what):
    err = float(np.abs(got - exp).max())
    scale = float(np.abs(exp).max())
    print(f"{what} {dt}: max abs err {err:.3e} (output scale {scale:.3e})")
    if dt != torch.float16:
        assert err < tol32, (what, err)
    else:
        assert err < rel16 * max(scale, 1.0), (what, err)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("C", [192, 96, 320, 1536])
def test_layernorm_non_power_of_two(dt, C):
    """Widths whose 16-byte vector count is no power of two (192: 24 / 48 vectors) against a float64 F.layer_norm; 300 rows (a partial
    last workgroup) into a wider output (ldy) whose other columns must stay untouched.  fp32 C = 1536 (384 vectors) is refused."""
    from givepose_amd import ops
    from givepose_amd._lib import GivePoseHipError
    x = (_rnd(300, C, seed=35) * 2 + 0.5).to(dt).double()
    lw, lb = 1 + 0.1 * _rnd(C, seed=36), 0.1 * _rnd(C, seed=37)
    out = torch.full((300, C + 32), 7.0, dtype=dt, device="cuda")
    if dt == torch.float32 and C == 1536:
        with pytest.raises(GivePoseHipError, match="unsupported C"):
            ops.layernorm(x.to("cuda", dt), lw.cuda(), lb.cuda(), out, eps=1e-5, ldy=C + 32)
        return
    ops.layernorm(x.to("cuda", dt), lw.cuda(), lb.cuda(), out, eps=1e-5, ldy=C + 32)
    ref = F.layer_norm(x, (C,), lw.double(), lb.double(), 1e-5)
    err = _rel(out[:, :C], ref)
    print(f"layernorm C={C} {dt}: rel err {err:.2e}")
    assert err < TOL[dt]
    assert bool((out[:, C:] == 7.0).all())
    if dt == torch.float16:       # GP_IN_F32: fp32 rows in, fp16 out
        xf = (_rnd(300, C, seed=38) * 2 + 0.5)
        o16 = torch.empty(300, C, dtype=torch.float16, device="cuda")
        ops.layernorm(xf.cuda(), lw.cuda(), lb.cuda(), o16, eps=1e-5)
        assert _rel(o16, F.layer_norm(xf.double(), (C,), lw.double(), lb.double(), 1e-5)) < TOL[dt]


@pytest.mark.parametrize("dt,C", [(torch.float16, 100), (torch.float16, 2056)])
def test_layernorm_refuses_other_widths(dt, C):
    from givepose_amd import ops
    from givepose_amd._lib import GivePoseHipError
    x = torch.zeros(4, C, dtype=dt, device="cuda")
    with pytest.raises(GivePoseHipError, match="unsupported C"):
        ops.layernorm(x, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), torch.empty_like(x))


def _attention_ref(qkv, B, heads, hd):
    q, k, v = qkv.double().reshape(B, 64, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
    a = ((q * hd ** -0.5) @ k.transpose(-2, -1)).softmax(-1)
    return (a @ v).transpose(1, 2).reshape(B * 64, heads * hd)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_attention64_hd24(dt):
    from givepose_amd import ops
    B, H = 5, 8
    qkv = (_rnd(B * 64, 3 * H * 24, seed=41) * 1.5).to(dt)
    out = torch.full((B * 64, H * 24), float("nan"), dtype=dt, device="cuda")
    ops.attention64_hd(qkv.cuda(), out, B, H, 24)
    err = _rel(out, _attention_ref(qkv, B, H, 24))
    print(f"attention64_hd 24 {dt}: rel err {err:.2e}")
    assert err < TOL[dt]


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_attention64_hd32_is_attention64(dt):
    from givepose_amd import ops
    B, H = 3, 8
    qkv = (_rnd(B * 64, 3 * H * 32, seed=42) * 1.5).to(dt).cuda()
    a, b = (torch.full((B * 64, H * 32), float("nan"), dtype=dt, device="cuda") for _ in range(2))
    ops.attention64(qkv, a, B, H)
    ops.attention64_hd(qkv, b, B, H, 32)
    assert torch.equal(a, b)
    assert _rel(a, _attention_ref(qkv.cpu(), B, H, 32)) < TOL[dt]


def test_attention64_hd_refuses_other_head_dims():
    from givepose_amd import ops
    from givepose_amd._lib import GivePoseHipError
    qkv = torch.zeros(64, 3 * 8 * 16, device="cuda")
    with pytest.raises(GivePoseHipError, match="head_dim"):
        ops.attention64_hd(qkv, torch.empty(64, 128, device="cuda"), 1, 8, 16)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_patchify_pnp_bitwise(dt):
    from givepose_amd import ops
    B, R, P = 3, 64, 8
    xyz4 = _rnd(B * R * R, 4, seed=43).cuda()
    c2 = _rnd(B, 2, R, R, seed=44).cuda()
    out = torch.full((B * 64, 320), float("nan"), dtype=dt, device="cuda")
    ops.patchify_pnp(xyz4, c2, out, B, R, P)
    x = torch.cat([xyz4[:, :3].reshape(B, R, R, 3).permute(0, 3, 1, 2), c2], 1)          # (B, 5, R, R): PoseNet.py:196-197
    ref = x.reshape(B, 5, 8, P, 8, P).permute(0, 2, 4, 3, 5, 1).reshape(B * 64, P * P * 5)  # rows (b, py, px), k = (ky*P+kx)*5 + c
    assert torch.equal(out, ref.to(dt))


# ------------------------------------------------------------------------------------------------ AttentionPnPNet module
@pytest.fixture(scope="module")
def pnp_input(golden):
    z = golden("att_pnp_module")
    r = np.random.Generator(np.random.Philox(key=[0, int(z["x_seed"])]))
    x = r.uniform(-0.8, 0.8, (2, 5, 64, 64)).astype(np.float32)
    assert zlib.crc32(x.tobytes()) == int(z["x_crc"])
    return T(x).cuda()


@pytest.mark.parametrize("dt", [torch.float32, SPLIT, torch.float16])
def test_run_pnp_golden(golden, pnp_input, dt):
    from givepose_amd import synth
    z = golden("att_pnp_module")
    net = _net(dt, pnp_head="att")
    data = {k: T(v).cuda() for k, v in synth.synth_batch(2, seed=5).items()}
    rot, t = net.run_pnp(pnp_input, data)
    flat = net._module_plan(2, "cuda")["buf"]["p_flat"].view(2, -1).float().cpu().numpy()
    _check(flat, z["flat"], dt, 1e-4, 2e-2, "att pnp flat")
    _check(rot.cpu().numpy(), z["rot"], dt, 1e-4, 2e-2, "att pnp rot")
    _check(t.cpu().numpy(), z["t"], dt, 1e-4, 2e-2, "att pnp t")


# ------------------------------------------------------------------------------------------------ end to end
def _e2e_batch(z):
    from givepose_amd import synth
    npb = synth.synth_batch(4, seed=int(z["batch_seed"]))
    assert zlib.crc32(np.ascontiguousarray(npb["roi_img"]).tobytes()) == int(z["roi_img_crc"])
    return {k: T(v) for k, v in npb.items()}


@pytest.mark.parametrize("mode", [torch.float32, SPLIT, torch.float16])
@pytest.mark.parametrize("tag", list(E2E))
def test_e2e_golden(golden, tag, mode):
    """Bounds of tests/test_pnp_flags_gpu.py::test_e2e_golden."""
    z = golden("att_pnp_e2e_" + tag)
    net = _net(mode, **E2E[tag])
    out = net.forward_device(_e2e_batch(z), "cuda")
    err = {k: float(np.abs(out[k].float().cpu().numpy() - z[k]).max()) for k in ("rot", "trans", "size", "pred_rot", "pred_t")}
    print(f"e2e {tag} {mode}", err)
    assert out["pred_rot"].shape == z["pred_rot"].shape
    if mode == torch.float16:
        assert err["rot"] < 3e-2 and err["size"] < 3e-2
        assert err["trans"] < 3e-2 * max(1.0, float(np.abs(z["trans"]).max()))
    else:
        assert err["rot"] < 1e-4 and err["trans"] < 1e-4 and err["size"] < 1e-4, err
        assert err["pred_rot"] < 1e-4 and err["pred_t"] < 1e-4, err


@functools.lru_cache(maxsize=1)
def _configs3_ref():
    import att_pnp_ref
    from givepose_amd import PoseNetConfig, synth
    from oracle import posenet_ref as O
    cfg = PoseNetConfig(pnp_head="att", nocsmap_encoder="att")
    data = {k: T(v) for k, v in synth.synth_batch(32, seed=1932).items()}
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return data, att_pnp_ref.posenet_att_forward_ref(O.load_params(synth.synth_state_dict(cfg, 0)), data, cfg)


@pytest.mark.parametrize("mode", [torch.float32, SPLIT])
def test_configs3_bs32_graph_matches_ref(mode):
    """BASELINE configs[3] (attention encoder + attention pose head) at its batch of 32 under hipGraph replay against the CPU
    restatement: R, t, s within 1e-4 (tests/test_hip_posenet.py::test_attention_encoder_variant_bs32_matches_oracle)."""
    from givepose_amd import PoseNet, PoseNetConfig
    data, ref = _configs3_ref()
    net = PoseNet(PoseNetConfig(pnp_head="att", nocsmap_encoder="att"), seed=0, use_graph=True, **MODES[mode]).cuda()
    for _ in range(3):        # eager warm-up, capture + replay, replay
        out = net(data, "cuda")
    err = {k: float((out[k].cpu() - ref[k]).abs().max()) for k in ("rot", "trans", "size", "nocs_coor", "ivfc_coor")}
    print("configs[3] bs32", mode, err)
    assert torch.equal(out["mask"].cpu(), ref["mask"])
    assert err["rot"] < 1e-4 and err["trans"] < 1e-4 and err["size"] < 1e-4, err
    assert err["nocs_coor"] < 2e-4 and err["ivfc_coor"] < 2e-4, err


def test_graph_groups_match_separate_forwards():
    """use_graph=True with groups [2, 1, 3] (a ragged plan padded to 8 crops) against three separate forwards, fp32: 5e-5 (as
    tests/test_grouped_launch.py bounds two schedules of the same frames).  The head couples no crops."""
    from givepose_amd import synth
    groups = [2, 1, 3]
    frames = [{k: T(v) for k, v in synth.synth_batch(n, seed=310 + i).items()} for i, n in enumerate(groups)]
    both = {k: torch.cat([f[k] for f in frames], 0) for k in frames[0]}
    keys = ("rot", "trans", "size", "nocs_coor", "ivfc_coor", "pred_rot", "pred_t")
    graph = _net(torch.float32, use_graph=True, pnp_head="att")
    for _ in range(3):
        og = {k: v.clone() for k, v in graph.forward_device(both, groups=groups).items() if k in keys}
    assert any(p["ragged"] for p in graph._plans.values())
    alone = _net(torch.float32, pnp_head="att")
    i = 0
    for f, n in zip(frames, groups):
        oa = alone.forward_device(f)
        d = {k: float((og[k][i:i + n] - oa[k]).abs().max()) for k in keys}
        print(f"graph+groups vs alone, frame of {n}:", d)
        assert all(v < 5e-5 for v in d.values()), d
        i += n


def test_inflight_slots():
    """Two slots in flight (inflight=2, hipGraph per slot) give each batch's own result."""
    from givepose_amd import synth
    a, b = ({k: T(v) for k, v in synth.synth_batch(3, seed=s).items()} for s in (320, 321))
    net = _net(torch.float32, use_graph=True, pnp_head="att")
    net.inflight = 2
    ref = [{k: v.clone() for k, v in net.forward_device(d).items() if k in ("rot", "trans")} for d in (a, b)]
    for _ in range(3):
        oa = net.forward_device(a, slot=0, wait=False)
        ob = net.forward_device(b, slot=1, wait=False)
    torch.cuda.synchronize()
    for o, r in ((oa, ref[0]), (ob, ref[1])):
        assert all(float((o[k] - r[k]).abs().max()) < 5e-5 for k in r)


# ------------------------------------------------------------------------------------------------ dispatch
def _launch_labels(net, data):
    """{kernel label: launches} of one eager forward (gp_timing_top)."""
    from givepose_amd import _lib
    lib = _lib.load()
    net.forward_device(data)
    torch.cuda.synchronize()
    _lib.check(lib.gp_timing_begin(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gp_timing_begin")
    net.forward_device(data)
    _lib.check(lib.gp_timing_end(), "gp_timing_end")
    out = {}
    for r in range(500):
        lab = ctypes.create_string_buffer(160)
        c, n, ms, fl, by = ctypes.c_int(), ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        if lib.gp_timing_top(r, lab, 160, ctypes.byref(c), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) != 0:
            break
        out[lab.value.decode()] = n.value
    return out


def test_dispatch_b4_fp16():
    """At B = 4 in fp16, fc1 || fc1_z (M 4, N 2048, K 12288, GELU) takes the row-vector kernel (variant 23), and no ConvPnPNet
    launch runs."""
    from givepose_amd import synth
    net = _net(torch.float16, pnp_head="att")
    lab = _launch_labels(net, {k: T(v) for k, v in synth.synth_batch(4, seed=3).items()})
    for l, n in sorted(lab.items()):
        if any(s in l for s in ("K12288", "K320 ", "N576", "N192 ", "N768", "attention64", "patchify", "layernorm", "K1024")):
            print(f"  {n:3d} x {l}")
    assert lab.get("gemm v23 M4 N2048 K12288 epi1") == 1, lab
    assert sum(n for l, n in lab.items() if "M4 N256 K1024 epi1" in l) == 2, lab
    assert not any("pnp_conv1" in l for l in lab), lab
    assert sum(n for l, n in lab.items() if "gp_attention64_hd" in l) == 3, lab
    assert sum(n for l, n in lab.items() if "gp_patchify_pnp" in l) == 1, lab
