"""Encoder layer 0 as a gather of the 3-channel map followed by one projection (gp_dcnv3_xyz_project).

conv1x1, input_proj, the bilinear samples, the mask-weighted tap sum and output_proj of the first DCNv3_C layer are linear in the sampled
value, and a corner outside the map contributes zero: the layer is a G = 4, D = 4 gather of the map [x, y, z, 1] (repeated per group) followed
by the 256 x 16 matrix posenet.enc0_xyz_pack forms.

  * CPU: that identity, pack function against the oracle chain, both in float64: <= 1e-12 of max|ref|.
  * GPU: the entry point against the float64 reference fed the SAME fp32 offsets and logits, per element
    |got - ref| <= 2^-11 |ref| + 1e-5 max|ref|   (one fp16 rounding at the store + the fp32 evaluation: its CPU restatement measures 6.4e-7 of
    max|ref|, which leaves about 15x for the device's exp and FMA contraction), and its GroupNorm statistics against torch group_norm of its
    own fp16 output at the tolerance of the fused-statistics test of gp_gemm (tests/test_hip_ops.py: 4e-3 of max|ref|).
  * GPU: the whole fp16 MAPEncoder against the reference's own outputs (goldens map_encoder_B1 / B4 / B5): rms error of the new path
    <= 1.05 x the rms error of the three-launch path (GP_ENC0_XYZ=0), both against the golden.
  * GPU: the launch labels of a forward at 64 crops.
"""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

PFX = "nocs_encoder.features.0."
AMP = 3.0        # offsets: uniform in +-AMP pixels


def _state(seed, dt=torch.float64):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * scale).to(dt)
    return {PFX + "conv.weight": r(256, 3, 1, 1, scale=0.5), PFX + "conv.bias": r(256, scale=0.2),
            PFX + "dcnv3.input_proj.weight": r(256, 256, scale=256 ** -0.5), PFX + "dcnv3.input_proj.bias": r(256, scale=0.2),
            PFX + "dcnv3.output_proj.weight": r(256, 256, scale=256 ** -0.5), PFX + "dcnv3.output_proj.bias": r(256, scale=0.2)}


def _inputs(n_crops, rows, seed):
    """xyz4 (n_crops*4096, 4) and the offset | logit rows (rows, 128) as fp32 tensors; the unused columns hold numbers that must not matter."""
    g = torch.Generator().manual_seed(seed)
    xyz4 = torch.rand(n_crops * 4096, 4, generator=g) - 0.5
    xyz4[:, 3] = 7.0                                                     # (the kernel does not read the 4th value)
    om = torch.randn(rows, 128, generator=g) * 2.0
    om[:, :72] = (torch.rand(rows, 72, generator=g) * 2 - 1) * AMP
    return xyz4, om


def _outside_fraction(om):
    """Share of the (pixel, group) samples with at least one bilinear corner outside the 64 x 64 map."""
    rows = om.shape[0]
    off = om[:, :72].double().reshape(rows, 4, 9, 2)
    pix = torch.arange(rows) % 1024
    wo, ho = (pix % 32).view(-1, 1, 1).double(), (pix // 32).view(-1, 1, 1).double()
    k = torch.arange(9)
    i, j = (k // 3).view(1, 1, 9).double(), (k % 3).view(1, 1, 9).double()      # tap order: w outer, h inner
    lw, lh = 2 * wo - 1 + i + off[..., 0], 2 * ho - 1 + j + off[..., 1]
    out = (torch.floor(lw) < 0) | (torch.floor(lw) + 1 > 63) | (torch.floor(lh) < 0) | (torch.floor(lh) + 1 > 63)
    return float(out.any(-1).double().mean())


def _gather_ref(xyz4, om, rows):
    """float64: the G = 4, D = 4 gather of [x, y, z, 1] by the oracle's DCNv3 core, from fp32 offsets / logits -> (rows, 16)."""
    from oracle.posenet_ref import dcnv3_forward_ref
    n = (rows + 1023) // 1024
    x = xyz4.double().reshape(n, 64, 64, 4).clone()
    x[..., 3] = 1.0
    pad = n * 1024 - rows                                               # (a ragged row count: the missing rows of the last crop gather with zero offsets)
    off = torch.cat([om[:, :72].double(), torch.zeros(pad, 72, dtype=torch.float64)], 0)
    msk = torch.cat([om[:, 72:108].double(), torch.zeros(pad, 36, dtype=torch.float64)], 0)
    msk = F.softmax(msk.reshape(-1, 4, 9), -1).reshape(-1, 36)
    v = dcnv3_forward_ref(x.repeat(1, 1, 1, 4), off, msk, 3, 2, 1, 1, 4, 4, 1.0)
    return v.reshape(n * 1024, 16)[:rows]


def test_pack_identity_against_oracle_chain_float64():
    from givepose_amd.posenet import enc0_xyz_pack
    from oracle.posenet_ref import dcnv3_forward_ref
    sd = _state(1)
    n = 2
    xyz4, om = _inputs(n, n * 1024, seed=2)
    frac = _outside_fraction(om)
    print(f"(pixel, group) samples with a corner outside the map: {frac:.3f}")
    assert frac >= 0.1
    x = xyz4[:, :3].double().reshape(n, 64, 64, 3)
    msk = F.softmax(om[:, 72:108].double().reshape(-1, 4, 9), -1).reshape(-1, 36)
    # the reference side: oracle/posenet_ref.py map_encoder_ref / dcnv3_module_ref with given offsets and mask
    c = F.linear(x, sd[PFX + "conv.weight"].reshape(256, 3), sd[PFX + "conv.bias"])
    p = F.linear(c, sd[PFX + "dcnv3.input_proj.weight"], sd[PFX + "dcnv3.input_proj.bias"])
    y = dcnv3_forward_ref(p, om[:, :72].double(), msk, 3, 2, 1, 1, 4, 64, 1.0)
    ref = F.linear(y, sd[PFX + "dcnv3.output_proj.weight"], sd[PFX + "dcnv3.output_proj.bias"]).reshape(-1, 256)
    m, b = enc0_xyz_pack(sd, PFX, dtype=torch.float64)
    got = _gather_ref(xyz4, om, n * 1024) @ m.t() + b
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"float64: max|got - ref| / max|ref| = {err:.3e}")
    assert err <= 1e-12
    m32, b32 = enc0_xyz_pack(sd, PFX)
    assert m32.dtype == torch.float32 and tuple(m32.shape) == (256, 16) and torch.equal(m32, m.float()) and torch.equal(b32, b.float())


@pytest.mark.gpu
@pytest.mark.parametrize("crops,rows", [(1, 1024), (5, 5 * 1024), (64, 64 * 1024), (128, 128 * 1024), (4, 3 * 1024 + 416), (33, 32 * 1024 + 224)])
def test_entry_point_against_float64_reference(crops, rows):
    from givepose_amd import ops as o
    from givepose_amd.posenet import enc0_xyz_pack
    m, b = enc0_xyz_pack(_state(3), PFX)
    xyz4, om = _inputs(crops, rows, seed=10 + crops)
    assert _outside_fraction(om) >= 0.1
    ref = _gather_ref(xyz4, om, rows) @ m.double().t() + b.double()
    out = torch.full((rows, 256), float("nan"), dtype=torch.float16, device="cuda")
    part = torch.zeros(crops * 32 * 32 * 2, device="cuda")
    o.dcnv3_xyz_project(xyz4.cuda(), om.cuda(), m.cuda(), b.cuda(), out, gn=(part, 32, 1024, 32))
    got = out.double().cpu()
    bound = 2.0 ** -11 * ref.abs() + 1e-5 * ref.abs().max()
    d = (got - ref).abs()
    print(f"crops {crops} rows {rows}: max|d| {float(d.max()):.3e}, max d / bound {float((d / bound).max()):.3f}, max|ref| {float(ref.abs().max()):.3e}")
    assert torch.isfinite(got).all()
    assert bool((d <= bound).all()), float((d / bound).max())
    if rows % 1024 == 0:      # the statistics the kernel leaves normalise its output as torch normalises that output
        gw, gb = (1 + 0.1 * torch.randn(256, generator=torch.Generator().manual_seed(5))), 0.1 * torch.randn(256, generator=torch.Generator().manual_seed(6))
        y = out.view(crops, 1024, 256)
        fused = o.groupnorm(y, gw.cuda(), gb.cuda(), torch.empty_like(y), 32, o.ACT_RELU, part, fused_stats=True, rows=32)
        gref = F.relu(F.group_norm(y.float().cpu().permute(0, 2, 1), 32, gw, gb, 1e-5)).permute(0, 2, 1)
        gerr = float((fused.float().cpu() - gref).abs().max() / gref.abs().max())
        print(f"crops {crops}: GroupNorm on the fused statistics against torch, relative error {gerr:.3e}")
        assert gerr < 4e-3


@pytest.mark.gpu
def test_entry_point_refuses_other_geometry():
    from givepose_amd import _lib, ops as o
    lib = _lib.load()
    z = torch.zeros(4096, 4, device="cuda")
    om, m, b = torch.zeros(1024, 128, device="cuda"), torch.zeros(256, 16, device="cuda"), torch.zeros(256, device="cuda")
    out, part = torch.zeros(1024, 256, dtype=torch.float16, device="cuda"), torch.zeros(2048, device="cuda")
    call = lambda rows=1024, H=64, K=3, stride=2, gn_rows=32: lib.gp_dcnv3_xyz_project(
        z.data_ptr(), om.data_ptr(), m.data_ptr(), b.data_ptr(), out.data_ptr(), part.data_ptr(), rows, H, 64, K, stride, 1, 1, 4, 128, 72, 1, 32, 1024, gn_rows,
        _lib.GP_F16, None)
    assert call() == 0
    assert call(H=32) != 0 and call(K=5) != 0 and call(stride=1) != 0 and call(gn_rows=64) != 0 and call(rows=1000) != 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        o.dcnv3_xyz_project(z, om, m, b, out, gn=(part, 32, 1024, 64))


@pytest.mark.gpu
def test_map_encoder_rms_error_against_golden(golden, monkeypatch):
    from givepose_amd import PoseNet, PoseNetConfig
    monkeypatch.setenv("GP_ENC0_XYZ", "0")
    old = PoseNet(PoseNetConfig(), dtype=torch.float16, seed=0).cuda()
    got_old = {B: old.run_map_encoder(torch.from_numpy(golden(f"map_encoder_B{B}")["x"])).cpu().numpy() for B in (1, 4, 5)}
    assert all("e_proj0" in p["buf"] and not p["enc0_xyz"] for p in old._plans.values())
    monkeypatch.delenv("GP_ENC0_XYZ")
    new = PoseNet(PoseNetConfig(), dtype=torch.float16, seed=0).cuda()
    for B in (1, 4, 5):
        exp = golden(f"map_encoder_B{B}")["expected"]
        got_new = new.run_map_encoder(torch.from_numpy(golden(f"map_encoder_B{B}")["x"])).cpu().numpy()
        rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - exp) ** 2)))
        e_old, e_new = rms(got_old[B]), rms(got_new)
        print(f"map_encoder B{B} fp16: rms error against the golden, three launches {e_old:.4e}, gather + projection {e_new:.4e} (ratio {e_new / e_old:.3f})")
        assert e_new <= 1.05 * e_old, (B, e_old, e_new)
    # the plans of the new path hold neither the projected full-resolution map nor the gathered one
    assert all(p["enc0_xyz"] and "e_proj0" not in p["buf"] and "e_g0" not in p["buf"] and "e_proj1" in p["buf"] for p in new._plans.values())


@pytest.mark.gpu
def test_launch_labels_at_64_crops():
    from givepose_amd import PoseNet, PoseNetConfig
    from test_hip_posenet import _batch, _launch_labels
    lab = _launch_labels(PoseNet(PoseNetConfig(), dtype=torch.float16, seed=0).cuda(), _batch(64, 3))
    n = lambda labels, pat: sum(v for l, v in labels.items() if re.search(pat, l))
    assert n(lab, r"dcnv3 N\d+ 64x64") == 0, lab
    assert n(lab, r"pointwise_k3 rows262144\b") == 0, lab                 # (64 x 4096: the full-resolution projection)
    assert n(lab, r"M65536 N256 K256 .*\+gn") == 0, lab
    assert n(lab, r"dcnv3_xyz_project") == 1, lab
    assert n(lab, r"dcnv3 N\d+ 32x32") == 1 and n(lab, r"dcnv3 N\d+ 16x16") == 1, lab     # layers 1 and 2 are untouched
    sp = _launch_labels(PoseNet(PoseNetConfig(), dtype=torch.float32, seed=0, split_gemm=True).cuda(), _batch(64, 3))
    assert n(sp, r"dcnv3 N64 64x64") == 1 and n(sp, r"pointwise_k3 rows262144\b") == 1 and n(sp, r"M65536 N256 K256 .*\+gn") == 1, sp
    assert n(sp, r"dcnv3_xyz_project") == 0, sp
