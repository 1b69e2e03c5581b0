"""CPU: the float64 restatement behind the coordinate-head backward tests (tests/xyz_backward_ref.py), its float32 yardstick, and the
gpx_ family's registration.

Yardstick figures: max|g32 - g64| / max|g64| per tensor, the float32 run of the restatement against its float64 run (torch on the
CPU), for the three end-to-end cases of tests/test_xyz_backward_gpu.py (R.CASES, (B, Cin, H0)).  The GPU test recomputes the figures
of its own case and allows 8 times them.  Recorded on the CPU (test_float32_yardstick prints all of them; the ranges here):

    case          saved tensors (pre, mean, rstd, act, up, coor)    parameter gradients        feat
    (3, 512, 2)   1.3e-07 .. 1.5e-06                                6.5e-07 .. 2.4e-06         1.8e-06
    (1, 1024, 8)  8.2e-08 .. 1.5e-06                                9.0e-08 .. 2.5e-06         1.8e-06
    (2, 512, 8)   8.4e-08 .. 1.2e-06                                5.5e-08 .. 2.3e-06         1.7e-06

A TopDownXyzHead has 23 distinct parameter tensors under 35 state_dict names (features.N.gn.* is features.N.norm.*).
"""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import xyz_backward_ref as R
from oracle import posenet_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


# ------------------------------------------------------------------------------------------------ the restatement
def oracle_grads(Cin, feat, g_coor):
    """float64 autograd through oracle.posenet_ref.xyz_head_ref -> ({name: grad} + "feat", coor)."""
    from givepose_amd import xyz_grad
    prefix = R.HEAD_OF[Cin] + "."
    P = {prefix + k: T(v).double().requires_grad_(True) for k, v in R.head_params(Cin).items()}
    f = T(feat).double().requires_grad_(True)
    coor = posenet_ref.xyz_head_ref(P, f, prefix)
    coor.backward(T(g_coor).double())
    return {**{k: P[prefix + k].grad.numpy() for k in xyz_grad.PARAM_KEYS}, "feat": f.grad.numpy()}, coor.detach().numpy()


@pytest.mark.parametrize("B,Cin,H0", [(2, 512, 2), (2, 1024, 2), (1, 512, 8)])
def test_restatement_is_the_oracle(B, Cin, H0):
    """The explicit formulas equal float64 autograd through xyz_head_ref: max|a - b| / max|b| <= 1e-12 per tensor."""
    feat, g = R.make_inputs(B, Cin, H0, seed=5)
    want, coor = oracle_grads(Cin, feat, g)
    got = R.head_run(R.head_params(Cin), feat, g)
    assert np.max(np.abs(got["saved"]["coor"] - coor)) <= 1e-12 * np.max(np.abs(coor))
    fig = R.rel_figures(got["grads"], want)
    print(f"restatement against the oracle B {B} Cin {Cin} H0 {H0}: {max(fig.values()):.2e}")
    assert len(fig) == 24
    for k, v in fig.items():
        assert v <= 1e-12, (k, v)
    assert all(np.any(v != 0) for v in want.values())


@pytest.mark.parametrize("H", [2, 3, 8, 32])
def test_bilinear_backward_is_the_transpose(H):
    """<up(x), g> = <x, up^T(g)> in float64, and up() is F.interpolate(align_corners=True)."""
    r = np.random.Generator(np.random.Philox(key=[H, 0x11]))
    x, g = T(r.standard_normal((2, 5, H, H))), T(r.standard_normal((2, 5, 2 * H, 2 * H)))
    y = R.up_forward(x)
    a, b = float((y * g).sum()), float((x * R.up_backward(g)).sum())
    assert abs(a - b) <= 1e-12 * float((y.abs() * g.abs()).sum())
    ref = torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    assert float((y - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    assert np.allclose(R.up_matrix(H).sum(1), 1.0, rtol=0, atol=1e-15)


def test_float32_yardstick():
    """Records the yardstick figures (module docstring): the float32 run of the restatement against its float64 run, per tensor and
    per case.  Nothing here is ill conditioned: every figure stays below 2e-5."""
    for case in R.CASES:
        _, _, _, fig, r64 = R.case_reference(case)
        assert len(fig) == 7 * 4 + 2 + 1 + 24
        groups = {"saved": [], "params": [], "feat": []}
        for k in sorted(fig):
            print(f"yardstick {case} {k} {fig[k]:.2e}")
            assert 0 < fig[k] < 2e-5, (case, k, fig[k])
            groups["feat" if k == "feat" else "saved" if k in r64["saved"] else "params"].append(fig[k])
        print(f"yardstick {case}: " + ", ".join(f"{n} {min(v):.1e} .. {max(v):.1e}" for n, v in groups.items()))


# ------------------------------------------------------------------------------------------------ registration and surface
def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build
    declared = set(re.findall(r"\b(gpx_[a-z0-9_]+)\s*\(", _header("givepose_xyzgrad.h")))
    assert declared == set(_lib.XYZGRAD_PROTOTYPES) and len(declared) == 16
    for other in (_lib.PROTOTYPES, _lib.HEADGRAD_PROTOTYPES, _lib.GRAD_PROTOTYPES):
        assert not set(_lib.XYZGRAD_PROTOTYPES) & set(other)
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gpx_[a-z0-9_]+)", out)) == declared
    for h in ("givepose_hip.h", "givepose_align.h", "givepose_loss.h", "givepose_grad.h", "givepose_headgrad.h"):
        assert "gpx_" not in _header(h), h
    assert "xyzgrad.hip" in build.SOURCES
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    # one GEMM for both families: the kernel is in the shared header and in neither source file
    csrc = os.path.join(ROOT, "givepose_amd", "csrc")
    assert "mfma_f32_32x32x2f32" in open(os.path.join(csrc, "grad_gemm.hpp")).read()
    for f in ("pnpgrad.hip", "xyzgrad.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "grad_gemm.hpp"' in src and "gemm_kernel" not in src and "__shared__ float As" not in src, f
    # the workspace queries answer on the host; a shape the entry point refuses has no workspace: 0, not a fault on the host
    assert lib.gpx_xyz_backward_workspace(2, 512, 8) >= 2 * 4 * 2 * 256 * 64 * 64 and lib.gpx_xyz_forward_workspace(2, 512, 8) >= 0
    assert lib.gpx_conv3x3s1_workspace(3, 256, 256, 16) > 0 and lib.gpx_deconv3x3s2_workspace(3, 64, 256, 2) > 0
    for bad in ((0, 512, 8), (2, 0, 8), (2, 512, 0), (5000, 512, 8), (2, 512, 65)):
        assert lib.gpx_xyz_backward_workspace(*bad) == 0 and lib.gpx_xyz_forward_workspace(*bad) == 0, bad
    assert lib.gpx_conv3x3s1_workspace(0, 8, 8, 8) == 0 and lib.gpx_deconv3x3s2_workspace(1, 8, 8, 0) == 0
    assert lib.gpx_conv1x1_backward_workspace(1, 256, 65, 9) == 0 and lib.gpx_gn_gelu_backward_workspace(0, 256) == 0
    assert ctypes.sizeof(_lib.XyzParams) == 23 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.XyzSaved) == 31 * ctypes.sizeof(ctypes.c_void_p)


def test_parameter_keys_aliases_and_shapes_match_the_state_dict():
    from givepose_amd import PoseNetConfig, synth, xyz_grad
    assert len(xyz_grad.PARAM_KEYS) == 23 == len(set(xyz_grad.PARAM_KEYS)) and len(xyz_grad.ALIASES) == 12
    assert set(xyz_grad.ALIASES.values()) <= set(xyz_grad.PARAM_KEYS) and not set(xyz_grad.ALIASES) & set(xyz_grad.PARAM_KEYS)
    manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_manifest.json")))["non_backbone_from_reference"]
    for head, Cin in (("xyz_deform_head", 512), ("xyz_nocs_head", 1024)):
        want = {k[len(head) + 1:]: tuple(s) for k, s in manifest.items() if k.startswith(head + ".")}
        assert len(want) == 35 and set(xyz_grad.PARAM_KEYS) | set(xyz_grad.ALIASES) == set(want)
        shapes = xyz_grad.param_shapes(Cin)
        assert list(shapes) == xyz_grad.PARAM_KEYS and all(shapes[k] == want[k] for k in shapes)
        assert all(want[a] == shapes[k] for a, k in xyz_grad.ALIASES.items())
        assert {k: tuple(v.shape) for k, v in R.head_params(Cin).items()} == shapes
    m = synth.param_manifest(PoseNetConfig())
    assert tuple(m["xyz_nocs_head.features.0.weight"]) == (1024, 256, 3, 3)
    sv = xyz_grad.saved_shapes(2, 512, 8)
    assert list(sv) == list(xyz_grad.SAVED_KEYS) and sv["coor"] == (2, 3, 64, 64) and sv["up"] == [(2, 256, 32, 32), (2, 256, 64, 64)]
    nbytes = 4 * sum(int(np.prod(s)) for v in xyz_grad.saved_shapes(1, 512, 8).values() for s in (v if isinstance(v, list) else [v]))
    assert 26.5 * 2 ** 20 < nbytes < 27 * 2 ** 20      # the figure the header states


def test_public_surface_and_refusals():
    import givepose_amd
    from givepose_amd import PoseNet, PoseNetConfig, _lib, xyz_grad
    assert givepose_amd.xyz_grad is xyz_grad
    p = inspect.signature(PoseNet.xyz_head_backward).parameters
    assert list(p) == ["self", "head", "feat", "g_coor", "device", "return_saved"]
    assert p["device"].default == "cuda" and p["return_saved"].default is False
    assert list(inspect.signature(PoseNet.head_grads_xyz).parameters) == list(inspect.signature(PoseNet.head_grads_pnp).parameters)
    assert "same tensor" in PoseNet.xyz_head_backward.__doc__ or "IS the tensor object" in PoseNet.xyz_head_backward.__doc__
    net = PoseNet(PoseNetConfig())
    feat, g = (T(a) for a in R.make_inputs(1, 512, 8, seed=1))
    with pytest.raises(ValueError, match="head"):
        net.xyz_head_backward("size_head", feat, g)
    with pytest.raises(ValueError, match="feat"):
        net.xyz_head_backward("xyz_nocs_head", feat, g, device="cpu")      # 512 channels into the 1024-channel head
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        net.xyz_head_backward("xyz_deform_head", feat, g, device="cpu")
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        xyz_grad.conv3x3s1_backward(torch.zeros(1, 5, 5, 5), torch.zeros(1, 3, 5, 5), torch.zeros(5, 3, 3, 3))
