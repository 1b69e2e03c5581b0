"""CPU: the float64 restatement behind the pose-head backward tests (tests/pnp_backward_ref.py), its float32 yardstick, and the
gph_ family's registration.

Yardstick figures: max|g32 - g64| / max|g64| per tensor, the float32 run of the gated restatement against its float64 run (same
gates, torch on the CPU), largest over the four end-to-end cases of tests/test_pnp_backward_gpu.py (B = 1, 3, 5 and B = 4 masked;
R.CASES).  The GPU test recomputes the figure of its own case and allows 8 times it.  Recorded on the CPU (this file's
test_float32_yardstick_and_gate_flips prints them):

    features.0.weight 3.7e-06   features.1.weight 9.7e-07   features.1.bias 9.6e-07
    features.3.weight 1.5e-06   features.4.weight 7.8e-07   features.4.bias 8.3e-07
    features.6.weight 7.8e-07   features.7.weight 8.1e-07   features.7.bias 9.1e-07
    fc1.weight 6.7e-07   fc1.bias 5.7e-07   fc1_z.weight 6.0e-07   fc1_z.bias 4.8e-07
    fc2.weight 6.6e-07   fc2.bias 1.1e-07   fc2_z.weight 7.4e-07   fc2_z.bias 7.7e-08
    fc_r.weight 4.9e-07  fc_r.bias 6.6e-08  fc_t.weight 9.2e-07    fc_t.bias 1.2e-07
    fc_z.weight 1.0e-06  fc_z.bias 2.2e-08  ivfc_coor 8.6e-07

(The three output biases' gradients are sums of the upstream gradient over the batch: at B = 1 the figure is 0 and the device's
value has to be exact, which it is -- 0 + g.)  Gate flips of the float32 forward against the float64 forward's own signs: 0 of
174592 B gated elements in every case, so none outside the layer's fp32 bound.

The state_dict of pnp_net has 23 tensors (3 conv weights, 3 x 2 GroupNorm, 7 x 2 linear).
"""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pnp_backward_ref as R
from oracle import posenet_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("masked", [False, True])
def test_restatement_with_its_own_gates_is_the_oracle(masked):
    """Gates = the signs of its own pre-activations: the gradients equal float64 autograd through oracle.posenet_ref.conv_pnp_ref."""
    params = R.head_params()
    ivfc, coord, mask, g_rot, g_t = R.make_inputs(2, seed=7, masked=masked)

    def oracle(P, iv, co, m):
        x = torch.cat([iv, co], dim=1)
        return posenet_ref.conv_pnp_ref(P, x if m is None else x * m)

    want = R.gated_grads(params, ivfc, coord, mask, g_rot, g_t, forward=oracle)
    got = R.gated_grads(params, ivfc, coord, mask, g_rot, g_t)
    assert np.array_equal(got["pred_rot"], want["pred_rot"]) or np.max(np.abs(got["pred_rot"] - want["pred_rot"])) < 1e-13
    fig = R.rel_figures(R.tensors_of(got), R.tensors_of(want))
    print("restatement against the oracle:", max(fig.values()))
    assert set(fig) == set(params) | {"ivfc_coor"}
    for k, v in fig.items():
        assert v <= 1e-12, (k, v)
    assert all(np.any(v != 0) for v in R.tensors_of(want).values())
    if masked:      # the mask reaches the gradient of the map: zero where it is zero
        assert np.all(got["ivfc_coor"][:, :, :20, 30:] == 0) and np.any(got["ivfc_coor"] != 0)


def test_given_gates_are_used():
    """A gate set that differs from the signs changes the gradient (the gates really are inputs)."""
    params = R.head_params()
    inp = R.make_inputs(1, seed=8)
    own = R.gated_grads(params, *inp)
    gates = {k: v.copy() for k, v in own["gates"].items()}
    gates["fc2"] = ~gates["fc2"]
    other = R.gated_grads(params, *inp, gates=gates)
    assert np.array_equal(other["gates"]["fc2"], gates["fc2"])
    assert np.max(np.abs(other["param_grads"]["pnp_net.fc1.weight"] - own["param_grads"]["pnp_net.fc1.weight"])) > 0
    assert np.array_equal(other["param_grads"]["pnp_net.fc1_z.weight"], own["param_grads"]["pnp_net.fc1_z.weight"])


def test_float32_yardstick_and_gate_flips():
    """Records the yardstick figures (module docstring) and checks the seeds of the end-to-end cases: the float32 forward's own signs
    differ from the float64 forward's only inside the layer's fp32 bound (none outside it), and for fewer than 1e-4 of the gated
    elements."""
    params = R.head_params()
    worst = {}
    for name, (B, seed, masked) in R.CASES.items():
        inp = R.make_inputs(B, seed, masked)
        own64 = R.gated_grads(params, *inp)
        fig, r64 = R.f32_figures(params, *inp, gates=own64["gates"])
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v < 2e-5, (name, k, v)          # float32 against float64: nothing here is ill conditioned
        own32 = R.gated_grads(params, *inp, dtype=torch.float32)
        bounds = R.forward_bounds(params, *inp[:3], own64)
        n, bad, diff = R.gate_flips(own32["gates"], own64, bounds)
        print(f"{name}: float32 gates that differ from float64's {diff} of {n}, outside the fp32 bound {bad}")
        assert bad == 0 and diff < 1e-4 * n, (name, bad, diff, n)
    for k in sorted(worst):
        print(f"yardstick {k} {worst[k]:.2e}")


# ------------------------------------------------------------------------------------------------ registration and surface
def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build
    declared = set(re.findall(r"\b(gph_[a-z0-9_]+)\s*\(", _header("givepose_headgrad.h")))
    assert declared == set(_lib.HEADGRAD_PROTOTYPES) and len(declared) == 10
    assert not set(_lib.HEADGRAD_PROTOTYPES) & set(_lib.PROTOTYPES)
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gph_[a-z0-9_]+)", out)) == declared
    for h in ("givepose_hip.h", "givepose_align.h", "givepose_loss.h", "givepose_grad.h"):
        assert "gph_" not in _header(h), h
    assert "pnpgrad.hip" in build.SOURCES
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    src = open(os.path.join(ROOT, "givepose_amd", "csrc", "pnpgrad.hip")).read()
    assert "mfma_f32_32x32x2f32" in src
    # the workspace queries answer on the host; the struct layouts are those of the header (pointers only)
    assert lib.gph_pnp_backward_workspace(4, 6) > 0 and lib.gph_pnp_forward_workspace(4, 6) > 0
    assert lib.gph_linear_backward_workspace(5, 2048, 8192) >= 4 * 5 * 2048
    # a shape the entry point refuses has no workspace: 0, not a fault on the host
    for bad in ((2, 128, 128, 1, 0), (2, 128, 128, 15, 128), (2, 128, 128, 0, 0), (0, 128, 128, 16, 1), (2, 5, 128, 64, 6)):
        assert lib.gph_conv3x3s2_backward_workspace(*bad) == 0, bad
    assert lib.gph_conv3x3s2_backward_workspace(2, 128, 128, 2, 0) >= 0 and lib.gph_linear_backward_workspace(0, 4, 4) == 0
    assert lib.gph_gn_relu_backward_workspace(0, 128) == 0 and lib.gph_pnp_backward_workspace(0, 6) == 0
    import ctypes
    assert ctypes.sizeof(_lib.PnpParams) == 23 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.PnpSaved) == 18 * ctypes.sizeof(ctypes.c_void_p)


def test_parameter_keys_and_shapes_match_the_state_dict():
    from givepose_amd import PoseNetConfig, pnp_grad, synth
    for r_type in ("allo_rot6d", "allo_quat"):
        cfg = PoseNetConfig(r_type=r_type)
        want = {k[len(R.PREFIX):]: tuple(s) for k, s in synth.param_manifest(cfg).items() if k.startswith(R.PREFIX)}
        got = pnp_grad.param_shapes(cfg.rot_dim)
        assert got == want and len(got) == 23 and list(got) == pnp_grad.PARAM_KEYS
    assert set(R.head_params()) == {R.PREFIX + k for k in pnp_grad.PARAM_KEYS}


def test_public_surface_and_refusals():
    import dataclasses

    import givepose_amd
    from givepose_amd import PoseNet, PoseNetConfig, _lib, pnp_grad
    assert givepose_amd.pnp_grad is pnp_grad
    p = inspect.signature(PoseNet.pnp_backward).parameters
    assert list(p) == ["self", "ivfc_coor", "roi_coord_2d", "g_pred_rot", "g_pred_t", "mask", "device", "return_saved"]
    assert p["mask"].default is None and p["device"].default == "cuda" and p["return_saved"].default is False
    assert list(inspect.signature(PoseNet.head_grads_pnp).parameters) == list(inspect.signature(PoseNet.head_grads).parameters)
    ivfc, coord, _, g_rot, g_t = (torch.from_numpy(a) if a is not None else None for a in R.make_inputs(1, seed=1))
    net = PoseNet(PoseNetConfig())
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        net.pnp_backward(ivfc, coord, g_rot, g_t, device="cpu")
    for flag, value in (("pnp_head", "att"), ("flat_op", "avg"), ("flat_op", "avg-max-min"), ("mask_attention_type", "concat")):
        net.cfg = dataclasses.replace(PoseNetConfig(), **{flag: value})
        with pytest.raises(NotImplementedError, match=flag):
            net.pnp_backward(ivfc, coord, g_rot, g_t)
        with pytest.raises(NotImplementedError, match=flag):
            net.head_grads_pnp({}, None)
    for r_type in ("allo_rot6d_y", "allo_quat", "euler"):
        net.cfg = dataclasses.replace(PoseNetConfig(), r_type=r_type)
        with pytest.raises(NotImplementedError, match="r_type"):
            net.head_grads_pnp({}, None)
    net.cfg = dataclasses.replace(PoseNetConfig(), mask_attention_type="mul")
    with pytest.raises(ValueError, match="mask"):
        net.pnp_backward(ivfc, coord, g_rot, g_t)
