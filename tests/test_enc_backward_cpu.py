"""CPU: the float64 restatement behind the map-encoder backward tests (tests/enc_backward_ref.py) against float64 autograd through
oracle.posenet_ref.map_encoder_ref, its float32 yardstick, the gate margins, and the gpe_ family's registration.

Recorded on the CPU with the committed inputs (R.CASES as (B, R); the tests print all of them.  The float32 figures depend on the
CPU's float32 kernels, so every run measures them again and the GPU test uses the figures of its own run):

    restatement against the oracle, largest max|a - b| / max|b| over the 50 tensors (bound 64 (B R^2 + 2304) 2^-53 = 1.8e-11 .. 7.5e-11):
        (1,16) 2.7e-14   (3,16) 2.1e-14   (5,16) 3.2e-14   (2,64) 4.0e-14   (5,16) as [2,3] 2.4e-14
    float32 yardstick max|g32 - g64| / max|g64| (the smaller of float32 autograd and the float32 restatement held at float64's gates):
        case     the 48 gradients        d coor    nocs_feat
        (1,16)   7.8e-08 .. 1.9e-05      6.4e-06   5.7e-06
        (3,16)   7.0e-08 .. 1.2e-05      8.9e-06   5.5e-06
        (5,16)   5.9e-08 .. 1.2e-05      5.4e-06   5.8e-06
        (2,64)   7.5e-08 .. 1.9e-05      1.6e-05   4.7e-06
      (float32 autograd alone reached 5.5e-05 at (1,16): one gate inside the margin set rounded to the other side)
    gate margins: delta_loc 1.9e-04 .. 3.6e-04, delta_u 3.6e-04 .. 5.2e-04; in the margin set at most 459 of 784 896 gates (0.058 %, at (2,64));
        the float32 run disagrees with float64 on no gate outside it
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

import enc_backward_cases as C
import enc_backward_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


# ------------------------------------------------------------------------------------------------ the restatement
def _flat(r):
    return {**r["grads"], "coor": r["coor"], "nocs_feat": r["nocs_feat"]}


@pytest.mark.parametrize("case,groups", [(c, None) for c in R.CASES] + [R.GROUPED], ids=lambda v: str(v).replace(" ", ""))
def test_restatement_is_the_oracle(case, groups):
    """The explicit formulas equal float64 autograd through map_encoder_ref, per tensor, within R.oracle_bound; with groups the oracle
    is one call per coupling batch with the parameter gradients summed."""
    params, coor, g = R.case_inputs(case)
    want = _flat(C.reference(case, groups)[0])
    got = _flat(R.enc_run(params, coor, g, groups=groups))
    fig = R.rel_figures(got, want)
    worst = max(fig, key=fig.get)
    print(f"restatement against the oracle {case} {groups}: {fig[worst]:.2e} ({worst}), bound {R.oracle_bound(*case):.2e}")
    assert len(fig) == 50
    for k, v in fig.items():
        assert v <= R.oracle_bound(*case), (k, v)
    assert all(np.any(v != 0) for v in want.values())


def test_coupling_changes_the_gradient():
    """[2,3] is not one batch of 5: the prefix of the second batch starts at its own first crop."""
    a, b = C.reference(R.GROUPED[0], R.GROUPED[1])[0], C.reference(R.GROUPED[0])[0]
    fig = R.rel_figures(a["grads"], b["grads"])
    assert min(fig.values()) > 1e-3, fig


@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_restatement_at_its_own_gates_is_unchanged(case):
    """Evaluated at the gates read from its own saved tensors, the restatement gives the same result bit for bit."""
    params, coor, g = R.case_inputs(case)
    a = R.enc_run(params, coor, g)
    b = R.enc_run(params, coor, g, gates=[R.gates_of(a["saved"][0], *case)])
    for k, v in _flat(a).items():
        assert np.array_equal(v, _flat(b)[k]), k


def test_float32_yardstick():
    """Records the yardstick figures (module docstring): float32 autograd against float64 autograd, per tensor and per case."""
    for case in R.CASES:
        fig = C.reference(case)[2]
        assert len(fig) == 50
        for k in sorted(fig):
            print(f"yardstick {case} {k} {fig[k]:.2e}")
            assert 0 < fig[k] < 1e-4, (case, k, fig[k])
        gr = [v for k, v in fig.items() if k not in ("coor", "nocs_feat")]
        print(f"yardstick {case}: gradients {min(gr):.1e} .. {max(gr):.1e}, coor {fig['coor']:.1e}, nocs_feat {fig['nocs_feat']:.1e}")


def test_gate_margins():
    """The margin set (R's docstring) holds at most 0.1 % of the gates, and outside it the float32 run agrees with float64 on every gate."""
    for case, groups in [(c, None) for c in R.CASES] + [R.GROUPED]:
        r64, r32, _, margins = C.reference(case, groups)
        total, inside, bad = C.gate_disagreements(r32["gates"], r64, margins)
        print(f"gates {case} {groups}: delta_loc {margins['delta_loc']:.2e}, delta_u {margins['delta_u']:.2e}, {inside} of {total} in the margin "
              f"set, {bad} disagreements outside it")
        assert inside <= 1e-3 * total and bad == 0
        assert margins["delta_loc"] < 1e-3 and margins["delta_u"] < 1e-3


# ------------------------------------------------------------------------------------------------ registration and surface
def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build
    declared = set(re.findall(r"\b(gpe_[a-z0-9_]+)\s*\(", _header("givepose_encgrad.h")))
    assert declared == set(_lib.ENCGRAD_PROTOTYPES) and len(declared) == 17
    for other in (_lib.PROTOTYPES, _lib.HEADGRAD_PROTOTYPES, _lib.GRAD_PROTOTYPES, _lib.XYZGRAD_PROTOTYPES):
        assert not set(_lib.ENCGRAD_PROTOTYPES) & set(other)
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gpe_[a-z0-9_]+)", out)) == declared
    for h in ("givepose_hip.h", "givepose_align.h", "givepose_loss.h", "givepose_grad.h", "givepose_headgrad.h", "givepose_xyzgrad.h"):
        assert "gpe_" not in _header(h), h
    assert "encgrad.hip" in build.SOURCES
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    # the contractions are the shared functor GEMM: no GEMM kernel of its own, and the scatter is the only atomic
    src = open(os.path.join(ROOT, "givepose_amd", "csrc", "encgrad.hip")).read()
    assert '#include "grad_gemm.hpp"' in src and "gemm_kernel" not in src and "__shared__ float As" not in src
    assert src.count("atomicAdd(") == 4 and all("gim" in line for line in src.splitlines() if "atomicAdd(" in line)
    # the workspace queries answer on the host; a shape the entry point refuses has no workspace
    assert lib.gpe_map_encoder_backward_workspace(2, 64) > 0 and lib.gpe_map_encoder_forward_workspace(2, 64) > 0
    for bad in ((0, 64), (2, 0), (2, 60), (5000, 64), (2, 1024)):
        assert lib.gpe_map_encoder_backward_workspace(*bad) == 0 and lib.gpe_map_encoder_forward_workspace(*bad) == 0, bad
    assert lib.gpe_linear_workspace(0, 3, 256) == 0 and lib.gpe_linear_workspace(27, 256, 72) > 0
    assert lib.gpe_dwln_backward_workspace(3, 6, 6, 256, 27) > 0 and lib.gpe_dwln_backward_workspace(3, 6, 6, 256, 109) == 0
    assert lib.gpe_dwln_backward_workspace(3, 6, 6, 200, 27) == 0 and lib.gpe_gn_relu_backward_workspace(0, 256) == 0
    assert lib.gpe_conv1x1_backward_workspace(1, 1024, 256, 64) > 0 and lib.gpe_conv1x1_backward_workspace(1, 0, 256, 64) == 0
    assert ctypes.sizeof(_lib.EncParams) == 48 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.EncSaved) == 39 * ctypes.sizeof(ctypes.c_void_p)


def test_parameter_keys_and_shapes_match_the_state_dict():
    from givepose_amd import PoseNetConfig, enc_grad, synth
    assert len(enc_grad.PARAM_KEYS) == 48 == len(set(enc_grad.PARAM_KEYS))
    manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_manifest.json")))["non_backbone_from_reference"]
    want = {k[len("nocs_encoder."):]: tuple(s) for k, s in manifest.items() if k.startswith("nocs_encoder.")}
    bn = {k for k in want if ".bn." in k}
    assert len(bn) == 15 and set(enc_grad.PARAM_KEYS) == set(want) - bn      # DCNv3_C.bn is never applied: no gradient entry
    assert not any(".bn." in k for k in enc_grad.PARAM_KEYS)
    shapes = enc_grad.param_shapes()
    assert list(shapes) == enc_grad.PARAM_KEYS and all(shapes[k] == want[k] for k in shapes)
    assert {k: tuple(v.shape) for k, v in R.enc_params().items()} == shapes
    m = synth.param_manifest(PoseNetConfig())
    assert all(tuple(m["nocs_encoder." + k]) == s for k, s in shapes.items())
    assert set(enc_grad.ATOMIC_FREE_KEYS) < set(enc_grad.PARAM_KEYS) and len(enc_grad.ATOMIC_FREE_KEYS) == 12
    sv = enc_grad.saved_shapes(2, 64)
    assert list(sv) == list(enc_grad.SAVED_KEYS) == list(R.SAVED_KEYS)
    assert sv["x"] == [(2, 64, 64, 256), (2, 32, 32, 256), (2, 16, 16, 256)] and sv["offset"][0] == (2048, 72) and sv["act"][2] == (2, 256, 8, 8)
    ref = R.batch_forward({k: T(v).double() for k, v in R.enc_params().items()}, torch.zeros(1, 3, 16, 16, dtype=torch.float64))
    assert {k: [tuple(t.shape) for t in v] for k, v in ref.items()} == enc_grad.saved_shapes(1, 16)
    nbytes = 4 * sum(int(np.prod(s)) for v in enc_grad.saved_shapes(1, 64).values() for s in v)
    assert 17.5 * 2 ** 20 < nbytes < 17.8 * 2 ** 20      # the figure the header states


def test_public_surface_and_refusals():
    import givepose_amd
    from givepose_amd import PoseNet, PoseNetConfig, _lib, enc_grad
    assert givepose_amd.enc_grad is enc_grad
    p = inspect.signature(PoseNet.map_encoder_backward).parameters
    assert list(p) == ["self", "coor", "g_nocs_feat", "groups", "device", "return_saved"]
    assert p["groups"].default is None and p["device"].default == "cuda" and p["return_saved"].default is False
    assert list(inspect.signature(PoseNet.feat_reducer_backward).parameters)[:3] == ["self", "feat", "g_conv_feat256"]
    assert list(inspect.signature(PoseNet.head_grads_feat).parameters) == list(inspect.signature(PoseNet.head_grads_xyz).parameters)
    assert "size head" in PoseNet.head_grads_feat.__doc__ and "NOT included" in PoseNet.head_grads_feat.__doc__
    coor, g = (T(a) for a in R.make_inputs(1, 16, seed=1))
    for flags, word in (({"nocsmap_encoder": "att"}, "nocsmap_encoder"), ({"use_dcn": ""}, "use_dcn")):
        net = PoseNet(PoseNetConfig(**flags))
        with pytest.raises(NotImplementedError, match=word):
            net.map_encoder_backward(coor, g)
        with pytest.raises(NotImplementedError, match=word):
            net.head_grads_feat({}, None)
    net = PoseNet(PoseNetConfig())
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        net.map_encoder_backward(coor, g, device="cpu")
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        enc_grad.linear_backward(torch.zeros(2, 4), torch.zeros(2, 3), torch.zeros(4, 3))
    assert net._enc_groups(6, None) == [6] and net._enc_groups(6, [1, 5]) == [1, 5]
    assert PoseNet(PoseNetConfig(), dcn_couple=2)._enc_groups(6, None) == [2, 2, 2]
