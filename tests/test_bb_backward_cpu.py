"""CPU: the float64 restatement behind the backbone backward tests (tests/bb_backward_ref.py) against float64 autograd through
oracle.posenet_ref.convnext_ref, and the gpb_ family's registration, names, shapes and saved-byte count.

Recorded on the CPU with the committed inputs (R.CASES; the test prints them):

    restatement against the oracle, largest max|a - b| / max|b| over the gradients, d img and feat (and the bound):
        A 2.5e-15 (1.8e-10)   B 2.6e-15 (2.1e-10)   C 2.3e-15 (1.4e-10)   D 4.2e-15 (1.1e-09)   E 2.7e-15 (4.4e-10)
    saved by the forward, ConvNeXt-Base at 256 x 256: 176 678 400 bytes per crop (176.7 MB), 11.31 GB at B = 64
"""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import bb_backward_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_is_the_oracle(case):
    """The explicit formulas equal float64 autograd through convnext_ref, per tensor, within R.oracle_bound."""
    from oracle import posenet_ref
    dims, depths, B, S = R.CASES[case]
    params, img, g = R.case_inputs(case)
    P = {"backbone." + k: T(v).double().requires_grad_() for k, v in params.items()}
    x = T(img).double().requires_grad_()
    feat = posenet_ref.convnext_ref(P, x, types.SimpleNamespace(convnext_depths=depths))[0]
    feat.backward(T(g).double())
    want = {**{k: P["backbone." + k].grad.numpy() for k in params}, "img": x.grad.numpy(), "feat": feat.detach().numpy()}
    got = R.reference(case)[0]
    assert list(got) == list(want) and len(got) == 4 + 4 * (len(dims) - 1) + 9 * sum(depths) + 2
    fig = R.rel_figures(got, want)
    worst = max(fig, key=fig.get)
    print(f"restatement against the oracle {case}: {fig[worst]:.2e} ({worst}), bound {R.oracle_bound(case):.2e}")
    for k, v in fig.items():
        assert v <= R.oracle_bound(case), (k, v)
    assert all(np.any(v != 0) for v in want.values())


def test_operator_formulas_are_autograd():
    """The operator restatements on odd shapes (maps smaller than the window, H != W) against float64 autograd."""
    import torch.nn.functional as F
    r = np.random.Generator(np.random.Philox(key=[7, 0xBB]))
    t = lambda *s: T(r.standard_normal(s))
    for N, H, W, C in ((2, 3, 3, 4), (1, 1, 1, 2), (1, 5, 9, 3)):
        x, w, b, dy = t(N, H, W, C).requires_grad_(), t(C, 1, 7, 7).requires_grad_(), t(C).requires_grad_(), t(N, H, W, C)
        y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=3, groups=C).permute(0, 2, 3, 1)
        y.backward(dy)
        assert torch.allclose(R.dw7_forward(x.detach(), w.detach(), b.detach()), y.detach(), rtol=1e-12, atol=1e-12)
        for a, want in zip(R.dw7_backward(dy, x.detach(), w.detach()), (x.grad, w.grad, b.grad)):
            assert torch.allclose(a, want, rtol=1e-12, atol=1e-12)
        dead = R.dead_taps(H, W)
        assert np.all(w.grad.numpy()[:, 0][:, dead] == 0) and np.all(np.any(w.grad.numpy()[:, 0][:, ~dead] != 0, axis=0))
    for nchw, shape, wshape in ((True, (2, 3, 8, 8), (5, 3, 4, 4)), (False, (2, 4, 6, 3), (5, 3, 2, 2))):
        x, w, b = t(*shape).requires_grad_(), t(*wshape).requires_grad_(), t(wshape[0]).requires_grad_()
        y = F.conv2d(x if nchw else x.permute(0, 3, 1, 2), w, b, stride=wshape[2]).permute(0, 2, 3, 1).reshape(-1, wshape[0])
        dy = t(*y.shape)
        y.backward(dy)
        assert torch.allclose(R.patch_forward(x.detach(), w.detach(), b.detach(), nchw), y.detach(), rtol=1e-12, atol=1e-12)
        for a, want in zip(R.patch_backward(dy, x.detach(), w.detach(), nchw), (x.grad, w.grad, b.grad)):
            assert torch.allclose(a, want, rtol=1e-12, atol=1e-12)


def test_param_keys_are_the_checkpoint_keys():
    """PARAM_KEYS(PoseNetConfig()) equals the backbone. lines of tests/golden/expected_checkpoint_keys.txt, in order and shape."""
    from givepose_amd import PoseNetConfig, bb_grad
    want = []
    for line in open(os.path.join(ROOT, "tests", "golden", "expected_checkpoint_keys.txt")):
        parts = line.split()
        if parts and parts[0].startswith("backbone."):
            want.append((parts[0][len("backbone."):], tuple(int(d) for d in parts[1].split("x"))))
    cfg = PoseNetConfig()
    assert len(want) == 340 and bb_grad.PARAM_KEYS(cfg) == [k for k, _ in want]
    assert list(bb_grad.param_shapes(cfg).items()) == want
    assert bb_grad.PARAM_KEYS(((64, 128), (1, 2))) == ["stem_0.weight", "stem_0.bias", "stem_1.weight", "stem_1.bias"] \
        + [f"stages_0.blocks.0.{k}" for k in R.BLOCK_KEYS] + [f"stages_1.downsample.{i}.{p}" for i in (0, 1) for p in ("weight", "bias")] \
        + [f"stages_1.blocks.{b}.{k}" for b in (0, 1) for k in R.BLOCK_KEYS]
    for bad in ((100, 128), (64, 96)):
        with pytest.raises(ValueError, match="multiple of 64"):
            bb_grad.PARAM_KEYS((bad, (1, 1)))


def test_saved_shapes_agree_with_the_formulas():
    """saved_shapes against a count made from the formulas: per block 7 C floats and two statistics per row, per norm C + 2; and
    against what the restatement saves."""
    from givepose_amd import PoseNetConfig, bb_grad
    for dims, depths, B, S in list(R.CASES.values()) + [((128, 256, 512, 1024), (3, 3, 27, 3), 1, 256)]:
        rows = [B * (S // (4 << s)) ** 2 for s in range(len(dims))]
        floats = rows[0] * (dims[0] + 2) + sum(rows[s - 1] * (dims[s - 1] + 2) for s in range(1, len(dims)))
        floats += sum(depths[s] * rows[s] * (7 * dims[s] + 2) for s in range(len(dims)))
        assert bb_grad.saved_bytes((dims, depths), B, S) == 4 * floats
        assert len(bb_grad.saved_shapes((dims, depths), B, S)) == 3 * len(dims) + 6 * sum(depths)
    per_crop = bb_grad.saved_bytes(PoseNetConfig(), 1, 256)
    print(f"ConvNeXt-Base at 256 x 256: {per_crop} bytes saved per crop ({per_crop / 1e6:.1f} MB), {64 * per_crop / 1e9:.2f} GB at B = 64")
    assert 165e6 < per_crop < 180e6      # the issue's estimate: about 170 MB
    dims, depths, B, S = R.CASES["A"]
    params, img, g = R.case_inputs("A")
    sv = R.backbone_run(params, img, g, dims, depths, want_saved=True)["saved"]
    want = bb_grad.saved_shapes((dims, depths), B, S)
    assert set(sv) == set(want) and all(tuple(sv[k].shape) == want[k] for k in want)
    with pytest.raises(ValueError, match="multiple of 32"):
        bb_grad.saved_shapes(PoseNetConfig(), 1, 48)


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build
    declared = set(re.findall(r"\b(gpb_[a-z0-9_]+)\s*\(", _header("givepose_bbgrad.h")))
    assert declared == set(_lib.BBGRAD_PROTOTYPES) and len(declared) == 17
    for other in (_lib.PROTOTYPES, _lib.HEADGRAD_PROTOTYPES, _lib.GRAD_PROTOTYPES, _lib.XYZGRAD_PROTOTYPES, _lib.ENCGRAD_PROTOTYPES):
        assert not set(_lib.BBGRAD_PROTOTYPES) & set(other)
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gpb_[a-z0-9_]+)", out)) == declared
    assert "bbgrad.hip" in build.SOURCES
    lib = _lib.load()
    # the contractions are the shared functor GEMM, and there is no atomic in the family
    src = open(os.path.join(ROOT, "givepose_amd", "csrc", "bbgrad.hip")).read()
    assert '#include "grad_gemm.hpp"' in src and "gemm_kernel" not in src and "__shared__ float As" not in src
    assert not re.search(r"\batomic\w*\s*\(", src)
    # the size queries answer on the host; a shape the entry point refuses has no workspace
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    base, deep = ints((128, 256, 512, 1024)), ints((3, 3, 27, 3))
    assert lib.gpb_param_count(deep, 4) == 340 and lib.gpb_param_count(ints((1, 0)), 2) == 0
    assert lib.gpb_backbone_forward_workspace(base, deep, 4, 2, 256) > 0 and lib.gpb_backbone_backward_workspace(base, deep, 4, 2, 256) > 0
    for dims, B, S in ((ints((128, 256, 500, 1024)), 2, 256), (base, 0, 256), (base, 2, 48), (base, 2, 0)):
        assert lib.gpb_backbone_forward_workspace(dims, deep, 4, B, S) == 0 and lib.gpb_backbone_backward_workspace(dims, deep, 4, B, S) == 0
    assert lib.gpb_dw7_backward_workspace(2, 3, 3, 64) > 0 and lib.gpb_dw7_backward_workspace(2, 3, 3, 96) == 0
    assert lib.gpb_block_workspace(1, 8, 8, 1024) > 0 and lib.gpb_block_workspace(1, 8, 8, 1000) == 0
    assert lib.gpb_layernorm_backward_workspace(300, 1024) > 0 and lib.gpb_layernorm_backward_workspace(0, 64) == 0
    assert lib.gpb_patch_conv_workspace(2, 32, 32, 3, 128, 4, 1) >= 0 and lib.gpb_patch_conv_workspace(2, 30, 32, 3, 128, 4, 1) == 0
    assert ctypes.sizeof(_lib.BbBlockParams) == 9 * ctypes.sizeof(ctypes.c_void_p)


def test_public_surface_and_refusals():
    import givepose_amd
    from givepose_amd import PoseNet, PoseNetConfig, _lib, bb_grad
    assert givepose_amd.bb_grad is bb_grad
    p = inspect.signature(PoseNet.backbone_backward).parameters
    assert list(p) == ["self", "img", "g_feat", "device", "return_saved"] and p["device"].default == "cuda" and p["return_saved"].default is False
    assert list(inspect.signature(PoseNet.head_grads_backbone).parameters) == list(inspect.signature(PoseNet.head_grads_feat).parameters)
    doc = PoseNet.head_grads_backbone.__doc__
    assert "fp32 recompute" in doc and "NOT included" in doc
    net = PoseNet(PoseNetConfig(main_backbone="resnet34"))
    with pytest.raises(NotImplementedError, match="resnet34"):
        net.backbone_backward(torch.zeros(1, 3, 32, 32), torch.zeros(1, 512, 1, 1))
    with pytest.raises(NotImplementedError, match="resnet34"):
        net.head_grads_backbone({}, None)
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        bb_grad.dw7_forward(torch.zeros(1, 2, 2, 64), torch.zeros(64, 1, 7, 7), torch.zeros(64))
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        PoseNet(PoseNetConfig()).backbone_backward(torch.zeros(1, 3, 32, 32), torch.zeros(1, 1024, 1, 1), device="cpu")
