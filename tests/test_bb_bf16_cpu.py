"""CPU: the restatement of the "bf16" precision of the backbone backward (tests/bb_bf16_ref.py) and the public surface of the mode
(include/givepose_bbgrad_bf16.h, givepose_amd/bb_grad.py, PoseNet.set_backward_precision)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bb_backward_ref as R
import bb_bf16_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


def test_round_bf16_is_nearest_even():
    """The integer restatement equals torch's conversion on random values of many magnitudes and on exact ties of both parities."""
    r = np.random.Generator(np.random.Philox(key=[7, 0xBF16]))
    x = T((r.standard_normal(1 << 16) * np.exp2(r.integers(-40, 40, 1 << 16))).astype(np.float32))
    assert torch.equal(Q.round_bf16(x), x.bfloat16().float())
    assert float((Q.round_bf16(x) != x).float().mean()) > 0.99          # random fp32 is not bf16-representable
    hi = T(r.integers(0x3000, 0x4F00, 4096).astype(np.int32)) << 16      # positive bf16 patterns, odd and even last bits
    ties = torch.cat([hi | 0x8000, (hi | 0x8000) | -2147483648]).view(torch.float32)
    got = Q.round_bf16(ties)
    assert torch.equal(got, ties.bfloat16().float())
    up = (torch.cat([hi, hi]) >> 16) & 1                                 # an odd pattern rounds away from zero, an even one stays
    assert torch.equal(got.abs().view(torch.int32), torch.cat([hi, hi]) + (up << 16))
    assert int(up.sum()) not in (0, up.numel())
    for near in (0x7FFF, 0x8001):                                       # one ulp to either side of the tie
        v = (hi | near).view(torch.float32)
        assert torch.equal(Q.round_bf16(v), v.bfloat16().float())
    with pytest.raises(AssertionError):
        Q.round_bf16(x.double())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_identity_hook_gives_the_unhooked_bits(dtype):
    """The block with the hook at its twelve operand sites is bb_backward_ref's block when the hook is the identity, bit for bit; the
    hook is called at exactly those sites."""
    r = np.random.Generator(np.random.Philox(key=[11, 0xBF16]))
    N, H, W, C = 2, 3, 3, 64
    shapes = {"gamma": (C,), "conv_dw.weight": (C, 1, 7, 7), "conv_dw.bias": (C,), "norm.weight": (C,), "norm.bias": (C,),
              "mlp.fc1.weight": (4 * C, C), "mlp.fc1.bias": (4 * C,), "mlp.fc2.weight": (C, 4 * C), "mlp.fc2.bias": (C,)}
    P = {k: T(r.standard_normal(s).astype(np.float32) * np.float32(0.3)).to(dtype) for k, s in shapes.items()}
    x, g = (T(r.standard_normal((N, H, W, C)).astype(np.float32)).to(dtype) for _ in range(2))
    calls = []

    def ident(t):
        calls.append(tuple(t.shape))
        return t
    want = R.block_forward(x, P)
    got = Q.block_forward(x, P, ident)
    assert len(calls) == 4
    want_b, got_b = R.block_backward(g, x, P, want), Q.block_backward(g, x, P, got, ident)
    assert len(calls) == 12
    for a, b in ((want, got), (want_b, got_b)):
        assert list(a) == list(b)
        for k in a:
            assert a[k].dtype == b[k].dtype == dtype and torch.equal(a[k], b[k]), k
    # the hooked block differs, by about a bf16 rounding and no more
    if dtype == torch.float32:
        hooked = Q.block_forward(x, P, Q.round_bf16)
        d = float((hooked["h"] - want["h"]).abs().max() / want["h"].abs().max())
        assert 2.0 ** -14 < d < 2.0 ** -6, d


def test_backbone_with_identity_hook_is_the_restatement():
    dims, depths, B, S = R.CASES["A"]
    params, img, g = R.case_inputs("A")
    want = R.reference("A")[1]
    got = R.flat(Q.backbone_run(params, img, g, dims, depths, torch.float32, Q.identity))
    assert list(got) == list(want) and all(np.array_equal(got[k], want[k]) for k in want)
    assert R.block_forward.__module__ == "bb_backward_ref"      # the module is as it was


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build
    hdr = _header("givepose_bbgrad_bf16.h")
    declared = set(re.findall(r"\b(gpbm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.BBGRAD_BF16_PROTOTYPES) and len(declared) == 9
    assert re.search(r"#define GPB_PREC_F32 0\b", hdr) and re.search(r"#define GPB_PREC_BF16 1\b", hdr)
    assert (_lib.GPB_PREC_F32, _lib.GPB_PREC_BF16) == (0, 1)
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gpbm_[a-z0-9_]+)", out)) == declared
    # the kernel lives in its own header; the fp32 functor GEMM and the families built on it are not touched by including it
    src = open(os.path.join(ROOT, "givepose_amd", "csrc", "bbgrad.hip")).read()
    assert '#include "grad_gemm_bf16.hpp"' in src
    k = open(os.path.join(ROOT, "givepose_amd", "csrc", "grad_gemm_bf16.hpp")).read()
    assert "__builtin_amdgcn_mfma_f32_32x32x16_bf16" in k and not re.search(r"\batomic\w*\s*\(", k)
    for other in ("pnpgrad.hip", "xyzgrad.hip", "encgrad.hip"):
        assert "grad_gemm_bf16" not in open(os.path.join(ROOT, "givepose_amd", "csrc", other)).read()
    # size queries: precision 0 is the fp32 query, an unknown precision has no workspace
    lib = _lib.load()
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    base, deep = ints((128, 256, 512, 1024)), ints((3, 3, 27, 3))
    assert lib.gpbm_block_workspace(1, 8, 8, 1024, 0) == lib.gpb_block_workspace(1, 8, 8, 1024) > 0
    assert lib.gpbm_block_workspace(1, 8, 8, 1024, 1) > 0 and lib.gpbm_block_workspace(1, 8, 8, 1000, 1) == 0
    assert lib.gpbm_block_workspace(1, 8, 8, 1024, 2) == 0 and lib.gpbm_block_workspace(1, 8, 8, 1024, -1) == 0
    for q, f in ((lib.gpbm_backbone_forward_workspace, lib.gpb_backbone_forward_workspace),
                 (lib.gpbm_backbone_backward_workspace, lib.gpb_backbone_backward_workspace)):
        assert q(base, deep, 4, 2, 256, 0) == f(base, deep, 4, 2, 256) > 0
        assert q(base, deep, 4, 2, 256, 1) > 0 and q(base, deep, 4, 2, 256, 7) == 0 and q(base, deep, 4, 2, 48, 1) == 0
    # the split of k depends on the shape alone: few tiles are split (partial sums in the workspace), 256 tiles are not
    assert lib.gpbm_matmul_bf16_workspace(64, 4096, 1024) == 4 * 16 * 64 * 4096
    assert lib.gpbm_matmul_bf16_workspace(2048, 2048, 96) == 0 and lib.gpbm_matmul_bf16_workspace(300, 200, 31) == 0
    assert lib.gpbm_matmul_bf16_workspace(0, 4, 4) == 0


def test_public_surface_and_refusals():
    from givepose_amd import PoseNet, PoseNetConfig, _lib, bb_grad
    for fn in (bb_grad.block_forward_save, bb_grad.block_backward, bb_grad.backbone_forward_save, bb_grad.backbone_backward):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["alloc", "precision"] and p["precision"].default == "fp32", fn.__name__
    p = inspect.signature(bb_grad.matmul_bf16).parameters
    assert list(p) == ["a", "b", "trans_a", "trans_b", "alloc"] and p["trans_a"].default is False and p["trans_b"].default is False
    # the precision is checked before anything touches a device
    for bad in ("fp16", "BF16", 1, None):
        with pytest.raises(ValueError, match="expected 'fp32' or 'bf16'"):
            bb_grad.block_forward_save(torch.zeros(1, 1, 1, 64), {}, precision=bad)
        with pytest.raises(ValueError, match="expected 'fp32' or 'bf16'"):
            bb_grad.backbone_backward({}, {}, torch.zeros(1, 3, 32, 32), torch.zeros(1, 1024, 1, 1), PoseNetConfig(), precision=bad)
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        bb_grad.matmul_bf16(torch.zeros(2, 2), torch.zeros(2, 2))
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        bb_grad.block_forward_save(torch.zeros(1, 1, 1, 64), {}, precision="bf16")
    net = PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1)))
    assert net.backward_precision == "fp32"
    assert net.set_backward_precision("bf16") is net and net.backward_precision == "bf16"
    assert net.set_backward_precision("fp32").backward_precision == "fp32"
    with pytest.raises(ValueError, match="expected 'fp32' or 'bf16'"):
        net.set_backward_precision("fp16")
    assert net.backward_precision == "fp32"
    with pytest.raises(AttributeError):
        net.backward_precision = "bf16"
    assert PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1))).backward_precision == "fp32"      # per instance
