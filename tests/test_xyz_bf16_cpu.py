"""CPU: the restatement of the "bf16" precision of the coordinate heads (tests/xyz_bf16_ref.py) and the public surface of the mode
(include/givepose_xyzgrad_bf16.h, givepose_amd/xyz_grad.py, PoseNet.set_backward_precision(mode, xyz_heads=))."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import xyz_backward_ref as R
import xyz_bf16_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = R.CASES[0]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_identity_hook_gives_the_unhooked_bits(dtype):
    """The head with the hook at the operands of its 3x3 layers is xyz_backward_ref's head when the hook is the identity, bit for bit, and
    the hook is called at exactly those sites: 2 per forward contraction, 3 per layer of the backward (dY serves dX and dW)."""
    params, feat, g, _, _ = R.case_reference(SMALL)
    calls = []

    def ident(t):
        calls.append(tuple(t.shape))
        return t
    want = R.head_run(params, feat, g, dtype)
    got = Q.head_run(params, feat, g, dtype, ident)
    assert len(calls) == 7 * 2 + 7 * 3
    assert calls[0] == (3, 512, 2, 2) and calls[1] == (512, 256, 3, 3) and calls[-3] == (3, 256, 4, 4)
    for part in ("saved", "grads"):
        assert list(want[part]) == list(got[part])
        for k, v in want[part].items():
            assert got[part][k].dtype == v.dtype and np.array_equal(got[part][k], v), (part, k)
    # the module is as it was
    assert R.conv3x3_forward is Q._PLAIN["conv3x3_forward"] and R.deconv_backward.__module__ == "xyz_backward_ref"


def test_hooked_figure_is_above_the_fp32_floor():
    """The bf16-hooked float32 figure against float64 is well above 2^-24 for every tensor that a contraction of a 3x3 layer feeds:
    the yardstick of the GPU test compares against a bf16-sized figure, not against the fp32 floor.  out_layer.bias is the one tensor no
    such contraction feeds -- it is the plain sum of g_coor -- and there the hooked run has the unhooked run's bits."""
    params, feat, g, fig32, r64 = R.case_reference(SMALL)
    hooked = Q.case_reference_bf16(SMALL)
    fig = R.rel_figures(hooked, Q.flat(r64))
    assert len(fig) == 31 + 24
    plain = Q.flat(R.head_run(params, feat, g, torch.float32))
    for k, v in fig.items():
        print(f"{SMALL} {k}: hooked {v:.2e}, float32 {fig32[k]:.2e}")
        if k == "out_layer.bias":
            assert np.array_equal(hooked[k], plain[k])
        else:
            assert v > 2.0 ** -16 and v > 16 * fig32[k], (k, v, fig32[k])      # 2^-16 = 256 x the floor
        assert v < 2.0 ** -4, (k, v)
    # the rounding is in the first contraction already
    d = np.max(np.abs(hooked["pre0"] - plain["pre0"])) / np.max(np.abs(plain["pre0"]))
    assert 2.0 ** -14 < d < 2.0 ** -6, d


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build
    hdr = _header("givepose_xyzgrad_bf16.h")
    declared = set(re.findall(r"\b(gpxm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.XYZGRAD_BF16_PROTOTYPES) and len(declared) == 10
    assert '#include "givepose_xyzgrad.h"' in hdr and "gpx_xyz_params" in hdr and "typedef" not in hdr      # the gpx_ structs, reused
    assert re.search(r"#define GPX_PREC_F32 0\b", hdr) and re.search(r"#define GPX_PREC_BF16 1\b", hdr)
    assert (_lib.GPX_PREC_F32, _lib.GPX_PREC_BF16) == (0, 1)
    for name, (args, res) in _lib.XYZGRAD_BF16_PROTOTYPES.items():      # the gpx_ prototype and a trailing int
        base = _lib.XYZGRAD_PROTOTYPES["gpx_" + name[len("gpxm_"):]]
        assert args == base[0] + [_lib.c_int] and res is base[1], name
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gpxm_[a-z0-9_]+)", out)) == declared
    # the gpx_ family is what it was
    gpx = set(re.findall(r"\b(gpx_[a-z0-9_]+)\s*\(", _header("givepose_xyzgrad.h")))
    assert gpx == set(_lib.XYZGRAD_PROTOTYPES) == set(re.findall(r" T (gpx_[a-z0-9_]+)", out)) and len(gpx) == 16
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)


def test_size_queries():
    """Precision 0 is the gpx_ query; a bad shape and an unknown precision have no workspace: 0, not a fault on the host."""
    from givepose_amd import _lib
    lib = _lib.load()
    for q, f, good, bads in ((lib.gpxm_conv3x3s1_workspace, lib.gpx_conv3x3s1_workspace, (3, 256, 256, 16), ((0, 8, 8, 8), (1, 8, 0, 8), (1, 8, 8, 5000))),
                             (lib.gpxm_deconv3x3s2_workspace, lib.gpx_deconv3x3s2_workspace, (3, 64, 256, 2), ((1, 8, 8, 0), (1, 0, 8, 2))),
                             (lib.gpxm_xyz_forward_workspace, lib.gpx_xyz_forward_workspace, (2, 512, 2), ((0, 512, 8), (2, 0, 8), (2, 512, 65))),
                             (lib.gpxm_xyz_backward_workspace, lib.gpx_xyz_backward_workspace, (2, 512, 8), ((0, 512, 8), (5000, 512, 8), (2, 512, 0)))):
        assert q(*good, 0) == f(*good) > 0
        assert q(*good, 1) > 0
        for prec in (2, -1, 7):
            assert q(*good, prec) == 0
        for bad in bads:
            assert q(*bad, 0) == 0 and q(*bad, 1) == 0 and f(*bad) == 0, bad
    # the bf16 form tiles 128 x 128 and splits k into chunks that are multiples of 32.  The largest of the three contractions of this
    # conv is dW, 256 x 2304 x 768: 36 tiles, 512 / 36 = 14 chunks wanted, 64 per chunk, 12 partial sums
    assert lib.gpxm_conv3x3s1_workspace(3, 256, 256, 16, 1) == 4 * 12 * 256 * 2304
    assert lib.gpxm_conv3x3s1_workspace(3, 256, 256, 16, 1) != lib.gpx_conv3x3s1_workspace(3, 256, 256, 16)
    # the two-map layout of the backward stays: two maps of the largest size in front of the scratch
    assert lib.gpxm_xyz_backward_workspace(2, 512, 8, 1) >= 2 * 4 * 2 * 256 * 64 * 64


def test_public_surface_and_setter():
    from givepose_amd import PoseNet, PoseNetConfig, _lib, xyz_grad
    for fn in (xyz_grad.conv3x3s1_forward, xyz_grad.conv3x3s1_backward, xyz_grad.deconv3x3s2_forward, xyz_grad.deconv3x3s2_backward,
               xyz_grad.xyz_forward_save, xyz_grad.xyz_backward):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["alloc", "precision"] and p["precision"].default == "fp32", fn.__name__
    # the precision is checked before anything touches a device
    z = torch.zeros(1, 3, 5, 5)
    for bad in ("fp16", "BF16", 1, None):
        with pytest.raises(ValueError, match="expected 'fp32' or 'bf16'"):
            xyz_grad.conv3x3s1_forward(z, torch.zeros(5, 3, 3, 3), precision=bad)
        with pytest.raises(ValueError, match="expected 'fp32' or 'bf16'"):
            xyz_grad.xyz_backward({}, {}, torch.zeros(1, 512, 2, 2), torch.zeros(1, 3, 16, 16), precision=bad)
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        xyz_grad.deconv3x3s2_forward(z, torch.zeros(3, 5, 3, 3), precision="bf16")
    net = PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1)))
    p = inspect.signature(PoseNet.set_backward_precision).parameters
    assert list(p) == ["self", "mode", "xyz_heads"] and p["xyz_heads"].default == "fp32"
    assert (net.backward_precision, net.xyz_backward_precision) == ("fp32", "fp32")
    assert net.set_backward_precision("bf16", xyz_heads="bf16") is net
    assert (net.backward_precision, net.xyz_backward_precision) == ("bf16", "bf16")
    net.set_backward_precision("bf16")      # every call sets both: the heads are back at fp32
    assert (net.backward_precision, net.xyz_backward_precision) == ("bf16", "fp32")
    net.set_backward_precision("fp32", xyz_heads="bf16")
    assert (net.backward_precision, net.xyz_backward_precision) == ("fp32", "bf16")
    for bad in ("fp16", "BF16", 1, None):
        with pytest.raises(ValueError, match="xyz_heads.*'fp32' or 'bf16'"):
            net.set_backward_precision("bf16", xyz_heads=bad)
    with pytest.raises(ValueError, match="set_backward_precision: 'fp16', expected 'fp32' or 'bf16'"):
        net.set_backward_precision("fp16", xyz_heads="bf16")
    assert (net.backward_precision, net.xyz_backward_precision) == ("fp32", "bf16")      # a refused call changes nothing
    assert net.set_backward_precision("fp32").xyz_backward_precision == "fp32"
    with pytest.raises(AttributeError):
        net.xyz_backward_precision = "bf16"
    assert PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1))).xyz_backward_precision == "fp32"      # per instance
