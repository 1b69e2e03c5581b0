"""CPU: the ordered d xp of the encoder's DCNv3 core (include/givepose_encgrad_ordered.h, gpeo_*): the numpy float32 restatement of its
contract (tests/enc_ordered_ref.py) against float64, the registration of the family, its source rules, the workspace queries and the
PoseNet switch.

The restatement against float64.  Per element |ordered - float64| <= the grad_input bound of tests/dcnv3_backward_reference.py,
(n + 6) (2^-24 a + 2^-126) with n the number of terms that reach the element and a the sum of their absolute values: that bound counts
5 roundings per term and n - 1 additions IN ANY ORDER, so the ascending-id order is one of the orders it covers; a bound of 0 asks
for an exact zero.  The float64 side is enc_backward_ref.core_backward; it forms the locations in float64, so it is the reference of
the same operands only where the float32 location is exact -- the cases here: offsets on a 2^-10 grid, the edge tables and the pile-up
case.  The continuous offsets of the second edge geometry are held against dcnv3_backward_reference.ref's own value, which is float64
at the float32 location.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dcnv3_backward_reference as DB
import dcnv3_reference as DR
import enc_backward_ref as R
import enc_ordered_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy

EDGES = DR.mk("core-edges-N2-5x8", torch.float32, N=2, H=5, W=8, s=2, iset="edges", logits=True)      # test_enc_backward_gpu.CORE_EDGE_CASES
C3 = DR.mk("core-c3-N1-7x4", torch.float32, N=1, H=7, W=4, s=2, logits=True)


def edge_case(c):
    I = DR.inputs(c)
    rows = DR.n_rows(c)
    return (I["x"].numpy(), I["off"].view(rows, 72).numpy(), I["mask"].view(rows, 36).numpy(), DB.grad_output(c).numpy()), (c.N, c.H, c.W)


def cases():
    return {"1x1x1": (O.random_case(1, 1, 1, seed=11, grid=2.0 ** -10), (1, 1, 1)),
            "edges-2x5x8": edge_case(EDGES),
            "random-3x8x8": (O.random_case(3, 8, 8, seed=12, grid=2.0 ** -10), (3, 8, 8)),
            "pile-up-1x16x16": (O.pile_up_case(), (1, 16, 16)),
            "threshold-1x8x8": (O.threshold_case(), (1, 8, 8)),
            "c3-1x7x4": edge_case(C3)}


def float64_bound(xp, off, mask, dy, N, H, W):
    """(value, bound) of grad_input from dcnv3_backward_reference on these operands (float32 location, float64 behind it)."""
    c = DR.mk(f"ordered-{N}-{H}-{W}", torch.float32, N=N, H=H, W=W, s=2, entry="any")
    r = DB.ref(dict(x=T(xp), off=T(off).reshape(-1), mask=T(mask).reshape(-1), gout=T(dy)), c)
    return tuple(t.numpy() for t in r["grad_input"])


@pytest.mark.parametrize("name", list(cases()))
def test_restatement_against_float64(name):
    (xp, off, logits, dy), (N, H, W) = cases()[name]
    mask = O.softmax_mask(logits)
    got, lengths = O.ordered_dxp(off, mask, dy, N, H, W)
    assert got.dtype == np.float32 and got.shape == (N, H, W, 256) and lengths.shape == (N, H, W, 4)
    v, bound = float64_bound(xp, off, mask, dy, N, H, W)
    if name != "c3-1x7x4":      # exact float32 locations: enc_backward_ref's float64 is the reference of the same operands
        l32, l64 = R.core_locations(T(off), N, H, W), R.core_locations(T(off).double(), N, H, W)
        assert all(torch.equal(a.double(), b) for a, b in zip(l32, l64))
        v64 = R.core_backward(T(xp).double(), T(off).double(), T(mask).double(), T(dy).double())[0].numpy()
        assert np.max(np.abs(v64 - v)) <= 1e-12 * max(1.0, np.max(np.abs(v)))
        v = v64
    err = np.abs(got.astype(np.float64) - v)
    print(f"{name}: max |ordered - float64| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}, lists up to {lengths.max()}")
    assert np.all(err <= bound) and np.any(v != 0)
    # a destination nothing reaches is +0 (not -0), and the list lengths are the reference's term counts
    empty = np.repeat(lengths == 0, 64, axis=-1).reshape(got.shape)
    assert np.all(got[empty].view(np.int32) == 0)
    n_terms = DB._evaluate(DR.mk("n", torch.float32, N=N, H=H, W=W, s=2, entry="any"),
                           dict(x=T(xp), off=T(off).reshape(-1), mask=T(mask).reshape(-1), gout=T(dy)), torch.float64)["n"]
    assert np.array_equal(n_terms.numpy().reshape(N, H, W, 4, 64)[..., 0], lengths)
    if name == "pile-up-1x16x16":
        assert lengths.max() == 64 * 9 > 64 and (lengths == 576).sum() == 16 and (lengths == 0).sum() == lengths.size - 16
        assert np.all(lengths[0, 2:4, 3:5] == 576)      # the cell around (w, h) = (3.25, 2.5)
    if name == "random-3x8x8":
        assert (lengths == 0).any() and (lengths == 1).any() and (lengths >= 2).any()
    if name == "threshold-1x8x8":      # either side of the gather's one-id-per-lane limit
        assert all(np.all(lengths[0, 2:4, 3:5, g] == n) for g, n in enumerate(O.THRESHOLD_COUNTS)) and lengths.sum() == 4 * sum(O.THRESHOLD_COUNTS)
        assert O.THRESHOLD_COUNTS[:3] == (64, 65, 63)


def test_order_matters_and_is_the_source_id():
    """The restatement really adds in ascending id: summing the same terms of a long list in descending order gives other bits."""
    (xp, off, logits, dy), (N, H, W) = cases()["pile-up-1x16x16"]
    mask = O.softmax_mask(logits)
    got, lengths = O.ordered_dxp(off, mask, dy, N, H, W)
    # the pixel (h, w) = (2, 3), group 0: corner 1 of all 576 taps, weight fmul(hh, hw) = 0.5 x 0.75
    wk = np.float32(0.5) * np.float32(0.75)
    terms = np.stack([wk * (dy[row, :64] * mask[row, q]) for row in range(64) for q in range(9)])      # id order: (row 9 + q) 4 + 0
    up, down = np.zeros(64, np.float32), np.zeros(64, np.float32)
    for t in terms:
        up = up + t
    for t in terms[::-1]:
        down = down + t
    assert np.array_equal(up.view(np.int32), got[0, 2, 3, :64].view(np.int32))
    assert not np.array_equal(down.view(np.int32), up.view(np.int32))


# ------------------------------------------------------------------------------------------------ registration and source rules
def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build
    hdr = _header("givepose_encgrad_ordered.h")
    declared = set(re.findall(r"\b(gpeo_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.ENCGRAD_ORDERED_PROTOTYPES) and len(declared) == 4
    tables = {n: getattr(_lib, n) for n in dir(_lib) if n.endswith("PROTOTYPES")}
    assert len(tables) >= 16 and "ENCGRAD_ORDERED_PROTOTYPES" in tables
    for n, other in tables.items():
        if n != "ENCGRAD_ORDERED_PROTOTYPES":
            assert not set(other) & declared and not any(k.startswith("gpeo_") for k in other), n
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "givepose_encgrad_ordered.h":
            assert "gpeo_" not in _header(name), name
    assert '#include "givepose_encgrad.h"' in hdr and "typedef" not in hdr      # gpe_enc_params / gpe_enc_saved are reused
    consts = {k: int(v) for k, v in re.findall(r"#define (GPE_SCATTER_[A-Z]+) (\d+)", hdr)}
    assert consts == {"GPE_SCATTER_ATOMIC": _lib.GPE_SCATTER_ATOMIC, "GPE_SCATTER_ORDERED": _lib.GPE_SCATTER_ORDERED} == {
        "GPE_SCATTER_ATOMIC": 0, "GPE_SCATTER_ORDERED": 1}
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gpeo_[a-z0-9_]+)", out)) == declared
    assert "encscatter.hip" in build.SOURCES and "encgrad.hip" in build.SOURCES
    bsrc = open(os.path.join(ROOT, "givepose_amd", "build.py")).read()
    assert "givepose_encgrad_ordered.h" in bsrc and "encscatter.hpp" in bsrc
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared)
    # the gpe_ forms with a trailing scatter (and, for the core, a workspace)
    P, E = _lib.ENCGRAD_ORDERED_PROTOTYPES, _lib.ENCGRAD_PROTOTYPES
    assert P["gpeo_map_encoder_backward"][0][:-1] == E["gpe_map_encoder_backward"][0]
    assert P["gpeo_dcnv3_core_backward"][0][:-3] == E["gpe_dcnv3_core_backward"][0]
    assert P["gpeo_map_encoder_backward_workspace"][0][:-1] == E["gpe_map_encoder_backward_workspace"][0]


def test_the_new_source_has_no_float_atomic_and_no_zero_fill():
    src = open(os.path.join(ROOT, "givepose_amd", "csrc", "encscatter.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    # the only atomics are integer increments of the counters / cursors: their result decides a count or a slot, never a sum
    targets = re.findall(r"\batomic\w*\s*\(\s*([^,]+),", code, flags=re.I)
    assert targets == ["slots + d"] and re.search(r"\bint\* slots\b", code) and not re.search(r"float\s*\*\s*slots", code)
    assert "memset" not in code.lower() and not re.search(r"\basm\b", code)
    assert "fmaf" not in code and code.count("#pragma clang fp contract(off)") == 2
    # encgrad.hip gained the switch and the call, and kept its four scatter lines
    enc = open(os.path.join(ROOT, "givepose_amd", "csrc", "encgrad.hip")).read()
    assert enc.count("atomicAdd(") == 4 and enc.count("if (SCATTER) atomicAdd(gim") == 4
    assert "encscatter::ordered_dxp(" in enc and "gather_kernel" not in enc


def test_gather_rounds_every_product_and_sum_on_its_own(tmp_path):
    """hipcc contracts a * b + c by default: the gather kernel's code must hold no fused multiply-add (its address arithmetic is
    integer), and it uses no scratch."""
    import shutil
    from givepose_amd import _lib, build
    build.build(verbose=False)
    lib = shutil.copy(_lib.LIB_PATH, tmp_path / "lib.so")
    subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", str(lib)], capture_output=True, text=True)
    found = 0
    for f in sorted(tmp_path.glob("lib.so.*gfx950")):
        whole = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(f)], text=True)
        # the kernel of csrc/encscatter.hip by its signature: (offset, mask, dy, start, end, ids, ...)
        for name, dis in re.findall(r"^[0-9a-f]+ <(\S*13gather_kernelEPKfS1_S1_PKiS3_S3_\S*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", whole, flags=re.M | re.S):
            assert "v_mul_f32" in dis and "v_add_f32" in dis and "s_load_dword" in dis and "s_endpgm" in dis, name
            assert not re.findall(r"\bv_(?:fma|fmac|mad|mac)_(?:f32|legacy_f32)\b", dis), name
            found += 1
    assert found == 1


def test_workspace_queries():
    from givepose_amd import _lib
    lib = _lib.load()
    A, Od = _lib.GPE_SCATTER_ATOMIC, _lib.GPE_SCATTER_ORDERED
    for N, R_ in ((1, 16), (2, 64), (64, 64)):
        atomic, ordered = lib.gpeo_map_encoder_backward_workspace(N, R_, A), lib.gpeo_map_encoder_backward_workspace(N, R_, Od)
        assert atomic == lib.gpe_map_encoder_backward_workspace(N, R_) > 0 and ordered > atomic      # the default's size is the parent's
        # the encoder's increase is layer 0's index: two ints per destination, the scan's tile sums, one id per corner
        ndest, rows = N * R_ * R_ * 4, N * (R_ // 2) ** 2
        up = lambda n: (n + 63) // 64 * 64
        index = 4 * (2 * up(ndest) + up(-(-ndest // 1024)) + up(rows * 144))
        assert lib.gpeo_dcnv3_core_backward_workspace(N, R_, R_, Od) == index and 0 < ordered - atomic <= index
    assert lib.gpeo_dcnv3_core_backward_workspace(2, 5, 8, A) == 0 < lib.gpeo_dcnv3_core_backward_workspace(2, 5, 8, Od)
    assert lib.gpeo_dcnv3_core_backward_workspace(1, 1, 1, Od) > 0
    for bad in ((0, 64), (2, 0), (2, 60), (5000, 64), (2, 1024)):
        assert lib.gpeo_map_encoder_backward_workspace(*bad, A) == 0 and lib.gpeo_map_encoder_backward_workspace(*bad, Od) == 0, bad
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 5000), (4096, 64, 64)):
        assert lib.gpeo_dcnv3_core_backward_workspace(*bad, Od) == 0, bad
    for mode in (-1, 2, 7):      # an unknown mode has no workspace and is refused by name before anything else is looked at
        assert lib.gpeo_map_encoder_backward_workspace(2, 64, mode) == 0 and lib.gpeo_dcnv3_core_backward_workspace(2, 8, 8, mode) == 0
        rc = lib.gpeo_dcnv3_core_backward(None, None, None, None, 2, 8, 8, None, None, None, None, mode, None, 0)
        assert rc != 0 and f"unknown scatter mode {mode}" in lib.gp_last_error().decode()
        rc = lib.gpeo_map_encoder_backward(None, None, None, None, 2, 64, None, None, None, 0, None, mode)
        assert rc != 0 and f"unknown scatter mode {mode}" in lib.gp_last_error().decode()
    assert ctypes.sizeof(_lib.EncParams) == 48 * ctypes.sizeof(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ Python surface
def test_enc_grad_keyword_and_keys():
    from givepose_amd import enc_grad
    for fn in (enc_grad.dcnv3_core_backward, enc_grad.enc_backward):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["alloc", "scatter"] and p["scatter"].default == "atomic" and p["alloc"].default is None
    assert enc_grad.ORDERED_FREE_KEYS == enc_grad.PARAM_KEYS and len(enc_grad.ORDERED_FREE_KEYS) == 48
    assert len(enc_grad.ATOMIC_FREE_KEYS) == 12 and set(enc_grad.ATOMIC_FREE_KEYS) < set(enc_grad.ORDERED_FREE_KEYS)
    assert enc_grad.scatter_mode("atomic") == 0 and enc_grad.scatter_mode("ordered") == 1
    z = torch.zeros(1, 1, 1, 256)
    for bad in ("sorted", "", None, 1):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            enc_grad.dcnv3_core_backward(z, torch.zeros(1, 72), torch.zeros(1, 36), torch.zeros(1, 256), scatter=bad)
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            enc_grad.enc_backward({}, [], torch.zeros(1, 3, 8, 8), torch.zeros(1, 256, 1, 1), scatter=bad)
    from givepose_amd import _lib
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):      # a known mode still has no CPU path
        enc_grad.dcnv3_core_backward(z, torch.zeros(1, 72), torch.zeros(1, 36), torch.zeros(1, 256), scatter="ordered")


def test_posenet_switch_surface_default_and_refusal():
    from givepose_amd import PoseNet, PoseNetConfig
    net = PoseNet(PoseNetConfig())
    assert net.encoder_scatter == "atomic" and isinstance(PoseNet.encoder_scatter, property) and PoseNet.encoder_scatter.fset is None
    with pytest.raises(AttributeError):
        net.encoder_scatter = "ordered"
    assert net.set_encoder_scatter("ordered") is net and net.encoder_scatter == "ordered"
    assert PoseNet(PoseNetConfig()).encoder_scatter == "atomic"      # per network, not global
    for bad in ("Ordered", "sorted", None, 1):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            net.set_encoder_scatter(bad)
        assert net.encoder_scatter == "ordered"      # a refused value changes nothing
    assert net.set_encoder_scatter("atomic").encoder_scatter == "atomic"
    assert list(inspect.signature(PoseNet.set_encoder_scatter).parameters) == ["self", "mode"]
    assert list(inspect.signature(PoseNet.map_encoder_backward).parameters) == ["self", "coor", "g_nocs_feat", "groups", "device", "return_saved"]
    doc = PoseNet.map_encoder_backward.__doc__
    assert "ordered" in doc and "equal" in doc and "rounding" in doc
