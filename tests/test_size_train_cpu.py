"""CPU: the train-mode size head (include/givepose_sizegrad.h, gps_*; givepose_amd/size_grad.py) -- the float64 restatement
tests/size_head_ref.py against the reference's own SizeHead in .train() (tests/golden/size_head_train_*.npz,
scripts/gen_golden_size_head.py), the numpy restatement of the seeded mask rule, the family's registration, names and shapes, and the
properties the GPU tests rely on (no ties, no y near zero in any case's float64 reference).

The restatement in float64 and the golden float64 run evaluate the same formulas in the same precision with the reference's own mask:
every stored figure is asked to 1e-12 of the tensor's largest magnitude; conv1.bias, whose gradient is analytically zero, to 1e-12 of
max_f sum_b |dh|, the size of the terms that cancel in it.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import size_head_ref as R

ROOT = R.ROOT
TOL = 1e-12


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_restatement_float64_reproduces_the_reference(name):
    gold = np.load(os.path.join(R.GOLDEN, f"size_head_train_{name}.npz"))
    case = R.golden_case(name)
    assert int(gold["input_crc"]) == R.case_crc(case), "the seeded inputs changed: regenerate with scripts/gen_golden_size_head.py"
    case["keep"] = gold["keep"]                     # the mask the reference drew
    ref = R.reference(case, torch.float64)
    B, C, HW = case["feat"].shape
    worst = 0.0
    for k in ("out",) + R.PARAM_KEYS:
        want, got = gold["f64_" + k], ref[k].numpy()
        scale = float(ref["dh"].abs().sum(0).max()) if k == "conv1.bias" else np.abs(want).max()
        assert got.shape == want.shape and np.abs(got - want).max() <= TOL * scale, k
        worst = max(worst, np.abs(got - want).max() / scale)
    arg = torch.from_numpy(gold["f64_feat_arg"].astype(np.int64))
    assert torch.equal(arg, ref["arg"])
    dense = torch.zeros(B, C, HW, dtype=torch.float64).scatter_(2, arg[:, :, None], torch.from_numpy(gold["f64_feat_values"])[:, :, None])
    assert float((dense - ref["feat"]).abs().max()) <= TOL * float(dense.abs().max())
    for calls in (1, 2):
        r = ref if calls == 1 else R.reference(case, torch.float64, calls=2)
        for k in ("running_mean", "running_var"):
            want = gold[f"f64_{k}_{calls}"]
            assert np.abs(r[k].numpy() - want).max() <= TOL * np.abs(want).max(), (k, calls)
        assert int(r["num_batches_tracked"]) == calls
    # the statistics the update takes are the restatement's: running = 0.9 * (0 | 1) + 0.1 * statistic
    assert np.abs(0.1 * ref["mean"].numpy() - gold["f64_running_mean_1"]).max() <= TOL * np.abs(gold["f64_running_mean_1"]).max()
    assert np.abs(0.9 + 0.1 * ref["var_unbiased"].numpy() - gold["f64_running_var_1"]).max() <= TOL
    print(f"{name}: largest |restatement - reference| / scale {worst:.2e}")


def test_every_case_is_free_of_ties_and_of_y_near_zero():
    """What the GPU operator test relies on, checked where it is cheap: on the float64 reference of every case."""
    for shape in R.SHAPES:
        for scale in R.SCALES:
            c, r64, _ = R.cached_reference(shape, scale)
            assert not R.has_ties(c["feat"]), (shape, scale)
            assert np.array_equal(c["feat"], c["feat"].astype(np.float16).astype(np.float32)), (shape, scale, "fp16-representable")
            assert R.gate_margin(r64) > R.GATE_MARGIN, (shape, scale, R.gate_margin(r64))
            assert 0 < c["keep"].mean() < 1
    for name in R.GOLDEN_CASES:
        c = R.golden_case(name)
        assert not R.has_ties(c["feat"]) and R.gate_margin(R.reference(c, torch.float64)) > R.GATE_MARGIN, name
    # "init": the batch variance is of the order of eps, so a wrong eps would show
    _, r64, _ = R.cached_reference((2, 64, 4, 16), "init")
    var = r64["var_unbiased"] / 2
    assert float(var.min()) < 10 * R.BN_EPS and float(var.max()) > 0.01 * R.BN_EPS


def test_untie_moves_the_first_of_equal_maxima_up_one_fp16_step():
    f = np.array([[[1.0, 3.0, 3.0, 2.0], [0.5, 0.25, 0.125, 0.0]]], np.float32)
    assert R.has_ties(f) and R.untie(f) == 1 and not R.has_ties(f)
    assert f[0, 0, 1] == np.float32(3.0) + np.float32(2.0 ** -9) and f[0, 0, 2] == 3.0 and f[0, 1, 0] == 0.5


# ------------------------------------------------------------------------------------------------ the seeded mask rule
def test_seeded_mask_share_repeatability_and_seed_dependence():
    n = 1 << 16
    sd = np.sqrt(0.8 * 0.2 / n)
    for seed in (0, 7, 0x0123456789ABCDEF, (1 << 64) - 1):
        m = R.keep_mask(seed, 512, 128)
        assert m.dtype == np.uint8 and m.shape == (512, 128) and set(np.unique(m)) == {0, 1}
        assert abs(m.mean() - 0.8) <= 4 * sd, (seed, m.mean())
        assert np.array_equal(m, R.keep_mask(seed, 512, 128))                    # the same seed repeats
        assert np.array_equal(m.reshape(-1)[:40 * 16], R.keep_mask(seed, 40, 16).reshape(-1))      # a unit's fate depends on b F + f alone
    a, b, c = R.keep_mask(7, 512, 128), R.keep_mask(8, 512, 128), R.keep_mask(7 + (1 << 32), 512, 128)
    for x, y in ((a, b), (a, c), (b, c)):                                        # two seeds differ, in either half of the seed
        assert abs((x != y).mean() - 2 * 0.8 * 0.2) <= 4 * np.sqrt(0.32 * 0.68 / n)
    # the rule, once by hand in Python integers
    M = 0xFFFFFFFF
    seed, idx = 0x0123456789ABCDEF, 12345
    hi, lo = seed >> 32, seed & M
    x = lo ^ ((idx * 0x9E3779B9) & M) ^ (((hi << 16) | (hi >> 16)) & M)
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M
    x ^= x >> 16
    assert R.keep_mask(seed, 512, 128).reshape(-1)[idx] == int(x >= int(0.2 * 2 ** 32)) and R.DROP_THRESHOLD == int(0.2 * 2 ** 32)


# ------------------------------------------------------------------------------------------------ registration, names, shapes
def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build
    raw = open(os.path.join(ROOT, "include", "givepose_sizegrad.h")).read()
    hdr = _header("givepose_sizegrad.h")
    declared = set(re.findall(r"\b(gps_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIZEGRAD_PROTOTYPES) and len(declared) == 4
    for other in (_lib.PROTOTYPES, _lib.HEADGRAD_PROTOTYPES, _lib.GRAD_PROTOTYPES, _lib.XYZGRAD_PROTOTYPES, _lib.ENCGRAD_PROTOTYPES, _lib.BBGRAD_PROTOTYPES,
                  _lib.OPTIM_PROTOTYPES):
        assert not set(_lib.SIZEGRAD_PROTOTYPES) & set(other)
    for name, (argtypes, _) in _lib.SIZEGRAD_PROTOTYPES.items():
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", hdr).group(1)
        assert len(decl.split(",")) == len(argtypes), name                 # one ctypes entry per declared parameter
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gps_[a-z0-9_]+)", out)) == declared
    assert "sizegrad.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "givepose_amd", "csrc", "sizegrad.hip")).read()
    assert not re.search(r"\batomic\w*\s*\(", src) and "memset" not in src.lower()          # no atomic, no memset plus scatter
    body = lambda a, b: src.split(a)[1].split(b)[0]
    fwd = body("int gps_size_forward_save(", "long long gps_size_backward_workspace(")
    # the pool kernel is one launch in three spellings (layout and dtype)
    assert len(re.findall(r"hipLaunchKernelGGL", fwd)) - 2 == _lib.GPS_FORWARD_LAUNCHES and fwd.count("pool_kernel<") == 3
    assert len(re.findall(r"hipLaunchKernelGGL", body("int gps_size_backward(", "int gps_bn_running_update("))) == _lib.GPS_BACKWARD_LAUNCHES
    consts = {k: int(v) for k, v in re.findall(r"#define (GPS_[A-Z_]+) (\d+)u?\b", hdr)}
    assert consts == {"GPS_CHUNK": _lib.GPS_CHUNK, "GPS_MAX_C": _lib.GPS_MAX_C, "GPS_FORWARD_LAUNCHES": _lib.GPS_FORWARD_LAUNCHES,
                      "GPS_BACKWARD_LAUNCHES": _lib.GPS_BACKWARD_LAUNCHES, "GPS_DROP_THRESHOLD": _lib.GPS_DROP_THRESHOLD}
    assert _lib.GPS_DROP_THRESHOLD == R.DROP_THRESHOLD and re.search(r"#define GPS_BN_EPS 1e-5\s", hdr)
    assert "LOWEST" in raw and "0x9E3779B9" in raw and "0x85EBCA6B" in raw and "0xC2B2AE35" in raw      # the tie rule and the mask rule are stated
    assert ctypes.sizeof(_lib.SizeParams) == 48 and ctypes.sizeof(_lib.SizeSaved) == 88
    # the size query answers on the host; sizes the entry points refuse have no workspace, and the refusal names the size
    lib = _lib.load()
    assert lib.gps_size_backward_workspace(64, 1024, 64, 128) == 64 * 128 * 4 and lib.gps_size_backward_workspace(3, 64, 1, 16) == 256
    for bad, word in (((1, 64, 4, 16), b"B = 1"), ((2, 96, 4, 16), b"C = 96"), ((2, 64, 4, 8), b"F = 8"), ((2, 64, 0, 16), b"HW = 0"),
                      ((2, 8192, 4, 16), b"C = 8192")):
        assert lib.gps_size_backward_workspace(*bad) == 0 and word in lib.gp_last_error(), bad


def test_names_and_shapes():
    import givepose_amd
    from givepose_amd import PoseNet, PoseNetConfig, _lib, size_grad
    assert givepose_amd.size_grad is size_grad
    assert size_grad.PARAM_KEYS == R.PARAM_KEYS == ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "bn1.weight", "bn1.bias")
    assert size_grad.param_shapes(1024, 128) == {"conv1.weight": (128, 1024, 1), "conv1.bias": (128,), "conv2.weight": (3, 128, 1),
                                                 "conv2.bias": (3,), "bn1.weight": (128,), "bn1.bias": (128,)}
    assert list(size_grad.param_shapes(64, 16)) == list(size_grad.PARAM_KEYS)
    assert size_grad.saved_shapes(5, 256, 32) == {"pooled": (5, 256), "arg": (5, 256), "h": (5, 32), "mean": (32,), "mean_lo": (32,), "rstd": (32,),
                                                  "rstd_lo": (32,), "d": (5, 32), "keep": (5, 32), "out": (5, 3), "var_unbiased": (32,)}
    assert tuple(size_grad.saved_shapes(2, 64, 16)) == size_grad.SAVED_KEYS == _lib.SizeSaved.FIELDS
    assert (size_grad.DROP_P, size_grad.BN_EPS, size_grad.BN_MOMENTUM) == (R.P_DROP, R.BN_EPS, R.BN_MOMENTUM)
    # the names are the model's own, in state_dict order, and the optimiser already lists them
    net = PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1)), dtype=torch.float32)
    sd = net.state_dict()
    names = [k for k in sd if k.startswith("size_head.")]
    assert names[:6] == ["size_head." + k for k in size_grad.PARAM_KEYS] and names[6:] == ["size_head." + k for k in size_grad.BUFFER_KEYS]
    cfg = net.cfg
    for k, shp in size_grad.param_shapes(cfg.convnext_dims[-1], cfg.feat_ts).items():
        assert tuple(sd["size_head." + k].shape) == shp, k
    # the public surface: the module-level entry point and the opt-in keyword, off by default
    p = inspect.signature(PoseNet.size_head_backward).parameters
    assert list(p) == ["self", "feat", "g_size", "keep", "seed", "device", "return_saved"] and p["keep"].default is None and p["seed"].default is None
    q = inspect.signature(PoseNet.train_step).parameters
    assert list(q)[-1] == "size_head" and q["size_head"].default is None
    # the chain's methods keep their shared parameter list (existing tests pin it); the two that reach feat take size_head= as a
    # keyword-only option through a decorator, off by default, checked before anything runs
    shared = list(inspect.signature(PoseNet.head_grads).parameters)
    for fn in (PoseNet.head_grads_feat, PoseNet.head_grads_backbone):
        assert list(inspect.signature(fn).parameters) == shared and fn.__kwdefaults__ == {"size_head": None} and "size_head=" in fn.__doc__, fn
        with pytest.raises(ValueError, match="size_head must be"):
            fn(net, {}, None, size_head={"sed": 1})
        with pytest.raises(ValueError, match="exactly one of keep and seed"):
            fn(net, {}, None, size_head={})
    for fn in (PoseNet.head_grads, PoseNet.head_grads_pnp, PoseNet.head_grads_xyz):
        with pytest.raises(TypeError, match="size_head"):
            fn(net, {}, None, size_head={"seed": 1})
    with pytest.raises(ValueError, match="size_head must be"):
        net.train_step({}, None, type("O", (), {"model": net})(), size_head={"sed": 1})
    for bad in ({}, {"seed": 1, "keep": torch.ones(2, 128, dtype=torch.uint8)}):
        with pytest.raises(ValueError, match="exactly one of keep and seed"):
            net._size_head_mask(bad, "test")
    with pytest.raises(ValueError, match="size_head must be"):
        net._size_head_mask({"sed": 1}, "test")
    with pytest.raises(ValueError, match="exactly one of keep and seed"):
        net.size_head_backward(torch.zeros(2, 1024, 8, 8), torch.zeros(2, 3))
    with pytest.raises(ValueError, match="exactly one of keep and seed"):
        net.size_head_backward(torch.zeros(2, 1024, 8, 8), torch.zeros(2, 3), keep=torch.ones(2, 128, dtype=torch.uint8), seed=3)
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        size_grad.size_forward_save(torch.zeros(2, 64, 2, 2), {}, seed=1)
