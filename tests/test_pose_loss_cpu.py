"""CPU: the float64 NumPy restatement of PoseLoss and of the train-time pose decode (tests/pose_loss_ref.py) against the fixtures
recorded from the reference (tests/golden/pose_loss_*.npz, scripts/gen_golden_pose_loss.py), and the ABI of the loss family:
include/givepose_loss.h == the library's gpl_* symbols == _lib.LOSS_PROTOTYPES, none of them in the other two headers."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import pose_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# float32 rounding times log2 of the longest sum (12 288 summands) plus the elementwise roundings of the reference's float32 terms
REF_BOUND = 16 * 2.0 ** -24


def rel(a, b):
    return float(np.max(np.abs(np.float64(a) - np.float64(b)) / np.where(b != 0, np.abs(np.float64(b)), 1.0)))


# ------------------------------------------------------------------------------------------------ restatement vs reference
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_reproduces_the_fixture(name):
    pred, data, cfg, z = R.load_fixture(name)
    ref = R.pose_loss_ref(pred, data, **cfg)
    err = rel(ref["terms"], z["terms"])
    print(f"{name}: restatement vs reference, max rel over the six terms {err:.2e}")
    assert z["terms"].dtype == np.float32 and z["terms"].shape == (6,)
    assert err < REF_BOUND, (name, ref["terms"], z["terms"])
    assert R.manifest()["loss"][name]["max_rel_reference_minus_restatement"] < REF_BOUND                    # the gap the generator saw
    assert np.array_equal(ref["index"], z["index"]), name                  # the chosen candidate of every crop
    assert bool(z["branch"]) == ref["branch"]
    sym1 = data["sym_info"][:, 0] == 1
    searched = sym1 & ref["branch"]
    assert np.array_equal(np.isfinite(ref["gap"]), searched) and np.all(ref["gap"][searched] >= 1e-9) and np.all(z["gap"][searched] >= 1e-9)
    # the winning rotation, rounded once to float32, is the reference's closest ground truth to the last float32 bit but one
    assert np.abs(ref["closest"] - z["closest"]).max() < 2.0 ** -23


def test_fixtures_hold_the_cases_they_are_there_for():
    seen = {"B": set(), "P": set(), "rows": set(), "masks": set(), "flags": set()}
    for name in R.CASES:
        pred, data, cfg, z = R.load_fixture(name)
        B, P = data["model_point"].shape[:2]
        seen["B"].add(B)
        seen["P"].add(P)
        seen["rows"].update(tuple(r) for r in data["sym_info"].tolist())
        sym1 = data["sym_info"][:, 0] == 1
        for m in (data["roi_mask_output"], data["roi_ivfc_mask_output"]):
            for b in range(B):
                s, n = float(m[b].sum()), int(np.count_nonzero(m[b]))
                kind = "zero" if n == 0 else "one" if n == 1 else "full" if s == 4096 else "soft" if np.any((m[b] > 0) & (m[b] < 1)) else "binary"
                seen["masks"].add(kind)
        seen["flags"].add((cfg["pose_loss_type"], cfg["r_loss"], "sym" in cfg["r_type"]))
        eq = R.CASES[name]["equal"]
        if eq is not None:
            assert np.array_equal(pred["rot"][eq], data["rotation"][eq]) and z["index"][eq] == -1
            if sym1[eq] and bool(z["branch"]):        # a tie: candidate 0 is the unrotated ground truth, the strict `<` keeps index -1
                assert R.candidates_re(pred["rot"][eq], data["rotation"][eq])[0] == R.re_deg(np.float64(pred["rot"][eq]), np.float64(data["rotation"][eq]))
        if name == "nosym":
            assert not sym1.any() and not bool(z["branch"])
        if name == "allsym":
            assert sym1.all() and bool(z["branch"])
        if name == "symtype":
            assert sym1.any() and not bool(z["branch"]) and np.all(z["index"] == -1)
        if name == "angle":      # one crop at trace = 3: (trace - 1) / 2 is clipped to 0.99999
            tr = np.einsum("ij,ij->", np.float64(pred["rot"][eq]), np.float64(data["rotation"][eq]))
            assert (tr - 1) / 2 > 0.99999
        if name == "smoothl1":   # both sides of beta = 0.5
            d = np.abs(np.float64(pred["rot"]) - R.pose_loss_ref(pred, data, **cfg)["closest"])
            assert d.min() < 0.5 < d.max()
        if bool(z["branch"]):
            assert np.any(z["index"][sym1] >= 0)
        # both Huber branches
        d = np.abs(pred["nocs_coor"] - data["nocs_coord"])
        assert (d > 0.03).any() and (d < 0.03).any()
    assert seen["B"] == {1, 3, 5} and seen["P"] == {1, 1000, 1024}
    assert {tuple(r) for r in R.SYM_ROWS} <= seen["rows"]
    assert seen["masks"] == {"zero", "one", "full", "soft", "binary"}
    assert {("l1", "l1", False), ("l1", "angle", False), ("smoothl1", "l1", False), ("l1", "l1", True)} <= seen["flags"]


def test_zero_mask_gives_zero_not_nan():
    pred, data = R.make_inputs(B=2, P=3, seed=31, masks=("zero",))
    t = R.pose_loss_ref(pred, data)["terms"]
    assert t[4] == 0.0 and t[5] == 0.0 and np.all(np.isfinite(t))


def test_decode_restatement_reproduces_the_fixture():
    """Bounds of tests/test_pnp_flags_gpu.py::test_pose_tail_rt_golden: 2e-6 on the rotation, 1e-5 (relative to the largest entry, at
    least 1) on the translation."""
    inp, z = R.load_decode_fixture()
    for name, (r_type, t_type) in R.DECODE_CASES.items():
        rot, trans = R.decode_train_ref(t_site=t_type == "site", is_allo="allo" in r_type, **inp)
        er, et = float(np.abs(rot - z[name + "__rot"]).max()), float(np.abs(trans - z[name + "__trans"]).max())
        print(f"decode {name}: rot {er:.2e} trans {et:.2e}")
        assert er < 2e-6 and et < 1e-5 * max(1.0, float(np.abs(z[name + "__trans"]).max()))
        assert trans[0, 0] == 0.0 and trans[0, 1] == 0.0                   # crop 0: exactly on the optical axis
        assert np.all(R.off_axis_angle(trans[1:]) >= 0.05)                 # the others: at least 0.05 rad off it
        if "allo" in r_type:
            assert np.abs(rot[0] - np.float64(inp["rot_allo"][0])).max() < 1e-12       # on the axis the correction is the identity
            assert np.abs(rot[1:] - np.float64(inp["rot_allo"][1:])).max() > 1e-2
        else:
            assert np.array_equal(rot, np.float64(inp["rot_allo"]))


# ------------------------------------------------------------------------------------------------ ABI of the family
def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_loss_header_equals_exported_symbols_and_prototypes():
    from givepose_amd import _lib, build
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (gpl_[a-z0-9_]+)", out))
    declared = set(re.findall(r"^int (gpl_[a-z0-9_]+)\s*\(", _header("givepose_loss.h"), re.M))
    assert declared == {"gpl_pose_decode_train", "gpl_pose_loss_partials", "gpl_pose_loss_reduce"}
    assert declared == exported, (declared - exported, exported - declared)
    assert set(_lib.LOSS_PROTOTYPES) == declared
    lib = _lib.load()
    for name, (argtypes, _) in _lib.LOSS_PROTOTYPES.items():
        assert getattr(lib, name).argtypes == argtypes
        decl = re.search(rf"^int {name}\s*\((.*?)\);", _header("givepose_loss.h"), re.M | re.S).group(1)
        assert len(decl.split(",")) == len(argtypes), name                 # one ctypes entry per declared parameter
    for k in ("RES", "SYM", "SPLIT", "PART", "RECORD", "OUT", "ACC"):
        v = re.search(rf"#define GPL_{k} (\d+)", _header("givepose_loss.h")).group(1)
        assert int(v) == getattr(_lib, "GPL_" + k), k


def test_no_loss_symbol_in_the_other_headers():
    assert "gpl_" not in _header("givepose_hip.h") and "gpl_" not in _header("givepose_align.h")
    assert not re.search(r"^int gpa?_", _header("givepose_loss.h"), re.M)
    pkg = open(os.path.join(ROOT, "givepose_amd", "loss.py")).read()
    for ep in ("gpl_pose_decode_train", "gpl_pose_loss_partials", "gpl_pose_loss_reduce"):
        assert re.search(rf"L\.{ep}\(", pkg), ep                             # every entry point has its Python wrapper


# ------------------------------------------------------------------------------------------------ the public surface
def test_loss_config_defaults_and_refusals():
    import givepose_amd
    from givepose_amd import LossAccumulator, LossConfig, PoseLoss
    assert givepose_amd.PoseLoss is PoseLoss and callable(LossAccumulator)
    c = LossConfig()
    assert {k: getattr(c, k) for k in R.DEFAULTS} == R.DEFAULTS
    with pytest.raises(Exception):
        c.r_loss = "angle"                                                  # frozen
    for bad in (dict(pose_loss_type="l2"), dict(r_loss="cos"), dict(r_type="nope"), dict(coor_gt_sym="x"), dict(coor_w=float("nan")),
                dict(tran_w="1")):
        with pytest.raises(ValueError):
            LossConfig(**bad)
    for k in ("coor", "radius"):
        with pytest.raises(NotImplementedError):
            LossConfig(coor_gt_sym=k)
    assert LossConfig(r_loss="angle", pose_loss_type="smoothl1", r_type="allo_rot6d_sym").r_type == "allo_rot6d_sym"
    from givepose_amd import loss
    assert loss.KEYS == R.KEYS
    with pytest.raises(ValueError):
        PoseLoss(cfg={"r_loss": "l1"})


def test_cpu_prediction_is_refused():
    import torch
    from givepose_amd import LossAccumulator, PoseLoss, _lib
    pred, data = R.make_inputs(B=1, P=1, seed=1)
    T = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        PoseLoss()(T(pred), T(data))
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        LossAccumulator().add(T(pred), T(data))


def test_forward_signature_unchanged_and_package_does_not_import_the_restatement():
    from givepose_amd import PoseNet
    assert list(inspect.signature(PoseNet.forward).parameters) == ["self", "data", "device", "do_loss", "pred_scale", "groups"]
    p = inspect.signature(PoseNet.forward).parameters
    assert p["do_loss"].default is False and p["device"].default == "cuda" and p["pred_scale"].default is None
    pkg = os.path.join(ROOT, "givepose_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "pose_loss_ref" not in src and not re.search(r"^\s*(from|import) (tests|oracle)\b", src, re.M), fn
