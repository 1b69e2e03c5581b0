"""CPU: the NumPy restatement of the alignment (tests/umeyama_ref.py) against the fixtures recorded from the reference
(tests/golden/umeyama_*.npz), and the ABI of the alignment family: include/givepose_align.h == the library's gpa_* symbols ==
_lib.ALIGN_PROTOTYPES, none of them in givepose_hip.h, each held by an operator-level GPU test (the checks tests/test_abi.py and
tests/test_ops_reference_cpu.py make for the gp_ family, repeated for the new one)."""
import ast
import os
import re
import subprocess

import numpy as np
import pytest

import umeyama_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry point -> the operator-level GPU test that holds it (not the pipeline test: that one runs the whole network)
CLOSURE = {
    "gpa_backproject": "tests/test_umeyama_gpu.py::test_fixtures_decisions_and_values",
    "gpa_umeyama": "tests/test_umeyama_gpu.py::test_fixtures_decisions_and_values",
    "gpa_crop_depth": "tests/test_umeyama_gpu.py::test_crop_depth_bit_exact",
}


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_reproduces_the_fixture(name):
    inputs, draws, PC, flag, crops = R.load_fixture(name)
    got, pc = R.pose_from_umeyama_ref(draws=draws, valid_depth_only=flag, **inputs)
    assert pc.dtype == np.float32 and np.array_equal(pc.view(np.uint32), PC.view(np.uint32))      # bit for bit
    for b, c in enumerate(crops):
        R.check_crop_against_fixture(c, R.restatement_as_got(got[b]), f"restatement vs fixture {name}[{b}]")
        if c["expect"] == "tiny":      # the documented departure: every sample is rank-deficient, nothing is counted
            assert got[b]["status"] == R.LOW_INLIERS and got[b]["iterations_run"] == R.MAX_ITER and not any(got[b]["counts"])
        elif c["n_points"]:
            assert R.decisive(got[b]), (name, b)


def test_fixtures_hold_the_cases_they_are_there_for():
    seen = {}
    for name in R.FIXTURES:
        inputs, draws, PC, flag, crops = R.load_fixture(name)
        assert draws.dtype == np.uint32 and draws.shape == (len(crops), R.MAX_ITER, R.SAMPLE)
        for b, c in enumerate(crops):
            assert c["n_points"] == len(c["index"])
            seen.setdefault("n", set()).add(c["n_points"])
            seen.setdefault("expect", set()).add(c["expect"])
            if c["expect"] == "two":
                assert c["iterations_run"] == 2 and not c["returned_none"]
            if c["expect"] == "none128":
                assert c["iterations_run"] == 128 and c["returned_none"]
            if c["expect"] == "reflection":
                assert c["sigma"][2] < 0
            # scattered masks: the kept pixels are no single run of consecutive pixels
            if 2 < c["n_points"] < R.RES * R.RES:
                assert np.any(np.diff(c["index"]) > 1)
        seen.setdefault("B", set()).add(len(crops))
    assert {0, 1, 2, 5, 37, 63, 64, 65, 700, 2500, 4096} <= seen["n"] and {1, 5} <= seen["B"]
    assert {"two", "none128", "reflection", "tiny", "ok"} <= seen["expect"]
    a, b = R.load_fixture("special"), R.load_fixture("special_valid_depth")
    assert (a[3], b[3]) == (False, True) and a[4][3]["n_points"] - b[4][3]["n_points"] == 60      # the zero-depth pixels, both ways


def test_draws_are_reduced_mod_n_points():
    """Adding a multiple of n_points to a draw changes nothing; the table is used as it is otherwise."""
    inputs, draws, PC, flag, crops = R.load_fixture("b1")
    n = crops[0]["n_points"]
    shifted = draws.astype(np.uint64) + np.uint64(n) * np.random.RandomState(0).randint(0, 1000, draws.shape).astype(np.uint64)
    assert shifted.max() < 2 ** 32 and np.array_equal(shifted % n, draws % n) and not np.array_equal(shifted, draws)
    a, _ = R.pose_from_umeyama_ref(draws=draws, **inputs)
    b, _ = R.pose_from_umeyama_ref(draws=shifted.astype(np.uint32), **inputs)
    assert a[0]["counts"] == b[0]["counts"] and np.array_equal(a[0]["fit"]["sRT"], b[0]["fit"]["sRT"])
    from givepose_amd import umeyama as Um
    d = Um.make_draws(3, seed=7)
    assert d.dtype == np.uint32 and d.shape == (3, 128, 5) and np.array_equal(d, Um.make_draws(3, seed=7)) and d.max() > 2 ** 31


def test_bounds_are_near_1e_11_on_the_fixtures():
    """The derived bounds are tight enough to mean something: the rotation bound of every fitted fixture crop is below 1e-10."""
    worst = 0.0
    for name in R.FIXTURES:
        for c in R.load_fixture(name)[4]:
            if "sigma" in c:
                worst = max(worst, R.bounds(c["n_inliers"], c["sigma"], c["var_s"], c["var_t"], c["mean_s"], c["mean_t"], c["scale"])[1])
    print("largest rotation bound on the fixtures", worst)
    assert 0 < worst < 1e-10


# ------------------------------------------------------------------------------------------------ ABI of the family
def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _declared():
    return set(re.findall(r"^int (gpa_[a-z0-9_]+)\s*\(", _header("givepose_align.h"), re.M))


def test_align_header_equals_exported_symbols_and_prototypes():
    from givepose_amd import _lib, build
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (gpa_[a-z0-9_]+)", out))
    declared = _declared()
    assert declared and declared == exported, (declared - exported, exported - declared)
    assert set(_lib.ALIGN_PROTOTYPES) == declared
    lib = _lib.load()
    for name, (argtypes, _) in _lib.ALIGN_PROTOTYPES.items():
        assert getattr(lib, name).argtypes == argtypes
        decl = re.search(rf"^int {name}\s*\((.*?)\);", _header("givepose_align.h"), re.M | re.S).group(1)
        assert len(decl.split(",")) == len(argtypes), name                      # one ctypes entry per declared parameter
    m = re.search(r"#define GP_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "givepose_hip.h")).read())
    assert int(m.group(1)) == _lib.ABI_VERSION == lib.gp_version() >= 328
    for k in ("RES", "MAX_POINTS", "MAX_ITER", "SAMPLE", "HYP_STRIDE", "FIT_STRIDE", "FIT32_STRIDE", "RECORD"):
        v = re.search(rf"#define GPA_{k} (\d+)", _header("givepose_align.h")).group(1)
        assert int(v) == getattr(_lib, "GPA_" + k), k
    enum = re.search(r"enum gpa_status \{(.*?)\}", _header("givepose_align.h"), re.S).group(1)
    assert {k: int(v) for k, v in re.findall(r"(GPA_[A-Z_]+) = (\d+)", enum)} == {
        "GPA_OK": _lib.GPA_OK, "GPA_NO_POINTS": _lib.GPA_NO_POINTS, "GPA_LOW_INLIERS": _lib.GPA_LOW_INLIERS, "GPA_DEGENERATE": _lib.GPA_DEGENERATE}
    assert (R.OK, R.NO_POINTS, R.LOW_INLIERS, R.DEGENERATE) == (_lib.GPA_OK, _lib.GPA_NO_POINTS, _lib.GPA_LOW_INLIERS, _lib.GPA_DEGENERATE)


def test_no_align_symbol_in_the_main_header():
    assert "gpa_" not in _header("givepose_hip.h")
    assert not re.search(r"^int gp_", _header("givepose_align.h"), re.M)


def test_closure_table_names_existing_operator_tests():
    assert set(CLOSURE) == _declared()
    from test_ops_reference_cpu import WHOLE_NETWORK
    for ep, target in CLOSURE.items():
        path, func = target.split("::")
        assert os.path.basename(path) not in WHOLE_NETWORK
        with open(os.path.join(ROOT, path)) as f:
            src = f.read()
        tree = ast.parse(src)
        node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == func]
        assert node and func.startswith("test_"), target
        assert "pytestmark = pytest.mark.gpu" in src
        assert not re.search(r"FramePipeline", ast.get_source_segment(src, node[0])), (ep, "the pipeline test runs the whole network")
    # every entry point has a Python wrapper in the package
    pkg = "".join(open(os.path.join(ROOT, "givepose_amd", f)).read() for f in ("umeyama.py", "preprocess.py"))
    for ep in CLOSURE:
        assert re.search(rf"L\.{ep}\(", pkg), ep


def test_public_surface_and_no_cpu_path():
    import torch
    import givepose_amd
    from givepose_amd import _lib
    assert callable(givepose_amd.pose_from_umeyama) and callable(givepose_amd.pose_from_umeyama_device)
    z = torch.zeros
    with pytest.raises(_lib.GivePoseHipError):      # HIP devices only
        givepose_amd.pose_from_umeyama_device(z(1, 3, 64, 64), z(1, 2, 64, 64), z(1, 3, 3), z(1, 1, 64, 64), z(1, 1, 64, 64))
