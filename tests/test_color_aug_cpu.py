"""CPU: the numpy restatement of PIL's four enhance operations (tests/color_aug_ref.py) against Pillow's recorded bytes
(tests/golden/color_aug_pil.npz) and, where Pillow is installed, against Pillow itself; the draws of givepose_amd.color_aug; and the ABI
of the colour-augmentation family: include/givepose_coloraug.h == the library's gpca_* symbols == _lib.COLORAUG_PROTOTYPES.  Every
image comparison is np.array_equal."""
import os
import re
import subprocess

import numpy as np
import pytest

import color_aug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "color_aug_pil.npz")
PROBS = np.array([c[1] for c in R.CHILDREN])               # by code - 1: sharpness, contrast, brightness, color


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_equals_pillows_recorded_bytes():
    g = np.load(GOLDEN)
    frames, factors = g["frames"], g["factors"]
    assert frames.shape == (3, 13, 17, 3) and os.path.getsize(GOLDEN) < 100 * 1024
    assert factors.min() == 0 and 1.0 in factors and factors.max() > 1 and ((factors > 0) & (factors < 1)).any()
    for i, a in enumerate(frames):
        assert np.array_equal(R.smooth(a), g["smooth"][i]), i
        assert np.array_equal(R.smooth(a, (-1, 0, 1)), g["smooth"][i]), i          # the other row order: no input tells them apart
        for code in (1, 2, 3, 4):
            for k, f in enumerate(factors):
                assert np.array_equal(R.apply_op(a, code, f), g["single"][i, code - 1, k]), (i, code, float(f))
    for p in range(len(g["plan_ops"])):
        got = R.run_plan(frames, np.repeat(g["plan_ops"][p:p + 1], 3, 0), np.repeat(g["plan_factors"][p:p + 1], 3, 0))
        assert np.array_equal(got, g["plan_out"][:, p]), p
    assert (g["plan_ops"] == 0).any() and (g["plan_ops"][:, 1:] == g["plan_ops"][:, :-1]).any()      # a "none" and a repeat are recorded


def _pillow_frames():
    r = np.random.Generator(np.random.Philox(key=[5, 0x6361]))
    H, W = 22, 31
    grey = np.full((H, W, 3), 100, np.uint8)
    half = grey.copy()
    half.reshape(-1, 3)[:H * W // 2] = 101                 # H W even: the mean of L is exactly 100.5 -> 101
    below = half.copy()
    below[0, 0] = 100                                      # one pixel fewer: just below 100.5 -> 100
    ramp = (np.add.outer(np.arange(H) * 9, np.arange(W) * 5)[..., None] * np.array([1, 2, 3]) % 256).astype(np.uint8)
    return {"noise": r.integers(0, 256, (H, W, 3), dtype=np.uint8), "zeros": np.zeros((H, W, 3), np.uint8),
            "full": np.full((H, W, 3), 255, np.uint8), "ramp": ramp, "half": half, "below": below}


def test_restatement_equals_pillow():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageFilter
    enh = {1: ImageEnhance.Sharpness, 2: ImageEnhance.Contrast, 3: ImageEnhance.Brightness, 4: ImageEnhance.Color}
    frames = _pillow_frames()
    assert R.contrast_mean(frames["half"]) == 101 and R.contrast_mean(frames["below"]) == 100
    r = np.random.Generator(np.random.Philox(key=[6, 0x6361]))
    factors = np.concatenate([[0.0, 1.0, 0.25, 0.5, 0.77, 1.23, 1.5, 2.0, 2.9, 3.0], r.uniform(0, 3, 6)]).astype(np.float32)
    for name, a in frames.items():
        im = Image.fromarray(a)
        sm = np.asarray(im.filter(ImageFilter.SMOOTH))
        assert np.array_equal(R.smooth(a), sm) and np.array_equal(R.smooth(a, (-1, 0, 1)), sm), name
        for code in (1, 2, 3, 4):
            for f in factors:
                assert np.array_equal(R.apply_op(a, code, f), np.asarray(enh[code](im).enhance(float(f)))), (name, code, float(f))
    # a sequence: each result is rounded to uint8 before the next operation reads it
    a = frames["noise"]
    b = Image.fromarray(a)
    for code, f in ((4, 2.5), (1, 1.75), (2, 0.625), (3, 1.25)):
        b = enh[code](b).enhance(f)
    assert np.array_equal(R.run_plan(a[None], np.array([[4, 1, 2, 3]]), np.array([[2.5, 1.75, 0.625, 1.25]], np.float32))[0], np.asarray(b))


def test_golden_generator_reproduces_the_committed_file(tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_color_aug", os.path.join(ROOT, "scripts", "gen_golden_color_aug.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    monkeypatch.setattr(gen, "OUT", str(tmp_path / "g.npz"))
    gen.main()
    new, old = np.load(tmp_path / "g.npz"), np.load(GOLDEN)
    for k in old.files:
        if k != "pillow":
            assert np.array_equal(new[k], old[k]), k


# ------------------------------------------------------------------------------------------------ the ABI
def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_coloraug_header_equals_exported_symbols_and_prototypes():
    from givepose_amd import _lib, build
    assert "coloraug.hip" in build.SOURCES
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (gpca_[a-z0-9_]+)", out))
    declared = set(re.findall(r"^int (gpca_[a-z0-9_]+)\s*\(", _header("givepose_coloraug.h"), re.M))
    assert declared == {"gpca_luma_partials", "gpca_apply"} and declared == exported, (declared - exported, exported - declared)
    assert set(_lib.COLORAUG_PROTOTYPES) == declared
    lib = _lib.load()
    for name, (argtypes, _) in _lib.COLORAUG_PROTOTYPES.items():
        assert getattr(lib, name).argtypes == argtypes
        decl = re.search(rf"^int {name}\s*\((.*?)\);", _header("givepose_coloraug.h"), re.M | re.S).group(1)
        assert len(decl.split(",")) == len(argtypes), name                      # one ctypes entry per declared parameter
    m = re.search(r"#define GP_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "givepose_hip.h")).read())
    assert int(m.group(1)) == _lib.ABI_VERSION == lib.gp_version() == 328
    defines = dict(re.findall(r"#define GPCA_(\w+) \(?(-?\d+)\)?", _header("givepose_coloraug.h")))
    assert len(defines) == 13
    for k, v in defines.items():
        assert int(v) == getattr(_lib, "GPCA_" + k), k


def test_no_coloraug_symbol_under_another_prefix():
    assert "gpca_" not in _header("givepose_hip.h") and "gpca_" not in _header("givepose_traindata.h")
    assert not re.search(r"^int (gp_|gpt_)", _header("givepose_coloraug.h"), re.M)
    from givepose_amd import color_aug, _lib
    assert color_aug.OPS == {"none": 0, "sharpness": 1, "contrast": 2, "brightness": 3, "color": 4}
    assert [color_aug.OPS[k] for k in ("none", "sharpness", "contrast", "brightness", "color")] == \
        [_lib.GPCA_OP_NONE, _lib.GPCA_OP_SHARPNESS, _lib.GPCA_OP_CONTRAST, _lib.GPCA_OP_BRIGHTNESS, _lib.GPCA_OP_COLOR]
    assert color_aug.OPS == R.OPS and color_aug.DRAW_TAG == R.DRAW_TAG


def test_the_kernels_round_every_product_and_sum_separately(tmp_path):
    """blend's and SMOOTH's multiplies and adds must not be contracted: the gpca kernels' code holds no fused multiply-add."""
    import shutil
    from givepose_amd import _lib, build
    build.build(verbose=False)
    lib = shutil.copy(_lib.LIB_PATH, tmp_path / "lib.so")
    subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", str(lib)], capture_output=True, text=True, check=True)
    seen = set()
    for f in sorted(tmp_path.glob("lib.so.*gfx950")):
        dis = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", str(f)], text=True)
        for name, body in re.findall(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.M | re.S):
            if "coloraug_luma_kernel" in name or "coloraug_apply_kernel" in name:
                seen.add("luma" if "luma" in name else "apply")
                assert not re.search(r"\bv_(fma|fmac|mad|mac)(mk|ak)?_(f32|legacy_f32)", body), name
                if "apply" in name:
                    assert body.count("v_mul_f32") > 20 and body.count("v_add_f32") > 20
    assert seen == {"luma", "apply"}


# ------------------------------------------------------------------------------------------------ the surface
def test_public_surface_and_refusals_by_name():
    import givepose_amd
    from givepose_amd import ColorAugmenter, color_aug, color_aug_draws, train_batch
    assert givepose_amd.color_aug is color_aug and color_aug.ColorAugmenter is ColorAugmenter and color_aug.color_aug_draws is color_aug_draws
    for t in ("aae", "cosy+aae", "new1", "code", "code_albu"):
        for call in (lambda: ColorAugmenter(480, 640, "cuda", aug_type=t), lambda: color_aug_draws(0, 4, aug_type=t)):
            with pytest.raises(ValueError, match=re.escape(repr(t)) + r".*(imgaug|cv2) operations.*does not restate"):
                call()
    with pytest.raises(ValueError, match="'hsv'"):
        ColorAugmenter(480, 640, "cuda", aug_type="hsv")
    with pytest.raises(RuntimeError, match="HIP device only"):
        ColorAugmenter(480, 640, "cpu")
    for hw in ((2, 640), (480, 2)):
        with pytest.raises(ValueError, match="at least 3"):
            ColorAugmenter(*hw, "cuda")
    with pytest.raises(ValueError, match="prob"):
        ColorAugmenter(480, 640, "cuda", prob=1.5)
    with pytest.raises(ValueError, match="seed"):
        color_aug_draws(-1, 4)
    with pytest.raises(ValueError, match="enable"):
        color_aug_draws(1, 4, enable=np.ones(3, bool))
    assert "imgaug's stream" in color_aug_draws.__doc__ and "ColorAugmenter" in train_batch.__doc__


def test_stage_tables_route_every_frame_from_frames_to_out():
    from givepose_amd import _lib
    from givepose_amd.color_aug import stage_tables
    ops = np.array([[0, 0, 0, 0], [3, 0, 0, 0], [0, 2, 0, 4], [1, 2, 3, 4], [4, 4, 4, 0], [0, 0, 0, 1]], np.int32)
    fac = np.arange(24, dtype=np.float32).reshape(6, 4) / 8
    rows, kmax = stage_tables(ops, fac)
    assert rows.shape == (4, 6, 4) and rows.dtype == np.int32 and kmax == 4
    FR, T0, T1, OUT = _lib.GPCA_BUF_FRAMES, _lib.GPCA_BUF_TMP0, _lib.GPCA_BUF_TMP1, _lib.GPCA_BUF_OUT
    for f in range(6):
        where, seen = FR, []
        for st in range(4):
            op, bits, src, dst = rows[st, f]
            if op == _lib.GPCA_OP_SKIP:
                continue
            assert src == where and dst != src and dst in (T0, T1, OUT), (f, st)
            where = dst
            if op != _lib.GPCA_OP_NONE:
                seen.append((op, np.int32(bits).view(np.float32)))
        assert where == OUT, f                                           # every frame ends in `out`, the untouched one by a copy
        assert seen == [(o, x) for o, x in zip(ops[f], fac[f]) if o != 0], f
    assert rows[0, 0, 0] == _lib.GPCA_OP_NONE and (rows[1:, 0, 0] == _lib.GPCA_OP_SKIP).all()
    # a position no frame uses is no stage; a plan without any operation is one copy stage
    rows, kmax = stage_tables(np.array([[0, 3, 0], [0, 0, 0]], np.int32), np.ones((2, 3), np.float32))
    assert rows.shape == (1, 2, 4) and kmax == 1 and rows[0, :, 0].tolist() == [3, 0] and rows[0, :, 3].tolist() == [OUT, OUT]
    rows, kmax = stage_tables(np.zeros((2, 4), np.int32), np.ones((2, 4), np.float32))
    assert rows.shape == (1, 2, 4) and kmax == 0 and (rows[0, :, 0] == _lib.GPCA_OP_NONE).all()


# ------------------------------------------------------------------------------------------------ the draws
def test_draws_are_a_function_of_the_seed_and_equal_the_frame_by_frame_form():
    from givepose_amd import color_aug_draws
    a, b, c = color_aug_draws(17, 300), color_aug_draws(17, 300), color_aug_draws(18, 300)
    assert a["ops"].shape == (300, 4) and a["ops"].dtype == np.int32 and a["factors"].dtype == np.float32
    assert np.array_equal(a["ops"], b["ops"]) and np.array_equal(a["factors"], b["factors"]) and not np.array_equal(a["ops"], c["ops"])
    ref = R.draws_ref(17, 300)
    assert np.array_equal(a["ops"], ref["ops"]) and np.array_equal(a["factors"], ref["factors"])
    en = np.arange(300) % 3 != 0
    d, ref = color_aug_draws(17, 300, enable=en), R.draws_ref(17, 300, enable=en)
    assert np.array_equal(d["ops"], ref["ops"]) and np.array_equal(d["factors"], ref["factors"])
    assert not d["ops"][~en].any() and np.array_equal(d["ops"][en], a["ops"][en])
    assert not color_aug_draws(17, 300, prob=0.0)["ops"].any()


def test_draws_follow_the_references_distribution():
    """F = 20 000 frames at a fixed seed; every rate within 4 standard errors sqrt(p (1 - p) / n) of its value.  What a plan shows of
    "augmented" is a frame with at least one operation, prob (1 - prod (1 - p_c)); an operation shows at rate prob p_c (p_c itself at
    prob = 1).  The drawn order shows where it can be read: the position of every operation in the frames that hold all four is
    uniform over the four places, and of two operations in one frame either comes first with probability 1/2."""
    from givepose_amd import color_aug_draws
    F = 20000

    def near(count, n, p, what):
        assert n > 0 and abs(count / n - p) <= 4 * np.sqrt(p * (1 - p) / n), (what, count / n, p, n)
    for prob in (0.8, 1.0):
        plan = color_aug_draws(20240, F, prob=prob)
        ops, fac = plan["ops"], plan["factors"]
        has = np.stack([(ops == c).any(1) for c in (1, 2, 3, 4)], 1)
        assert (np.stack([(ops == c).sum(1) for c in (1, 2, 3, 4)], 1) <= 1).all()          # no operation twice
        near(int(has.any(1).sum()), F, prob * (1 - np.prod(1 - PROBS)), ("augmented", prob))
        for c in range(4):
            near(int(has[:, c].sum()), F, prob * PROBS[c], ("operation", c + 1, prob))
        live = ops != 0
        assert (live[:, :-1] >= live[:, 1:]).all()                                          # compacted to the left
        assert (fac[~live] == 1).all()
        for c, (_, _, lo, hi) in enumerate(R.CHILDREN):
            f = fac[ops == c + 1]
            assert f.min() >= lo and f.max() <= hi and f.max() - f.min() > 0.98 * (hi - lo), c
            near(int((f < (lo + hi) / 2).sum()), len(f), 0.5, ("factor below the middle", c + 1))
        full = ops[has.all(1)]
        for c in (1, 2, 3, 4):
            for pos in range(4):
                near(int((full[:, pos] == c).sum()), len(full), 0.25, ("position", c, pos, prob))
        where = np.where(has, np.stack([np.argmax(ops == c, 1) for c in (1, 2, 3, 4)], 1), -1)
        for a in range(4):
            for b in range(a + 1, 4):
                both = has[:, a] & has[:, b]
                near(int((where[both, a] < where[both, b]).sum()), int(both.sum()), 0.5, ("order", a + 1, b + 1, prob))
