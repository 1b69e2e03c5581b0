"""CPU: the float64 NumPy restatement of the loss gradient and of the decode backward (tests/pose_loss_grad_ref.py) against the
fixtures recorded from the reference under torch autograd (tests/golden/pose_loss_grad_*.npz,
scripts/gen_golden_pose_loss_grad.py), against central differences of the forward restatement, the exact zeros, the mutations the
fixtures reject, and the ABI of the gradient family: include/givepose_grad.h == the library's gpg_* symbols ==
_lib.GRAD_PROTOTYPES, none of them in the other headers.

Bounds (u = 2^-53; the constants live in tests/pose_loss_grad_ref.py for the GPU tests to share; every figure is
|difference| / max|reference| over one tensor, printed before it is asserted, and the figure the generator saw is in
tests/golden/pose_loss_grad_manifest.json).
  F64_BOUND     the restatement and the reference's float64 autograd evaluate the same expression; an element goes through at most
                24 roundings, and it holds one long sum taken in another order: the mask sum (4096 summands) or the P-point sum
                (1024): (4096 + 24) u = 4.6e-13.  Measured 3.7e-15.
  DECODE_BOUND  the decode backward is a chain of at most 200 roundings (an ulp or two of sin, cos, acos and sqrt counted as four):
                200 u = 2.2e-14, times the conditioning of the axis normalisation, 1 / |axis_raw|: the crops off the optical axis sit
                at least 0.05 rad off it (tests/test_pose_loss_cpu.py asserts it), 1 / sin(0.05) = 20: DECODE_OFF = 4.4e-13; for the
                crop on the axis the two `+ eps` normalisations divide by eps = 1e-4: DECODE_ON = 2.2e-10 on its pred_t.  Measured
                3.6e-15 and 7e-18 (of a gradient of 260, against 0.4 on the other crops).
  F32_BOUND     the reference in float32 against the restatement.  In the quadratic Huber branch the gradient is |x| / 0.03 and
                x = pred * mask - (rot_sym gt) * mask is at most 8 float32 roundings of values below 1 away from the float64 one
                (three products and two sums of the rotation, rot_sym's own sum, the two mask products, the difference):
                8 * 2^-24 / 0.03 relative to the linear branch's slope 1, plus 8 * 2^-24 for the factors in front: 1.64e-5.
                Measured 1.84e-6.
  FD_TOL        central differences with h = 2^-11 of a piecewise linear / quadratic function are exact away from the kinks up to
                the rounding of the forward (1e-15 of a total of a few units, over 2 h: 1e-12 absolute); the smallest gradients are
                the map ones, coor_w / (B sum(mask)) = 1e-5: 1e-6 relative.  The angle form is smooth, not piecewise quadratic: its
                truncation error is h^2 f''' / 6, 4e-8 f''', and f''' reaches 1e3 near the clip: 1e-4.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import pose_loss_grad_ref as G
import pose_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_BOUND, F32_BOUND = G.F64_BOUND, G.F32_BOUND
DECODE_OFF, DECODE_ON = G.DECODE_BOUND * G.DECODE_COND_OFF, G.DECODE_BOUND * G.DECODE_COND_ON
FD_H, FD_TOL, FD_TOL_ANGLE, DECODE_FD_TOL = 2.0 ** -11, 1e-6, 1e-4, 1e-5
MAPS = ("nocs_coor", "ivfc_coor")
VARIANTS = {"ones": None, "gout": G.make_gout()}


def rel(got, ref):
    ref = np.asarray(ref, np.float64)
    m = float(np.abs(ref).max())
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (m if m > 0 else 1.0))


def fixture_errors(name, mutate=None, prefix=""):
    """Worst |restatement - fixture| / max|fixture| per tensor of one case, both variants -> {key: figure}."""
    pred, data, cfg, z = G.load_grad_fixture(name)
    pix = G.sample_pixels(name, pred["rot"].shape[0])
    out = {}
    for v, w in VARIANTS.items():
        if prefix and v != "ones":
            continue
        g = G.pose_loss_grad_ref(pred, data, gout=w, mutate=mutate, **cfg)
        for k in ("rot", "trans", "size"):
            out[f"{v}__{k}"] = rel(g[k], z[f"{prefix}{v}__{k}"])
        for k in MAPS:
            s, tot, ab = G.sampled(g[k], pix)
            out[f"{v}__{k}"] = rel(s, z[f"{prefix}{v}__{k}_s"])
            if not prefix:       # the sums of the whole map: every pixel takes part, not only the sample
                den = np.maximum(z[f"{v}__{k}_abs"], 1e-300)
                with np.errstate(invalid="ignore"):
                    out[f"{v}__{k}_sums"] = float(max(np.max(np.abs(tot - z[f"{v}__{k}_sum"]) / den), np.max(np.abs(ab - z[f"{v}__{k}_abs"]) / den)))
    return out


# ------------------------------------------------------------------------------------------------ restatement vs reference
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_reproduces_the_float64_fixture(name):
    err = fixture_errors(name)
    worst = max(err.values())
    print(f"{name}: restatement vs the reference's float64 autograd, worst |diff| / max|g| {worst:.2e}  {err}")
    assert worst < F64_BOUND, err
    seen = G.manifest()["loss"][name]
    assert max(v["f64_minus_restatement"] for v in seen.values()) < F64_BOUND                       # the figure the generator saw
    pred, data, cfg, z = G.load_grad_fixture(name)
    B = pred["rot"].shape[0]
    assert z["ones__rot"].dtype == np.float64 and z["ones__rot"].shape == (B, 3, 3) and z["gout__nocs_coor_s"].shape == (B, 3, G.SAMPLE)
    assert G.SAMPLE >= 256 and np.all(np.diff(G.sample_pixels(name, B), axis=1) > 0)


@pytest.mark.parametrize("name", list(R.CASES))
def test_float32_reference_against_the_restatement(name):
    err = fixture_errors(name, prefix="f32_")
    worst = max(err.values())
    print(f"{name}: the reference's float32 autograd vs the restatement, worst |diff| / max|g| {worst:.2e}  {err}")
    assert worst < F32_BOUND, err
    seen = G.manifest()["loss"][name]
    assert max(v["f32_minus_restatement"] for v in seen.values()) < F32_BOUND
    pred, data, cfg, z = G.load_grad_fixture(name)
    for v in VARIANTS:                                     # no sign disagreement between the two precisions
        for k in ("rot", "trans", "size"):
            nz = z[f"{v}__{k}"] != 0
            assert np.array_equal(np.sign(z[f"f32_{v}__{k}"][nz]), np.sign(z[f"{v}__{k}"][nz])), (v, k)
    for k in MAPS:
        nz = z[f"ones__{k}_s"] != 0
        assert np.array_equal(np.sign(z[f"f32_ones__{k}_s"][nz]), np.sign(z[f"ones__{k}_s"][nz])), k


def test_decode_restatement_reproduces_the_float64_fixture():
    inp, extra, z = G.load_decode_grad_fixture()
    assert inp["pred_t"].shape[0] == 4                     # B = 3 would change the reference's torch.cross without `dim`
    Ra = G.rot6d_to_mat_ref(extra["rot6d"])
    for name, (r_type, t_type) in R.DECODE_CASES.items():
        kw = dict(t_site=t_type == "site", is_allo="allo" in r_type)
        g = G.decode_train_backward_ref(extra["g_rot_ego"], extra["g_trans"], rot6d=extra["rot6d"], **kw, **{**inp, "rot_allo": Ra})
        e6, e_on, e_off = rel(g["rot6d"], z[name + "__rot6d"]), rel(g["pred_t"][:1], z[name + "__pred_t"][:1]), rel(g["pred_t"][1:], z[name + "__pred_t"][1:])
        print(f"decode {name}: rot6d {e6:.2e} pred_t on the axis {e_on:.2e} (max|g| {np.abs(z[name + '__pred_t'][0]).max():.3g}) off it {e_off:.2e} "
              f"(max|g| {np.abs(z[name + '__pred_t'][1:]).max():.3g})")
        assert e6 < DECODE_OFF and e_off < DECODE_OFF and e_on < DECODE_ON
        m = G.manifest()["decode"][name]
        assert m["rot6d"] < DECODE_OFF and m["pred_t_off_axis"] < DECODE_OFF and m["pred_t_on_axis"] < DECODE_ON
        if not kw["t_site"]:                               # t_type 'center': the centroid's gradient is multiplied by 0
            assert np.all(g["pred_t"][:, :2] == 0) and np.all(z[name + "__pred_t"][:, :2] == 0)
        if not kw["is_allo"]:                              # ego: g_rot_ego passes through
            assert np.array_equal(g["rot_allo"], np.float64(extra["g_rot_ego"]))
    # the reference's behaviour on the optical axis is reproduced, not smoothed: 1 / eps shows in d pred_t of crop 0
    on, off = np.abs(z["allo_site__pred_t"][0]).max(), np.abs(z["allo_site__pred_t"][1:]).max()
    assert on > 50 * off and on > 100


# ------------------------------------------------------------------------------------------------ central differences
def _total(pred, data, w, cfg):
    f = R.pose_loss_ref(pred, data, **cfg)
    return float(np.dot(w, f["terms"])), f["index"]


def _central(pred, data, w, cfg, key, idx):
    """Central difference of sum_k w_k term_k in pred[key][idx]; the steps are the float32 values actually reached.
    -> (derivative, True when the chosen candidates did not change)."""
    x0 = pred[key][idx]
    hi, lo = np.float32(x0 + FD_H), np.float32(x0 - FD_H)
    p = {k: v.copy() for k, v in pred.items()}
    p[key][idx] = hi
    fp, ip = _total(p, data, w, cfg)
    p[key][idx] = lo
    fm, im = _total(p, data, w, cfg)
    return (fp - fm) / (np.float64(hi) - np.float64(lo)), np.array_equal(ip, im)


def _check_fd(pred, data, w, cfg, key, indices, g, tol, what):
    scale, n, worst = float(np.abs(g[key]).max()), 0, 0.0
    for idx in indices:
        fd, same = _central(pred, data, w, cfg, key, idx)
        if not same:
            continue
        n += 1
        worst = max(worst, abs(fd - g[key][idx]) / scale)
    print(f"{what} {key}: {n} elements, worst |central difference - restatement| / max|g| {worst:.2e}")
    assert worst < tol, (what, key, worst)
    return n


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_against_central_differences(name):
    pred, data = R.case_inputs(name)
    cfg = R.case_cfg(name)
    B = pred["rot"].shape[0]
    d = lambda a: np.asarray(a, np.float32).astype(np.float64)
    smooth, angle = cfg["pose_loss_type"] == "smoothl1", cfg["r_loss"] == "angle"
    away = lambda x: (np.abs(x) > 4 * FD_H) & (~smooth | (np.abs(np.abs(x) - 0.5) > 4 * FD_H))
    sc = d(data["nocs_scale"])[:, None]
    # trans and size, all terms weighted
    w = G.make_gout() + np.array([0, 0, 0.75, 0, 0, 0])
    g = G.pose_loss_grad_ref(pred, data, gout=w, **cfg)
    n = 0
    for key, gt in (("trans", "translation"), ("size", "real_size")):
        ok = away(d(pred[key]) - d(data[gt]) / sc)
        n += _check_fd(pred, data, w, cfg, key, [tuple(i) for i in np.argwhere(ok)], g, FD_TOL, name)
    assert n >= 4 * B
    # Rot1 alone (the P-point sum has a kink per point: it is checked below with few points)
    w1 = np.array([1.5, 0, 0, 0, 0, 0.0])
    g1 = G.pose_loss_grad_ref(pred, data, gout=w1, **cfg)
    Rc = g1["forward"]["closest"]
    if angle:
        u = (R._trace_abt(Rc, d(pred["rot"])) - 1.0) / 2.0
        ok = np.broadcast_to((np.abs(u) < 0.99999 - 0.01)[:, None, None], (B, 3, 3))
    else:
        ok = away(d(pred["rot"]) - Rc)
    n = _check_fd(pred, data, w1, cfg, "rot", [tuple(i) for i in np.argwhere(ok)], g1, FD_TOL_ANGLE if angle else FD_TOL, name + " Rot1")
    assert n >= (1 if name == "b1" else 9)
    # the maps: seeded pixels inside the mask, away from 0 and from the Huber threshold
    r = np.random.Generator(np.random.Philox(key=[0xFD, R.CASES[name]["seed"]]))
    w2 = np.array([0, 0, 0, 0, 1.25, -0.5])
    g2 = G.pose_loss_grad_ref(pred, data, gout=w2, **cfg)
    for key, gk, mk in (("nocs_coor", "nocs_coord", "roi_mask_output"), ("ivfc_coor", "ivfc_coord", "roi_ivfc_mask_output")):
        m = d(data[mk])
        # |x| from the gradient itself: in the quadratic branch |g| = scale m^2 |x| / H, in the linear one scale m^2
        cand = np.argwhere(np.broadcast_to(m > 0.05, pred[key].shape))
        pick = cand[r.choice(len(cand), min(48, len(cand)), replace=False)] if len(cand) else []
        idx = []
        for i in map(tuple, pick):
            gmax = np.abs(g2[key][i[0]] / np.maximum(m[i[0]] ** 2, 1e-30)).max()          # scale of this crop: the linear slope
            ratio = abs(g2[key][i]) / (m[i[0], 0, i[2], i[3]] ** 2) / gmax                  # |x| / H below the threshold, 1 above
            x_est = ratio * G.H
            if x_est > 6 * FD_H and (ratio == 1.0 or G.H - x_est > 6 * FD_H):
                idx.append(i)
        n = _check_fd(pred, data, w2, cfg, key, idx[:10], g2, FD_TOL, name)
        assert n >= (1 if "one" in R.CASES[name]["masks"] or "zero" in R.CASES[name]["masks"] else 5)


@pytest.mark.parametrize("flags", [{}, dict(pose_loss_type="smoothl1"), dict(r_type="allo_rot6d_sym")])
def test_point_matching_against_central_differences(flags):
    """Few points, so that an element of rot can sit away from every point's kink."""
    cfg = {**R.DEFAULTS, **flags}
    pred, data = R.make_inputs(B=3, P=3, seed=71)
    d = lambda a: np.asarray(a, np.float32).astype(np.float64)
    w = np.array([0, 0, 0, 2.0, 0, 0.0])
    g = G.pose_loss_grad_ref(pred, data, gout=w, **cfg)
    Rc, rot, pts = g["forward"]["closest"], d(pred["rot"]), d(data["model_point"]).copy()
    zero = ("sym" in cfg["r_type"]) & (data["sym_info"][:, 0] == 1)
    pts[zero, :, 0] = 0
    pts[zero, :, 2] = 0
    res = np.einsum("bcj,bqj->bcq", rot - Rc, pts)                       # pp - gp per (crop, channel, point)
    margin = 4 * FD_H * np.abs(pts).max()
    ok = (np.abs(res) > margin) & (~(cfg["pose_loss_type"] == "smoothl1") | (np.abs(np.abs(res) - 0.5) > margin))
    idx = [(b, c, j) for b in range(3) for c in range(3) for j in range(3) if ok[b, c].all()]
    n = _check_fd(pred, data, w, cfg, "rot", idx, g, FD_TOL, f"point matching {flags}")
    assert n >= 9
    assert np.all(g["trans"] == 0) and np.all(g["size"] == 0)            # point matching reaches rot only
    if zero.any():                                                       # 'sym' r_type: the x and z coordinates of symmetric crops are zeroed
        assert np.all(g["rot"][zero][:, :, 0] == 0) and np.all(g["rot"][zero][:, :, 2] == 0) and np.any(g["rot"][zero][:, :, 1] != 0)


def test_decode_restatement_against_central_differences():
    """Float64 central differences of decode_train_ref after rot6d_to_mat_ref, away from the optical axis (crop 0 sits on |v| = 0,
    where the curvature is 1 / eps).  h = 2^-11: truncation h^2 f''' / 6 = 4e-8 f'''; the normalisations
    of rot6d vectors of norm 0.5 to 2 and of translations of norm 1 have third derivatives up to 100 times the first:
    DECODE_FD_TOL = 1e-5 of max|g|."""
    inp, extra = R.make_decode_inputs(), G.make_decode_grad_inputs()
    gE, gT = np.float64(extra["g_rot_ego"]), np.float64(extra["g_trans"])
    for name, (r_type, t_type) in R.DECODE_CASES.items():
        kw = dict(t_site=t_type == "site", is_allo="allo" in r_type)

        def f(pt, d6):
            # decode_train_ref takes float32 inputs: it is given the identity, which returns the allo-to-ego matrix itself (the
            # identity for an ego type), and the float64 rotation of the raw vector is multiplied in here, unrounded
            M, trans = R.decode_train_ref(**{**inp, "pred_t": pt, "rot_allo": np.broadcast_to(np.eye(3, dtype=np.float32), (4, 3, 3))}, **kw)
            return float((np.einsum("bik,bkj->bij", M, G.rot6d_to_mat_ref(d6)) * gE).sum() + (trans * gT).sum())

        g = G.decode_train_backward_ref(extra["g_rot_ego"], extra["g_trans"], rot6d=extra["rot6d"], **kw, **inp)
        worst = 0.0
        for key, arr, first in (("pred_t", inp["pred_t"], 1), ("rot6d", extra["rot6d"], 0)):
            scale = np.abs(g[key][first:]).max()
            for b in range(first, 4):
                for i in range(arr.shape[1]):
                    hi, lo = arr.copy(), arr.copy()
                    hi[b, i], lo[b, i] = np.float32(arr[b, i] + FD_H), np.float32(arr[b, i] - FD_H)
                    args = (lambda a: (a, extra["rot6d"])) if key == "pred_t" else (lambda a: (inp["pred_t"], a))
                    fd = (f(*args(hi)) - f(*args(lo))) / (np.float64(hi[b, i]) - np.float64(lo[b, i]))
                    worst = max(worst, abs(fd - g[key][b, i]) / scale)
        print(f"decode {name}: worst |central difference - restatement| / max|g| {worst:.2e}")
        assert worst < DECODE_FD_TOL


# ------------------------------------------------------------------------------------------------ exact zeros
def test_exact_zeros():
    for name in R.CASES:
        pred, data = R.case_inputs(name)
        cfg = R.case_cfg(name)
        g = G.pose_loss_grad_ref(pred, data, **cfg)
        for k, mk in (("nocs_coor", "roi_mask_output"), ("ivfc_coor", "roi_ivfc_mask_output")):
            out = np.broadcast_to(data[mk] == 0, g[k].shape)
            assert np.all(g[k][out] == 0) and np.all(np.isfinite(g[k])), (name, k)      # masked-out pixels, the all-zero crops: 0, not NaN
            assert np.any(g[k] != 0)
        eq = R.CASES[name]["equal"]
        if eq is not None:
            if cfg["r_loss"] == "angle":            # the crop at trace = 3: the clip passes no gradient; point matching is 0 as pred == gt
                assert np.all(g["rot"][eq] == 0)
                u = (R._trace_abt(g["forward"]["closest"], np.float64(pred["rot"])) - 1.0) / 2.0
                assert u[eq] > 0.99999 and np.all(np.abs(np.delete(u, eq)) < 0.99999) and np.all(np.delete(g["rot"], eq, 0) != 0)
            else:                                   # sign(0) = 0 in Rot1 and in every point
                assert np.all(g["rot"][eq] == 0) and np.all(np.delete(g["rot"], eq, 0) != 0)
    kinds = [k for n in R.CASES for k in R.CASES[n]["masks"]]
    assert "zero" in kinds and "one" in kinds


def test_a_zero_in_gout_leaves_that_term_out():
    pred, data = R.case_inputs("b5")
    cfg = R.case_cfg("b5")
    w = G.make_gout()
    assert w[2] == 0 and np.all(np.delete(w, 2) != 0)
    g = G.pose_loss_grad_ref(pred, data, gout=w, **cfg)
    assert np.all(g["size"] == 0) and np.all(g["trans"] != 0)
    only_pm = G.pose_loss_grad_ref(pred, data, gout=[0, 0, 0, 1, 0, 0], **cfg)
    only_r1 = G.pose_loss_grad_ref(pred, data, gout=[1, 0, 0, 0, 0, 0], **cfg)
    both = G.pose_loss_grad_ref(pred, data, gout=[1, 0, 0, 1, 0, 0], **cfg)
    assert np.array_equal(both["rot"], only_r1["rot"] + only_pm["rot"]) and np.all(both["nocs_coor"] == 0)


# ------------------------------------------------------------------------------------------------ rejected mutations
@pytest.mark.parametrize("mutation,case,key", [
    ("mask_once", "b5", "nocs_coor"),        # crop 1 of b5 has a soft mask: mask^1 and mask^2 differ there
    ("sign0_one", "b5", "rot"),              # crop 2 of b5: pred == gt, sign(0) must be 0
    ("no_eps", "b3", "nocs_coor"),           # the one-pixel mask: 1 / 1 against 1 / (1 + 1e-5); the zero mask: NaN
    ("div3", "nosym", "ivfc_coor"),
    ("clip_pass", "angle", "rot"),           # crop 1 of angle sits above the clip
    ("huber_swap", "smoothl1", "nocs_coor"),
    ("pm_to_trans", "b3", "trans"),
])
def test_the_fixtures_reject_the_mutation(mutation, case, key):
    assert mutation in G.MUTATIONS
    clean, bad = fixture_errors(case), fixture_errors(case, mutate=mutation)
    print(f"{mutation} on {case}: {key} {clean['ones__' + key]:.2e} -> {bad['ones__' + key]:.2e}")
    assert clean["ones__" + key] < F64_BOUND
    assert not bad["ones__" + key] < 1e4 * F64_BOUND                     # far outside the bound, or NaN
    assert {m for m, _, _ in test_the_fixtures_reject_the_mutation.pytestmark[0].args[1]} == set(G.MUTATIONS)


# ------------------------------------------------------------------------------------------------ ABI of the family
def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_grad_header_equals_exported_symbols_and_prototypes():
    from givepose_amd import _lib, build
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (gpg_[a-z0-9_]+)", out))
    declared = set(re.findall(r"^int (gpg_[a-z0-9_]+)\s*\(", _header("givepose_grad.h"), re.M))
    assert declared == {"gpg_pose_loss_grad", "gpg_pose_decode_train_backward"}
    assert declared == exported, (declared - exported, exported - declared)
    assert set(_lib.GRAD_PROTOTYPES) == declared
    lib = _lib.load()
    for name, (argtypes, _) in _lib.GRAD_PROTOTYPES.items():
        assert getattr(lib, name).argtypes == argtypes
        decl = re.search(rf"^int {name}\s*\((.*?)\);", _header("givepose_grad.h"), re.M | re.S).group(1)
        assert len(decl.split(",")) == len(argtypes), name                 # one ctypes entry per declared parameter
    for k in ("TERMS", "SMALL", "DECODE"):
        v = re.search(rf"#define GPG_{k} (\d+)", _header("givepose_grad.h")).group(1)
        assert int(v) == getattr(_lib, "GPG_" + k), k
    assert set(re.findall(r" T (gpl_[a-z0-9_]+)", out)) == set(_lib.LOSS_PROTOTYPES)      # the forward family is as it was


def test_no_grad_symbol_in_the_other_headers_and_no_restatement_in_the_package():
    for h in ("givepose_hip.h", "givepose_align.h", "givepose_loss.h"):
        assert "gpg_" not in _header(h), h
    assert not re.search(r"^int gp[al]?_", _header("givepose_grad.h"), re.M)
    pkg = os.path.join(ROOT, "givepose_amd")
    src = open(os.path.join(pkg, "loss.py")).read()
    for ep in ("gpg_pose_loss_grad", "gpg_pose_decode_train_backward"):
        assert re.search(rf"L\.{ep}\(", src), ep                             # every entry point has its Python wrapper
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            s = open(os.path.join(pkg, fn)).read()
            assert "pose_loss_grad_ref" not in s and "pose_loss_ref" not in s, fn
    assert "lossgrad.hip" in __import__("givepose_amd.build", fromlist=["SOURCES"]).SOURCES


# ------------------------------------------------------------------------------------------------ the public surface
def test_public_surface_and_cpu_refusal():
    import inspect

    import torch

    import givepose_amd
    from givepose_amd import PoseLoss, PoseNet, _lib, loss
    assert givepose_amd.pose_decode_train_backward is loss.pose_decode_train_backward and givepose_amd.pose_decode_train is loss.pose_decode_train
    assert list(inspect.signature(PoseLoss.value_and_grad).parameters) == ["self", "pred_dict", "data", "gout", "return_details"]
    assert list(inspect.signature(PoseLoss.with_grad).parameters) == ["self", "pred_dict", "data"]
    p = inspect.signature(PoseNet.head_grads).parameters
    assert list(p) == ["self", "data", "pose_loss", "device", "gout", "groups"] and p["device"].default == "cuda" and p["gout"].default is None
    assert loss.GRAD_KEYS == G.GRAD_KEYS
    pred, data = R.make_inputs(B=1, P=1, seed=1)
    T = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        PoseLoss().value_and_grad(T(pred), T(data))
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        PoseLoss().with_grad(T(pred), T(data))
    inp, extra = R.make_decode_inputs(), G.make_decode_grad_inputs()
    with pytest.raises(_lib.GivePoseHipError, match="HIP device only"):
        loss.pose_decode_train_backward(**T({k: extra[k] for k in ("g_rot_ego", "g_trans")}), **T(inp))
