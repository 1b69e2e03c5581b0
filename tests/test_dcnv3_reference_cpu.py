"""tests/dcnv3_reference.py on the CPU, before a kernel is held against it (no GPU).

  agreement          with oracle.posenet_ref.dcnv3_forward_ref and the C oracle (oracle/dcnv3_ref.c, where it was built) at <= 1e-12 of scale
                     on the dyadic / edges sets, where the type of the location cannot matter; with the dcnv3_s* and dcnv3_any_fwd_* goldens
                     at their existing tolerances
  self-consistency   the opmath restatement (the kernel's association) within HALF the bound in front of the store on every case, its
                     correctly rounded store within the whole bound
  sensitivity        every mutation of dcnv3_reference.MUTATIONS is rejected; the table of which case rejects which is printed (-s)
  coverage           every edge class in every edges case, >= 10 % of the (pixel, group) samples of every +-3 case with a corner outside
                     the map, every kernel form reached, the location exact on the restricted sets
"""
import numpy as np
import pytest
import torch

import dcnv3_reference as D

F16, F32, F64 = torch.float16, torch.float32, torch.float64


def _square(c):
    return c.kh == c.kw and c.sh == c.sw and c.ph == c.pw and c.dh == c.dw


def _dense(c, I):
    """(offset, mask weights) as dense float64 (rows, .) tensors."""
    ow, oh, _ = D._read_slots(c, I)
    m, _ = D._mask_weights(c, I, F64)
    return torch.stack([ow, oh], -1).reshape(D.n_rows(c), -1), m.reshape(D.n_rows(c), -1)


# ------------------------------------------------------------------------------------------------ agreement
EXACT = [c for c in D.CASES if c.iset in ("edges", "dyadic") and c.poison is None]


@pytest.mark.parametrize("case", [c for c in EXACT if _square(c)], ids=lambda c: c.name)
def test_agrees_with_the_python_oracle(case):
    from oracle.posenet_ref import dcnv3_forward_ref
    I = D.inputs(case)
    v, _ = D.ref(I, case)
    off, m = _dense(case, I)
    o = dcnv3_forward_ref(I["x"].double(), off, m, case.kh, case.sh, case.ph, case.dh, case.G, case.D, case.os, case.rc).reshape(v.shape)
    assert float((o - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max()))


def _c_oracle():
    from oracle import dcnv3_c            # (builds itself with `make` where build() has not)
    return dcnv3_c


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.name)
def test_agrees_with_the_c_oracle(case):
    dc = _c_oracle()
    I = D.inputs(case)
    v, _ = D.ref(I, case)
    off, m = _dense(case, I)
    o = dc.dcnv3_forward_any_c(I["x"].double().numpy(), off.numpy(), m.numpy(), case.kh, case.kw, case.sh, case.sw, case.ph, case.pw, case.dh, case.dw,
                               case.G, case.D, case.os, case.rc)
    o = torch.from_numpy(o).reshape(v.shape)
    assert float((o - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max()))


def _golden_case(z, any_layout, dt):
    if any_layout:
        kh, kw, sh, sw, ph, pw, dh, dw, G, Dc, rc = (int(v) for v in z["params"])
    else:
        K, s, p, d, G, Dc, rc = (int(v) for v in z["params"])
        kh = kw = K; sh = sw = s; ph = pw = p; dh = dw = d
    N, H, W, _ = z["input"].shape
    c = D.mk("golden", dt, N, H, W, G=G, D=Dc, k=(kh, kw), ss=(sh, sw), pp=(ph, pw), dd=(dh, dw), os=float(z["offset_scale"]), rc=rc,
             entry="any" if any_layout else "fwd", om=dt)
    n = D.n_rows(c) * G * D.n_taps(c)
    I = dict(x=torch.from_numpy(z["input"]).to(dt), om=None, poison=None, off=torch.from_numpy(z["offset"]).reshape(-1)[:2 * n].to(dt),
             mask=torch.from_numpy(z["mask"]).reshape(-1)[:n].to(dt))
    return c, I


@pytest.mark.parametrize("name", ["dcnv3_s1", "dcnv3_s2_B1", "dcnv3_s2_B4", "dcnv3_s2_B5"])
def test_agrees_with_the_fp32_goldens(golden, name):
    z = golden(name)
    c, I = _golden_case(z, False, F32)
    v, _ = D.ref(I, c)
    assert np.abs(v.numpy().reshape(z["expected"].shape) - z["expected"]).max() < 5e-6          # tests/test_hip_ops.py::test_dcnv3_golden_fp32


@pytest.mark.parametrize("name", ["dcnv3_any_fwd_ref", "dcnv3_any_fwd_hw", "dcnv3_any_fwd_dil_rc"])
def test_agrees_with_the_any_goldens(golden, name):
    z = golden(name)
    c, I = _golden_case(z, True, F64)
    v, _ = D.ref(I, c)
    exp = np.asarray(z["expected"], dtype=np.float64)
    assert np.abs(v.numpy().reshape(exp.shape) - exp).max() < 1e-6 * max(1.0, np.abs(exp).max())  # tests/test_hip_dcnv3_any.py TOL[float64]


# ------------------------------------------------------------------------------------------------ self-consistency
def test_opmath_evaluation_within_half_the_bound_and_its_store_within_the_bound():
    worst, worst_stored = (0.0, ""), (0.0, "")
    for c in D.CASES:
        I = D.inputs(c)
        v, bound = D.ref(I, c)
        _, pre = D.ref(I, c, stored=False)
        got = D.f32(I, c)
        assert got.dtype == D.opmath(c) and got.shape == v.shape
        assert bool(torch.isfinite(v).all()) and bool((bound >= 0).all()) and bool((bound >= pre).all())
        ratio, msg = D.check(got, v, pre, f"{c.name} opmath")
        assert ratio <= 0.5, msg or f"{c.name}: the opmath evaluation is at {ratio:.3f} of the bound in front of the store"
        rs, msg = D.check(got.to(c.dt), v, bound, f"{c.name} opmath, stored")
        assert msg is None, msg
        worst, worst_stored = max(worst, (ratio, c.name)), max(worst_stored, (rs, c.name))
    print(f"CPU_RATIO gp_dcnv3_forward opmath {worst[0]:.4f} {worst[1]} (behind the store {worst_stored[0]:.4f} {worst_stored[1]})")


def test_zero_bound_where_every_tap_is_outside_and_buffers():
    c = D.BY_NAME["h-A-edges-weights-ld108"]
    I = D.inputs(c)
    v, bound = D.ref(I, c)
    zero = bound == 0
    assert bool(zero.any()) and bool((v[zero] == 0).all())
    buf = D.with_tail(v, 256)
    assert D.check_buffer(buf, v, bound)[1] is None
    bad = buf.clone()
    bad[int(zero.reshape(-1).nonzero()[0])] = 2.0 ** -24                     # an exact zero is asked for
    assert D.check_buffer(bad, v, bound)[1] is not None
    bad = buf.clone()
    bad[-1] = 0.0
    assert D.check_buffer(bad, v, bound)[1] is not None


# ------------------------------------------------------------------------------------------------ coverage
def test_every_edge_class_in_every_edges_case():
    for c in D.CASES:
        if c.iset == "edges":
            k = D.classify(c, D.inputs(c))
            assert all(n > 0 for n in k.values()), (c.name, k)


def test_continuous_sets_reach_outside_the_map():
    for c in D.CASES:
        if c.iset == "c3":
            f = D.outside_fraction(c, D.inputs(c))
            assert f >= 0.1, (c.name, f)


def test_every_kernel_form_is_reached_and_the_listed_shapes_route_as_listed():
    reached = D.forms_reached()
    missing = [f for f in D.FORMS if f not in reached]
    assert not missing, missing
    for f in D.FORMS:
        print(f"FORM {f}: {len(reached[f])} cases, e.g. {reached[f][0]}")
    by = D.BY_NAME
    assert D.form_taken(by["h-A-c3-logits-ld108"]) == "dcnv3_wave8_kernel<float,DPP>" and D.grid_x(by["h-A-c3-logits-ld108"]) == 6
    assert D.grid_x(by["h-B-c3-logits-ld108"]) == 13 and D.grid_x(by["h-C-c3-logits-ld108"]) == 4 and D.grid_x(by["h-D-c3-weights-ld108"]) == 4
    assert D.form_taken(by["f-A-c12-logits-om16"]) == "dcnv3_wave_kernel<float,half,3,PATCH>"
    assert D.form_taken(by["h-w3-A-c3-logits-ld108"]) == "dcnv3_wave_kernel<half,float,3>" and D.n_rows(by["h-w3-A-c3-logits-ld108"]) == 105
    assert D.form_taken(by["f-K4-c3-logits-ld192"]) == "dcnv3_wave_kernel<float,float>" and D.n_rows(by["f-K4-c3-logits-ld192"]) % 4 == 3
    assert D.form_taken(by["h-gen-G8D64K3-edges-ld220"]) == "dcnv3_generic_kernel<half,float>"
    for c in D.PATCH_CASES:
        Ho, Wo = D.out_hw(c)
        assert Ho % 4 == 0 and Wo % 4 == 0 and ("wave8" in D.form_taken(c)) == (c.dt == F16) and "PATCH" in D.form_taken(c, {"GP_DCN_WAVE8": "0"})
    assert all(c.H != c.W for c in D.FWD_CASES if "-B-" not in c.name)        # the one square shape is kept for xcd_chunk's remainder


def test_location_is_exact_on_the_restricted_sets():
    for c in D.CASES:
        I = D.inputs(c)
        assert c.os == 1.0 or c.iset in ("edges", "dyadic"), c.name
        if c.iset in ("edges", "dyadic"):
            a, b = D.locations(c, I, F32), D.locations(c, I, F64)
            assert bool((a[0].double() == b[0]).all()) and bool((a[1].double() == b[1]).all()), c.name
        for k, dt in (("x", c.dt), ("off", c.om_dt), ("mask", c.om_dt)):
            assert I[k].dtype == dt


def test_poisoned_cases_have_every_kind_of_output():
    for c in D.CASES:
        if c.poison is not None:
            I = D.inputs(c)
            hard, soft = D.poison_sets(I, c)
            lh, lw, _ = D.locations(c, I, F32)
            outr = ~((lh > -1) & (lw > -1) & (lh < c.H) & (lw < c.W))
            clean = ~(hard | soft).reshape(D.n_rows(c), c.G, c.D)[:, :, 0]
            first = torch.arange(D.n_rows(c)) < D.n_rows(c) // c.N               # the poisoned image's rows
            assert bool(hard.any()) and bool((clean & outr.any(-1) & first.view(-1, 1)).any()), c.name
            assert not bool(torch.isfinite(I["x"][0, 0, 0]).any())


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("mut", [m for m, _ in D.MUTATIONS])
def test_mutation_is_rejected(mut):
    eligible = [c for c in D.CASES if dict(D.MUTATIONS)[mut](c) and c.poison is None]
    assert eligible, "no case can expose this mutation"
    rejecting = []
    for c in eligible:
        I = D.inputs(c)
        v, bound = D.ref(I, c)
        wrong, _ = D.ref(I, c, mut=mut)
        ratio, msg = D.check_buffer(D.with_tail(wrong), v, bound, f"{mut} {c.name}")
        if msg is not None:
            rejecting.append((c, ratio))
    low = min(rejecting, key=lambda t: t[1]) if rejecting else (None, 0.0)
    passed = [c.name for c in eligible if c.name not in {r.name for r, _ in rejecting}]
    print(f"MUTATION {mut}: rejected on {len(rejecting)} of {len(eligible)} eligible cases, smallest ratio {low[1]:.3g} ({low[0].name if low[0] else ''})"
          + (f"; passes on {passed}" if passed else ""))
    assert rejecting, f"{mut} passes the checker on every eligible case"
    if mut == "mask_fp16":
        assert any(c.dt == F16 for c, _ in rejecting)
    if mut == "products_fp16":
        assert any(c.dt == F32 for c, _ in rejecting)
    if mut not in ("mask_fp16",):          # structural mutations: every eligible case must expose them
        assert not passed, f"{mut} passes the checker on {passed}"
