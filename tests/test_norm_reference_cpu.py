"""The checker of tests/norm_reference.py on the CPU, before a kernel is held against it (the rules of tests/test_ops_reference_cpu.py).

  self-consistency   every operation evaluated in torch float32 stays within HALF its bound in front of an fp16 store and within the whole
                     bound behind it, on every input set the GPU tests use (the large cases included); fp32 outputs: half the bound.
                     gp_groupnorm_upsample2x rounds its intermediate tensor to fp16: that rounding counts in full, like a store's
  honest bounds      zero-mean fp16 cases: the median over elements of bound / max(|v|, 1e-3) is at most 3 x 2^-11; the offset cases
                     really have median |mean| / std > 10
  routing            form_taken(case) is the form every gp_dwconv_ln case names (a forced act code on a shape the kernel refuses would
                     fall through to the strip kernel and test nothing), and the GroupNorm regimes of the large cases are the intended ones
  sensitivity        every deliberately wrong float64 variant (norm_reference.MUTATIONS) is rejected on the cases named for it
"""
import pytest
import torch

import norm_reference as N


def _rows(t):
    return t if t.dim() == 2 else t.reshape(1, -1)


# ------------------------------------------------------------------------------------------------ self-consistency
_LARGE_OPS = [n for n, o in N.OPS.items() if any(N.is_large(c) for c in o.cases)]


@pytest.mark.parametrize("name,large", [(n, False) for n in N.OPS] + [(n, True) for n in _LARGE_OPS],
                         ids=[n.replace(" ", "_") for n in N.OPS] + [n.replace(" ", "_") + "-large" for n in _LARGE_OPS])
def test_float32_evaluation_within_half_the_bound(name, large):
    op = N.OPS[name]
    worst, worst16 = (0.0, ""), 0.0
    for case in (c for c in op.cases if N.is_large(c) == large):
        I = op.inputs(case)
        v, bound = op.ref(I, case)
        got = op.f32(I, case)
        assert got.shape == v.shape and got.dtype == torch.float32, (name, case.name)
        assert bool(torch.isfinite(v).all()) and bool((bound >= 0).all())
        dt = N.out_dtype(name, case)
        if dt == torch.float16 and op.pre is not None:
            r16, msg16 = N.check(got.to(dt), v, bound, f"{name} {case.name} float32, stored")
            assert msg16 is None, msg16
            worst16 = max(worst16, r16)
            bound = op.pre(I, case)[1]
            if name in N.ROUNDING_IN_PRE:        # an fp16 intermediate: its rounding in full, half of the rest
                bound = 2 * N.ROUNDING_IN_PRE[name](I, case) + (bound - N.ROUNDING_IN_PRE[name](I, case))
        else:
            got = got.to(dt)
        ratio, msg = N.check(got, v, bound, f"{name} {case.name} float32")
        worst = max(worst, (ratio, case.name))
        assert ratio <= 0.5, msg or f"{name} {case.name}: float32 evaluation at {ratio:.3f} of the bound"
    print(f"CPU_RATIO {name}{' LARGE' if large else ''} {worst[0]:.4f} {worst[1]}" + (f" (behind the fp16 store {worst16:.4f})" if worst16 else ""))


@pytest.mark.parametrize("name", list(N.OPS))
def test_correct_buffer_is_accepted_and_a_touched_sentinel_is_not(name):
    op = N.OPS[name]
    case = next(c for c in op.cases if getattr(c, "mode", "") == "ldy") if name in ("gp_layernorm", "gp_groupnorm_apply") else op.cases[0]
    v, bound = (_rows(t) for t in op.ref(op.inputs(case), case))
    ldy, col0 = (N.ln_ldy(case), 0) if name == "gp_layernorm" else N.gn_layout(case) if name == "gp_groupnorm_apply" else (v.shape[1], 0)
    buf = N.filled_buffer(v, ldy, col0, v.shape[1])
    assert N.check_strided(buf, v, bound, ldy, col0)[1] is None
    for touched in (buf.numel() - 1, (col0 + v.shape[1]) % ldy if ldy > v.shape[1] else buf.numel() - 2):
        bad = buf.clone()
        bad[touched] = 0.0
        assert N.check_strided(bad, v, bound, ldy, col0)[1] is not None, touched
    nan = buf.clone()
    nan[col0] = N.NAN
    assert N.check_strided(nan, v, bound, ldy, col0)[1] is not None


# ------------------------------------------------------------------------------------------------ honest bounds
def _median_relative_bound(v, bound):
    return float((bound / v.abs().clamp_min(1e-3)).median())


def test_bounds_of_zero_mean_fp16_cases_are_tight():
    """On the normalised values themselves (no activation: behind a ReLU or GELU half the values are at or near zero, where the ratio
    measures the floor of 1e-3 and not the bound)."""
    worst = {}
    for name, zero_mean in [("gp_dwconv_ln", lambda c: c.dt == N.f16 and not c.offset and not c.large and c.act == N.ACT_NONE),
                            ("gp_layernorm", lambda c: c.dt == N.f16 and c.mode != "inf32"),
                            ("gp_groupnorm_apply", lambda c: c.dt == N.f16 and not c.bigmean and not c.large and c.act == N.ACT_NONE)]:
        op = N.OPS[name]
        for case in filter(zero_mean, op.cases):
            m = _median_relative_bound(*op.ref(op.inputs(case), case))
            worst[name] = max(worst.get(name, (0.0, "")), (m, case.name))
            assert worst[name][0] > 0
            assert m <= N.TIGHT, f"{name} {case.name}: median bound / |v| {m:.3g} > {N.TIGHT:.3g}"
    for name, (m, cid) in worst.items():
        print(f"TIGHTNESS {name} {m:.3g} {cid}")


def test_offset_cases_have_a_large_mean():
    cases = [c for c in N.DW_CASES if c.offset]
    assert {c.form for c in cases} >= {N.STRIP_PPT2, N.MFMA_11, N.TALL_J8, N.TALL_WIDE, N.QUARTER, N.PAIR_TH2}      # each one-pass family and the strip kernel
    for case in cases:
        r = N.dw_mean_over_std(case)
        assert r > 10, (case.name, r)
    for case in (c for c in N.DW_CASES if not c.offset and not c.large):
        assert N.dw_mean_over_std(case) < 0.5, case.name
    for case in (c for c in N.GN_CASES if c.bigmean):
        x = N.gn_inputs(case)["x"].double()
        cpg = case.C // N.GN_G
        g3 = x[:, :, 3 * cpg:4 * cpg]
        assert 18 < float(g3.mean().abs() / g3.std()) < 22
    for case in (c for c in N.LN_CASES if c.mode == "inf32"):
        x = N.ln_inputs(case)["x"].double()
        assert float((x.mean(1).abs() / x.std(1)).median()) > 500        # rounding these rows to fp16 first leaves steps of 2^-4 on a spread of 0.1


# ------------------------------------------------------------------------------------------------ routing
def test_every_dwconv_case_reaches_the_form_it_names():
    assert N.routing_env_is_default(), "a GP_DW* variable is set: gp_dwconv_ln's routing is not the default one"
    for c in N.DW_CASES:
        assert N.form_taken(c.B, c.H, c.W, c.C, c.KS, c.code, c.npix, c.dt) == c.form, c.name
    assert len({c.name for c in N.DW_CASES}) == len(N.DW_CASES)
    # a forced code on a shape its guard refuses falls through: the restatement shows it
    assert N.form_taken(2, 12, 16, 128, 7, 110, 2 * 12 * 16, N.f16) == N.STRIP_PPT2       # H % 8 != 0: not the tall kernel (nor, with dbg = 10, an MFMA one)
    assert N.form_taken(3, 8, 32, 256, 3, 120, 768, N.f16) == N.REFUSED                   # 120 + no activation
    assert N.form_taken(2, 16, 24, 1024, 7, 104, 768, N.f16) == N.STRIP_PPT2              # no 8-slab fp16 instantiation
    # the thresholds between two kernels, from either side
    assert N.form_taken(129, 8, 16, 512, 7, 0, 129 * 128, N.f16) == N.QUARTER and N.form_taken(130, 8, 16, 512, 7, 0, 130 * 128, N.f16) == N.TALL_J8
    assert N.form_taken(4, 12, 64, 512, 7, 0, 4 * 768, N.f16) == N.STRIP_PPT2 and N.form_taken(8, 12, 16, 256, 7, 0, 8 * 192, N.f16) == N.STRIP_PPT2
    assert N.form_taken(42, 12, 64, 512, 7, 0, 42 * 768, N.f16) == N.MFMA_42
    assert N.form_taken(32, 8, 8, 1024, 7, 0, 32 * 64, N.f16) == N.PAIR_TH2 and N.form_taken(30, 8, 8, 1024, 7, 0, 30 * 64, N.f16) == N.STRIP_PPT2
    assert N.form_taken(4, 64, 64, 256, 3, N.ACT_GELU, 16384, N.f16) == N.DW3_TH2 and N.form_taken(4, 64, 64, 256, 3, N.ACT_GELU, 16320, N.f16) == N.STRIP_PPT2


def test_every_form_has_a_case():
    forms = {(c.form, c.C, c.dt, c.KS) for c in N.DW_CASES}
    want = {(N.STRIP_PPT2, 512, N.f16, 7), (N.STRIP_PPT2, 256, N.f16, 3), (N.STRIP_PPT8, 1024, N.f16, 7), (N.MFMA_11, 128, N.f16, 7),
            (N.MFMA_21, 256, N.f16, 7), (N.MFMA_42, 512, N.f16, 7), (N.MFMA_41, 512, N.f16, 7), (N.TALL_WIDE, 128, N.f16, 7), (N.TALL_WIDE, 256, N.f16, 7),
            (N.PAIR_TH4, 1024, N.f16, 7), (N.PAIR_TH2, 1024, N.f16, 7), (N.DW3_TH4, 256, N.f16, 3), (N.DW3_TH2, 256, N.f16, 3)}
    want |= {(f, C, N.f16, 7) for f in (N.TALL_J8, N.TALL_J9, N.QUARTER, N.TILED) for C in (128, 256, 512)}
    want |= {(N.TILED, C, N.f32, 7) for C in (128, 256, 512, 1024)} | {(N.STRIP_F32, C, N.f32, KS) for C in (64, 1024) for KS in (3, 7)}
    assert want <= forms, want - forms
    families = {c.form.split("<")[0] for c in N.DW_CASES}
    assert families == {"strip", "lds-tiled", "mfma", "tall", "pair", "dw3tile"}
    assert {c.form.split("<")[0] for c in N.DW_CASES if c.eps == 0.25} == families     # one eps = 0.25 case per form family
    assert any(c.eps == 0.25 for c in N.DW_CASES if c.form == N.QUARTER) and any(c.eps == 0.25 for c in N.DW_CASES if c.form == N.STRIP_F32)


def test_groupnorm_regimes():
    assert N.gn_pxb(3, 16) == 256 and N.gn_pxb(3, 35) == 256 and N.gn_pxb(3, 100) == 64 and N.gn_pxb(2, 1024) == 64
    for case in N.GN_CASES:
        regime = (N.gn_pxb(case.B, case.HW), N.gn_apply_pxb(case.B, case.HW))
        assert regime == (N.GN_LARGE_REGIMES[case.name] if case.large else (256 if case.HW < 64 else 64, 32)), case.name
        if case.rows is not None:
            assert case.HW % case.rows == 0
    assert {N.GN_LARGE_REGIMES[c.name] for c in N.GN_CASES if c.large} == {(64, 64), (256, 128)}
    assert (N.gn_pxb(128, 4096), N.gn_apply_pxb(128, 4096)) == (256, 256)       # the regime that has no case (norm_reference.GN_LARGE_REGIMES)
    tails = {c.HW % N.gn_pxb(c.B, c.HW) for c in N.GN_CASES}
    assert 36 in tails and 35 in tails and 0 in tails


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("name,mut", [(n, m) for n, m, _ in N.MUTATIONS], ids=[f"{n.replace(' ', '_')}-{m}" for n, m, _ in N.MUTATIONS])
def test_mutation_is_rejected(name, mut):
    exposing = [f for n, m, f in N.MUTATIONS if (n, m) == (name, mut)][0]
    cases = [c for c in N.OPS[name].cases if exposing(c)]
    assert cases and not any(N.is_large(c) for c in cases), "no input set exposes this mutation"
    low = (float("inf"), "")
    for case in cases:
        buf, v, bound, ldy, col0 = N.mutant_buffer(name, case, mut)
        if buf.numel() > v.shape[0] * ldy + v.shape[1]:          # a longer buffer: the values a kernel writes behind the end
            ratio, msg = N.check_buffer(buf, v, bound, f"{name} {mut} {case.name}")
        else:
            ratio, msg = N.check_strided(buf, v, bound, ldy, col0, f"{name} {mut} {case.name}")
        assert msg is not None, f"{name} {case.name}: mutation {mut} passes the checker (ratio {ratio:.3g})"
        low = min(low, (ratio, case.name))
    print(f"MUTATION {name} {mut}: {len(cases)} cases, smallest ratio {low[0]:.3g} ({low[1]})")
