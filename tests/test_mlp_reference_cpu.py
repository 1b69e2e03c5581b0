"""CPU: the checker of the fused ConvNeXt MLP (tests/mlp_reference.py) is itself tested.

  * An emulation of the kernel's arithmetic (mlp_reference.emulate: fp32 accumulation chunk by chunk with the bias as initial value, the
    GELU as gelu16_slice computes it on fp16 values with the GELU16_C coefficients -- or the fp32 polynomial --, the hidden tensor
    rounded to fp16, gamma * acc rounded to fp16, then an fp16 add of the residual) stays inside the bound on every A, B and C case of
    C = 128 and 256 and on the smallest C = 512 case of each family: the reference alone does not exceed its own bound.
  * Each deliberately wrong variant of the emulation is rejected by the family named beside it; two legitimate variants are accepted.
  * The case table is complete: every kernel gp_convnext_mlp's dispatch can launch is a form of the table, every refusal of the
    library is a row of the refusal table, and givepose_amd.ops refuses malformed arguments before the library is reached.
"""
import os
import re

import numpy as np
import pytest
import torch

import mlp_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_FORMS = ("c128w4", "c128s32", "c128g0", "c256", "c256g0")          # (c128w8 computes what c128w4 computes: same arithmetic)


def _emul(form, case, mut=None):
    f = mr.FORMS[form]
    return mr.emulate(mr.operands(f.C, case), f.gelu, f.s32, mut=mut, rows=f.rows)


def _ratio(form, case, mut=None):
    return mr.check_case(form, case, _emul(form, case, mut))


# ---------------------------------------------------------------------------------------------------------------- inside the bound
@pytest.mark.parametrize("family", mr.FAMILIES)
@pytest.mark.parametrize("form", EMUL_FORMS + ("c512",))
def test_emulation_meets_the_bound(form, family):
    cs = mr.cases(form, family)
    if form == "c512":
        cs = cs[:1]                                              # the smallest case of the family
    for case in cs:
        ratio, msg = _ratio(form, case)
        print(f"\n{mr.case_name(form, case)}: emulation max err/bound {ratio:.3g}")
        assert msg is None, msg


def test_operands_reach_both_gelu_tails_and_stay_in_fp16_range():
    """Family A's pre-activations go well beyond +-4.4 on both sides; nothing leaves the finite fp16 range (asserted in reference())."""
    for C in (128, 256, 512):
        case = mr.cases({128: "c128w4", 256: "c256", 512: "c512"}[C], "A")[0]
        v1 = mr._stage1(C, case).v
        assert float(v1.max()) > 20.0 and float(v1.min()) < -20.0, (C, float(v1.min()), float(v1.max()))
        assert float((v1.abs() > 4.4).double().mean()) > 0.05
        assert float(v1.abs().max()) < 65504.0


def test_family_c_places_every_finite_fp16_value_under_the_selectors():
    for form in ("c128w4", "c256", "c512"):
        f = mr.FORMS[form]
        seen = set()
        for case in mr.cases(form, "C"):
            op = mr.operands(f.C, case)
            fam, M, s = case
            seen |= set(np.unique(op.w1[4 * torch.arange(f.C) + s].numpy().astype(np.float16).view(np.uint16)).tolist())
            assert M >= f.C
        assert len(seen) == 63488, (form, len(seen))


# ---------------------------------------------------------------------------------------------------------------- mutations
# (mutation, family that must reject it, form)
REJECTED = [
    ("pack_nt_fq", "B", "c128w4"), ("pack_nt_fq", "B", "c256"),
    ("pack_s32_for_16", "B", "c128w4"),
    ("b1_prev_chunk", "B", "c128w4"), ("b1_prev_chunk", "B", "c256g0"),
    ("skip_last_chunk", "B", "c128w4"), ("skip_last_chunk", "B", "c256"),
    ("stale_stage", "B", "c128w4"), ("stale_stage", "B", "c128s32"),
    ("gamma_mod16", "A", "c128w4"), ("gamma_mod16", "A", "c256"),
    ("b2_after_gamma", "A", "c128w4"), ("b2_after_gamma", "A", "c256g0"),
    ("no_clamp", "C", "c128w4"), ("no_clamp", "A", "c128w4"), ("no_clamp", "C", "c256"),
    ("sigmoid", "C", "c128w4"), ("sigmoid", "C", "c128g0"),
]


@pytest.mark.parametrize("mut,family,form", REJECTED)
def test_mutation_is_rejected(mut, family, form):
    """Families B and C: all four selectors together pin a mutation (skip_last_chunk only touches the channels whose selected unit
    lies in the last chunk, ...), so "rejected by the family" means: by at least one of its cases -- and the smallest dense case for A."""
    cs = mr.cases(form, family)[:1] if family == "A" else mr.cases(form, family)
    worst = 0.0
    for case in cs:
        ratio, msg = _ratio(form, case, mut)
        worst = max(worst, ratio)
    print(f"\n{mut} on {form}, family {family}: max err/bound {worst:.3g}")
    assert worst > 1.0, (mut, form, family, worst)


def test_b1_prev_chunk_is_invisible_to_family_c():
    """Family C sets b1 = 0: it cannot see a wrong b1 index.  Written down so that nobody relies on C for it (B does see it)."""
    for case in mr.cases("c128w4", "C"):
        ratio, msg = _ratio("c128w4", case, "b1_prev_chunk")
        assert msg is None, msg


def test_rows_written_without_the_xcd_remap_are_rejected_at_nine_workgroups():
    for form, M in (("c256", 2304), ("c128w4", 1152 + 1152)):           # 9 workgroups of 256 rows; 18 of 128 (remainder 2)
        case = ("A", M, None)
        assert case in mr.cases(form, "A")
        n = M // mr.FORMS[form].rows
        assert n % 8 != 0 and [mr.xcd_chunk(b, n) for b in range(n)] != list(range(n))
        assert sorted(mr.xcd_chunk(b, n) for b in range(n)) == list(range(n))       # bijective
        ratio, msg = _ratio(form, case, "no_xcd_remap")
        print(f"\nno_xcd_remap on {form} M{M}: max err/bound {ratio:.3g}")
        assert ratio > 1.0


def test_one_extra_row_written_at_M_trips_the_sentinels():
    M, C = 256, 128
    buf = torch.full((M + mr.SENT_ROWS, C), mr.SENT).half()
    assert mr.sentinels_intact(buf, M)
    buf[M] = 0.5
    assert not mr.sentinels_intact(buf, M)
    buf[M] = mr.SENT
    buf[M + mr.SENT_ROWS - 1, C - 1] = 0.0
    assert not mr.sentinels_intact(buf, M)


@pytest.mark.parametrize("mut", ["reverse_chunks", "single_rounding"])
def test_legitimate_variant_is_accepted(mut):
    """Negative controls: another accumulation order of the chunks, and a residual add with a single rounding instead of the lean
    epilogue's two, differ from the emulation in some bits and must both pass -- the bound is not tighter than correct code needs."""
    changed = 0
    for form, family in (("c128w4", "A"), ("c256", "A"), ("c128w4", "B"), ("c128g0", "A")):
        case = mr.cases(form, family)[0]
        got = _emul(form, case, mut)
        changed += int((got != _emul(form, case)).sum())
        ratio, msg = mr.check_case(form, case, got)
        print(f"\n{mut} on {mr.case_name(form, case)}: max err/bound {ratio:.3g}")
        assert msg is None, msg
    assert changed > 0, "the variant changes no bit: it tests nothing"


def test_swapping_two_hidden_units_is_far_outside_the_bound():
    f = mr.FORMS["c128w4"]
    case = mr.cases("c128w4", "B")[0]
    op = mr.operands(f.C, case)
    w2 = op.w2.clone()
    w2[:, [40, 44]] = w2[:, [44, 40]]
    ratio, msg = mr.check_case("c128w4", case, mr.emulate(op._replace(w2=w2), f.gelu))
    assert ratio > 10.0, ratio


# ---------------------------------------------------------------------------------------------------------------- the pack orders
def test_pack_orders_are_permutations_and_match_the_kernels_fragment_layouts():
    p16, p32 = mr.perm16(), mr.perm32()
    assert sorted(p16) == list(range(32)) and sorted(p32) == list(range(32)) and list(p16) != list(p32)
    # 16x16x32: lane (fr, fq) holds, after GEMM1, h[nt*16 + fq*4 + j] in register (nt, j); as B fragment those 8 values are k = fq*8 + nt*4 + j
    for fq in range(4):
        for nt in range(2):
            for j in range(4):
                assert p16[fq * 8 + nt * 4 + j] == nt * 16 + fq * 4 + j
    # 32x32x16: accumulator register r of half hh = unit 8 (r / 4) + 4 hh + r % 4; K block kb holds registers 8 kb .. 8 kb + 7 as e
    for kb in range(2):
        for hh in range(2):
            for e in range(8):
                r = 8 * kb + e
                assert p32[kb * 16 + hh * 8 + e] == 8 * (r // 4) + 4 * hh + r % 4


# ---------------------------------------------------------------------------------------------------------------- completeness
def _mlp_source():
    with open(os.path.join(ROOT, "givepose_amd", "csrc", "mlp.hip")) as f:
        return f.read()


def test_case_table_covers_every_launch_of_the_dispatch():
    launched = mr.launches_in_source(_mlp_source())
    table = {f.kernel for f in mr.FORMS.values()} | set(mr.PACK_KERNELS)
    assert launched == table, (sorted(launched - table), sorted(table - launched))
    assert len(mr.FORMS) == 7
    for f in mr.FORMS.values():                     # every form has all three numeric families, none of them expected to be refused
        for fam in mr.FAMILIES:
            cs = mr.cases(f.name, fam)
            assert len(cs) == 4
            for fam_, M, s in cs:
                assert mr.expected(f.C, M, f.s32, f.env) is None, (f.name, fam_, M)
                assert M % f.rows == 0
        wgs = [M // f.rows for M in mr.dense_M(f.name)]
        assert min(wgs) < 8 and max(wgs) > 8 and any(w > 8 and w % 8 for w in wgs), (f.name, wgs)
    assert {s for s in mr.ENV_SETTINGS} == {f.env for f in mr.FORMS.values() if f.env}
    assert sorted(n for ns in mr.ENV_SETTINGS.values() for n in ns) == sorted(f.name for f in mr.FORMS.values() if f.env)


def test_refusal_table_covers_every_require_of_the_entry_point():
    """Every GP_REQUIRE message of gp_convnext_mlp that an argument can trigger is the fragment of some row (the null-operand check
    cannot be reached through tensors: an empty tensor is refused by its M first; the second GP_MLP_S32 check repeats the first)."""
    src = _mlp_source()
    body = src[src.index('extern "C" int gp_convnext_mlp('):]
    msgs = re.findall(r'GP_REQUIRE\(.*?"(gp_convnext_mlp: [^"]*)"', body, re.S)
    assert len(msgs) >= 8
    unreachable = ("null operand", "GP_MLP_S32 is built for C = 128")
    for m in msgs:
        if any(u in m for u in unreachable):
            continue
        parts = [p.strip() for p in re.split(r"%l?d", m[len("gp_convnext_mlp: "):]) if len(p.strip()) >= 8]
        assert any(any(p in r.frag or r.frag in p for p in parts) for r in mr.REFUSALS if r.level == "lib"), m
    names = {r.name for r in mr.REFUSALS}
    for need in ("M0", "M100", "M384", "M192-C512", "C64", "C384", "fp32-raw", "fp32-tensors", "offset8", "out-is-x", "s32-C256",
                 "gelu16off-s32", "gelu16off-C512"):
        assert need in names, need
    for r in mr.REFUSALS:
        assert mr.expected(r.C, r.M, env=r.env, what=r.what) is r, r.name


def test_ops_wrapper_refuses_before_the_library_is_reached(monkeypatch):
    """givepose_amd.ops checks device, dtype, shape and contiguity itself: with the library loader made to fail, a CPU tensor and
    then (host tensors made to answer is_cuda, so that the checks behind the device check are reached) every malformed operand of the
    refusal table raise the wrapper's own error."""
    from givepose_amd import ops

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "_L", no_library)
    C, M = 128, 256
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)
    f = lambda *s: torch.zeros(*s)
    with pytest.raises(RuntimeError, match="x must be a CUDA tensor"):
        ops.convnext_mlp(h(M, C), h(4 * C, C), f(4 * C), h(C, 4 * C), f(C), f(C), h(M, C), h(M, C))
    with pytest.raises(RuntimeError, match="w2 must be a CUDA tensor"):
        ops.convnext_mlp_pack_w2(h(C, 4 * C))
    # the checks behind the device check, on stand-ins that claim to be on the device
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    good = dict(x=h(M, C), w1=h(4 * C, C), b1=f(4 * C), w2p=h(C, 4 * C), b2=f(C), gamma=f(C), residual=h(M, C), out=h(M, C))
    bad = {
        "fp32-tensors": dict(x=f(M, C)), "fp32-out": dict(out=f(M, C)), "fp16-b1": dict(b1=h(4 * C)), "fp16-gamma": dict(gamma=h(C)),
        "strided-out": dict(out=h(M, 2 * C)[:, :C]), "strided-w1": dict(w1=h(C, 4 * C).t()), "w1-shape": dict(w1=h(C, 4 * C)),
        "b1-shape": dict(b1=f(C)), "w2p-shape": dict(w2p=h(4 * C, C)), "b2-shape": dict(b2=f(4 * C)), "gamma-shape": dict(gamma=f(2 * C)),
        "res-shape": dict(residual=h(M // 2, C)), "x-3d": dict(x=h(2, M // 2, C)),
    }
    assert set(bad) | {"cpu-x"} == {r.name for r in mr.REFUSALS if r.level == "ops"}
    for name, change in bad.items():
        frag = mr.REFUSAL_BY_NAME[name].frag
        with pytest.raises((TypeError, RuntimeError)) as e:
            ops.convnext_mlp(**{**good, **change})
        assert frag in str(e.value), (name, str(e.value))
    with pytest.raises(AssertionError, match="the library was reached"):       # and a well-formed call does get through to it
        ops.convnext_mlp(**good)
    for w2, frag in ((f(C, 4 * C), "w2: expected torch.float16"), (h(C, 2 * C), "w2: expected shape (C, 4C)"), (h(4 * C, C).t(), "w2 tensor has to be contiguous")):
        with pytest.raises((TypeError, RuntimeError)) as e:
            ops.convnext_mlp_pack_w2(w2)
        assert frag in str(e.value), str(e.value)

