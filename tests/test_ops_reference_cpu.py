"""The checker of tests/ops_reference.py on the CPU, before a kernel is held against it.

  self-consistency   every operation evaluated in torch float32 stays within HALF its bound on every input set the GPU tests use (the
                     other half is room for the kernel's summation order, which the bound covers on paper); with an fp16 store, whose
                     correct rounding alone may use all of e_out, half the bound in front of the store and the whole bound behind it
  sensitivity        deliberately wrong float64 implementations (ops_reference.MUTATIONS) are rejected on those same input sets
  closure            every `int gp_*(` of include/givepose_hip.h is mapped to the operator-level test that covers it
  head kernels       (gp_convnext_stem ... gp_groupnorm_apply_xyz) additionally: every kernel instantiation is taken by some case, the inputs
                     reach the branches the case comments claim, and the pose decode -- which has no static bound -- rejects its mutants by
                     the yardstick rule on a well-conditioned float64 reference
"""
import ast
import os
import re

import pytest
import torch

import ops_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ self-consistency
@pytest.mark.parametrize("name", list(R.OPS))
def test_float32_evaluation_within_half_the_bound(name):
    op = R.OPS[name]
    worst, worst16 = (0.0, ""), 0.0
    for case in op.cases:
        I = op.inputs(case)
        v, bound = op.ref(I, case)
        got = op.f32(I, case)
        assert got.shape == v.shape and got.dtype == torch.float32, (name, case)
        assert bool(torch.isfinite(v).all()) and bool((bound >= 0).all())
        dt = R.case_dtype(case)
        if dt == torch.float16 and op.pre is not None:
            # a correct fp16 rounding may use all of e_out by itself: half the bound in front of the store, the whole bound behind it
            r16, msg16 = R.check(got.to(dt), v, bound, f"{name} {R.case_id(case)} float32, stored")
            assert msg16 is None, msg16
            worst16 = max(worst16, r16)
            bound = op.pre(I, case)[1]
        else:
            got = got.to(dt)
        ratio, msg = R.check(got, v, bound, f"{name} {R.case_id(case)} float32")
        worst = max(worst, (ratio, R.case_id(case)))
        assert ratio <= 0.5, msg or f"{name} {R.case_id(case)}: float32 evaluation at {ratio:.3f} of the bound"
    print(f"CPU_RATIO {name} {worst[0]:.4f} {worst[1]}" + (f" (behind the fp16 store {worst16:.4f})" if worst16 else ""))


@pytest.mark.parametrize("name", list(R.OPS))
def test_correct_buffer_is_accepted_and_a_touched_sentinel_is_not(name):
    op = R.OPS[name]
    case = op.cases[0]
    v, bound = op.ref(op.inputs(case), case)
    buf = R.with_tail(v, v.shape[-1] if v.dim() > 1 else 1)
    assert R.check_buffer(buf, v, bound)[1] is None
    buf[-1] = 0.0
    assert R.check_buffer(buf, v, bound)[1] is not None
    nan = R.with_tail(v)
    nan[0] = R.NAN
    assert R.check_buffer(nan, v, bound)[1] is not None


# ------------------------------------------------------------------------------------------------ the input sets reach the edges
def _pre_activations(name, case):
    I = R.OPS[name].inputs(case)
    if name == "gp_sn_stem":
        return R.sn_stem_pre(I)[0], 2
    if name == "gp_sn_pointwise":
        return R.sn_pw_pre(I, case)[0], case[4]
    if name == "gp_sn_depthwise":
        return R.sn_dw_pre(I, case)[0], case[6]
    if name == "gp_sn_se":
        return R.sn_se_pre(I)[0], 2          # the hard-sigmoid gate has the Hardswish's break points
    raise KeyError(name)


@pytest.mark.parametrize("name", ["gp_sn_stem", "gp_sn_pointwise", "gp_sn_depthwise", "gp_sn_se"])
def test_pre_activations_reach_every_branch(name):
    union = {}
    for case in R.OPS[name].cases:
        p, act = _pre_activations(name, case)
        br = R.act_branches(p, act)
        if p.numel() >= R.BRANCH_MIN_VALUES:
            assert all(br), (name, case, br)
        union[act] = tuple(a or b for a, b in zip(union.get(act, (False,) * 3), br))
    assert all(all(b) for b in union.values()), union


def test_se_gates_differ_between_images_and_reach_both_ends():
    for case in R.SN_PW_CASES:
        if case[5]:
            se = R.sn_pw_inputs(case)["se"]
            assert float((se[1:] - se[:-1]).abs().max(1).values.min()) > 0.3, case
    for case in R.SN_SE_CASES:
        v, _ = R.sn_se_ref(R.sn_se_inputs(case), case)
        assert bool((v == 0).any()) and bool((v == 1).any()) and bool(((v > 0) & (v < 1)).any()), case


def test_maxpool_border_windows_are_all_negative():
    for case in R.MAXPOOL_CASES:
        assert R.maxpool_border_windows_all_negative(R.maxpool_inputs(case), case), case


def test_head_inputs():
    for case in R.SN_HEAD_CASES:
        I = R.sn_head_inputs(case)
        B, FD, NC, use_hw = case
        if NC >= B:
            assert len({tuple(r) for r in I["one_hot"].tolist()}) == B
        if not use_hw:
            assert bool((I["roi_wh"] == 1e6).all()) and bool((I["w3"][:, FD + NC:] != 0).all())


def test_group_tables_stay_inside_x():
    q = R.DWG_HW * R.DWG_HW // 4
    for t in R.DWG_TABLES + [R.DWG_CLAMP_TABLE]:
        g = torch.minimum(torch.tensor(t).clamp_min(0), torch.arange(R.DWG_B))
        last = 4 * g * q + (torch.arange(R.DWG_B) - g) * q + q - 1            # the last pixel each crop's rows read, unwrapped
        assert int(last.max()) < 4 * R.DWG_B * q
    assert torch.equal(R.dwg_source_pixels(R.DWG_CLAMP_TABLE, R.DWG_B, q), R.dwg_source_pixels(R.DWG_CLAMPED, R.DWG_B, q))


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("name,mut", [(n, m) for n, m, _ in R.MUTATIONS], ids=[f"{n}-{m}" for n, m, _ in R.MUTATIONS])
def test_mutation_is_rejected(name, mut):
    op = R.OPS[name]
    exposing = [f for n, m, f in R.MUTATIONS if (n, m) == (name, mut)][0]
    cases = [c for c in op.cases if exposing(c)]
    assert cases, "no input set exposes this mutation"
    for case in cases:
        I = op.inputs(case)
        v, bound = op.ref(I, case)
        wrong, _ = op.ref(I, case, mut=mut)
        buf = wrong.reshape(-1) if wrong.numel() > v.numel() else R.with_tail(wrong)
        ratio, msg = R.check_buffer(buf, v, bound, f"{name} {mut} {R.case_id(case)}")
        assert msg is not None, f"{name} {R.case_id(case)}: mutation {mut} passes the checker (ratio {ratio:.3g})"


# ------------------------------------------------------------------------------------------------ head entry and exit kernels
def _forms(name):
    if name == "gp_convnext_stem":
        return {R.stem_form(c) for c in R.STEM_CASES}, R.STEM_FORMS
    if name == "gp_deconv_col2im":
        return {R.col2im_form(c) for c in R.COL2IM_CASES}, R.COL2IM_FORMS
    if name == "gp_xyz_out_layer":
        return {R.xyz_out_geometry(c)[0] for c in R.XYZ_OUT_CASES}, {"xyz_out<f16>", "xyz_out<f32>"}
    if name == "gp_pointwise_k3":
        return {R.pk3_geometry(c)[0] for c in R.PK3_CASES}, {"pointwise_k3<half>", "pointwise_k3<float>"}
    if name in R.SMALLCIN_CIN:
        return {R.smallcin_form(name, c) for c in R.SMALLCIN_CASES}, R.SMALLCIN_FORMS[name]
    if name == "gp_pool_mmm":
        return {R.pool_geometry(c)[0] for c in R.POOL_CASES}, {"pool_mmm<half>", "pool_mmm<float>"}
    if name == "gp_size_head":
        return {R.size_geometry(c)[0] for c in R.SIZE_CASES}, {"size_pool<f16>", "size_pool<f32>"}
    if name == "gp_attention64":
        return {R.att_form(c) for c in R.ATT_CASES_32}, {"attention64<half,32>", "attention64<float,32>"}
    if name == "gp_attention64_hd":
        return {R.att_form(c) for c in R.ATT_CASES_HD}, {f"attention64<{t},{hd}>" for t in ("half", "float") for hd in (24, 32)}
    if name == "gp_pose_tail_rt":
        return {R.pose_form(c) for c in R.POSE_CASES}, {"pose_tail<4>", "pose_tail<6>"}
    if name == "gp_groupnorm_apply_xyz":
        return {R.gnxyz_form(c) for c in R.GNXYZ_CASES}, R.GNXYZ_FORMS
    raise KeyError(name)


@pytest.mark.parametrize("name", R.HEAD_OPS)
def test_every_instantiation_is_taken_by_some_case(name):
    taken, listed = _forms(name)
    assert taken == listed, (sorted(listed - taken), sorted(taken - listed))
    assert sum(1 for n, _, _ in R.MUTATIONS if n == name) >= 2


def test_stem_cases():
    geo = {c: R.stem_geometry(c) for c in R.STEM_CASES}
    B, H, W = R.STEM_LARGE[:3]
    form, pxb, rpw = geo[R.STEM_LARGE]
    factors = (B, H // 4 // rpw, W // 4 // pxb)
    assert form == "stem_mfma<4>" and factors[0] * factors[1] * factors[2] == 256 and min(factors) > 1      # the threshold itself, every factor of the block index above 1
    assert [c for c in R.STEM_CASES if c[0] * c[1] * c[2] // 16 * R.STEM_C0 > 600_000] == [R.STEM_LARGE]     # the one LARGE case
    assert any(c[4] == 0.25 for c in R.STEM_CASES)
    assert {c[2] // 4 // geo[c][1] for c in R.STEM_CASES} >= {1, 2, 3, 4}                                   # column blocks per row
    m = R.stem_inputs(R.STEM_CASES[0])["img"].mean((0, 2, 3))
    assert float(m.abs().min()) > 1.4 and bool((m > 0).any()) and bool((m < 0).any())


def test_col2im_summand_counts():
    for case in R.COL2IM_CASES:
        B, H, W = case[:3]
        assert R.col2im_summand_counts(case) == {1: (H + 1) * (W + 1), 2: (H + 1) * (W - 1) + (H - 1) * (W + 1), 4: (H - 1) * (W - 1)}, case
    assert any(c[1] != c[2] for c in R.COL2IM_CASES)


def test_xyz_out_and_pointwise_cases_have_their_tails():
    geo = [R.xyz_out_geometry(c) for c in R.XYZ_OUT_CASES]
    assert all(g[4] != 0 for g in geo)                                        # a row tail in every form
    assert any(g[1] == 1 and g[2] == 64 for g in geo) and any(1 < g[1] < 64 for g in geo)      # several pixels per wave
    assert any(g[3] == 2 for g in geo) and all(c[0] > 1 and c[1] != c[0] * c[1] for c in R.XYZ_OUT_CASES)
    for Cout, dt in {(c[1], c[2]) for c in R.PK3_CASES}:
        geos = [R.pk3_geometry(c) for c in R.PK3_CASES if (c[1], c[2]) == (Cout, dt)]
        pg = geos[0][1]
        assert sorted((g[2], g[3]) for g in geos) == [(1, 1), (1, 8 * pg - 1), (2, 1)], (Cout, dt)      # below, one short of and one past a workgroup
    assert {c[1] for c in R.PK3_CASES if c[2] == torch.float32} == {4, 256, 1024}


def test_smallcin_cases_reach_both_edges_and_the_mask_is_soft():
    B, Rr, Cout, _ = R.SMALLCIN_CASES[0]
    assert Rr // 2 == 4 and (B * (Rr // 2)) % (256 // (Cout // 4)) != 0         # one pixel quad spans a row; the last block is not full
    for name in R.SMALLCIN_CIN:
        for case in R.SMALLCIN_CASES:
            I = R.smallcin_inputs(name, case)
            m = I["mask"]
            assert bool((m == 0).any()) and bool(((m > 0) & (m < 1)).any()) and not bool((m >= 1).any())
            assert bool((I["xyz4"][:, 3] == 7.0).all())
    # the masked operand is rounded once to fp32: the float64 reference starts from those values
    case = R.SMALLCIN_CASES[1]
    I = R.smallcin_inputs("gp_pnp_conv1_masked", case)
    x64 = R._smallcin_x(I, "gp_pnp_conv1_masked", case, R.F64)
    assert torch.equal(x64, x64.float().double()) and bool((x64 == 0).any())


def test_pool_and_size_inputs():
    empty = set()
    for case in R.POOL_CASES:
        x = R.pool_inputs(case)["x"]
        assert bool((x[..., 0] < 0).all()) and bool((x[..., 1] > 0).all()), case
        empty.add(R.pool_geometry(case)[2] > 0)
    assert empty == {True, False}                                              # pixel groups that see no pixel, and full ones
    geo = [R.size_geometry(c) for c in R.SIZE_CASES]
    assert any(g[1] == 2 and g[2] == 1 for g in geo) and any(g[3] > 0 for g in geo)
    for case in R.SIZE_CASES:
        I = R.size_inputs(case)
        assert bool((I["feat"][..., ::5] < 0).all())
        n = I["mean_size"].norm(dim=1)
        assert float(n.max() / n.min()) > 2


def test_attention_rows_are_peaked_and_flat():
    for case in R.ATT_CASES_HD:
        lead, flat = R.att_row_kinds(R.att_inputs(case), case)
        assert lead >= R.ATT_PEAK and flat < 0.1, (case, lead, flat)


def test_groupnorm_apply_xyz_inputs():
    for case in R.GNXYZ_CASES:
        assert R.gnxyz_mean_over_std(R.gnxyz_inputs(case), case) > 18, case
    assert {c[1] // R.GNXYZ_ROWS for c in R.GNXYZ_CASES} == {1, 25}


def test_pose_reference_is_well_conditioned():
    """Every normalised vector has a norm of at least 0.1 of the logits' scale; every ray is at least 1e-2 rad off the optical axis, but the
    one crop that lies exactly on it (the angle == 0 branch); per-crop intrinsics differ."""
    kinds = set()
    for case in R.POSE_CASES:
        I = R.pose_inputs(case)
        o = R.pose_fc(I, case, R.F64)[0]
        _, (cond, angle) = R.pose_decode(o, I, case)
        scale = float(o[:, :case[1]].pow(2).mean().sqrt())
        assert all(float(n.min()) >= 0.1 * scale for n in cond), case
        assert float(angle[R.POSE_ON_AXIS]) == 0.0, case
        off = torch.cat([angle[:R.POSE_ON_AXIS], angle[R.POSE_ON_AXIS + 1:]])
        assert float(off.min()) >= 1e-2, (case, float(off.min()))
        assert bool((o[:, case[1] + 2] > 0).all())                             # depth in front of the camera
        fx = I["cam_K"][:, 0]
        assert len(set(fx.tolist())) == R.POSE_B
        kinds.add(case[:5])
    assert len(kinds) == 5 * 2 * 2 * 2 and {c[5] for c in R.POSE_CASES} == {256, 260} and R.POSE_GOLDEN_CALL in R.POSE_CASES


@pytest.mark.parametrize("mut", [m for m, _ in R.POSE_DECODE_MUTATIONS])
def test_pose_decode_mutation_is_rejected(mut):
    """The decode is held to YARDSTICK x the float32 evaluation's own figure per tensor (floor 2^-24): the float32 evaluation passes it by
    definition, each mutant must miss it on every case it bears on."""
    exposing = dict(R.POSE_DECODE_MUTATIONS)[mut]
    cases = [c for c in R.POSE_CASES if exposing(c)]
    assert cases
    for case in cases:
        I = R.pose_inputs(case)
        want, ref32 = R.pose_decode_refs(I, case)
        wrong, _ = R.pose_decode_refs(I, case, mut)
        fig = R.yardstick_figures(wrong, want, ref32)
        assert any(dev > R.YARDSTICK * cpu for dev, cpu in fig.values()), (mut, case, fig)


def test_pose_decode_float32_figures():
    worst = {}
    for case in R.POSE_CASES:
        want, ref32 = R.pose_decode_refs(R.pose_inputs(case), case)
        for k, (dev, cpu) in R.yardstick_figures(ref32, want, ref32).items():
            worst[k] = max(worst.get(k, 0.0), cpu)
    print("CPU float32 decode figures " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v < 1e-5 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------ closure
H = "tests/test_hip_ops.py::"
S = "tests/test_scalenet_ops_gpu.py::"
M = "tests/test_misc_ops_conformance.py::"
E = "tests/test_evalmap_gpu.py::test_kernels_against_reference_fixtures"
NC = "tests/test_norm_conformance_gpu.py::"
A = "tests/test_att_pnp_gpu.py::"
DC = "tests/test_dcnv3_conformance_gpu.py::"
HC = "tests/test_head_ops_conformance_gpu.py::"
# entry point -> the operator-level test that holds it against a reference of its own operation (never a whole-network test); graph,
# timing, version and device-info calls -> the test that exercises them
CLOSURE = {
    "gp_version": "tests/test_abi.py::test_ctypes_prototypes_cover_header",
    "gp_device_info": M + "test_device_info",
    "gp_dcnv3_forward": DC + "test_dcnv3_forward",
    "gp_dcnv3_forward_any": DC + "test_dcnv3_forward",
    "gp_dcnv3_backward": "tests/test_hip_dcnv3_any.py::test_backward_stride2_quarter_buffer_and_autograd_function",
    "gp_gemm": "tests/test_gemm_conformance.py::test_gemm_conformance",
    "gp_gemm_gn_rows": H + "test_gemm_small_m_latency_variant",
    "gp_split_planes": "tests/test_split_gemm.py::test_split_planes_reconstruct",
    "gp_convnext_mlp_pack_w2": "tests/test_mlp_conformance_gpu.py::test_pack_w2_bit_exact",
    "gp_convnext_mlp_pack_w2_s32": "tests/test_mlp_conformance_gpu.py::test_pack_w2_bit_exact",
    "gp_convnext_mlp": "tests/test_mlp_conformance_gpu.py::test_mlp_conformance",
    "gp_convnext_stem": HC + "test_convnext_stem",
    "gp_dwconv_ln": NC + "test_dwconv_ln",
    "gp_dwconv_ln_groups": M + "test_dwconv_ln_groups",
    "gp_dwconv7_raw_stats": NC + "test_dwconv7_raw_stats",
    "gp_layernorm": NC + "test_layernorm",
    "gp_groupnorm_chunks": NC + "test_groupnorm",
    "gp_groupnorm_stats": NC + "test_groupnorm",
    "gp_groupnorm_apply": NC + "test_groupnorm",
    "gp_groupnorm_upsample2x": NC + "test_groupnorm_upsample2x",
    "gp_groupnorm_apply_xyz": HC + "test_groupnorm_apply_xyz",
    "gp_upsample_bilinear2x": NC + "test_upsample_bilinear2x",
    "gp_deconv_col2im": HC + "test_deconv_col2im",
    "gp_xyz_out_layer": HC + "test_xyz_out_layer",
    "gp_pointwise_k3": HC + "test_pointwise_k3",
    "gp_dcnv3_xyz_project": "tests/test_enc0_xyz.py::test_entry_point_against_float64_reference",
    "gp_pnp_conv1": HC + "test_smallcin_conv",
    "gp_pnp_conv1_masked": HC + "test_smallcin_conv",
    "gp_pool_mmm": HC + "test_pool_mmm",
    "gp_xyz_conv3x3_s2": HC + "test_smallcin_conv",
    "gp_size_head": HC + "test_size_head",
    "gp_pose_tail": HC + "test_pose_tail",
    "gp_pose_tail_rt": HC + "test_pose_tail_rt",
    "gp_patchify_xyz": M + "test_patchify_xyz",
    "gp_attention64": HC + "test_attention64",
    "gp_attention64_hd": HC + "test_attention64_hd",
    "gp_patchify_pnp": A + "test_patchify_pnp_bitwise",
    "gp_resnet_stem": M + "test_resnet_stem",
    "gp_maxpool3x3s2": M + "test_maxpool3x3s2",
    "gp_mask_resize_nearest": H + "test_mask_resize_bit_exact",
    "gp_crop_rois": "tests/test_preprocess.py::test_crop_rois_hip_bit_exact",
    "gp_pred_rt": "tests/test_preprocess.py::test_pred_rt_hip_vs_oracle",
    "gp_pack_poses": M + "test_pack_poses",
    "gp_graph_begin": M + "test_graph_capture_and_replay",
    "gp_graph_end": M + "test_graph_capture_and_replay",
    "gp_graph_launch": M + "test_graph_capture_and_replay",
    "gp_graph_destroy": M + "test_graph_capture_and_replay",
    "gp_sn_stem": S + "test_sn_stem",
    "gp_sn_pointwise": S + "test_sn_pointwise",
    "gp_sn_depthwise": S + "test_sn_depthwise",
    "gp_sn_avgpool": S + "test_sn_avgpool",
    "gp_sn_se": S + "test_sn_se",
    "gp_sn_head": S + "test_sn_head",
    "gp_eval_normalise": E,
    "gp_eval_pair_overlaps": E,
    "gp_eval_match": E,
    "gp_eval_ap": E,
    "gp_timing_begin": M + "test_timing_report_and_top",
    "gp_timing_end": M + "test_timing_report_and_top",
    "gp_timing_report": M + "test_timing_report_and_top",
    "gp_timing_top": M + "test_timing_report_and_top",
}
# whole-network suites: no table entry may point into them
WHOLE_NETWORK = ("test_hip_posenet.py", "test_ragged_frames.py", "test_grouped_launch.py", "test_scale_net.py", "test_pipeline_gpu.py",
                 "test_runner_h2d.py", "test_multirank_gpu.py", "test_hip_modules.py", "test_bench_spawn.py")


def _header_entry_points():
    with open(os.path.join(ROOT, "include", "givepose_hip.h")) as f:
        return set(re.findall(r"^int (gp_\w+)\(", f.read(), re.M))


def _wrappers():
    """entry point -> public names of the package that call it: the function, and for a method its class (ops.maxpool3x3s2,
    preprocess.RoiCropper.__call__ -> RoiCropper, evalmap.MapAccumulator.compute -> compute, MapAccumulator)."""
    out = {}
    pkg = os.path.join(ROOT, "givepose_amd")
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py"):
            continue
        with open(os.path.join(pkg, fn)) as f:
            src = f.read()

        def visit(node, owners):
            for ch in ast.iter_child_nodes(node):
                if isinstance(ch, (ast.FunctionDef, ast.ClassDef)):
                    names = owners + [ch.name]
                    if isinstance(ch, ast.FunctionDef):
                        for ep in set(re.findall(r"\bgp_\w+", ast.get_source_segment(src, ch) or "")):
                            out.setdefault(ep, set()).update(n for n in names if not n.startswith("_"))
                    visit(ch, names)
        visit(ast.parse(src), [])
    return out


def test_closure_table_equals_the_header():
    hdr = _header_entry_points()
    assert len(hdr) > 50
    assert set(CLOSURE) == hdr, (sorted(hdr - set(CLOSURE)), sorted(set(CLOSURE) - hdr))


def test_closure_entries_name_existing_operator_tests():
    wrappers = _wrappers()
    parsed = {}
    for ep, target in CLOSURE.items():
        path, func = target.split("::")
        assert os.path.basename(path) not in WHOLE_NETWORK, (ep, target)
        if path not in parsed:
            with open(os.path.join(ROOT, path)) as f:
                src = f.read()
            parsed[path] = (src, {n.name for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)})
        src, funcs = parsed[path]
        assert func.startswith("test_") and func in funcs, (ep, target)
        mentioned = re.search(rf"\b{ep}\b", src) or any(re.search(rf"\b{w}\b", src) for w in wrappers.get(ep, ()))
        assert mentioned, f"{path} mentions neither {ep} nor one of its wrappers {sorted(wrappers.get(ep, ()))}"
