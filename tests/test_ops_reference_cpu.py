"""The checker of tests/ops_reference.py on the CPU, before a kernel is held against it.

  self-consistency   every operation evaluated in torch float32 stays within HALF its bound on every input set the GPU tests use (the
                     other half is room for the kernel's summation order, which the bound covers on paper); with an fp16 store, whose
                     correct rounding alone may use all of e_out, half the bound in front of the store and the whole bound behind it
  sensitivity        deliberately wrong float64 implementations (ops_reference.MUTATIONS) are rejected on those same input sets
  closure            every `int gp_*(` of include/givepose_hip.h is mapped to the operator-level test that covers it
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


# ------------------------------------------------------------------------------------------------ closure
H = "tests/test_hip_ops.py::"
S = "tests/test_scalenet_ops_gpu.py::"
M = "tests/test_misc_ops_conformance.py::"
E = "tests/test_evalmap_gpu.py::test_kernels_against_reference_fixtures"
P = "tests/test_pnp_flags_gpu.py::"
NC = "tests/test_norm_conformance_gpu.py::"
A = "tests/test_att_pnp_gpu.py::"
DC = "tests/test_dcnv3_conformance_gpu.py::"
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
    "gp_convnext_stem": H + "test_stem",
    "gp_dwconv_ln": NC + "test_dwconv_ln",
    "gp_dwconv_ln_groups": M + "test_dwconv_ln_groups",
    "gp_dwconv7_raw_stats": NC + "test_dwconv7_raw_stats",
    "gp_layernorm": NC + "test_layernorm",
    "gp_groupnorm_chunks": NC + "test_groupnorm",
    "gp_groupnorm_stats": NC + "test_groupnorm",
    "gp_groupnorm_apply": NC + "test_groupnorm",
    "gp_groupnorm_upsample2x": NC + "test_groupnorm_upsample2x",
    "gp_groupnorm_apply_xyz": H + "test_groupnorm_apply_xyz",
    "gp_upsample_bilinear2x": NC + "test_upsample_bilinear2x",
    "gp_deconv_col2im": H + "test_upsample_and_col2im",
    "gp_xyz_out_layer": H + "test_xyz_out_pointwise_smallcin",
    "gp_pointwise_k3": H + "test_xyz_out_pointwise_smallcin",
    "gp_dcnv3_xyz_project": "tests/test_enc0_xyz.py::test_entry_point_against_float64_reference",
    "gp_pnp_conv1": H + "test_xyz_out_pointwise_smallcin",
    "gp_pnp_conv1_masked": P + "test_pnp_conv1_masked_bitwise",
    "gp_pool_mmm": P + "test_pool_mmm",
    "gp_xyz_conv3x3_s2": H + "test_xyz_out_pointwise_smallcin",
    "gp_size_head": H + "test_size_head_golden",
    "gp_pose_tail": H + "test_pose_tail_golden",
    "gp_pose_tail_rt": P + "test_pose_tail_rt_golden",
    "gp_patchify_xyz": M + "test_patchify_xyz",
    "gp_attention64": A + "test_attention64_hd32_is_attention64",
    "gp_attention64_hd": A + "test_attention64_hd24",
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
