"""GPU: the kernels at the network's entry and exits on their own, through givepose_amd.ops, against the float64 references and per-element
bounds of tests/ops_reference.py -- gp_convnext_stem, gp_deconv_col2im, gp_xyz_out_layer, gp_pointwise_k3, gp_xyz_conv3x3_s2 / gp_pnp_conv1 /
gp_pnp_conv1_masked, gp_pool_mmm, gp_size_head, gp_attention64 / gp_attention64_hd, gp_pose_tail / gp_pose_tail_rt (csrc/misc.hip) and
gp_groupnorm_apply_xyz (csrc/norm.hip).  They produce nocs_coor, ivfc_coor, size, rot, trans and the trunk's first layer; the older tests of
test_hip_ops.py, test_pnp_flags_gpu.py and test_att_pnp_gpu.py run one shape each against one relative-error figure.

Every case: each output buffer is NaN with one more row of sentinels behind it; every element within its bound (the worst ratio and its
index are printed on failure) and the sentinels intact; a second launch gives the same bits.  Inputs, cases and bounds are the ones
tests/test_ops_reference_cpu.py has checked on the CPU.  The pose tail's decode (rot_allo, rot_ego, trans) is ill-conditioned by nature and
has no static bound: per tensor max |got - float64| / max |float64| is held to 8 x the same figure of the float32 evaluation (floor 2^-24).
The largest ratios of an MI355X run: profiles/op_conformance.txt.

No environment variable is set here; the forms behind an A/B variable that the library reads once per process are skipped when it is set."""
import os

import pytest
import torch

import ops_reference as R

pytestmark = pytest.mark.gpu


def ops():
    from givepose_amd import ops as o
    return o


def _dev(I):
    return {k: v.cuda().contiguous() for k, v in I.items()}


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _buffer(n, row, dtype):
    buf = torch.full((n + row,), R.NAN, dtype=dtype, device="cuda")
    buf[n:] = R.SENTINEL
    return buf


def _default_routing(names):
    if any(k in os.environ for k in names):
        pytest.skip(f"one of {names} is set: the routing restated in tests/ops_reference.py is the default one")


def run_case(what, parts, launch, dtype=torch.float32):
    """parts: [(v, bound, row length)] or [(n values, None, row length)] for an output that is only checked for its sentinels and for equal
    bits; launch(*front views of the buffers) writes them.  Returns the first launch's buffers (with their tails)."""
    runs = []
    for _ in range(2):
        bufs = [_buffer(v if isinstance(v, int) else v.numel(), row, dtype) for v, _, row in parts]
        launch(*[b[:b.numel() - row] for b, (_, _, row) in zip(bufs, parts)])
        torch.cuda.synchronize()
        runs.append(bufs)
    worst = 0.0
    for i, (v, bound, row) in enumerate(parts):
        buf = runs[0][i]
        if isinstance(v, int):
            tail = buf[v:].cpu()
            assert bool((tail == R.SENTINEL).all()) and bool(torch.isfinite(buf[:v]).all()), f"{what} output {i}: sentinel overwritten or a value not written"
        else:
            ratio, msg = R.check_buffer(buf, v, bound, f"{what} output {i}")
            assert msg is None, msg
            worst = max(worst, ratio)
        assert torch.equal(_bits(buf), _bits(runs[1][i])), f"{what} output {i}: a second launch gives other bits"
    print(f"GPU_RATIO {what} {worst:.4f}")
    return runs[0]


# ------------------------------------------------------------------------------------------------ gp_convnext_stem
@pytest.mark.parametrize("case", R.STEM_CASES, ids=R.case_id)
def test_convnext_stem(case):
    """conv 4x4 s4 + LayerNorm, every form: the MFMA forms split image and taps into fp16 hi + lo and must stay an fp32-accurate
    convolution (the bound has nothing of order 2^-11 |x||w|)."""
    _default_routing(R.STEM_ENV)
    o = ops()
    B, H, W, dt, eps = case
    I = R.stem_inputs(case)
    v, bound = R.stem_ref(I, case)
    D = _dev(I)
    run_case(f"gp_convnext_stem {R.case_id(case)} {R.stem_form(case)}", [(v, bound, R.STEM_C0)],
             lambda y: o.convnext_stem(D["img"], D["w"], D["b"], D["ln_w"], D["ln_b"], y.view(B, H // 4, W // 4, R.STEM_C0), eps), dt)


# ------------------------------------------------------------------------------------------------ gp_deconv_col2im
@pytest.mark.parametrize("case", R.COL2IM_CASES, ids=R.case_id)
def test_deconv_col2im(case):
    o = ops()
    B, H, W, C, odt, cdt = case
    I = R.col2im_inputs(case)
    v, bound = R.col2im_ref(I, case)
    cols = I["cols"].cuda()
    run_case(f"gp_deconv_col2im {R.case_id(case)}", [(v, bound, C)], lambda y: o.deconv_col2im(cols, y.view(B, 2 * H, 2 * W, C), B, H, W, C), odt)


# ------------------------------------------------------------------------------------------------ gp_xyz_out_layer
def _two_maps(v, bound, B, HW):
    n = B * 3 * HW
    return [(v[:n], bound[:n], HW), (v[n:], bound[n:], 4)]


def _same_maps(bufs, B, HW):
    nchw, nhwc4 = bufs[0][:B * 3 * HW].view(B, 3, HW), bufs[1][:B * HW * 4].view(B, HW, 4)
    assert torch.equal(_bits(nhwc4[..., :3].permute(0, 2, 1).contiguous()), _bits(nchw)) and bool((nhwc4[..., 3] == 0).all())


@pytest.mark.parametrize("case", R.XYZ_OUT_CASES, ids=R.case_id)
def test_xyz_out_layer(case):
    """Both maps, the NCHW one and the (rows, 4) one whose 4th column is exactly 0, with a row tail in every form."""
    o = ops()
    B, HW, C, dts = case
    I = R.xyz_out_inputs(case)
    v, bound = R.xyz_out_ref(I, case)
    D = _dev(I)
    bufs = run_case(f"gp_xyz_out_layer {R.case_id(case)}", _two_maps(v, bound, B, HW),
                    lambda nchw, nhwc4: o.xyz_out_layer(D["x"], D["w"], D["b"], nchw.view(B, 3, HW), nhwc4.view(B * HW, 4)))
    _same_maps(bufs, B, HW)


# ------------------------------------------------------------------------------------------------ gp_pointwise_k3
@pytest.mark.parametrize("case", R.PK3_CASES, ids=R.case_id)
def test_pointwise_k3(case):
    o = ops()
    rows, Cout, dt = case
    I = R.pk3_inputs(case)
    v, bound = R.pk3_ref(I, case)
    D = _dev(I)
    run_case(f"gp_pointwise_k3 {R.case_id(case)}", [(v, bound, Cout)], lambda y: o.pointwise_k3(D["xyz4"], D["w"], D["b"], y.view(rows, Cout)), dt)


# ------------------------------------------------------------------------------------------------ tiny-Cin 3x3 s2 convolutions
@pytest.mark.parametrize("case", R.SMALLCIN_CASES, ids=R.case_id)
@pytest.mark.parametrize("name", list(R.SMALLCIN_CIN))
def test_smallcin_conv(name, case):
    """gp_xyz_conv3x3_s2, gp_pnp_conv1 and gp_pnp_conv1_masked (a soft mask with exact zeros, against float64 conv(x * m)) in the VALU form and,
    at fp16 R = 64, the hi / lo-split MFMA form."""
    _default_routing(R.SMALLCIN_ENV)
    o = ops()
    B, Rr, Cout, dt = case
    I = R.smallcin_inputs(name, case)
    v, bound = R.smallcin_ref(name, I, case)
    D = _dev(I)

    def launch(y):
        y = y.view(B, Rr // 2, Rr // 2, Cout)
        if name == "gp_xyz_conv3x3_s2":
            o.xyz_conv3x3_s2(D["xyz4"], D["w"], y, B, Rr)
        elif name == "gp_pnp_conv1":
            o.pnp_conv1(D["xyz4"], D["coord2d"], D["w"], y, B, Rr)
        else:
            o.pnp_conv1_masked(D["xyz4"], D["coord2d"], D["mask"], D["w"], y, B, Rr)

    run_case(f"{name} {R.case_id(case)} {R.smallcin_form(name, case)}", [(v, bound, Cout)], launch, dt)


# ------------------------------------------------------------------------------------------------ gp_pool_mmm
@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
def test_pool_mmm(case):
    """[mean | max | min][:k]: maximum and minimum are the operand's bits (bound 0), also where a pixel group of the workgroup sees no pixel
    and where a channel is negative (positive) everywhere."""
    o = ops()
    k, C, HW, dt = case
    I = R.pool_inputs(case)
    v, bound = R.pool_ref(I, case)
    x = I["x"].cuda()
    run_case(f"gp_pool_mmm {R.case_id(case)}", [(v, bound, k * C)], lambda y: o.pool_mmm(x, y.view(R.POOL_B, k * C), k), dt)


# ------------------------------------------------------------------------------------------------ gp_size_head
@pytest.mark.parametrize("case", R.SIZE_CASES, ids=R.case_id)
def test_size_head(case):
    o = ops()
    B, HW, C, Fh, dts = case
    I = R.size_inputs(case)
    v, bound = R.size_ref(I, case)
    D = _dev(I)
    scratch = torch.full((B * (Fh + C),), R.NAN, device="cuda")
    run_case(f"gp_size_head {R.case_id(case)}", [(v, bound, 3)],
             lambda y: o.size_head(D["feat"], D["w1"], D["b1"], D["w2"], D["b2"], D["mean_size"], y.view(B, 3), scratch))


# ------------------------------------------------------------------------------------------------ gp_attention64 / gp_attention64_hd
def _attention(case, call):
    B, heads, HD, dt = case
    I = R.att_inputs(case)
    lead, flat = R.att_row_kinds(I, case)
    assert lead >= R.ATT_PEAK and flat < 0.1
    v, bound = R.att_ref(I, case)
    qkv = I["qkv"].cuda()
    return run_case(f"{call} {R.case_id(case)}", [(v, bound, heads * HD)],
                    lambda y: (ops().attention64(qkv, y.view(B, 64, heads * HD), B, heads) if call == "gp_attention64" else
                               ops().attention64_hd(qkv, y.view(B, 64, heads * HD), B, heads, HD)), dt)[0]


@pytest.mark.parametrize("case", R.ATT_CASES_32, ids=R.case_id)
def test_attention64(case):
    """Half of the query rows have one score 20 above the rest, the others a flat distribution."""
    _attention(case, "gp_attention64")


@pytest.mark.parametrize("case", R.ATT_CASES_HD, ids=R.case_id)
def test_attention64_hd(case):
    got = _attention(case, "gp_attention64_hd")
    if case[2] == 32:           # head_dim 32 forwards to gp_attention64
        assert torch.equal(_bits(got), _bits(_attention(case, "gp_attention64")))


# ------------------------------------------------------------------------------------------------ gp_pose_tail / gp_pose_tail_rt
POSE_OUT = (("pred_t", 3), ("rot_allo", 9), ("rot_ego", 9), ("trans", 3))


def _pose_tail(case, rt):
    o = ops()
    kind, RD, is_allo, site, wild, ldh = case
    B = R.POSE_B
    I = R.pose_inputs(case)
    v, bound = R.pose_ref(I, case)
    want, ref32 = R.pose_decode_refs(I, case)
    D = _dev(I)
    W = {"fc_r.w": D["w_r"], "fc_r.b": D["b_r"], "fc_t.w": D["w_t"], "fc_t.b": D["b_t"], "fc_z.w": D["w_z"], "fc_z.b": D["b_z"]}
    first = "pred_rot" if rt else "rot6d"

    def launch(pr, pt, ra, re, tr):
        outs = {first: pr, "pred_t": pt, "rot_allo": ra, "rot_ego": re, "trans": tr}
        if rt:
            o.pose_tail_rt(D["h"], D["hz"], ldh, W, D["cam_K"], D["bbox_center"], D["resize_ratio"], D["roi_wh"], wild, site, RD, kind, is_allo, outs, B)
        else:
            o.pose_tail(D["h"], D["hz"], ldh, W, D["cam_K"], D["bbox_center"], D["resize_ratio"], D["roi_wh"], wild, site, outs, B)

    what = f"{'gp_pose_tail_rt' if rt else 'gp_pose_tail'} {R.ROT_NAMES[kind]}-{R.case_id(case[2:])}"
    parts = [(v[:, :RD].contiguous(), bound[:, :RD].contiguous(), RD), (v[:, RD:].contiguous(), bound[:, RD:].contiguous(), 3), (B * 9, None, 9), (B * 9, None, 9),
             (B * 3, None, 3)]
    bufs = run_case(what, parts, launch)
    got = {k: bufs[i + 1][:B * n].view(B, n) for i, (k, n) in enumerate(POSE_OUT)}
    worst = 0.0
    for k, (dev, cpu) in R.yardstick_figures(got, want, ref32).items():
        print(f"{what} {k}: device {dev:.2e}, CPU float32 {cpu:.2e}, ratio {dev / cpu:.2f}")
        assert dev <= R.YARDSTICK * cpu, (what, k, dev, cpu)
        worst = max(worst, dev / cpu)
    print(f"GPU_RATIO {what} decode-vs-float32 {worst:.4f}")
    assert torch.equal(_bits(got["rot_ego"][R.POSE_ON_AXIS]), _bits(got["rot_allo"][R.POSE_ON_AXIS]))      # the crop on the optical axis: angle == 0
    return bufs


@pytest.mark.parametrize("case", R.POSE_CASES, ids=lambda c: f"{R.ROT_NAMES[c[0]]}-{R.case_id(c[2:])}")
def test_pose_tail_rt(case):
    """Dense fc weights (256-term dot products with the (n + 2) u a bound), every rot_kind x is_allo x site x wild6d, ldh 256 and 260,
    per-crop intrinsics (wild6d scales by crop 0's fx) and one crop exactly on the optical axis."""
    _pose_tail(case, True)


@pytest.mark.parametrize("case", [c for c in R.POSE_CASES if c[0] == R.ROT_6D and c[2] == 1], ids=lambda c: R.case_id(c[3:]))
def test_pose_tail(case):
    """gp_pose_tail is gp_pose_tail_rt's (6, GP_ROT_6D, is_allo 1) call: the same checks, and the same bits."""
    a, b = _pose_tail(case, False), _pose_tail(case, True)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


# ------------------------------------------------------------------------------------------------ gp_groupnorm_apply_xyz
@pytest.mark.parametrize("case", R.GNXYZ_CASES, ids=R.case_id)
def test_groupnorm_apply_xyz(case):
    """GroupNorm (statistics from the caller's 64-row partial sums, one group at |mean| = 20 std) + GELU + the 1x1 layer to 3 outputs: the two
    MFMA forms (fp32-accurate and packed fp16), the VALU form in both types.  The two maps hold the same bits, the 4th column 0."""
    _default_routing(R.GNXYZ_ENV)
    o = ops()
    from givepose_amd._lib import ACT_GELU
    B, HW, C, dts, p16 = case
    I = R.gnxyz_inputs(case)
    v, bound = R.gnxyz_ref(I, case)
    D = _dev(I)
    bufs = run_case(f"gp_groupnorm_apply_xyz {R.case_id(case)} {R.gnxyz_form(case)}", _two_maps(v, bound, B, HW),
                    lambda nchw, nhwc4: o.groupnorm_apply_xyz(D["x"], D["gn_w"], D["gn_b"], D["out_w"], D["out_b"], nchw.view(B, 3, HW), nhwc4.view(B * HW, 4),
                                                              R.GNXYZ_G, ACT_GELU, D["partial"], eps=R.GNXYZ_EPS, rows=R.GNXYZ_ROWS, packed16=bool(p16)))
    _same_maps(bufs, B, HW)
