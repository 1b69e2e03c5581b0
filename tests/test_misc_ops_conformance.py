"""GPU: gp_resnet_stem, gp_maxpool3x3s2, gp_patchify_xyz (csrc/misc.hip) and gp_dwconv_ln_groups (csrc/norm.hip) on their own, through
givepose_amd.ops, against the float64 references and per-element bounds of tests/ops_reference.py -- the network tests reach them only
in front of a 34-layer trunk or inside a whole PoseNet.  Max-pool and patchify are exact: the reference's bits.

Every case: the output buffer is NaN with one more row of sentinels behind it; every element within its bound (the worst ratio and its
index are printed on failure) and the sentinels intact; a second launch gives the same bits.  Inputs, cases and bounds are the ones
tests/test_ops_reference_cpu.py has checked on the CPU.  The largest ratios of an MI355X run: profiles/op_conformance.txt.

At the end: the entry points that carry no arithmetic of their own and that no other operator-level test calls -- gp_pack_poses,
gp_device_info, the gp_timing_* report and hipGraph capture / replay of one launch (gp_graph_*)."""
import ctypes

import pytest
import torch

import ops_reference as R

pytestmark = pytest.mark.gpu


def ops():
    from givepose_amd import ops as o
    return o


def _err():
    from givepose_amd._lib import GivePoseHipError
    return GivePoseHipError


def _dev(I):
    return {k: v.cuda().contiguous() for k, v in I.items()}


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _buffer(n, row, dtype):
    buf = torch.full((n + row,), R.NAN, dtype=dtype, device="cuda")
    buf[n:] = R.SENTINEL
    return buf


def run_case(what, v, bound, launch, dtype):
    """launch(buf) writes v.numel() values at the front of buf.  Returns the first launch's buffer."""
    n, row = v.numel(), v.shape[-1]
    bufs = []
    for _ in range(2):
        buf = _buffer(n, row, dtype)
        launch(buf)
        torch.cuda.synchronize()
        bufs.append(buf)
    ratio, msg = R.check_buffer(bufs[0], v, bound, what)
    print(f"GPU_RATIO {what} {ratio:.4f}")
    assert msg is None, msg
    assert torch.equal(_bits(bufs[0]), _bits(bufs[1])), f"{what}: a second launch gives other bits"
    return bufs[0]


# ------------------------------------------------------------------------------------------------ gp_resnet_stem
@pytest.mark.parametrize("case", R.RESNET_STEM_CASES, ids=R.case_id)
def test_resnet_stem(case):
    o = ops()
    B, H, W, dt = case
    I = R.resnet_stem_inputs(case)
    v, bound = R.resnet_stem_ref(I, case)
    assert bool((v == 0).any()) and bool((v > 0).any())                 # both sides of the ReLU
    if W == 256:
        assert bool((I["img"][..., 122:134] != 0).all())                # the seam between the two 64-pixel blocks of a row reads real pixels
    D = _dev(I)
    run_case(f"gp_resnet_stem {R.case_id(case)}", v, bound, lambda y: o.resnet_stem(D["img"], D["w"], D["b"], y.view(-1)[:v.numel()].view(v.shape)), dt)


def test_resnet_stem_refuses_width_64():
    o = ops()
    D = _dev(R.resnet_stem_inputs(R.RESNET_STEM_CASES[0]))
    with pytest.raises(_err()):
        o.resnet_stem(torch.zeros(1, 3, 4, 64, device="cuda"), D["w"], D["b"], torch.zeros(1, 2, 32, 64, device="cuda"))


# ------------------------------------------------------------------------------------------------ gp_maxpool3x3s2
@pytest.mark.parametrize("case", R.MAXPOOL_CASES, ids=R.case_id)
def test_maxpool3x3s2(case):
    """Bit-equal to F.max_pool2d(x, 3, 2, 1), whose padding is -inf: every window at the border is all negative."""
    o = ops()
    B, H, W, C, dt = case
    I = R.maxpool_inputs(case)
    assert R.maxpool_border_windows_all_negative(I, case)
    v, bound = R.maxpool_ref(I, case)
    assert not bool(bound.any())
    x = I["x"].cuda()
    got = run_case(f"gp_maxpool3x3s2 {R.case_id(case)}", v, bound, lambda y: o.maxpool3x3s2(x, y), dt)
    assert torch.equal(_bits(got[:v.numel()].cpu()), _bits(v.to(dt).reshape(-1)))


def test_maxpool3x3s2_refuses_fp16_c12():
    with pytest.raises(_err()):
        ops().maxpool3x3s2(torch.zeros(1, 4, 4, 12, dtype=torch.float16, device="cuda"), torch.zeros(1, 2, 2, 12, dtype=torch.float16, device="cuda"))


# ------------------------------------------------------------------------------------------------ gp_patchify_xyz
@pytest.mark.parametrize("case", R.PATCHIFY_CASES, ids=R.case_id)
def test_patchify_xyz(case):
    """Bit-equal to the reshaped map (fp16: one round-to-nearest-even conversion); the map's 4th channel is NaN and must not arrive."""
    o = ops()
    B, Rr, P, dt = case
    I = R.patchify_inputs(case)
    assert bool(torch.isnan(I["xyz4"][:, 3]).all())
    v, bound = R.patchify_ref(I, case)
    x = I["xyz4"].cuda()
    got = run_case(f"gp_patchify_xyz {R.case_id(case)}", v, bound, lambda y: o.patchify_xyz(x, y, B, Rr, P), dt)
    assert torch.equal(_bits(got[:v.numel()].cpu()), _bits(v.to(dt).reshape(-1)))


def test_patchify_xyz_refuses_r12_p8():
    with pytest.raises(_err()):
        ops().patchify_xyz(torch.zeros(144, 4, device="cuda"), torch.zeros(4, 192, device="cuda"), 1, 12, 8)


# ------------------------------------------------------------------------------------------------ gp_dwconv_ln_groups
def _dwg_launch(D, KS, act, table):
    o = ops()
    t = torch.tensor(table, dtype=torch.int32, device="cuda")
    return lambda y: o.dwconv_ln_groups(D["x"], D["wt"], D["bias"], D["ln_w"], D["ln_b"], y, KS, t, eps=R.DWG_EPS, act=act)


@pytest.mark.parametrize("case", R.DWG_CASES, ids=R.case_id)
def test_dwconv_ln_groups(case):
    """Output row c q + j = depth-wise conv + LayerNorm + activation at flat full-resolution pixel 4 g q + (c - g) q + j of x, every
    element within the bound."""
    dt, C, KS, act, table = case
    v, bound = R.dwg_ref(R.dwg_inputs(case), case)
    assert tuple(v.shape) == (R.DWG_B * R.DWG_HW * R.DWG_HW // 4, C)
    run_case(f"gp_dwconv_ln_groups {R.case_id(case)}", v, bound, _dwg_launch(_dev(R.dwg_inputs(case)), KS, act, table), dt)


def _dwg_out(D, cfg, table):
    dt, C, KS, act = cfg
    n = R.DWG_B * R.DWG_HW * R.DWG_HW // 4 * C
    y = _buffer(n, C, dt)
    _dwg_launch(D, KS, act, table)(y)
    return y[:n].view(-1, C)


@pytest.mark.parametrize("cfg", [c for c in R.DWG_CONFIGS if c[2] == 3], ids=R.case_id)
def test_dwconv_ln_groups_same_bits_as_dwconv_ln(cfg):
    """KS = 3, where both entry points launch the same strip form: with the all-zero table the output is gp_dwconv_ln's flat prefix of
    B q pixels, and with [0, 0, 2, 2, 2] the rows of each batch are gp_dwconv_ln on that batch's crops alone."""
    o = ops()
    dt, C, KS, act = cfg
    D = _dev(R.dwg_inputs(cfg + (None,)))
    B, q = R.DWG_B, R.DWG_HW * R.DWG_HW // 4

    def plain(x, n_pixels):
        y = torch.full((n_pixels, C), R.NAN, dtype=dt, device="cuda")
        o.dwconv_ln(x, D["wt"], D["bias"], D["ln_w"], D["ln_b"], y, KS, eps=R.DWG_EPS, act=act, n_pixels=n_pixels)
        return y

    assert torch.equal(_bits(_dwg_out(D, cfg, (0,) * B)), _bits(plain(D["x"], B * q)))
    got = _dwg_out(D, cfg, (0, 0, 2, 2, 2))
    assert torch.equal(_bits(got[:2 * q]), _bits(plain(D["x"][:2].contiguous(), 2 * q)))
    assert torch.equal(_bits(got[2 * q:]), _bits(plain(D["x"][2:].contiguous(), 3 * q)))


def test_dwconv_ln_groups_clamps_its_table():
    """Entries are clamped to [0, crop]: [-1, 7, 2, 9, 2] gives the bits of [0, 1, 2, 3, 2].  (The kernel reads inside x by
    construction; this is a statement about values.)"""
    cfg = R.DWG_CONFIGS[0]
    D = _dev(R.dwg_inputs(cfg + (None,)))
    assert torch.equal(_bits(_dwg_out(D, cfg, R.DWG_CLAMP_TABLE)), _bits(_dwg_out(D, cfg, R.DWG_CLAMPED)))


@pytest.mark.parametrize("H,W,alias", [(16, 8, False), (3, 16, False), (16, 16, True)])
def test_dwconv_ln_groups_refuses(H, W, alias):
    o = ops()
    cfg = R.DWG_CONFIGS[0]
    D = _dev(R.dwg_inputs(cfg + (None,)))
    x = torch.zeros(1, H, W, 256, dtype=torch.float16, device="cuda")
    y = x if alias else torch.zeros(H * W * 256, dtype=torch.float16, device="cuda")
    with pytest.raises(_err()):
        o.dwconv_ln_groups(x, D["wt"], D["bias"], D["ln_w"], D["ln_b"], y, 3, torch.zeros(1, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------------------ entry points without arithmetic
def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_pack_poses():
    """gp_pack_poses: (B,15) = [R row-major 9 | t 3 | size 3], the operands' bits."""
    from givepose_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    B = 37
    rot, t, size = (torch.randn(B, n, generator=g).cuda() for n in (9, 3, 3))
    out = _buffer(B * 15, 15, torch.float32)
    L.check(L.load().gp_pack_poses(rot.data_ptr(), t.data_ptr(), size.data_ptr(), out.data_ptr(), B, _st()), "gp_pack_poses")
    v = torch.cat([rot, t, size], 1).cpu()
    assert R.check_buffer(out, v, torch.zeros_like(v), "gp_pack_poses")[1] is None


def test_device_info():
    from givepose_amd import _lib as L
    cu, arch = ctypes.c_int(), ctypes.create_string_buffer(64)
    L.check(L.load().gp_device_info(ctypes.byref(cu), arch, 64), "gp_device_info")
    props = torch.cuda.get_device_properties(torch.cuda.current_device())
    assert cu.value == props.multi_processor_count and arch.value.decode().startswith("gfx950")
    short = ctypes.create_string_buffer(b"x" * 8, 8)
    L.check(L.load().gp_device_info(None, short, 4), "gp_device_info")            # truncated and terminated inside the caller's length
    assert short.raw[:4] == b"gfx\0" and short.raw[4:] == b"xxxx"


def test_timing_report_and_top():
    """gp_timing_begin / end / report / top: two max-pool launches and one ResNet stem are counted in their classes with the
    algorithmic figures the launchers declare."""
    from givepose_amd import _lib as L
    o, lib = ops(), L.load()
    x = R.maxpool_inputs(R.MAXPOOL_CASES[-1])["x"].cuda()                # (2, 8, 8, 64) fp32
    y = torch.empty(2, 4, 4, 64, device="cuda")
    D = _dev(R.resnet_stem_inputs(R.RESNET_STEM_CASES[0]))               # (2, 3, 4, 128)
    ys = torch.empty(2, 2, 64, 64, device="cuda")
    torch.cuda.synchronize()
    L.check(lib.gp_timing_begin(_st()), "gp_timing_begin")
    try:
        o.maxpool3x3s2(x, y)
        o.maxpool3x3s2(x, y)
        o.resnet_stem(D["img"], D["w"], D["b"], ys)
    finally:
        L.check(lib.gp_timing_end(), "gp_timing_end")

    def report(cls):
        n, ms, fl, by = ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        rc = lib.gp_timing_report(cls, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by))
        return rc, n.value, ms.value, fl.value, by.value

    rc, n, ms, fl, by = report(L.KC_ELEMENTWISE)
    assert (rc, n, fl, by) == (0, 2, 0.0, 2 * x.numel() * 4 * 1.25) and ms > 0
    rc, n, ms, fl, by = report(L.KC_SMALL)
    assert (rc, n, fl) == (0, 1, 2.0 * 2 * 2 * 64 * 147 * 64) and ms > 0
    assert all(report(c)[:2] == (0, 0) for c in (L.KC_GEMM, L.KC_DCNV3, L.KC_DWCONV_LN, L.KC_NORM))
    assert report(L.KC_COUNT)[0] == -1
    seen = {}
    for r in range(4):
        lab = ctypes.create_string_buffer(160)
        c, n, ms, fl, by = ctypes.c_int(), ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        if lib.gp_timing_top(r, lab, 160, ctypes.byref(c), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) != 0:
            break
        seen[lab.value.decode()] = (c.value, n.value)
    assert seen == {"gp_maxpool3x3s2": (L.KC_ELEMENTWISE, 2), "gp_resnet_stem": (L.KC_SMALL, 1)}
    o.maxpool3x3s2(x, y)                                                 # after gp_timing_end nothing more is counted
    torch.cuda.synchronize()
    assert report(L.KC_ELEMENTWISE)[1] == 2


def test_graph_capture_and_replay():
    """gp_graph_begin / end / launch / destroy: one captured max-pool launch does not run at capture time, and every replay writes
    the eager launch's bits."""
    from givepose_amd import _lib as L
    lib = L.load()
    case = R.MAXPOOL_CASES[-1]
    x = R.maxpool_inputs(case)["x"].cuda()
    B, H, W, C, dt = case
    eager = torch.empty(B, H // 2, W // 2, C, device="cuda")
    ops().maxpool3x3s2(x, eager)
    y = torch.full_like(eager, R.SENTINEL)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = ctypes.c_void_p(side.cuda_stream)
    L.check(lib.gp_graph_begin(sp), "gp_graph_begin")
    try:
        rc = lib.gp_maxpool3x3s2(x.data_ptr(), y.data_ptr(), B, H, W, C, L.GP_F32, sp)
    finally:
        ge = ctypes.c_void_p()
        rc_end = lib.gp_graph_end(sp, ctypes.byref(ge))
    L.check(rc, "gp_maxpool3x3s2")
    L.check(rc_end, "gp_graph_end")
    assert ge.value
    try:
        side.synchronize()
        assert bool((y == R.SENTINEL).all())                             # captured, not run
        for _ in range(2):
            L.check(lib.gp_graph_launch(ge, sp), "gp_graph_launch")
            side.synchronize()
            assert torch.equal(_bits(y), _bits(eager))
            y.fill_(R.SENTINEL)
            torch.cuda.synchronize()
    finally:
        L.check(lib.gp_graph_destroy(ge), "gp_graph_destroy")
