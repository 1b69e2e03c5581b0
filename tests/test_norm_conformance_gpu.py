"""GPU: every kernel form of the norm family on its own, through givepose_amd.ops, against the float64 references and per-element bounds
of tests/norm_reference.py (derived from term counts and number formats; tests/test_norm_reference_cpu.py has checked the inputs, the
bounds, the routing and the mutations on the CPU).  tests/test_hip_ops.py compares these kernel forms with each other bit for bit;
this file does not repeat that.  The largest ratios of an MI355X run: profiles/norm_conformance.txt.

Every case: the output is NaN with a row of sentinels behind it and inside every ldy gap; every element within its bound (the worst ratio
and its index are printed on failure); the sentinels intact; a second launch gives the same bits.  Forced forms go through the documented
act codes only, on shapes their guards accept (norm_reference.form_taken restates the routing and the CPU file asserts it for every case).

Instantiations a forward pass can launch, and the case(s) that reach each (`norm_reference.DW_CASES` etc.; fp16 unless stated):

  gp_dwconv_ln
    dwconv_ln_kernel<half, 7, 2>            f16-C512-B2-8x16-k7 (+ offset, eps .25, prefixes n 37 / n 19), f16-C128-B2-8x8-k7
    dwconv_ln_kernel<half, 3, 2>            f16-C256-B2-8x16-k3 gelu / relu / lrelu / none, prefixes n 37 / n 19
    dwconv_ln_kernel<half, 7, 8>            f16-C1024-B33-8x8-k7, and its prefix n 2109 (a partial last strip)
    dwconv_ln_kernel<float, 3 | 7, 8>       f32-C64 / C1024-B2-8x8-k3-gelu / k7, prefixes n 37, eps .25
    dwconv7_ln_tiled_kernel<half, 1|2|4>    f16-C128 / 256 / 512-B2-16x24-k7-code104
    dwconv7_ln_tiled_kernel<float,2|4|8|16> f32-C128 / 256 / 512 / 1024-B2-16x24-k7-code104
    dwconv7_ln_mfma_kernel<1, 1>            f16-C128-B2-12x32 (+ offset)
    dwconv7_ln_mfma_kernel<2, 1>            f16-C256-B4-12x48 (+ eps .25)
    dwconv7_ln_mfma_kernel<4, 2>            f16-C512-B5-12x64
    dwconv7_ln_mfma_kernel<4, 1>            f16-C512-B43-12x64                      LARGE: 516 workgroups, 16.9 M values
    dwconv7_ln_tall_kernel<2|4|8, 8>        f16-C128 / 256 / 512-B2-8x16-code110    (zero rows above and below)
    dwconv7_ln_tall_kernel<2|4|8, 9>        f16-C128 / 256 / 512-B2-24x16-code110   (an interior tile)
    dwconv7_ln_tall_kernel<2|4, 6, WIDE>    f16-C128 / 256-B2-16x48-code110
    dwconv7_ln_tall_kernel<2|4|8, 8, TH 4>  f16-C128 / 256 / 512-B2-12x16-code112
    dwconv7_ln_tall_kernel<16, 8, TH 4|2, PAIR>  f16-C1024-B4-12x8-code113 / code114
    dwconv3_ln_tile_kernel<4 | 2>           f16-C256-B3-8x32-k3-gelu-code121 / code126, whole and n 384 (1.5 images)
    not covered: dwconv_ln_kernel<half, 3, 8> (only behind GP_DW3_NARROW=0, an A/B switch); the timing ablations (act codes 101 / 102 /
    105 .. 109 / 111), GP_DW_STAMPS builds and every other form that only a GP_DW* variable selects; the GP_OUT_PLANES store of the fp32
    kernels (the split-operand output format: tests/test_split_gemm.py)
  gp_dwconv7_raw_stats
    dwconv7_ln_mfma_kernel<1, 1, RAW>       C128-B2-12x32 (one slab), C512-B2-12x32 (four slabs: grid.y)
  gp_layernorm
    layernorm_kernel<half> / <float>        f16-C128 / 1024 / 2048 (CT > 64: the two-stage reduction), f32-C64 / 512 / 1024; rows 1, PG - 1, PG + 1, 300;
                                            ldy = C + one vector, in place, eps .25
    layernorm_kernel<half, float>           f16-C128-inf32 (GP_IN_F32)
    layernorm_padded_kernel<half|float>     f16-C192, f32-C192;   <half, float>: f16-C192-inf32
  gp_groupnorm_chunks / _stats / _apply
    gn_partial_kernel<half|float>           every GN case without rows=: 64-pixel chunks (with a 36-pixel tail), one 256-pixel chunk at HW < 64,
                                            256-pixel chunks at B HW >= 262144 (LARGE, B 64)
    gn_apply_kernel<half|float>             granularity 32 (the small cases), 64 and 128 (LARGE: C64-B32 / B64-HW4096: 8.4 / 16.8 M values); every
                                            activation, ldy = 2 C, in place, eps .25, caller-supplied statistics in 64- / 32- / 16-row chunks, a group
                                            at |mean| = 20 std
    not covered: granularity 256 (C 64, B 128, HW 4096: 33.5 M values; reference and comparison take 3.5 s and 3 GB on the CPU alone)
  gp_groupnorm_upsample2x
    gn_upsample2x_kernel<4 | 2 | 1>         C512 / C256 / C128, C64 at (3, 8, 24) and (1, 5, 7)
  gp_upsample_bilinear2x
    upsample2x_rows_kernel<half|float>      (2, 3, 7, C 64), (1, 8, 5, C 256)
    upsample2x_kernel<half|float>           (1, 4, 3, C 96): C / VEC no power of two
"""
import ctypes

import pytest
import torch

import norm_reference as N

pytestmark = pytest.mark.gpu


def ops():
    from givepose_amd import ops as o
    return o


def _dev(I):
    return {k: v.cuda().contiguous() for k, v in I.items()}


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _id(case):
    return case.name


def run_case(what, v, bound, launch, dtype, ldy=None, col0=0, init=None):
    """launch(buf) writes the rows of v (rows, C) at stride ldy, columns [col0, col0 + C) of the flat buffer.  init: what an in-place case
    finds there instead of NaN.  Returns the first launch's buffer."""
    rows, C = v.shape
    ldy = C if ldy is None else ldy
    bufs = []
    for _ in range(2):
        buf = N.blank_buffer(rows, C, ldy, col0, C, dtype).cuda()
        if init is not None:
            buf[:rows * ldy].view(rows, ldy)[:, col0:col0 + C] = init.reshape(rows, C)
        launch(buf)
        torch.cuda.synchronize()
        bufs.append(buf)
    ratio, msg = N.check_strided(bufs[0], v, bound, ldy, col0, what)
    print(f"GPU_RATIO {what} {ratio:.4f}")
    assert msg is None, msg
    assert torch.equal(_bits(bufs[0]), _bits(bufs[1])), f"{what}: a second launch gives other bits"
    return bufs[0]


# ------------------------------------------------------------------------------------------------ gp_dwconv_ln
@pytest.mark.parametrize("case", N.DW_CASES, ids=_id)
def test_dwconv_ln(case):
    if not N.routing_env_is_default():
        pytest.skip("a GP_DW* variable is set: gp_dwconv_ln's routing is not the default one the cases assume")
    o = ops()
    assert N.form_taken(case.B, case.H, case.W, case.C, case.KS, case.code, case.npix, case.dt) == case.form
    I = N.dw_inputs(case)
    v, bound = N.dw_ref(I, case)
    assert tuple(v.shape) == (case.npix, case.C)
    D = _dev(I)
    run_case(f"gp_dwconv_ln {case.form} {case.name}", v, bound,
             lambda y: o.dwconv_ln(D["x"], D["wt"], D["bias"], D["ln_w"], D["ln_b"], y, case.KS, eps=case.eps, act=case.code, n_pixels=case.npix), case.dt)


# ------------------------------------------------------------------------------------------------ gp_dwconv7_raw_stats
@pytest.mark.parametrize("case", N.RAW_CASES, ids=_id)
def test_dwconv7_raw_stats(case):
    """y: the conv output with one fp16 rounding; stats: the moments of the values the kernel STORED, in the layout (pixel, 2, C / 128)."""
    o = ops()
    I = N.raw_inputs(case)
    v, bound = N.raw_y_ref(I, case)
    D = _dev(I)
    nst = v.shape[0] * 2 * (case.C // 128)
    stats = []

    def launch(y):
        st = torch.full((nst + 64,), N.NAN, device="cuda")
        st[nst:] = N.SENTINEL
        o.dwconv7_raw_stats(D["x"], D["wt"], D["bias"], y, st)
        stats.append(st)

    y = run_case(f"gp_dwconv7_raw_stats y {case.name}", v, bound, launch, torch.float16)
    sv, sb = N.raw_stats_of(y[:v.numel()].cpu().view(v.shape))
    ratio, msg = N.check_buffer(stats[0], sv, sb, f"gp_dwconv7_raw_stats stats {case.name}")
    print(f"GPU_RATIO gp_dwconv7_raw_stats stats {case.name} {ratio:.4f}")
    assert msg is None, msg
    assert torch.equal(_bits(stats[0]), _bits(stats[1]))


# ------------------------------------------------------------------------------------------------ gp_layernorm
@pytest.mark.parametrize("case", N.LN_CASES, ids=_id)
def test_layernorm(case):
    o = ops()
    I = N.ln_inputs(case)
    v, bound = N.ln_ref(I, case)
    D = _dev(I)
    ldy = N.ln_ldy(case)
    if case.mode == "inf32":
        assert D["x"].dtype == torch.float32 and case.dt == torch.float16          # the wrapper then asks for GP_IN_F32
    if case.mode == "inplace":
        def launch(buf):
            xv = buf[:v.numel()].view(case.rows, case.C)
            o.layernorm(xv, D["ln_w"], D["ln_b"], xv, eps=case.eps)
    else:
        def launch(buf):
            o.layernorm(D["x"], D["ln_w"], D["ln_b"], buf, eps=case.eps, ldy=ldy if case.mode == "ldy" else 0)
    run_case(f"gp_layernorm {case.name}", v, bound, launch, case.dt, ldy=ldy, init=D["x"] if case.mode == "inplace" else None)


# ------------------------------------------------------------------------------------------------ gp_groupnorm_chunks / _stats / _apply
@pytest.mark.parametrize("case", N.GN_CASES, ids=_id)
def test_groupnorm(case):
    """ops.groupnorm = gp_groupnorm_stats (unless the case supplies the statistics) + gp_groupnorm_apply: the partial sums in their layout
    ((b chunks + chunk) G + g) 2 + {sum, sum of squares} and the normalised rows, each against float64."""
    o = ops()
    B, HW, C = case.B, case.HW, case.C
    I = N.gn_inputs(case)
    v, bound = N.gn_ref(I, case)
    sv, sb = N.gn_stats_ref(I, case)
    chunk = N.gn_chunk_rows(case)
    if case.rows is None:
        assert o.groupnorm_chunks(B, HW) == N.cdiv(HW, chunk) and sv.numel() == B * N.cdiv(HW, chunk) * N.GN_G * 2
    D = _dev(I)
    ldy, col0 = N.gn_layout(case)
    supplied = None if case.rows is None else N.gn_supplied_partials(I, case).cuda()
    parts = []

    def launch(buf):
        part = torch.full((sv.numel() + 2 * N.GN_G,), N.NAN, device="cuda")
        part[sv.numel():] = N.SENTINEL
        if supplied is not None:
            part[:sv.numel()] = supplied
        if case.mode == "inplace":
            x = out = buf[:B * HW * C].view(B, HW, C)
        else:
            x, out = D["x"], buf[:B * HW * ldy].view(B, HW, ldy)[:, :, col0:col0 + C]
        o.groupnorm(x, D["gn_w"], D["gn_b"], out, N.GN_G, case.act, part, eps=case.eps, ldy=ldy, fused_stats=supplied is not None, rows=case.rows or 64)
        parts.append(part)

    run_case(f"gp_groupnorm_apply {case.name}", v, bound, launch, case.dt, ldy=ldy, col0=col0, init=D["x"] if case.mode == "inplace" else None)
    ratio, msg = N.check_buffer(parts[0], sv, sb, f"gp_groupnorm_stats {case.name}")
    if supplied is None:
        print(f"GPU_RATIO gp_groupnorm_stats {case.name} {ratio:.4f}")
    assert msg is None, msg                     # (supplied statistics: untouched, and the sentinel behind them intact)
    assert torch.equal(_bits(parts[0]), _bits(parts[1]))


# ------------------------------------------------------------------------------------------------ gp_groupnorm_upsample2x
@pytest.mark.parametrize("case", N.GU_CASES, ids=_id)
def test_groupnorm_upsample2x(case):
    """Held to the float64 bound (tests/test_hip_ops.py keeps the bit-equality with the two passes).  The statistics come from
    gp_groupnorm_stats in its own chunking (chunks = 0); HW = 35 has no `rows` the wrapper could divide by, hence the raw entry points."""
    from givepose_amd import _lib as L
    lib = L.load()
    B, H, W, C = case.B, case.H, case.W, case.C
    I = N.gu_inputs(case)
    v, bound = N.gu_ref(I, case)
    assert tuple(v.shape) == (B * 4 * H * W, C)
    D = _dev(I)
    P, st = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    part = torch.zeros(B * N.cdiv(H * W, N.gn_pxb(B, H * W)) * N.GN_G * 2, device="cuda")
    L.check(lib.gp_groupnorm_stats(P(D["x"]), P(part), B, H * W, C, N.GN_G, L.GP_F16, st), "gp_groupnorm_stats")

    def launch(y):
        L.check(lib.gp_groupnorm_upsample2x(P(D["x"]), P(part), P(D["gn_w"]), P(D["gn_b"]), P(y), B, H, W, C, N.GN_G, case.eps, case.act, 0, L.GP_F16, st),
                "gp_groupnorm_upsample2x")

    run_case(f"gp_groupnorm_upsample2x {case.name}", v, bound, launch, torch.float16)


# ------------------------------------------------------------------------------------------------ gp_upsample_bilinear2x
@pytest.mark.parametrize("case", N.UP_CASES, ids=_id)
def test_upsample_bilinear2x(case):
    o = ops()
    I = N.up_inputs(case)
    v, bound = N.up_ref(I, case)
    x = I["x"].cuda()
    run_case(f"gp_upsample_bilinear2x {case.name}", v, bound, lambda y: o.upsample_bilinear2x(x, y), case.dt)
