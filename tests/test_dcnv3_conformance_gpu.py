"""GPU: every kernel form of the DCNv3 forward on its own -- gp_dcnv3_forward through givepose_amd.ops.dcnv3_forward_into, gp_dcnv3_forward_any
through the C ABI -- against the float64 reference and the per-element bound of tests/dcnv3_reference.py (derived from rounding counts and
number formats; tests/test_dcnv3_reference_cpu.py has checked the inputs, the bound, the routing and the mutations on the CPU).  The largest
ratios of an MI355X run: profiles/dcnv3_conformance.txt.

Every case: the output buffer is NaN with a row of sentinels behind it; the offset / mask rows hold sentinels in every ld gap (a value read
from there sends its tap 12288 pixels away or weighs it by -12288); every element within its bound (the worst ratio and its index are
printed on failure), exactly 0 where every tap is outside the map; the sentinels intact; a second launch gives the same bits.  The fp16
patch cases also run the per-call arms GP_DCN_WAVE8=0 and GP_DCN_LDSBC=1, which must give the bits of the default.

Instantiations and the cases that reach them (dcnv3_reference.CASES; h- = fp16 storage, f- = fp32; A = N 3, 8 x 16, stride 2: 4 x 8 outputs,
grid.x 6; B = N 13, 8 x 8: grid.x 13 (the one square map: xcd_chunk's remainder); C = N 2, 4 x 8, stride 1: grid.x 4; D = N 2, 16 x 8,
stride 2: 8 x 4 outputs, grid.x 4; every other map is non-square):

  gp_dcnv3_forward
    dcnv3_wave8_kernel<float | half, DPP>        h-A / h-B / h-C / h-D (c3, c12, edges; logits and weights; fp32 rows at ld 108 / 128, fp16 rows dense; os 1,
                                                 0.5, 2), h-dil2-pad2-* (dil 2, pad 2), h-pad0-* (9 x 17, pad 0), h-pad2-* (6 x 14, pad 2)
    dcnv3_wave8_kernel<float | half, LB>         the same cases under GP_DCN_LDSBC=1
    dcnv3_wave_kernel<half, ., 3, PATCH>         the same cases under GP_DCN_WAVE8=0
    dcnv3_wave_kernel<float, float, 3, PATCH>    f-A / f-B / f-C / f-D, f-dil2-pad2-*, f-pad0-*, f-pad2-*;  <float, half, 3, PATCH>: f-A-c12-logits-om16
    dcnv3_wave_kernel<., ., 3>                   h- / f-w3-A (N 3, 10 x 14, stride 2: 105 rows, the last workgroup partial), -w3-B (N 1, 6 x 10, stride 1)
    dcnv3_wave_kernel<., .> (run-time K)         h- / f-rc-* (K 3, remove_center, P 8; fp16 rows at ld 100), -K4-* (P 16, stride 2, 35 rows), -K2-* (P 4, 35 rows;
                                                 fp16 rows at ld 50), -K1-* (P 1)
    dcnv3_generic_kernel<., .>                   *-gen-G3D8K5-* (dil 1, pad 2, os 1.5), -gen-G1D4K3-*, -gen-G4D32K3s2-* (logits), -gen-G8D64K3-*; 35 rows each
  gp_dcnv3_forward_any
    dcnv3_any_fwd_kernel<double | float | half>  any-*-9x8-D71-* (72 taps: two owner chunks, with D > 64), any-*-3x5-D1 / -D30, any-*-rc-axes-*
                                                 (remove_center, stride 1 x 2, pad 1 x 0, dil 1 x 2); any-f-3x5-D30-edges-inf / any-h-...-nan:
                                                 one input pixel +Inf / NaN -- outputs that reach it only as the clamped address of an
                                                 out-of-range tap are finite and within bound, outputs that sample it are not finite

Not covered: the measurement arm GP_DCN_FOLD=1 (another association by design); the A/B switches GP_DCN_PATCH and GP_DCN_XCD, which are read
once per process; GP_DCN_LDS_PAD.  The backward, per element in the same way: tests/dcnv3_backward_reference.py and
tests/test_dcnv3_backward_conformance_gpu.py (goldens and the reference test's channel counts: tests/test_hip_dcnv3_any.py).
"""
import ctypes
import os

import pytest
import torch

import dcnv3_reference as D

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view({torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _device_inputs(c, I):
    x = I["x"].cuda().contiguous()
    if I["om"] is not None:
        om = I["om"].cuda()
        return x, om, om[D.lds(c)[2]:]
    return x, I["off"].cuda(), I["mask"].cuda()


def _launch(c, x, off, mask, out):
    Ho, Wo = D.out_hw(c)
    out4 = out.view(c.N, Ho, Wo, c.G * c.D)
    if c.entry == "any":
        from givepose_amd import _lib as L
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        code = {torch.float16: L.GP_F16, torch.float32: L.GP_F32, torch.float64: L.GP_F64}[c.dt]
        L.check(L.load().gp_dcnv3_forward_any(P(x), P(off), P(mask), P(out4), c.N, c.H, c.W, c.G, c.D, c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, c.dh, c.dw,
                                              c.os, c.rc, 256, code, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gp_dcnv3_forward_any")
    else:
        from givepose_amd import ops as o
        off_ld, mask_ld, _ = D.lds(c)
        o.dcnv3_forward_into(x, off, mask, out4, c.kh, c.sh, c.ph, c.dh, c.G, c.D, c.os, remove_center=c.rc, off_ld=off_ld, mask_ld=mask_ld,
                             mask_is_logits=c.logits)
    torch.cuda.synchronize()


def _run(c, dev, n, env=None):
    """One launch into a fresh NaN buffer with a row of sentinels behind it; env: variables set around the call."""
    buf = torch.full((n + c.G * c.D,), D.NAN, dtype=c.dt)
    buf[n:] = D.SENTINEL
    buf = buf.cuda()
    env = env or {}
    os.environ.update(env)
    try:
        _launch(c, *dev, buf[:n])
    finally:
        for k in env:
            os.environ.pop(k, None)
    return buf


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_dcnv3_forward(case):
    c = case
    I = D.inputs(c)
    v, bound = D.ref(I, c)
    n = v.numel()
    dev = _device_inputs(c, I)
    first, second = _run(c, dev, n), _run(c, dev, n)
    got = first.cpu()
    what = f"{'gp_dcnv3_forward_any' if c.entry == 'any' else 'gp_dcnv3_forward'} {D.form_taken(c)} {c.name}"
    if c.poison is not None:
        hard, soft = (t.reshape(-1) for t in D.poison_sets(I, c))
        out = got[:n].double()
        assert not bool(torch.isfinite(out[hard]).any()), f"{what}: an output that samples the non-finite pixel is finite"
        free = hard | soft                                   # held to nothing more: the reference CUDA and the select differ on `soft`
        got = got.clone()
        got[:n][free] = v.reshape(-1)[free].to(c.dt)
        print(f"{what}: {int(hard.sum())} outputs sample the pixel, {int(soft.sum())} at zero weight, {int((~free).sum())} must be finite")
    ratio, msg = D.check_buffer(got, v, bound, what)
    print(f"GPU_RATIO {what} {ratio:.4f}")
    assert msg is None, msg
    assert torch.equal(_bits(first), _bits(second)), f"{what}: a second launch gives other bits"
    if "wave8" in D.form_taken(c):
        for k, val in D.WAVE8_ARMS:
            arm = _run(c, dev, n, {k: val})
            assert torch.equal(_bits(arm), _bits(first)), f"{what}: {k}={val} ({D.form_taken(c, {k: val})}) gives other bits than the default"
