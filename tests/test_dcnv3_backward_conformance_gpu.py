"""GPU: the DCNv3 backward, dcnv3_any_bwd_kernel<double | float | half> (csrc/dcnv3_any.hip), per element against the float64 reference and
the bounds of tests/dcnv3_backward_reference.py (derived from rounding counts; tests/test_dcnv3_backward_reference_cpu.py has checked the
reference, the bounds and the mutations on the CPU).  The ratio lines of an MI355X run: profiles/dcnv3_backward_conformance.txt.

Every case goes through the C ABI gp_dcnv3_backward.  The three gradient buffers are of the opmath type (float for half operands), NaN
before the launch -- the entry zeroes them itself -- with a row of sentinels in front and behind: the sentinels must be intact (the three
memset sizes and every store stay inside, also for half operands, where the gradient is 4 bytes wide and the operand 2); every element
within its bound and exactly 0 where the bound is 0 (a tap outside the map, an input element nothing reaches, the unconsumed tail of the
full-resolution offset / mask buffers of the PoseNet geometry); a second launch gives the same BITS in grad_offset / grad_mask (one writer
per element) and in the grad_input elements at most two terms reach, and differs by at most twice the bound where the atomics may add
in another order.  The half cases run once more through givepose_amd.dcnv3_backward (results in half, the bound with that rounding), the
PoseNet-geometry cases through DCNv3Function.apply(...).backward(grad_output).

Largest |error| / bound over the cases of an MI355X run, at the C ABI: grad_input 0.36 (any-h-rc-axes-c3), grad_offset 0.26 and grad_mask
0.32 (any-d-3x5-D1-edges).  Behind the rounding to half of the Python entry: 0.99 / 0.97 / 0.98 -- that bound is the rounding itself, which a
correctly rounded store may use up.  Nothing is tuned to these: the bounds come from the counts alone.
"""
import ctypes

import pytest
import torch

import dcnv3_backward_reference as B
import dcnv3_reference as D

pytestmark = pytest.mark.gpu
F16 = torch.float16


def _bits(t):
    return t.contiguous().view({torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _guarded(n, row, dt):
    """NaN x n with `row` sentinels in front and behind -> (whole buffer, the view handed to the entry)."""
    buf = torch.full((n + 2 * row,), D.NAN, dtype=dt)
    buf[:row] = D.SENTINEL
    buf[row + n:] = D.SENTINEL
    buf = buf.cuda()
    return buf, buf[row:row + n]


def _launch(c, dev):
    """One gp_dcnv3_backward into fresh guarded buffers -> {tensor: (whole buffer, front row)}."""
    from givepose_amd import _lib as L
    x, off, mask, gout = dev
    GP = c.G * D.n_taps(c)
    om = D.opmath(c)
    sizes = dict(grad_input=(x.numel(), c.G * c.D), grad_offset=(off.numel(), 2 * GP), grad_mask=(mask.numel(), GP))
    bufs = {k: _guarded(n, row, om) + (row,) for k, (n, row) in sizes.items()}
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    code = {torch.float16: L.GP_F16, torch.float32: L.GP_F32, torch.float64: L.GP_F64}[c.dt]
    L.check(L.load().gp_dcnv3_backward(P(x), P(off), P(mask), P(gout), *(P(bufs[k][1]) for k in B.TENSORS), off.numel(), mask.numel(), c.N, c.H, c.W,
                                       c.G, c.D, c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, c.dh, c.dw, c.os, c.rc, 256, code,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gp_dcnv3_backward")
    torch.cuda.synchronize()
    return {k: (whole.cpu(), row) for k, (whole, _, row) in bufs.items()}


def _device_inputs(c, I):
    return tuple(I[k].cuda().contiguous() for k in ("x", "off", "mask", "gout"))


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: c.name)
def test_dcnv3_backward(case):
    c = case
    I = B.inputs(c)
    want = B.buffers(c, B.ref(I, c))
    dev = _device_inputs(c, I)
    first, second = _launch(c, dev), _launch(c, dev)
    reach = B._true(c)["n"].reshape(-1)
    failures = []
    for k in B.TENSORS:
        v, bound = want[k]
        what = f"gp_dcnv3_backward dcnv3_any_bwd_kernel<{D._tn(c.dt)}> {c.name} {k}"
        (a, row), (b, _) = first[k], second[k]
        assert a.dtype == D.opmath(c) and a.numel() == v.numel() + 2 * row
        front_ok = bool((a[:row] == D.SENTINEL).all()) and bool((b[:row] == D.SENTINEL).all())
        ratio, msg = D.check_buffer(a[row:], v, bound, what)
        print(f"GPU_RATIO {c.name} {k} {ratio:.4f}")
        if not front_ok:
            failures.append(f"{what}: the sentinel in front of the buffer was overwritten")
        if msg is not None:
            failures.append(msg)
        _, msg = D.check_buffer(b[row:], v, bound, what + " (second launch)")
        if msg is not None:
            failures.append(msg)
        ga, gb = a[row:row + v.numel()], b[row:row + v.numel()]
        if k == "grad_input":
            few = reach <= 2
            if not torch.equal(_bits(ga[few]), _bits(gb[few])):
                failures.append(f"{what}: a second launch gives other bits where at most two terms reach the element")
            d = (ga.double() - gb.double()).abs()
            if not bool((d <= 2 * bound).all()):
                failures.append(f"{what}: two launches differ by more than twice the bound ({float((d - 2 * bound).max()):.3g} over)")
        elif not torch.equal(_bits(ga), _bits(gb)):
            failures.append(f"{what}: a second launch gives other bits ({int((_bits(ga) != _bits(gb)).sum())} elements): more than one writer")
    assert not failures, "\n".join(failures)


def _geom(c):
    return c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, c.dh, c.dw, c.G, c.D, c.os


def _shaped(c, I):
    """The operands in the shapes of the Python entry points: offset / mask (N, rows per image, G P 2) / (., G P)."""
    GP = c.G * D.n_taps(c)
    per = B.buf_rows(c) // c.N
    Ho, Wo = D.out_hw(c)
    return (I["x"].cuda(), I["off"].view(c.N, per, 2 * GP).cuda(), I["mask"].view(c.N, per, GP).cuda(), I["gout"].view(c.N, Ho, Wo, c.G * c.D).cuda())


def _check_all(c, got, want, what):
    failures = []
    for k, g in zip(B.TENSORS, got):
        v, bound = want[k]
        assert g.dtype == c.dt and g.numel() == v.numel(), (what, k, g.dtype, g.numel())
        ratio, msg = D.check(g, v, bound, f"{what} {c.name} {k}")
        print(f"GPU_RATIO {what} {c.name} {k} {ratio:.4f}")
        if msg is not None:
            failures.append(msg)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", [c for c in B.CASES if c.dt == F16], ids=lambda c: c.name)
def test_dcnv3_backward_half_results(case):
    """givepose_amd.dcnv3_backward on half operands: the three results in half, held to the bound that includes the final rounding."""
    from givepose_amd import dcnv3_backward
    c = case
    I = B.inputs(c)
    x, off, mask, gout = _shaped(c, I)
    got = dcnv3_backward(x, off, mask, *_geom(c), gout, 256, c.rc)
    assert tuple(got[0].shape) == tuple(x.shape) and tuple(got[1].shape) == tuple(off.shape) and tuple(got[2].shape) == tuple(mask.shape)
    _check_all(c, got, B.buffers(c, B.ref(I, c, stored=F16)), "givepose_amd.dcnv3_backward")


@pytest.mark.parametrize("case", [c for c in B.CASES if B.full_buffers(c)], ids=lambda c: c.name)
def test_dcnv3_function_backward_posenet_geometry(case):
    """DCNv3Function.apply(...).backward(grad_output) with offset / mask at the full resolution: the unconsumed rows get exact zeros."""
    from givepose_amd import DCNv3Function
    c = case
    I = B.inputs(c)
    x, off, mask, gout = (t.requires_grad_(i < 3) for i, t in enumerate(_shaped(c, I)))
    out = DCNv3Function.apply(x, off, mask, *_geom(c), 256, c.rc)
    out.backward(gout)
    _check_all(c, (x.grad, off.grad, mask.grad), B.buffers(c, B.ref(I, c, stored=F16 if c.dt == F16 else None)), "DCNv3Function.backward")
