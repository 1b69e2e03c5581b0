"""tests/dcnv3_backward_reference.py on the CPU, before a kernel is held against it (no GPU).

  agreement          with the float64 goldens tests/golden/dcnv3_any_bwd_*.npz (the reference operator's own autograd) at their existing
                     tolerance; with the C oracle's backward (oracle/dcnv3_ref.c) at <= 1e-12 of scale on every double case and on the
                     "edges" / "dyadic" sets of the float / half cases, where the type of the location cannot matter; with torch autograd
                     of a differentiable float64 restatement of the forward on a "c3" case
  self-consistency   the opmath restatement (per-lane chain, then the butterfly) within HALF the bound in front of the store on every case
                     and tensor, its rounding to half within the bound of givepose_amd.dcnv3_backward
  sensitivity        every mutation of dcnv3_backward_reference.MUTATIONS is rejected; where is printed (-s)
  coverage           every edge class in every "edges" case; exact zeros and positive bounds in all three tensors of every case; every
                     element of every buffer carries a finite bound and a change of twice its bound (or of one ulp of zero) is rejected
"""
import numpy as np
import pytest
import torch

import dcnv3_backward_reference as B
import dcnv3_reference as D

F16, F32, F64 = torch.float16, torch.float32, torch.float64
T = torch.from_numpy


def _geom(c):
    return c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, c.dh, c.dw, c.G, c.D, c.os, c.rc


def _scale(v):
    return max(1.0, float(v.abs().max()))


# ------------------------------------------------------------------------------------------------ agreement
@pytest.mark.parametrize("name", ["dcnv3_any_bwd_D1", "dcnv3_any_bwd_D16", "dcnv3_any_bwd_D30", "dcnv3_any_bwd_hw"])
def test_agrees_with_the_float64_goldens(golden, name):
    z = golden(name)
    kh, kw, sh, sw, ph, pw, dh, dw, G, Dc, rc = (int(v) for v in z["params"])
    N, H, W, _ = z["input"].shape
    c = D.mk("golden-" + name, F64, N, H, W, G=G, D=Dc, k=(kh, kw), ss=(sh, sw), pp=(ph, pw), dd=(dh, dw), os=float(z["offset_scale"]), rc=rc, entry="any")
    assert z["offset"].size == D.n_rows(c) * G * D.n_taps(c) * 2
    I = dict(x=T(z["input"]), off=T(z["offset"]).reshape(-1), mask=T(z["mask"]).reshape(-1), gout=T(z["grad_output"]).reshape(D.n_rows(c), G * Dc))
    r = B.ref(I, c)
    for k in B.TENSORS:
        exp = T(np.asarray(z[k], dtype=np.float64)).reshape(-1)
        assert float((r[k][0].reshape(-1) - exp).abs().max()) < 1e-6 * _scale(exp), (name, k)      # tests/test_hip_dcnv3_any.py TOL[float64]


@pytest.mark.parametrize("case", [c for c in B.CASES if c.dt == F64 or c.iset in ("edges", "dyadic")], ids=lambda c: c.name)
def test_agrees_with_the_c_oracle(case):
    from oracle import dcnv3_c            # (builds itself with `make` where build() has not)
    c = case
    I = B.inputs(c)
    want = B.buffers(c, B.ref(I, c))
    got = dcnv3_c.dcnv3_backward_any_c(*(I[k].double().numpy() for k in ("x", "off", "mask", "gout")), *_geom(c))
    for k, g in zip(B.TENSORS, got):
        v = want[k][0]
        assert float((T(g).reshape(-1) - v).abs().max()) <= 1e-12 * _scale(v), (c.name, k)


def test_agrees_with_autograd_of_a_float64_forward():
    """The forward written with differentiable torch operations (floor detached: the derivative of the bilinear weights at a fixed cell)."""
    c = B.BY_NAME["any-d-rc-axes-c3"]
    I = B.inputs(c)
    R_, G, Dc, P, H, W = D.n_rows(c), c.G, c.D, D.n_taps(c), c.H, c.W
    x = I["x"].clone().requires_grad_()
    off = I["off"].clone().requires_grad_()
    m = I["mask"].clone().requires_grad_()
    p0h, p0w, b = D._p0(c, F64)
    taps = D.tap_positions(c)
    ti, tj = (torch.tensor([float(t[k] * d) for t in taps], dtype=F64) for k, d in ((0, c.dw), (1, c.dh)))
    o = off.view(R_, G, P, 2)
    lw_, lh_ = p0w.view(-1, 1, 1) + (ti + o[..., 0]) * c.os, p0h.view(-1, 1, 1) + (tj + o[..., 1]) * c.os
    inr = ((lh_ > -1) & (lw_ > -1) & (lh_ < H) & (lw_ < W)).detach()
    fh, fw = lh_.detach().floor(), lw_.detach().floor()
    lh, lw = lh_ - fh, lw_ - fw
    y0, x0 = fh.long(), fw.long()
    xf = x.view(c.N * H * W, G, Dc)
    gidx = torch.arange(G).view(1, -1, 1).expand(R_, G, P)
    out = 0
    for yy, xx, wt in ((y0, x0, (1 - lh) * (1 - lw)), (y0, x0 + 1, (1 - lh) * lw), (y0 + 1, x0, lh * (1 - lw)), (y0 + 1, x0 + 1, lh * lw)):
        ok = inr & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        lin = b.view(-1, 1, 1) * (H * W) + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)
        out = out + (torch.where(ok, wt, torch.zeros_like(wt)) * m.view(R_, G, P)).unsqueeze(-1) * xf[lin, gidx]
    out.sum(2).backward(I["gout"].view(R_, G, Dc))
    r = B.ref(I, c)
    for k, g in zip(B.TENSORS, (x.grad, off.grad, m.grad)):
        v = r[k][0]
        assert float((g.reshape(-1) - v.reshape(-1)).abs().max()) <= 1e-12 * _scale(v), k


# ------------------------------------------------------------------------------------------------ self-consistency
def test_opmath_evaluation_within_half_the_bound_and_its_half_store_within_the_bound():
    worst = {k: (0.0, "") for k in B.TENSORS}
    for c in B.CASES:
        I = B.inputs(c)
        r, got = B.ref(I, c), B.f32(I, c)
        for k in B.TENSORS:
            v, bound = r[k]
            assert got[k].dtype == D.opmath(c) and got[k].shape == v.shape
            assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(bound).all()) and bool((bound >= 0).all())
            ratio, msg = D.check(got[k], v, bound, f"{c.name} {k} opmath")
            assert ratio <= 0.5, msg or f"{c.name} {k}: the opmath evaluation is at {ratio:.3f} of the bound"
            worst[k] = max(worst[k], (ratio, c.name))
        if c.dt == F16:
            rs = B.ref(I, c, stored=F16)
            for k in B.TENSORS:
                _, msg = D.check(got[k].to(F16), *rs[k], f"{c.name} {k} opmath, rounded to half")
                assert msg is None, msg
    for k in B.TENSORS:
        print(f"CPU_RATIO gp_dcnv3_backward opmath {k} {worst[k][0]:.4f} {worst[k][1]}")


# ------------------------------------------------------------------------------------------------ coverage
def test_every_edge_class_in_every_edges_case():
    edges = [c for c in B.CASES if c.iset == "edges"]
    assert len(edges) >= 9
    for c in edges:
        k = D.classify(c, D.inputs(c))
        assert all(n > 0 for n in k.values()), (c.name, k)


def test_cases_hold_what_was_asked_for():
    by = B.BY_NAME
    assert all(sum(c.dt == dt for c in B.CASES) == len(B.CASES) // 3 for dt in (F64, F32, F16)) and not any(c.poison is not None for c in B.CASES)
    assert all(c.N <= 3 and c.H <= 16 and c.W <= 16 for c in B.CASES)
    pn = by["bwd-f-pn-D64-edges-full"]
    assert (pn.G, pn.D, pn.kh, pn.sh, pn.ph) == (4, 64, 3, 2, 1) and pn.H != pn.W and pn.H % 2 == 1 and D.out_hw(pn) == (3, 4)
    assert B.buf_rows(pn) == pn.N * pn.H * pn.W > D.n_rows(pn)
    I = B.inputs(pn)
    assert I["off"].numel() == B.buf_rows(pn) * 72 and bool((I["off"][D.n_rows(pn) * 72:] == D.SENTINEL).all()) and bool((I["mask"][D.n_rows(pn) * 36:] == D.SENTINEL).all())
    assert by["bwd-h-pn-D16-c3-full"].D == 16 and by["bwd-f-D128-c3"].D == 128
    assert D.n_rows(by["bwd-f-partial-G3D8-edges-os2"]) * 3 % 4 != 0
    assert any(D.n_taps(c) > 64 and c.D > 64 for c in B.CASES) and any(c.rc and c.sh != c.sw and c.ph != c.pw and c.dh != c.dw for c in B.CASES)
    for c in B.CASES:
        g = B.inputs(c)["gout"].view(D.n_rows(c), c.G, c.D)
        assert g.dtype == c.dt and bool((g[::7] == 0).all()) and bool((g[2] != 0).any())
        assert int((g[1, c.G - 1] != 0).sum()) == 1


def test_zero_and_positive_bounds_in_every_tensor_and_no_element_exempt():
    gen = torch.Generator().manual_seed(7)
    for c in B.CASES:
        I = B.inputs(c)
        bufs = B.buffers(c, B.ref(I, c))
        GP = c.G * D.n_taps(c)
        sizes = dict(grad_input=I["x"].numel(), grad_offset=I["off"].numel(), grad_mask=I["mask"].numel())
        assert sizes["grad_offset"] == B.buf_rows(c) * GP * 2 and sizes["grad_mask"] == B.buf_rows(c) * GP
        for k in B.TENSORS:
            v, bound = bufs[k]
            assert v.numel() == bound.numel() == sizes[k], (c.name, k)                 # one bound per element of the buffer the entry is handed
            assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all())
            zero, pos = bound == 0, bound > 0
            assert bool(zero.any()) and bool(pos.any()) and bool((v[zero] == 0).all()), (c.name, k, int(zero.sum()), int(pos.sum()))
            assert D.check_buffer(D.with_tail(v), v, bound)[1] is None
            for idx in (zero.nonzero().reshape(-1), pos.nonzero().reshape(-1)):
                i = int(idx[int(torch.randint(idx.numel(), (1,), generator=gen))])
                bad = v.clone()
                bad[i] += max(2 * float(bound[i]), 2.0 ** -149)
                assert D.check_buffer(D.with_tail(bad), v, bound)[1] is not None, (c.name, k, i)
        if B.full_buffers(c):
            n = D.n_rows(c) * GP
            assert bool((bufs["grad_offset"][1][2 * n:] == 0).all()) and bool((bufs["grad_mask"][1][n:] == 0).all())
        lh, lw, _ = D.locations(c, D.inputs(c), D.opmath(c))
        outside = ~((lh > -1) & (lw > -1) & (lh < c.H) & (lw < c.W))
        r = B.ref(I, c)
        assert bool(outside.any()) and bool((r["grad_mask"][1][outside] == 0).all()) and bool((r["grad_offset"][1][outside] == 0).all())
        e = B._true(c)
        assert bool((r["grad_input"][1][e["n"] == 0] == 0).all())


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("mut", [m for m, _ in B.MUTATIONS])
def test_mutation_is_rejected(mut):
    eligible = [c for c in B.CASES if dict(B.MUTATIONS)[mut](c)]
    assert eligible, "no case can expose this mutation"
    rejecting = []
    for c in eligible:
        I = B.inputs(c)
        want = B.buffers(c, B.ref(I, c))
        wrong = B.buffers(c, B.ref(I, c, mut=None if mut == "tail_not_zero" else mut), mut=mut)
        hit = []
        for k in B.TENSORS:
            ratio, msg = D.check_buffer(D.with_tail(wrong[k][0]), *want[k], f"{mut} {c.name} {k}")
            if msg is not None:
                hit.append((k, ratio))
        if hit:
            rejecting.append((c, hit))
    passed = [c.name for c in eligible if c.name not in {r.name for r, _ in rejecting}]
    where = sorted({k for _, hit in rejecting for k, _ in hit})
    print(f"MUTATION {mut}: rejected on {len(rejecting)} of {len(eligible)} eligible cases, in {where}" + (f"; passes on {passed}" if passed else ""))
    assert rejecting, f"{mut} passes the checker on every eligible case"
    assert not passed, f"{mut} passes the checker on {passed}"
