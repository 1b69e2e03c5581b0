"""Float64 reference of gp_gemm and the per-element error bound its outputs must meet (tests/test_gemm_conformance.py).

The reference works from the operands as the kernel sees them (fp16-rounded values for fp16 storage, fp32 values for fp32
storage and the split-operand mode) and computes, in float64,
    v = X W^T + b        a = |X| |W|^T + |b|
(conv mode: F.conv2d of x / w and of |x| / |w|, permuted back to channels-last), then the epilogue.  Every element must meet
    |got - ref| <= L_epi * e_acc + e_act + e_out
  e_acc = c_acc * a      fp32 accumulation, worst case for any summation order (see c_acc below)
  L_epi                  1 for the ReLU forms, |gamma| for SCALE_RES, 1.13 (max |GELU'|) for GELU
  e_act                  the error the GELU form's comment in csrc/common.hpp claims, plus the fp32 epilogue arithmetic
  e_out                  rounding of the stored value (fp16: 2^-11 |ref| + 2^-25; fp32: 2^-24 |ref|; the lean residual epilogue
                         rounds gamma * v to fp16 before its packed fp16 residual add: + 2^-11 |gamma v|)
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U16, U32 = 2.0 ** -11, 2.0 ** -24
EPI_NONE, EPI_GELU, EPI_RELU, EPI_LRELU, EPI_SCALE_RES, EPI_RES_RELU, EPI_LNFOLD_GELU = range(7)
EPI_NAMES = {EPI_NONE: "none", EPI_GELU: "gelu", EPI_RELU: "relu", EPI_LRELU: "lrelu", EPI_SCALE_RES: "scale_res",
             EPI_RES_RELU: "res_relu", EPI_LNFOLD_GELU: "lnfold_gelu"}
RES_EPIS = (EPI_SCALE_RES, EPI_RES_RELU)

# GELU forms and the error their comments in csrc/common.hpp claim
GELU_POLY2 = "poly2"      # gelu_poly2 (fp16 storage): 4.1e-5 for |v| <= 4.4; beyond the clamp x (1 - 5.4e-6) resp. x 5.4e-6
GELU_PK16 = "pk16"        # gelu16_xn (variants 20 / 21): |R error| 1.95e-4 in exact arithmetic, Horner on packed fp16
GELU_ERF = "erf"          # gelu_erf (fp32 storage, split-operand mode, fp32 residual stream, split-K reduce): A&S 7.1.26, 1.5e-7


def set_threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


def c_acc(K, split=False):
    """Worst-case relative accumulation error per unit of a = sum |x||w| + |b|: K products and the bias are K + 1 fp32 terms,
    so at most K roundings of a partial sum, plus one of a product (fp32 operands) -- (K + 1) 2^-24.  The split-operand mode
    adds its representation error, 2^-22 |x||w| per product for each of the two dropped / rounded low parts and the missing
    lo x lo term (include/givepose_hip.h, gp_gemm_desc.split_shift)."""
    return (K + 1) * U32 + (3 * 2.0 ** -22 if split else 0.0)


def gelu_exact(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def gelu_act_err(v, form):
    av = v.abs()
    if form == GELU_POLY2:
        return 4.1e-5 + torch.where(av > 4.4, 5.4e-6 * av, torch.zeros_like(av)) + 2 * U32 * av
    if form == GELU_PK16:
        # fit 1.95e-4 + x rounded to fp16 before the packed arithmetic (|GELU'| <= 1.13) + the fp16 Horner: u = a/2 - 1 in [-1, 1],
        # 8 roundings of intermediates <= 0.33 (2^-11 x 2^-2 each, propagated with |du| <= 1) -> 8 x 2^-13
        return 1.95e-4 + 1.13 * U16 * av + 8 * 2.0 ** -13
    if form == GELU_ERF:
        # |erf error| 1.5e-7 -> 0.5 |v| 1.5e-7; v_rcp / v_exp (1 ulp each) and the fp32 products: a few 2^-24 of |v|
        return (0.75e-7 + 8 * U32) * av + 1e-30
    raise ValueError(form)


class Lin:
    """v and a of one operand set, shared by all epilogues of that shape (float64, CPU)."""

    def __init__(self, v, a, K, split=False):
        self.v, self.a, self.K, self.split = v, a, K, split
        self.e_acc = c_acc(K, split) * a


def lin_plain(x, w, b=None, split=False):
    x, w = x.double(), w.double()
    v = x @ w.t()
    a = x.abs() @ w.abs().t()
    if b is not None:
        v = v + b.double()
        a = a + b.double().abs()
    return Lin(v, a, x.shape[1], split)


def lin_conv(x_nhwc, w_packed, KH, KW, stride, pad, b=None, split=False):
    """x (B,H,W,Cin) channels-last, w_packed (Cout, KH*KW*Cin) with K = (kh*KW+kw)*Cin+ci, as gp_gemm's conv mode."""
    B, H, W_, Cin = x_nhwc.shape
    Cout = w_packed.shape[0]
    x = x_nhwc.double().permute(0, 3, 1, 2)
    w = w_packed.double().view(Cout, KH, KW, Cin).permute(0, 3, 1, 2)
    v = F.conv2d(x, w, None, stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(-1, Cout)
    a = F.conv2d(x.abs(), w.abs(), None, stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(-1, Cout)
    if b is not None:
        v = v + b.double()
        a = a + b.double().abs()
    return Lin(v, a, KH * KW * Cin, split)


def epilogue(lin, epi, out, gelu_form=GELU_POLY2, r=None, g=None, lean_res=False):
    """(ref, bound, pre) for `out` in {"f16", "f32", "planes"}: ref the exact value, bound the per-element bound of the stored
    value, pre the bound of the fp32 value before the store (what the fused GroupNorm statistics sum)."""
    v, e_acc = lin.v, lin.e_acc
    z = torch.zeros_like(v)
    gv = z
    if epi == EPI_NONE:
        ref, L, e_act = v, 1.0, z
    elif epi == EPI_RELU:
        ref, L, e_act = v.clamp_min(0), 1.0, z
    elif epi == EPI_LRELU:
        # 0.1f is 0.1 (1 + 1.5e-8), and the product rounds once
        ref, L, e_act = torch.where(v > 0, v, 0.1 * v), 1.0, torch.where(v > 0, z, 2 * U32 * v.abs())
    elif epi == EPI_GELU:
        ref, L, e_act = gelu_exact(v), 1.13, gelu_act_err(v, gelu_form)
    elif epi == EPI_SCALE_RES:
        rr, gg = r.double(), g.double()[None, :]
        gv = gg * v
        ref, L, e_act = rr + gv, gg.abs(), U32 * gv.abs()
    elif epi == EPI_RES_RELU:
        rr = r.double()
        gv = v
        ref, L, e_act = (rr + v).clamp_min(0), 1.0, z
    else:
        raise ValueError(epi)
    pre = L * e_acc + e_act + U32 * (ref.abs() + gv.abs())        # fp32 epilogue arithmetic (the residual add, gamma * v)
    big = ref.abs() + pre
    if out == "f16":
        e_out = U16 * big + 2.0 ** -25
        if lean_res and epi in RES_EPIS:
            e_out = e_out + U16 * (gv.abs() + pre) + 2.0 ** -25
    elif out == "planes":
        e_out = 2.0 ** -22 * big + 2.0 ** -35
    else:
        e_out = U32 * big
    return ref, pre + e_out, pre


def check(got, ref, bound, what="", worst=6):
    """(max err / bound, message): message is None when every element meets its bound, else the worst elements with their
    coordinates.  NaN / inf outputs always fail."""
    got = got.detach().double().cpu()
    ref, bound = ref.double().cpu(), bound.double().cpu()
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = err / bound
    mx = float(ratio.max()) if ratio.numel() else 0.0
    if mx <= 1.0:
        return mx, None
    flat = ratio.flatten()
    idx = torch.topk(flat, min(worst, flat.numel())).indices
    lines = [f"{what}: max err/bound {mx:.3g}, {int((ratio > 1).sum())} of {ratio.numel()} elements over"]
    for i in idx.tolist():
        coord = np.unravel_index(i, tuple(ratio.shape))
        lines.append(f"  at {tuple(int(c) for c in coord)}: got {float(got.flatten()[i]):.9g} ref {float(ref.flatten()[i]):.9g} "
                     f"err {float(err.flatten()[i]):.3g} bound {float(bound.flatten()[i]):.3g}")
    return mx, "\n".join(lines)


def gn_reference(ref, pre, Bimg, hw, groups, rows=64):
    """Per statistics chunk (b, chunk, group): float64 (sum, sum of squares) of the exact outputs over `rows` rows and the
    group's channels, with the bound of the kernel's fp32 sums (element bounds summed, plus fp32 summation of n terms)."""
    N = ref.shape[1]
    cpg = N // groups
    n = rows * cpg
    shp = (Bimg, hw // rows, rows, groups, cpg)
    r = ref.reshape(shp)
    p = pre.reshape(shp)
    s = r.sum((2, 4))
    q = (r * r).sum((2, 4))
    sa = r.abs().sum((2, 4))
    s_b = p.sum((2, 4)) + n * U32 * sa
    q_b = ((2 * r.abs() + p) * p).sum((2, 4)) + (n + 1) * U32 * q
    return torch.stack([s, q], -1).reshape(-1), torch.stack([s_b, q_b], -1).reshape(-1)
