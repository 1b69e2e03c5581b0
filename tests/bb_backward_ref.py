"""Float64 restatement of the backbone backward family (include/givepose_bbgrad.h, gpb_*) by explicit formulas: every operator and the
ConvNeXt backbone as a whole.  No autograd and no import of oracle/ here: tests/test_bb_backward_cpu.py shows that these formulas equal
float64 autograd through oracle.posenet_ref.convnext_ref.  The Linears, GELU and its slope are those of tests/enc_backward_ref.py.

The function is smooth (GELU, LayerNorm): there are no gates and no margin sets, and one reference serves every run.

Bounds derived here.
  * ORACLE: restatement against float64 autograd, max|a - b| / max|b| per tensor <= oracle_bound(case)
        = 64 (1 + sum(depths)) (B (S/4)^2 + 4 max(dims)) 2^-53.
    Both sides are float64 evaluations of the same formulas in another order.  A sum of L terms has a worst-case relative error
    L 2^-53 against the sum of the absolute terms; the longest sums are over the B (S/4)^2 rows of stage 0 (its parameter gradients)
    and the widest contraction is fc2's 4 max(dims).  A gradient passes up to sum(depths) blocks and the stem, each of about ten such
    stages, one of them a normalisation that amplifies by the ratio of a row's absolute sum to its norm: the factor 64 per block
    covers both, as in enc_backward_ref.oracle_bound (64 for three layers there; here it grows with the depth).
  * CHAIN: a contraction on the device is a k-ordered fmaf chain (possibly split and merged in order) and an ordered row sum is a
    tree of depth <= K: |got - ref| <= (K + 8) 2^-24 sum_k |a_k| |b_k| per element, K counted on all-ones operands (the project's
    bound of tests/test_xyz_backward_gpu.py).  It holds the depth-wise 7x7 (forward: bias + 49 taps; dX: 49 taps; dW, db: the N H W
    rows) and the patch convs.
  * YARDSTICK: everything else (LayerNorm, the block, the backbone, the chain) is held to 8 times the error of a CPU float32 run of
    the same formulas on the same inputs, per tensor, as max|got - ref| / max|ref|, floored at 2^-24 (one rounding of the largest
    element).
"""
import functools

import numpy as np
import torch

from enc_backward_ref import gelu, gelu_slope, linear_backward, linear_forward, rel_figures  # noqa: F401

WEIGHT_SEED = 0
U24 = 2.0 ** -24
BASE = (128, 256, 512, 1024)
# name -> (dims, depths, B, S)
CASES = {"A": (BASE, (1, 1, 2, 1), 1, 32), "B": (BASE, (1, 1, 2, 1), 3, 64), "C": ((64, 128, 192, 320), (2, 1, 3, 1), 2, 96),
         "D": (BASE, (3, 3, 27, 3), 2, 32), "E": (BASE, (1, 1, 1, 1), 2, 256)}
INPUT_SEED = {"A": 51, "B": 52, "C": 53, "D": 54, "E": 55}
BLOCK_KEYS = ("gamma", "conv_dw.weight", "conv_dw.bias", "norm.weight", "norm.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
              "mlp.fc2.bias")


def oracle_bound(case):
    dims, depths, B, S = CASES[case]
    return 64 * (1 + sum(depths)) * (B * (S // 4) ** 2 + 4 * max(dims)) * 2.0 ** -53


def bb_params(dims, depths, seed=WEIGHT_SEED):
    """{name over bb_grad.PARAM_KEYS: float32 numpy array} of the seeded synthetic backbone (givepose_amd.synth)."""
    from givepose_amd import bb_grad, synth
    return {k: synth.synth_tensor("backbone." + k, s, seed) for k, s in bb_grad.param_shapes((dims, depths)).items()}


def make_inputs(case):
    """img (B,3,S,S) in the range of a normalised crop and an upstream gradient like feat, float32, from a seeded Philox stream."""
    dims, depths, B, S = CASES[case]
    r = np.random.Generator(np.random.Philox(key=[INPUT_SEED[case], 0xBB]))
    last = S // (4 << (len(dims) - 1))
    return r.standard_normal((B, 3, S, S)).astype(np.float32), r.standard_normal((B, dims[-1], last, last)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ depth-wise 7x7, pad 3, channels-last
def _pad3(x):      # (N,H,W,C) -> (N,H+6,W+6,C), zeros around each image
    N, H, W, C = x.shape
    p = x.new_zeros(N, H + 6, W + 6, C)
    p[:, 3:3 + H, 3:3 + W] = x
    return p


def dw7_forward(x, w, b):
    """x (N,H,W,C), w (C,1,7,7), b (C) -> (N,H,W,C)."""
    N, H, W, C = x.shape
    xp = _pad3(x)
    y = b.expand(N, H, W, C).clone()
    for kh in range(7):
        for kw in range(7):
            y = y + xp[:, kh:kh + H, kw:kw + W] * w[:, 0, kh, kw]
    return y


def dw7_backward(dy, x, w):
    """-> dx (N,H,W,C), dw (C,1,7,7), db (C)."""
    N, H, W, C = x.shape
    xp, dp = _pad3(x), _pad3(dy)
    dw = torch.zeros_like(w)
    dx = torch.zeros_like(x)
    for kh in range(7):
        for kw in range(7):
            dw[:, 0, kh, kw] = (dy * xp[:, kh:kh + H, kw:kw + W]).sum((0, 1, 2))
            dx = dx + dp[:, 6 - kh:6 - kh + H, 6 - kw:6 - kw + W] * w[:, 0, kh, kw]      # dy at (y + 3 - kh, x + 3 - kw)
    return dx, dw, dy.sum((0, 1, 2))


def dead_taps(H, W):
    """(7,7) bool: the taps that meet no pixel of an H x W map."""
    kh, kw = np.arange(7)[:, None], np.arange(7)[None, :]
    return (np.abs(kh - 3) >= H) | (np.abs(kw - 3) >= W)


# ------------------------------------------------------------------------------------------------ LayerNorm over channels, eps 1e-6
def ln_forward(x, w, b):
    """x (rows,C) -> y, mean, rstd."""
    mean = x.mean(1)
    rstd = 1 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + 1e-6)
    return (x - mean[:, None]) * rstd[:, None] * w + b, mean, rstd


def ln_backward(dy, x, mean, rstd, w):
    """At the given statistics -> dx, dw, db."""
    xh = (x - mean[:, None]) * rstd[:, None]
    dxh = dy * w
    dx = rstd[:, None] * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


# ------------------------------------------------------------------------------------------------ patch conv
def patch_matrix(x, p, nchw):
    """x (N,Cin,H,W) if nchw else (N,H,W,Cin) -> rows (b,oh,ow) x columns (ci,kh,kw)."""
    if nchw:
        N, Cin, H, W = x.shape
        return x.reshape(N, Cin, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(N * (H // p) * (W // p), Cin * p * p)
    N, H, W, Cin = x.shape
    return x.reshape(N, H // p, p, W // p, p, Cin).permute(0, 1, 3, 5, 2, 4).reshape(N * (H // p) * (W // p), Cin * p * p)


def patch_unmatrix(m, shape, p, nchw):
    """The inverse of patch_matrix: every input element is one element of the matrix."""
    if nchw:
        N, Cin, H, W = shape
        return m.reshape(N, H // p, W // p, Cin, p, p).permute(0, 3, 1, 4, 2, 5).reshape(shape)
    N, H, W, Cin = shape
    return m.reshape(N, H // p, W // p, Cin, p, p).permute(0, 1, 4, 2, 5, 3).reshape(shape)


def patch_forward(x, w, b, nchw):
    """conv2d(x, w, b, stride = kernel) -> rows (N H/p W/p, Cout)."""
    return linear_forward(patch_matrix(x, w.shape[2], nchw), w.reshape(w.shape[0], -1), b)


def patch_backward(dy, x, w, nchw):
    """-> dx like x, dw like w, db."""
    p = w.shape[2]
    dm, dw, db = linear_backward(dy, patch_matrix(x, p, nchw), w.reshape(w.shape[0], -1))
    return patch_unmatrix(dm, x.shape, p, nchw), dw.reshape(w.shape), db


# ------------------------------------------------------------------------------------------------ the block
def block_forward(x, P):
    """x (N,H,W,C), P {name over BLOCK_KEYS} -> {"dwout", "mean", "rstd", "h", "y2", "out"} in the layouts of bb_grad.block_forward_save."""
    N, H, W, C = x.shape
    dwout = dw7_forward(x, P["conv_dw.weight"], P["conv_dw.bias"]).reshape(-1, C)
    z, mean, rstd = ln_forward(dwout, P["norm.weight"], P["norm.bias"])
    h = linear_forward(z, P["mlp.fc1.weight"], P["mlp.fc1.bias"])
    y2 = linear_forward(gelu(h), P["mlp.fc2.weight"], P["mlp.fc2.bias"])
    return {"dwout": dwout, "mean": mean, "rstd": rstd, "h": h, "y2": y2, "out": x + (P["gamma"] * y2).reshape(x.shape)}


def block_backward(g, x, P, sv):
    """g = d out (N,H,W,C) -> {"dx"} and the nine parameter gradients."""
    N, H, W, C = x.shape
    g2 = g.reshape(-1, C)
    out = {"gamma": (g2 * sv["y2"]).sum(0)}
    z = (sv["dwout"] - sv["mean"][:, None]) * sv["rstd"][:, None] * P["norm.weight"] + P["norm.bias"]
    da, out["mlp.fc2.weight"], out["mlp.fc2.bias"] = linear_backward(g2 * P["gamma"], gelu(sv["h"]), P["mlp.fc2.weight"])
    dz, out["mlp.fc1.weight"], out["mlp.fc1.bias"] = linear_backward(da * gelu_slope(sv["h"]), z, P["mlp.fc1.weight"])
    du, out["norm.weight"], out["norm.bias"] = ln_backward(dz, sv["dwout"], sv["mean"], sv["rstd"], P["norm.weight"])
    dx, out["conv_dw.weight"], out["conv_dw.bias"] = dw7_backward(du.reshape(x.shape), x, P["conv_dw.weight"])
    out["dx"] = g + dx
    return out


# ------------------------------------------------------------------------------------------------ the backbone
def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def backbone_run(params, img, g_feat, dims, depths, dtype=torch.float64, want_saved=False):
    """Forward and backward by the formulas above -> {"feat", "img": numpy, "grads": {name: numpy}} (and "saved": {name: tensor} over
    bb_grad.saved_shapes)."""
    P = {k: _t(v, dtype) for k, v in params.items()}
    img, g_feat = _t(img, dtype), _t(g_feat, dtype)
    B, S = img.shape[0], img.shape[2]
    n = len(dims)
    side = [S // (4 << s) for s in range(n)]
    sv, tape = {}, []      # tape: ("block", stage, b) / ("down", stage)
    pre = patch_forward(img, P["stem_0.weight"], P["stem_0.bias"], True)
    x, sv["stem.mean"], sv["stem.rstd"] = ln_forward(pre, P["stem_1.weight"], P["stem_1.bias"])
    sv["stem.pre"] = pre
    for s in range(n):
        if s:
            q = f"stages_{s}.downsample."
            sv[q + "pre"] = x
            z, sv[q + "mean"], sv[q + "rstd"] = ln_forward(x, P[q + "0.weight"], P[q + "0.bias"])
            x = patch_forward(z.reshape(B, side[s - 1], side[s - 1], dims[s - 1]), P[q + "1.weight"], P[q + "1.bias"], False)
            tape.append(("down", s, 0))
        for b in range(depths[s]):
            q = f"stages_{s}.blocks.{b}."
            r = block_forward(x.reshape(B, side[s], side[s], dims[s]), {k: P[q + k] for k in BLOCK_KEYS})
            sv[q + "x"] = x
            for k in ("dwout", "mean", "rstd", "h", "y2"):
                sv[q + k] = r[k]
            x = r["out"].reshape(-1, dims[s])
            tape.append(("block", s, b))
    feat = x.reshape(B, side[-1], side[-1], dims[-1]).permute(0, 3, 1, 2).contiguous()
    grads = {}
    g = g_feat.permute(0, 2, 3, 1).reshape(-1, dims[-1])
    for kind, s, b in reversed(tape):
        if kind == "block":
            q = f"stages_{s}.blocks.{b}."
            shp = (B, side[s], side[s], dims[s])
            r = block_backward(g.reshape(shp), sv[q + "x"].reshape(shp), {k: P[q + k] for k in BLOCK_KEYS}, {k: sv[q + k] for k in ("dwout", "mean", "rstd", "h", "y2")})
            g = r.pop("dx").reshape(-1, dims[s])
            grads.update({q + k: v for k, v in r.items()})
        else:
            q = f"stages_{s}.downsample."
            z = (sv[q + "pre"] - sv[q + "mean"][:, None]) * sv[q + "rstd"][:, None] * P[q + "0.weight"] + P[q + "0.bias"]
            dz, grads[q + "1.weight"], grads[q + "1.bias"] = patch_backward(g, z.reshape(B, side[s - 1], side[s - 1], dims[s - 1]), P[q + "1.weight"], False)
            g, grads[q + "0.weight"], grads[q + "0.bias"] = ln_backward(dz.reshape(-1, dims[s - 1]), sv[q + "pre"], sv[q + "mean"], sv[q + "rstd"], P[q + "0.weight"])
    dpre, grads["stem_1.weight"], grads["stem_1.bias"] = ln_backward(g, sv["stem.pre"], sv["stem.mean"], sv["stem.rstd"], P["stem_1.weight"])
    dimg, grads["stem_0.weight"], grads["stem_0.bias"] = patch_backward(dpre, img, P["stem_0.weight"], True)
    out = {"feat": feat.numpy(), "img": dimg.numpy(), "grads": {k: grads[k].numpy() for k in params}}
    if want_saved:
        out["saved"] = sv
    return out


def flat(r):
    return {**r["grads"], "img": r["img"], "feat": r["feat"]}


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    dims, depths, B, S = CASES[case]
    return (bb_params(dims, depths),) + make_inputs(case)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(the float64 restatement, the CPU float32 restatement) of a case, each flat: the gradients in state_dict order, "img", "feat".
    Computed once and shared; callers must not modify it."""
    dims, depths, B, S = CASES[case]
    params, img, g = case_inputs(case)
    return tuple(flat(backbone_run(params, img, g, dims, depths, dt)) for dt in (torch.float64, torch.float32))
