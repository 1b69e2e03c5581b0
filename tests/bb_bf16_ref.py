"""Restatement of the "bf16" precision of the backbone backward family (include/givepose_bbgrad_bf16.h, gpbm_*): the ConvNeXt block
of tests/bb_backward_ref.py with a rounding hook `q` at the twelve operand sites of its six contractions, and the backbone built on it.

The sites (two per contraction), as the device stages them:
    fc1 forward      h   = q(LN_out) q(W1)^T + b1
    fc2 forward      y2  = q(GELU(h)) q(W2)^T + b2
    d W2             gamma (q(g)^T q(GELU(h)))
    d a              q(g) q(gamma W2), then d h = d a GELU'(h)
    d W1             q(d h)^T q(LN_out)
    d LN_out         q(d h) q(W1)
Everything else -- the depth-wise 7x7, LayerNorm, GELU and its slope, the row sums d gamma, d b2, d b1 -- reads unrounded values.

With q the identity the functions below are bb_backward_ref's own expressions in its own order, and give its bits
(tests/test_bb_bf16_cpu.py).  That fixes where the layer scale sits: bb_backward_ref contracts (g gamma) with a and with W2, so here
q(g) gamma is contracted with q(a) and with q(W2), where the device contracts q(g) with q(a) (scaling the fp32 sum by gamma) and with
q(gamma W2).  The first pair is the same number up to fp32 rounding; the second rounds W2 before the scale instead of after it: one
bf16 rounding per operand element either way, so the error figure the yardstick takes from this restatement is that of the device's
arithmetic.

round_bf16 is round-to-nearest-even on the fp32 bit pattern by integer arithmetic, independent of torch's bfloat16 conversion.
"""
import contextlib
import functools

import torch

import bb_backward_ref as R
from enc_backward_ref import gelu, gelu_slope


def identity(t):
    return t


def round_bf16(t):
    """float32 -> the nearest bf16 value (ties to even) as float32.  Finite values below the bf16 maximum only."""
    assert t.dtype == torch.float32
    b = t.contiguous().view(torch.int32)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & -65536
    return r.view(torch.float32).view(t.shape)


def block_forward(x, P, q=identity):
    """bb_backward_ref.block_forward with the hook at fc1's and fc2's operands."""
    N, H, W, C = x.shape
    dwout = R.dw7_forward(x, P["conv_dw.weight"], P["conv_dw.bias"]).reshape(-1, C)
    z, mean, rstd = R.ln_forward(dwout, P["norm.weight"], P["norm.bias"])
    h = R.linear_forward(q(z), q(P["mlp.fc1.weight"]), P["mlp.fc1.bias"])
    y2 = R.linear_forward(q(gelu(h)), q(P["mlp.fc2.weight"]), P["mlp.fc2.bias"])
    return {"dwout": dwout, "mean": mean, "rstd": rstd, "h": h, "y2": y2, "out": x + (P["gamma"] * y2).reshape(x.shape)}


def block_backward(g, x, P, sv, q=identity):
    """bb_backward_ref.block_backward with the hook at the operands of d W2, d a, d W1 and d LN_out."""
    N, H, W, C = x.shape
    g2 = g.reshape(-1, C)
    out = {"gamma": (g2 * sv["y2"]).sum(0)}
    z = (sv["dwout"] - sv["mean"][:, None]) * sv["rstd"][:, None] * P["norm.weight"] + P["norm.bias"]
    da, out["mlp.fc2.weight"] = (q(g2) * P["gamma"]) @ q(P["mlp.fc2.weight"]), (q(g2) * P["gamma"]).T @ q(gelu(sv["h"]))
    out["mlp.fc2.bias"] = (g2 * P["gamma"]).sum(0)
    dh = da * gelu_slope(sv["h"])
    dz, out["mlp.fc1.weight"], out["mlp.fc1.bias"] = q(dh) @ q(P["mlp.fc1.weight"]), q(dh).T @ q(z), dh.sum(0)
    du, out["norm.weight"], out["norm.bias"] = R.ln_backward(dz, sv["dwout"], sv["mean"], sv["rstd"], P["norm.weight"])
    dx, out["conv_dw.weight"], out["conv_dw.bias"] = R.dw7_backward(du.reshape(x.shape), x, P["conv_dw.weight"])
    out["dx"] = g + dx
    return out


@contextlib.contextmanager
def _blocks(q):
    """bb_backward_ref.backbone_run finds its block through the module: run it on the hooked block."""
    keep = R.block_forward, R.block_backward
    R.block_forward = lambda x, P: block_forward(x, P, q)
    R.block_backward = lambda g, x, P, sv: block_backward(g, x, P, sv, q)
    try:
        yield
    finally:
        R.block_forward, R.block_backward = keep


def backbone_run(params, img, g_feat, dims, depths, dtype=torch.float32, q=round_bf16, want_saved=False):
    """bb_backward_ref.backbone_run with the hooked block: the stem and the downsamples stay unrounded, as on the device."""
    with _blocks(q):
        return R.backbone_run(params, img, g_feat, dims, depths, dtype, want_saved)


@functools.lru_cache(maxsize=None)
def reference_bf16(case):
    """The CPU float32 restatement of a case of bb_backward_ref.CASES with the bf16 hook, flat like bb_backward_ref.reference.
    Computed once and shared; callers must not modify it."""
    dims, depths, B, S = R.CASES[case]
    params, img, g = R.case_inputs(case)
    return R.flat(backbone_run(params, img, g, dims, depths))
