"""Float64 restatement of the map-encoder backward family (include/givepose_encgrad.h, gpe_*) by explicit formulas: every operator
and the encoder as a whole.  No autograd and no import of oracle/ here: tests/test_enc_backward_cpu.py shows that these formulas equal
float64 autograd through oracle.posenet_ref.map_encoder_ref.

Gates.  Two kinds of decision make the encoder piecewise smooth: the ReLU after each GroupNorm (is the pre-activation > 0) and, for
every (row, group, tap) of a DCNv3 core, the cell (h_low, w_low) = floor(location) together with the test that the location lies
inside (-1, H) x (-1, W).  `enc_run(..., gates=...)` evaluates forward and backward AT GIVEN GATES: the bilinear weights are formed
from the given cell (lh = h - h_low, continuous across a cell border) and the ReLU passes where the given mask says so.  A float32
run that rounds a location to the other side of an integer then has a float64 reference of the same branch.  `gates_of` reads the
gates from saved tensors (offset rows and the pre-norm / output maps), in the arithmetic of the tensors' dtype.

Bounds derived here.
  * ORACLE: restatement against float64 autograd, max|a - b| / max|b| per tensor <= oracle_bound(N, R) = 64 (N R^2 + 2304) 2^-53.
    Both sides are float64 evaluations of the same formulas in another order.  A sum of L terms has a worst-case relative error
    L 2^-53 against the sum of the absolute terms; the longest sums are over the N R^2 rows of layer 0 (conv / input_proj gradients),
    and 2304 = 256 x 9 covers the contraction widths.  A gradient passes three layers of about twenty such stages, two of them
    normalisations that amplify by the ratio of a row's absolute sum to its norm: the factor 64 covers both.
  * CHAIN: a contraction on the device is a k-ordered fmaf chain (possibly split and merged in order) and an ordered row sum is a
    tree of depth <= K: |got - ref| <= (K + 8) 2^-24 sum_k |a_k| |b_k| per element, K counted on all-ones operands (the project's
    bound of tests/test_xyz_backward_gpu.py).
  * YARDSTICK: everything else is held to 8 times the error of a CPU float32 run of the same inputs, per tensor, as
    max|got - ref| / max|ref|.
  * MARGIN: delta_loc = 16 x the float32 oracle's largest deviation of a sampling location from float64, delta_u the same for the ReLU
    pre-activations; only gates whose float64 location is within delta_loc of an integer (or pre-activation within delta_u of 0) may
    differ between a float32 run and float64, and they are at most 0.1 % of all gates.
"""
import functools
import math

import numpy as np
import torch

LAYER_IDS = (0, 3, 6)
WEIGHT_SEED = 0
CASES = ((1, 16), (3, 16), (5, 16), (2, 64))          # (B, R), one coupling batch each
GROUPED = ((5, 16), (2, 3))                           # (B, R) run as the coupling batches [2, 3]
INPUT_SEED = {(1, 16): 41, (3, 16): 42, (5, 16): 43, (2, 64): 44}
U24 = 2.0 ** -24


def oracle_bound(N, R):
    return 64 * (N * R * R + 2304) * 2.0 ** -53


def enc_params(seed=WEIGHT_SEED):
    """{name over enc_grad.PARAM_KEYS: float32 numpy array} of the seeded synthetic encoder (givepose_amd.synth)."""
    from givepose_amd import PoseNetConfig, enc_grad, synth
    m = synth.param_manifest(PoseNetConfig())
    return {k: synth.synth_tensor("nocs_encoder." + k, m["nocs_encoder." + k], seed) for k in enc_grad.PARAM_KEYS}


def make_inputs(B, R, seed):
    """coor (B,3,R,R) in the range of a NOCS map and an upstream gradient (B,256,R/8,R/8), float32."""
    r = np.random.Generator(np.random.Philox(key=[seed, 0xE7C]))
    coor = (r.random((B, 3, R, R)) - 0.5).astype(np.float32)
    g = r.standard_normal((B, 256, R // 8, R // 8)).astype(np.float32)
    return coor, g


def rel_figures(got, ref):
    """name -> max|got - ref| / max|ref| (float64)."""
    out = {}
    for k, r in ref.items():
        r = np.asarray(r, np.float64)
        g = np.asarray(got[k], np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        out[k] = float(np.max(np.abs(g - r)) / np.max(np.abs(r)))
    return out


# ------------------------------------------------------------------------------------------------ Linear, conv1x1
def linear_forward(X, W, b=None):
    Y = X @ W.T
    return Y if b is None else Y + b


def linear_backward(dY, X, W):
    return dY @ W, dY.T @ X, dY.sum(0)


def conv1x1_backward(dY, X, W):
    """dY (B,Cout,HW), X (B,Cin,HW), W (Cout,Cin) -> dX, dW, db."""
    B, Cout = dY.shape[:2]
    d, x, w = dY.reshape(B, Cout, -1), X.reshape(B, X.shape[1], -1), W.reshape(Cout, -1)
    return torch.einsum("bop,oi->bip", d, w).reshape(X.shape), torch.einsum("bop,bip->oi", d, x).reshape(W.shape), d.sum((0, 2))


# ------------------------------------------------------------------------------------------------ depth-wise 3x3 + LN + GELU on a prefix
def gelu(u):
    return 0.5 * u * (1 + torch.erf(u / math.sqrt(2)))


def gelu_slope(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def _pad_hw(x):      # (N,H,W,C) -> (N,H+2,W+2,C), zeros around each image
    N, H, W, C = x.shape
    p = x.new_zeros(N, H + 2, W + 2, C)
    p[:, 1:-1, 1:-1] = x
    return p


def dwln_forward(xin, dw_w, dw_b, ln_w, ln_b, n):
    N, H, W, C = xin.shape
    xp = _pad_hw(xin)
    u = dw_b.expand(N, H, W, C).clone()
    for kh in range(3):
        for kw in range(3):
            u = u + xp[:, kh:kh + H, kw:kw + W] * dw_w[:, 0, kh, kw]
    u = u.reshape(-1, C)[:n]
    mean = u.mean(1)
    rstd = 1 / torch.sqrt(((u - mean[:, None]) ** 2).mean(1) + 1e-6)
    x1 = gelu((u - mean[:, None]) * rstd[:, None] * ln_w + ln_b)
    return {"dwout": u, "mean": mean, "rstd": rstd, "x1": x1}


def dwln_backward(dx1, xin, sv, dw_w, ln_w, ln_b):
    """-> dxin (N,H,W,C), d_dw_w (C,1,3,3), d_dw_b, d_ln_w, d_ln_b."""
    N, H, W, C = xin.shape
    n = dx1.shape[0]
    xh = (sv["dwout"] - sv["mean"][:, None]) * sv["rstd"][:, None]
    dy = dx1 * gelu_slope(xh * ln_w + ln_b)
    d_ln_w, d_ln_b = (dy * xh).sum(0), dy.sum(0)
    dxh = dy * ln_w
    du = sv["rstd"][:, None] * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    full = xin.new_zeros(N * H * W, C)
    full[:n] = du
    full = full.reshape(N, H, W, C)
    xp, dp = _pad_hw(xin), _pad_hw(full)
    d_dw_w = torch.zeros_like(dw_w)
    dxin = torch.zeros_like(xin)
    for kh in range(3):
        for kw in range(3):
            d_dw_w[:, 0, kh, kw] = (full * xp[:, kh:kh + H, kw:kw + W]).sum((0, 1, 2))
            dxin = dxin + dp[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W] * dw_w[:, 0, kh, kw]      # du at (y + 1 - kh, x + 1 - kw)
    return dxin, d_dw_w, du.sum(0), d_ln_w, d_ln_b


# ------------------------------------------------------------------------------------------------ the DCNv3 core: 3x3, stride 2, pad 1
def core_rows(N, H, W):
    return N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)


def core_locations(offset, N, H, W):
    """-> loc_w, loc_h (rows,4,9) in offset's dtype, formed as the kernels form them: (2 wo - 1) + (i + off), tap q = 3 i + j."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rows = N * Ho * Wo
    off = offset.reshape(-1)[:rows * 72].reshape(rows, 4, 9, 2)
    r = torch.arange(rows)
    wo, ho = (r % Wo).to(off.dtype), (r // Wo % Ho).to(off.dtype)
    q = torch.arange(9)
    i, j = (q // 3).to(off.dtype), (q % 3).to(off.dtype)
    return (2 * wo - 1)[:, None, None] + (i + off[..., 0]), (2 * ho - 1)[:, None, None] + (j + off[..., 1])


def cells_of(offset, N, H, W):
    """The sampling gates of offset rows, in their own dtype: {"valid", "h_low", "w_low"} (rows,4,9)."""
    lw, lh = core_locations(offset, N, H, W)
    return {"valid": (lh > -1) & (lw > -1) & (lh < H) & (lw < W), "h_low": torch.floor(lh).long(), "w_low": torch.floor(lw).long()}


def _corners(offset, N, H, W, cells):
    """The four corners of every tap at the given cells: [(flat pixel index (rows,4,9), weight, d weight / d h, d weight / d w, exists)]."""
    lw_, lh_ = core_locations(offset, N, H, W)
    cells = cells if cells is not None else cells_of(offset, N, H, W)
    h0, w0, valid = cells["h_low"], cells["w_low"], cells["valid"]
    lh, lw = lh_ - h0, lw_ - w0
    hh, hw = 1 - lh, 1 - lw
    rows = lw_.shape[0]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    b = (torch.arange(rows) // (Ho * Wo))[:, None, None]
    out = []
    for hy, wx, wt, dh, dw in ((h0, w0, hh * hw, -hw, -hh), (h0, w0 + 1, hh * lw, -lw, hh), (h0 + 1, w0, lh * hw, hw, -lh),
                               (h0 + 1, w0 + 1, lh * lw, lw, lh)):
        ok = valid & (hy >= 0) & (hy <= H - 1) & (wx >= 0) & (wx <= W - 1)
        pix = (b * H + hy.clamp(0, H - 1)) * W + wx.clamp(0, W - 1)
        out.append((pix, wt, dh, dw, ok.to(wt.dtype)))
    return out


def core_forward(xp, offset, logits, cells=None):
    """xp (N,H,W,256) -> mask (rows,36) probabilities, y (rows,256)."""
    N, H, W, _ = xp.shape
    rows = core_rows(N, H, W)
    m = torch.softmax(logits.reshape(-1)[:rows * 36].reshape(rows, 4, 9), -1)
    x = xp.reshape(N * H * W, 4, 64)
    g = torch.arange(4)[None, :, None]
    y = xp.new_zeros(rows, 4, 64)
    for pix, wt, _, _, ok in _corners(offset, N, H, W, cells):
        y = y + ((wt * ok * m)[..., None] * x[pix, g]).sum(2)
    return m.reshape(rows, 36), y.reshape(rows, 256)


def core_backward(xp, offset, mask, dy, cells=None):
    """-> dxp (N,H,W,256), doffset (rows,72), dmask_logits (rows,36)."""
    N, H, W, _ = xp.shape
    rows = core_rows(N, H, W)
    m, d = mask.reshape(rows, 4, 9), dy.reshape(rows, 4, 1, 64)
    x = xp.reshape(N * H * W, 4, 64)
    g = torch.arange(4)[None, :, None]
    dxp = xp.new_zeros(N * H * W * 4, 64)
    gm, gh, gw = (xp.new_zeros(rows, 4, 9) for _ in range(3))
    for pix, wt, dh, dw, ok in _corners(offset, N, H, W, cells):
        dot = (d * x[pix, g]).sum(-1) * ok                     # <dy, the corner's pixel> per (row, group, tap)
        gm, gh, gw = gm + wt * dot, gh + dh * dot * m, gw + dw * dot * m
        dxp.index_add_(0, (pix * 4 + g).reshape(-1), ((wt * ok * m)[..., None] * d).reshape(-1, 64))
    dlog = m * (gm - (m * gm).sum(-1, keepdim=True))
    return dxp.reshape(N, H, W, 256), torch.stack((gw, gh), -1).reshape(rows, 72), dlog.reshape(rows, 36)


# ------------------------------------------------------------------------------------------------ GroupNorm + ReLU
def gn_stats(x, G=32, eps=1e-5):
    B, C = x.shape[:2]
    xg = x.reshape(B, G, -1)
    mean = xg.mean(2)
    return mean, 1 / torch.sqrt(((xg - mean[:, :, None]) ** 2).mean(2) + eps)


def _expand(v, x, G):
    B, C = x.shape[:2]
    return v.repeat_interleave(C // G, 1).reshape((B, C) + (1,) * (x.dim() - 2))


def _bc(p, x):
    return p.reshape((1, -1) + (1,) * (x.dim() - 2))


def gn_relu_forward(x, mean, rstd, gamma, beta, G=32, relu=None):
    """-> out, the pre-activation u.  relu: the gate (bool, like x) in the place of u > 0."""
    u = (x - _expand(mean, x, G)) * _expand(rstd, x, G) * _bc(gamma, x) + _bc(beta, x)
    return u * ((u > 0) if relu is None else relu), u


def gn_relu_backward(dout, x, mean, rstd, gamma, beta, G=32, relu=None):
    """-> dx, dgamma, dbeta."""
    B, C = x.shape[:2]
    xh = (x - _expand(mean, x, G)) * _expand(rstd, x, G)
    u = xh * _bc(gamma, x) + _bc(beta, x)
    dy = dout * ((u > 0) if relu is None else relu)
    red = (0,) + tuple(range(2, x.dim()))
    dgamma, dbeta = (dy * xh).sum(red), dy.sum(red)
    dxh = dy * _bc(gamma, x)
    m1 = dxh.reshape(B, G, -1).mean(2)
    m2 = (dxh * xh).reshape(B, G, -1).mean(2)
    return _expand(rstd, x, G) * (dxh - _expand(m1, x, G) - xh * _expand(m2, x, G)), dgamma, dbeta


# ------------------------------------------------------------------------------------------------ the encoder
SAVED_KEYS = ("x", "xp", "dwout", "ln_mean", "ln_rstd", "x1", "offset", "mask", "y", "pre", "gn_mean", "gn_rstd", "act")


def _layer_keys(l):
    i = LAYER_IDS[l]
    q = f"features.{i}."
    return {"conv_w": q + "conv.weight", "conv_b": q + "conv.bias", "dw_w": q + "dcnv3.dw_conv.0.weight", "dw_b": q + "dcnv3.dw_conv.0.bias",
            "ln_w": q + "dcnv3.dw_conv.1.1.weight", "ln_b": q + "dcnv3.dw_conv.1.1.bias", "off_w": q + "dcnv3.offset.weight",
            "off_b": q + "dcnv3.offset.bias", "mask_w": q + "dcnv3.mask.weight", "mask_b": q + "dcnv3.mask.bias",
            "in_w": q + "dcnv3.input_proj.weight", "in_b": q + "dcnv3.input_proj.bias", "out_w": q + "dcnv3.output_proj.weight",
            "out_b": q + "dcnv3.output_proj.bias", "gn_w": f"features.{i + 1}.weight", "gn_b": f"features.{i + 1}.bias"}


def batch_forward(P, coor, gates=None):
    """One coupling batch: coor (N,3,R,R) -> the saved tensors {key: [layer 0, 1, 2]} (layouts of enc_grad.saved_shapes)."""
    sv = {k: [] for k in SAVED_KEYS}
    inp = coor
    for l in range(3):
        p = {k: P[n] for k, n in _layer_keys(l).items()}
        N, Cin, H, _ = inp.shape
        Ho = H // 2
        n = N * Ho * Ho
        x = linear_forward(inp.permute(0, 2, 3, 1).reshape(-1, Cin), p["conv_w"].reshape(256, Cin), p["conv_b"])
        xp = linear_forward(x, p["in_w"], p["in_b"])
        d = dwln_forward(x.reshape(N, H, H, 256), p["dw_w"], p["dw_b"], p["ln_w"], p["ln_b"], n)
        offset = linear_forward(d["x1"], p["off_w"], p["off_b"])
        gate = None if gates is None else gates[l]
        mask, y = core_forward(xp.reshape(N, H, H, 256), offset, linear_forward(d["x1"], p["mask_w"], p["mask_b"]), gate)
        pre = linear_forward(y, p["out_w"], p["out_b"]).reshape(N, Ho, Ho, 256).permute(0, 3, 1, 2).contiguous()
        mean, rstd = gn_stats(pre)
        act, _ = gn_relu_forward(pre, mean, rstd, p["gn_w"], p["gn_b"], relu=None if gate is None else gate["relu"])
        for k, v in (("x", x.reshape(N, H, H, 256)), ("xp", xp.reshape(N, H, H, 256)), ("dwout", d["dwout"]), ("ln_mean", d["mean"]),
                     ("ln_rstd", d["rstd"]), ("x1", d["x1"]), ("offset", offset), ("mask", mask), ("y", y), ("pre", pre), ("gn_mean", mean),
                     ("gn_rstd", rstd), ("act", act)):
            sv[k].append(v)
        inp = act
    return sv


def batch_backward(P, sv, coor, g_feat, gates=None):
    """-> ({name: gradient}, d coor) of one coupling batch."""
    grads, da = {}, g_feat
    for l in (2, 1, 0):
        names = _layer_keys(l)
        p = {k: P[n] for k, n in names.items()}
        v = {k: sv[k][l] for k in SAVED_KEYS}
        inp = sv["act"][l - 1] if l else coor
        N, Cin, H, _ = inp.shape
        Ho = H // 2
        gate = None if gates is None else gates[l]
        g = {}
        dpre, g["gn_w"], g["gn_b"] = gn_relu_backward(da, v["pre"], v["gn_mean"], v["gn_rstd"], p["gn_w"], p["gn_b"],
                                                      relu=None if gate is None else gate["relu"])
        dy, g["out_w"], g["out_b"] = linear_backward(dpre.permute(0, 2, 3, 1).reshape(-1, 256), v["y"], p["out_w"])
        dxp, doff, dml = core_backward(v["xp"], v["offset"], v["mask"], dy, gate)
        a, g["off_w"], g["off_b"] = linear_backward(doff, v["x1"], p["off_w"])
        b, g["mask_w"], g["mask_b"] = linear_backward(dml, v["x1"], p["mask_w"])
        dx, g["dw_w"], g["dw_b"], g["ln_w"], g["ln_b"] = dwln_backward(a + b, v["x"], {"dwout": v["dwout"], "mean": v["ln_mean"], "rstd": v["ln_rstd"]},
                                                                       p["dw_w"], p["ln_w"], p["ln_b"])
        c, g["in_w"], g["in_b"] = linear_backward(dxp.reshape(-1, 256), v["x"].reshape(-1, 256), p["in_w"])
        dx = dx.reshape(-1, 256) + c
        din, cw, g["conv_b"] = linear_backward(dx, inp.permute(0, 2, 3, 1).reshape(-1, Cin), p["conv_w"].reshape(256, Cin))
        g["conv_w"] = cw.reshape(256, Cin, 1, 1)
        for k, n in names.items():
            grads[n] = g[k]
        da = din.reshape(N, H, H, Cin).permute(0, 3, 1, 2).contiguous()
    return grads, da


def gates_of(sv, N, R):
    """The gates of one batch's saved tensors (a reference run's or the device's, any dtype): per layer {"relu", "valid", "h_low", "w_low"}."""
    out = []
    for l in range(3):
        H = R >> l
        out.append({"relu": sv["act"][l] > 0, **cells_of(sv["offset"][l], N, H, H)})
    return out


def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def enc_run(params, coor, g_feat, groups=None, gates=None, dtype=torch.float64):
    """Forward and backward over the coupling batches `groups` (None: one), the parameter gradients added in batch order.
    gates: per batch, per layer, the gates to evaluate at.  -> {"saved": [per batch], "grads": {name: numpy}, "coor", "nocs_feat"}."""
    P = {k: _t(v, dtype) for k, v in params.items()}
    coor, g_feat = _t(coor, dtype), _t(g_feat, dtype)
    groups = [coor.shape[0]] if groups is None else list(groups)
    saved, total, dcoor, i0 = [], None, [], 0
    for bi, N in enumerate(groups):
        gt = None if gates is None else gates[bi]
        sv = batch_forward(P, coor[i0:i0 + N], gt)
        g, dc = batch_backward(P, sv, coor[i0:i0 + N], g_feat[i0:i0 + N], gt)
        total = g if total is None else {k: total[k] + g[k] for k in g}
        saved.append(sv)
        dcoor.append(dc)
        i0 += N
    return {"saved": saved, "grads": {k: v.numpy() for k, v in total.items()}, "coor": torch.cat(dcoor).numpy(),
            "nocs_feat": torch.cat([s["act"][2] for s in saved]).numpy()}


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    B, R = case
    return (enc_params(),) + make_inputs(B, R, INPUT_SEED[case])
