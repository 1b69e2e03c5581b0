"""Float64 references, per-element error bounds and the shared input sets of the small fp32 kernels that the network tests only reach
end to end: csrc/scalenet.hip (gp_sn_*), gp_resnet_stem / gp_maxpool3x3s2 / gp_patchify_xyz (csrc/misc.hip) and gp_dwconv_ln_groups
(csrc/norm.hip).  No GPU here: tests/test_ops_reference_cpu.py checks this file against itself, tests/test_scalenet_ops_gpu.py and
tests/test_misc_ops_conformance.py hold the kernels against it.

Every operation is an `Op`: its cases, the seeded inputs of a case (fp32 CPU tensors, computed once and shared), `ref(inputs, case)`
-> (v, bound) in float64 and `f32(inputs, case)`, the same operation in torch float32 (in front of the store), `pre` the
bound in front of an fp16 store (a correctly rounded fp16 store alone may use all of e_out, so the float32 evaluation is held to half of
`pre` before the store and to the whole bound behind it).  v is the exact value on the operands the kernel
sees (fp16 operands already rounded, weights in the kernel's layout); bound is built from a = the same expression on absolute values
(sum |x||w| + |b|) with u = 2^-24:

  dot products      L_act (n + 2) u a + e_act + e_out      n products accumulated onto the bias by fmaf in any order: at most n
                    roundings of a partial sum (each partial sum is bounded by a), so (n + 2) u a has room for the first-order
                    term's (1 + u)^n growth.  L_act: the largest slope of the activation (1 none / ReLU, 1.5 Hardswish at x = 3, 1/6
                    hard-sigmoid); e_act = 4 u |v| for the Hardswish / hard-sigmoid arithmetic (the add of 3, two products, the
                    rounded constant 1/6); e_out = u |v| (fp32) or 2^-11 (|v| + the bound so far) + 2^-25 (fp16, subnormals).
  chained layers    (gp_sn_se, gp_sn_head) the bound of layer k enters layer k + 1 as sum |w| bound_k beside that layer's own term.
  exact ops         bound 0: the value must be the reference's bit for bit.
  ref(..., mut=...) deliberately wrong float64 implementations (MUTATIONS): the checker must reject each on the input sets below.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from gemm_reference import GELU_ERF, GELU_POLY2, gelu_act_err, gelu_exact

U32, U16 = 2.0 ** -24, 2.0 ** -11
NAN = float("nan")
SENTINEL = -12288.0          # -3 x 2^12, exact in fp16 and fp32: fills the row behind every output buffer and must survive
F64 = torch.float64

Op = namedtuple("Op", "name cases inputs ref f32 pre", defaults=(None,))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _d(t):
    return t.double()


# ------------------------------------------------------------------------------------------------ checker
def check(got, v, bound, what="", worst=4):
    """(largest |got - v| / bound, message): message None when every element meets its bound.  bound == 0 asks for the exact value;
    NaN / inf in `got` always fail."""
    got, v, bound = got.detach().double().cpu().reshape(-1), v.double().reshape(-1), bound.double().reshape(-1)
    if got.numel() != v.numel():
        return float("inf"), f"{what}: {got.numel()} values for {v.numel()} expected"
    err = (got - v).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    mx = float(ratio.max()) if ratio.numel() else 0.0
    if mx <= 1.0:
        return mx, None
    lines = [f"{what}: max err/bound {mx:.3g}, {int((ratio > 1).sum())} of {ratio.numel()} elements over"]
    for i in torch.topk(ratio, min(worst, ratio.numel())).indices.tolist():
        lines.append(f"  at flat index {i}: got {float(got[i]):.9g} ref {float(v[i]):.9g} err {float(err[i]):.3g} bound {float(bound[i]):.3g}")
    return mx, "\n".join(lines)


def check_buffer(buf, v, bound, what=""):
    """A flat output buffer of v.numel() values followed by a tail that was filled with SENTINEL before the launch."""
    buf = buf.detach().cpu().reshape(-1)
    n = v.numel()
    tail = buf[n:].double()
    if tail.numel() == 0 or not bool((tail == SENTINEL).all()):
        return float("inf"), f"{what}: the sentinel behind the output was overwritten ({tail[:4].tolist()})"
    return check(buf[:n], v, bound, what)


def with_tail(values, tail=1):
    """What a correct kernel leaves in such a buffer (mutants that write past the end change the tail)."""
    return torch.cat([values.double().reshape(-1), torch.full((tail,), SENTINEL, dtype=F64)])


def store(v, dtype):
    """One rounding to the storage type (round-to-nearest-even), back in float64."""
    return v.to(dtype).double()


def e_out(v, pre, dtype):
    if dtype == torch.float16:
        return U16 * (v.abs() + pre) + 2.0 ** -25
    return U32 * v.abs()


# ------------------------------------------------------------------------------------------------ Scale_net activations
L_SN = {0: 1.0, 1: 1.0, 2: 1.5}


def sn_act(p, act, mut=None):
    if act == 1:
        return p.clamp_min(0)
    if act == 2:
        if mut == "hs_no_upper_clamp":
            return p * (p + 3).clamp_min(0) / 6
        if mut == "hs_div_before_clamp":
            return p * ((p + 3) / 6).clamp(0, 6)
        return p * (p + 3).clamp(0, 6) / 6
    return p


def act_branches(p, act):
    """Which branches of the activation the pre-activation values reach: (below, inside, above)."""
    if act == 2:
        return bool((p < -3).any()), bool(((p > -3) & (p < 3)).any()), bool((p > 3).any())
    if act == 1:
        return bool((p < 0).any()), True, bool((p > 0).any())
    return True, True, True


def _dot(p, a, n, act, extra=2, mut=None):
    """(act(p), bound before the store) of a dot product of n terms with pre-activation value p."""
    ref = sn_act(p, act, mut)
    e = L_SN[act] * (n + extra) * U32 * a
    if act == 2:
        e = e + 4 * U32 * ref.abs()
    return ref, e


# ------------------------------------------------------------------------------------------------ gp_sn_stem
SN_STEM_CASES = [(2, 6, 10), (3, 32, 48)]


@functools.lru_cache(None)
def sn_stem_inputs(case):
    B, H, W = case
    g = _gen(100 + H)
    return dict(img=_rn(g, B, 3, H, W), w=_rn(g, 27, 16, scale=4 * 27 ** -0.5), b=_rn(g, 16))


def _conv_w(w_tap_major, cout, cin, k):
    return w_tap_major.t().reshape(cout, cin, k, k)


def sn_stem_pre(I):
    w = _conv_w(_d(I["w"]), 16, 3, 3)
    p = F.conv2d(_d(I["img"]), w, _d(I["b"]), stride=2, padding=1).permute(0, 2, 3, 1)
    a = F.conv2d(_d(I["img"]).abs(), w.abs(), _d(I["b"]).abs(), stride=2, padding=1).permute(0, 2, 3, 1)
    return p.contiguous(), a.contiguous()


def sn_stem_ref(I, case, mut=None):
    p, a = sn_stem_pre(I)
    ref, e = _dot(p, a, 27, 2, mut=mut)
    return ref, e + U32 * ref.abs()


def sn_stem_f32(I, case):
    p = F.conv2d(I["img"], _conv_w(I["w"], 16, 3, 3), I["b"], stride=2, padding=1).permute(0, 2, 3, 1)
    return F.hardswish(p)


# ------------------------------------------------------------------------------------------------ gp_sn_pointwise
def _pw_cases():
    out = []
    for i, (M, N, K, HW) in enumerate([(70, 24, 16, 35), (130, 68, 18, 65), (64, 96, 576, 16), (8, 4, 2, 4)]):
        for act in (0, 1, 2):
            for se, res in ([(0, 0), (1, 0), (0, 1), (1, 1)] if i < 2 else [(0, 0)]):
                out.append((M, N, K, HW, act, se, res))
    return out


SN_PW_CASES = _pw_cases()


@functools.lru_cache(None)
def _pw_operands(M, N, K, HW):
    g = _gen(200 + M + K)
    # gates of one image are independent of the next image's: uniform in [0.05, 1)
    return dict(x=_rn(g, M, K), w=_rn(g, N, K, scale=4 * K ** -0.5), b=_rn(g, N), se=torch.rand(M // HW, K, generator=g) * 0.95 + 0.05,
                res=_rn(g, M, N, scale=2.0))


def sn_pw_inputs(case):
    return _pw_operands(*case[:4])


def sn_pw_pre(I, case, mut=None):
    M, N, K, HW, act, se, res = case
    x, w, b = _d(I["x"]), _d(I["w"]), _d(I["b"])
    if se:
        rows = torch.arange(M) // HW
        if mut == "se_row_plus_one":
            rows = ((torch.arange(M) + 1) // HW).clamp_max(M // HW - 1)
        x = x * _d(I["se"])[rows]
    return x @ w.t() + b, x.abs() @ w.abs().t() + b.abs()


def sn_pw_ref(I, case, mut=None):
    M, N, K, HW, act, se, res = case
    p, a = sn_pw_pre(I, case, mut)
    if res and mut == "res_before_act":
        return sn_act(p + _d(I["res"]), act), torch.zeros_like(p)
    ref, e = _dot(p, a, K, act, extra=3 if se else 2, mut=mut)      # the gate multiplies x first: one more rounding per term
    if res:
        v = ref + _d(I["res"])
        return v, e + 2 * U32 * v.abs()                              # the add after the activation, and the store
    return ref, e + U32 * ref.abs()


def sn_pw_f32(I, case):
    M, N, K, HW, act, se, res = case
    x = I["x"]
    if se:
        x = x * I["se"][torch.arange(M) // HW]
    p = x @ I["w"].t() + I["b"]
    y = F.relu(p) if act == 1 else F.hardswish(p) if act == 2 else p
    return y + I["res"] if res else y


# ------------------------------------------------------------------------------------------------ gp_sn_depthwise
def _dw_cases():
    out, i = [], 0
    for H, W in [(7, 5), (1, 1), (8, 8), (13, 6)]:
        for KS in (3, 5):
            for stride in (1, 2):
                out.append((2, H, W, (4, 24)[(i // 3) % 2], KS, stride, i % 3))
                i += 1
    return out


SN_DW_CASES = _dw_cases()


@functools.lru_cache(None)
def sn_dw_inputs(case):
    B, H, W, C, KS, stride, act = case
    g = _gen(300 + H * 7 + KS + stride)
    return dict(x=_rn(g, B, H, W, C), w=_rn(g, KS * KS, C, scale=6.0 / KS), b=_rn(g, C, scale=3.0))


def _dw_conv(x_nhwc, w_tap, b, KS, stride, mode="zeros"):
    C = x_nhwc.shape[-1]
    x = x_nhwc.permute(0, 3, 1, 2)
    w = w_tap.t().reshape(C, 1, KS, KS)
    if mode == "edge":
        x = F.pad(x, (KS // 2,) * 4, mode="replicate")
        return F.conv2d(x, w, b, stride=stride, groups=C).permute(0, 2, 3, 1).contiguous()
    return F.conv2d(x, w, b, stride=stride, padding=KS // 2, groups=C).permute(0, 2, 3, 1).contiguous()


def sn_dw_pre(I, case, mut=None):
    B, H, W, C, KS, stride, act = case
    p = _dw_conv(_d(I["x"]), _d(I["w"]), _d(I["b"]), KS, stride, "edge" if mut == "clamp_to_edge" else "zeros")
    a = _dw_conv(_d(I["x"]).abs(), _d(I["w"]).abs(), _d(I["b"]).abs(), KS, stride)
    return p, a


def sn_dw_ref(I, case, mut=None):
    B, H, W, C, KS, stride, act = case
    p, a = sn_dw_pre(I, case, mut)
    ref, e = _dot(p, a, KS * KS, act, mut=mut)
    if mut == "stride2_size_floor":
        # a kernel that takes Ho = H / stride writes (B, H/s, W/s, C) densely into the front of the buffer and leaves the rest untouched
        Ho, Wo = H // stride, W // stride
        buf = torch.full((ref.numel(),), NAN, dtype=F64)
        buf[:B * Ho * Wo * C] = ref[:, :Ho, :Wo].reshape(-1)
        return buf.view_as(ref), e
    return ref, e + U32 * ref.abs()


def sn_dw_f32(I, case):
    B, H, W, C, KS, stride, act = case
    p = _dw_conv(I["x"], I["w"], I["b"], KS, stride)
    return F.relu(p) if act == 1 else F.hardswish(p) if act == 2 else p


# ------------------------------------------------------------------------------------------------ gp_sn_avgpool
SN_POOL_CASES = [(3, HW, C) for HW in (1, 3, 49, 64) for C in (16, 72, 576)]


@functools.lru_cache(None)
def sn_pool_inputs(case):
    B, HW, C = case
    return dict(x=_rn(_gen(400 + HW + C), B, HW, C) + 0.5)


def sn_pool_ref(I, case, mut=None):
    B, HW, C = case
    x = _d(I["x"])
    div = (HW + 3) // 4 * 4 if mut == "padded_lane_divisor" else HW
    return x.sum(1) / div, (HW + 2) * U32 * x.abs().sum(1) / HW


def sn_pool_f32(I, case):
    return I["x"].mean(1)


# ------------------------------------------------------------------------------------------------ gp_sn_se
SN_SE_CASES = [(3, 16, 8), (3, 96, 24), (3, 300, 160), (3, 576, 144)]


@functools.lru_cache(None)
def sn_se_inputs(case):
    B, C, S = case
    g = _gen(500 + C)
    return dict(pooled=_rn(g, B, C), w1=_rn(g, S, C, scale=C ** -0.5), b1=_rn(g, S, scale=0.5), w2=_rn(g, C, S, scale=5 * S ** -0.5), b2=_rn(g, C))


def sn_se_pre(I):
    """(pre-gate value, its bound): fc1 + ReLU, then fc2 with fc1's bound carried through |w2|."""
    x, w1, b1, w2, b2 = (_d(I[k]) for k in ("pooled", "w1", "b1", "w2", "b2"))
    C, S = w2.shape
    h = (x @ w1.t() + b1).clamp_min(0)
    e1 = (C + 2) * U32 * (x.abs() @ w1.abs().t() + b1.abs())
    p = h @ w2.t() + b2
    e2 = (S + 2) * U32 * ((h + e1) @ w2.abs().t() + b2.abs()) + e1 @ w2.abs().t()
    return p, e2


def sn_se_ref(I, case, mut=None):
    p, e2 = sn_se_pre(I)
    v = (p + 3).clamp(0, 6) / 6
    return v, e2 / 6 + 4 * U32 * v.abs() + U32 * v.abs()


def sn_se_f32(I, case):
    h = F.relu(I["pooled"] @ I["w1"].t() + I["b1"])
    return F.hardsigmoid(h @ I["w2"].t() + I["b2"])


# ------------------------------------------------------------------------------------------------ gp_sn_head
SN_HEAD_F = 576
SN_HEAD_CASES = [(3, 8, 6, 1), (3, 24, 6, 0), (3, 64, 16, 1), (3, 1, 1, 1)]


@functools.lru_cache(None)
def sn_head_inputs(case):
    B, FD, NC, use_hw = case
    g = _gen(600 + FD)
    Fd = SN_HEAD_F
    one_hot = torch.zeros(B, NC)
    one_hot[torch.arange(B), torch.arange(B) % NC] = 1.0
    n3 = FD + NC + 2          # with use_hw = 0 the two last columns of w3 are storage behind the weights that must not be read
    roi_wh = torch.rand(B, 2, generator=g) * 200 + 20 if use_hw else torch.full((B, 2), 1e6)
    return dict(f_roi=_rn(g, B, Fd).abs(), f_full=_rn(g, B, Fd).abs(), one_hot=one_hot, roi_wh=roi_wh, mean_size=torch.rand(B, 3, generator=g) * 0.3 + 0.05,
                w1=_rn(g, 128, 2 * Fd, scale=(2 * Fd) ** -0.5), b1=_rn(g, 128, scale=0.3), w2=_rn(g, FD, 128 + NC, scale=(128 + NC) ** -0.5),
                b2=_rn(g, FD, scale=0.3), w3=_rn(g, 1, n3, scale=n3 ** -0.5), b3=_rn(g, 1, scale=0.3))


def sn_head_ref(I, case, mut=None):
    B, FD, NC, use_hw = case
    f = torch.cat([_d(I["f_roi"]), _d(I["f_full"])], 1)
    w1, b1, w2, b2, w3, b3 = (_d(I[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3"))
    oh, z = _d(I["one_hot"]), torch.zeros(B, NC, dtype=F64)
    x1 = (f @ w1.t() + b1).clamp_min(0)
    e1 = (2 * SN_HEAD_F + 2) * U32 * (f.abs() @ w1.abs().t() + b1.abs())
    x1c, e1c = (torch.cat([oh, x1], 1), torch.cat([z, e1], 1)) if mut == "one_hot_before_line1" else (torch.cat([x1, oh], 1), torch.cat([e1, z], 1))
    x2 = (x1c @ w2.t() + b2).clamp_min(0)
    e2 = (128 + NC + 2) * U32 * ((x1c + e1c) @ w2.abs().t() + b2.abs()) + e1c @ w2.abs().t()
    cols, errs = [x2, oh], [e2, z]
    if use_hw or mut == "use_hw0_reads_roi_wh":
        wh = _d(I["roi_wh"]) if mut == "roi_wh_not_scaled" else _d(I["roi_wh"]) / 100
        cols.append(wh)
        errs.append(2 * U32 * wh.abs())
    x2c, e2c = torch.cat(cols, 1), torch.cat(errs, 1)
    n3 = x2c.shape[1]
    w3 = w3[:, :n3]
    y = (x2c @ w3.t() + b3)[:, 0]
    e3 = ((n3 + 2) * U32 * ((x2c + e2c) @ w3.abs().t() + b3.abs()) + e2c @ w3.abs().t())[:, 0]
    ms = _d(I["mean_size"])
    nrm = (ms * ms).sum(1).sqrt()
    v = y + nrm
    return v, e3 + 4 * U32 * nrm + U32 * v.abs()       # sum of squares and sqrtf: 2 u relative each


def sn_head_f32(I, case):
    B, FD, NC, use_hw = case
    x1 = F.relu(torch.cat([I["f_roi"], I["f_full"]], 1) @ I["w1"].t() + I["b1"])
    x2 = F.relu(torch.cat([x1, I["one_hot"]], 1) @ I["w2"].t() + I["b2"])
    x2c = torch.cat([x2, I["one_hot"]] + ([I["roi_wh"] / 100] if use_hw else []), 1)
    return (x2c @ I["w3"][:, :x2c.shape[1]].t() + I["b3"])[:, 0] + torch.linalg.norm(I["mean_size"], dim=1)


# ------------------------------------------------------------------------------------------------ gp_resnet_stem
RESNET_STEM_CASES = [(B, H, W, dt) for (B, H, W) in [(2, 4, 128), (1, 6, 256)] for dt in (torch.float32, torch.float16)]


@functools.lru_cache(None)
def _rs_operands(B, H, W):
    g = _gen(700 + W)
    return dict(img=_rn(g, B, 3, H, W), w=_rn(g, 147, 64, scale=147 ** -0.5), b=_rn(g, 64, scale=0.5))


def resnet_stem_inputs(case):
    return _rs_operands(*case[:3])


def _rs_conv(img, w, b, mode="zeros"):
    wc = _conv_w(w, 64, 3, 7)
    if mode == "edge":
        return F.conv2d(F.pad(img, (3, 3, 3, 3), mode="replicate"), wc, b, stride=2).permute(0, 2, 3, 1).contiguous()
    return F.conv2d(img, wc, b, stride=2, padding=3).permute(0, 2, 3, 1).contiguous()


def resnet_stem_ref(I, case, mut=None, stored=True):
    """stored=False: the bound of the fp32 value in front of the store."""
    dt = case[3]
    p = _rs_conv(_d(I["img"]), _d(I["w"]), _d(I["b"]), "edge" if mut == "clamp_to_edge" else "zeros")
    a = _rs_conv(_d(I["img"]).abs(), _d(I["w"]).abs(), _d(I["b"]).abs())
    v = p.clamp_min(0)
    pre = (147 + 2) * U32 * a
    return v, pre + e_out(v, pre, dt) if stored else pre


def resnet_stem_f32(I, case):
    return F.relu(_rs_conv(I["img"], I["w"], I["b"]))


# ------------------------------------------------------------------------------------------------ gp_maxpool3x3s2 (exact)
MAXPOOL_CASES = [(B, H, W, C, dt) for (B, H, W, C) in [(2, 4, 6, 8), (1, 2, 2, 64), (2, 8, 8, 64)] for dt in (torch.float16, torch.float32)]


@functools.lru_cache(None)
def maxpool_inputs(case):
    B, H, W, C, dt = case
    # randn - 3: nearly every value is negative already; the handful in 8192 that is not is pulled below zero, so that EVERY window at
    # the border is all negative
    return dict(x=(_rn(_gen(800 + H), B, H, W, C) - 3).clamp_max(-2.0 ** -6).to(dt))


def maxpool_ref(I, case, mut=None):
    x = _d(I["x"]).permute(0, 3, 1, 2)
    v = F.max_pool2d(F.pad(x, (1, 1, 1, 1), value=0.0), 3, 2, 0) if mut == "zero_padding" else F.max_pool2d(x, 3, 2, 1)
    v = v.permute(0, 2, 3, 1).contiguous()
    return v, torch.zeros_like(v)


def maxpool_f32(I, case):
    return F.max_pool2d(I["x"].float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


def maxpool_border_windows_all_negative(I, case):
    """Every window that touches the padding holds only negative values (a pool padded with 0 then returns 0 there)."""
    v, _ = maxpool_ref(I, case)
    Ho, Wo = v.shape[1:3]
    border = torch.zeros(Ho, Wo, dtype=torch.bool)
    border[0, :] = True
    border[:, 0] = True                                               # even H, W: only the first window row / column is padded
    return bool((v[:, border] < 0).all())


# ------------------------------------------------------------------------------------------------ gp_patchify_xyz (exact)
PATCHIFY_CASES = [(B, R, P, dt) for (B, R, P) in [(2, 16, 8), (1, 8, 8), (2, 64, 8), (3, 12, 4)] for dt in (torch.float32, torch.float16)]


@functools.lru_cache(None)
def _patchify_operands(B, R):
    x = _rn(_gen(900 + R), B * R * R, 4)
    x[:, 3] = NAN
    return dict(xyz4=x)


def patchify_inputs(case):
    return _patchify_operands(*case[:2])


def patchify_ref(I, case, mut=None):
    """Flat buffer of the rows plus ONE tail value (SENTINEL): the form check_buffer takes, so that a kernel that stores the map's 4th
    channel -- every such store but the last is overwritten by the next pixel's first channel -- is seen at the end of the buffer."""
    B, R, P, dt = case
    n = R // P
    x = I["xyz4"].view(B, n, P, n, P, 4)
    perm = (0, 1, 3, 4, 2, 5) if mut == "ky_kx_swapped" else (0, 1, 3, 2, 4, 5)
    v = store(x.permute(*perm)[..., :3].reshape(B * n * n, P * P * 3), dt)
    if mut == "writes_fourth_channel":
        out = with_tail(v)
        out[-1] = NAN
        return out, torch.zeros_like(v)
    return v, torch.zeros_like(v)


def patchify_f32(I, case):
    B, R, P, dt = case
    n = R // P
    return I["xyz4"].view(B, n, P, n, P, 4).permute(0, 1, 3, 2, 4, 5)[..., :3].reshape(B * n * n, P * P * 3)


# ------------------------------------------------------------------------------------------------ gp_dwconv_ln_groups
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
DWG_B, DWG_HW = 5, 16
DWG_TABLES = [(0, 0, 2, 2, 2), (0, 1, 2, 3, 4), (0, 0, 0, 0, 0)]
DWG_CLAMP_TABLE, DWG_CLAMPED = (-1, 7, 2, 9, 2), (0, 1, 2, 3, 2)
DWG_CONFIGS = [(torch.float16, 256, 3, ACT_GELU), (torch.float16, 256, 7, ACT_NONE), (torch.float32, 64, 3, ACT_GELU)]
DWG_CASES = [cfg + (t,) for cfg in DWG_CONFIGS for t in DWG_TABLES] + [DWG_CONFIGS[0] + (DWG_CLAMP_TABLE,)]
DWG_EPS = 1e-6


@functools.lru_cache(None)
def _dwg_operands(dt, C, KS):
    g = _gen(1000 + C + KS)
    B, H = DWG_B, DWG_HW
    return dict(x=_rn(g, B, H, H, C).to(dt), wt=_rn(g, KS * KS, C, scale=1.0 / KS).to(dt), bias=_rn(g, C, scale=0.3), ln_w=1 + _rn(g, C, scale=0.3),
                ln_b=_rn(g, C, scale=0.3))


def dwg_inputs(case):
    return _dwg_operands(*case[:3])


def dwg_source_pixels(table, B, q, mut=None):
    """Flat full-resolution pixel of x behind every output row: row c q + j <- 4 g q + (c - g) q + j, g = table[c] clamped to [0, c]."""
    c = torch.arange(B * q) // q
    j = torch.arange(B * q) % q
    g = torch.tensor(table, dtype=torch.long)[c]
    if mut != "table_not_clamped":
        g = torch.minimum(g.clamp_min(0), c)
    if mut == "no_group_shift":
        g = torch.zeros_like(g)
    return (4 * g * q + (c - g) * q + j) % (4 * B * q)      # (an unclamped table leaves x: modelled as wrapping round)


@functools.lru_cache(None)
def _dwg_full(dt, C, KS, act):
    """The operation at every full-resolution pixel: (v, bound of the stored value, bound in front of the store) of shape (B H W, C)."""
    I = _dwg_operands(dt, C, KS)
    x, wt, b, lw, lb = (_d(I[k]) for k in ("x", "wt", "bias", "ln_w", "ln_b"))
    c = _dw_conv(x, wt, b, KS, 1).reshape(-1, C)
    e_c = (KS * KS + 1 + 2) * U32 * _dw_conv(x.abs(), wt.abs(), b.abs(), KS, 1).reshape(-1, C)
    E = e_c.max(1, keepdim=True).values
    mu = c.mean(1, keepdim=True)
    var = c.var(1, unbiased=False, keepdim=True)
    sigma = (var + DWG_EPS).sqrt()
    yh = (c - mu) / sigma
    e_stat = (C + 4) * U32 * (mu.abs() + (c * c).mean(1, keepdim=True).sqrt())
    z = lw * yh + lb
    e_lin = lw.abs() / sigma * (2 + yh.abs()) * (E + e_stat) + 4 * U32 * ((lw * yh).abs() + lb.abs())
    if act == ACT_GELU:
        v, pre = gelu_exact(z), 1.13 * e_lin + gelu_act_err(z, GELU_POLY2 if dt == torch.float16 else GELU_ERF)
    elif act == ACT_RELU:
        v, pre = z.clamp_min(0), e_lin
    else:
        v, pre = z, e_lin
    return v, pre + e_out(v, pre, dt), pre


def dwg_ref(I, case, mut=None, stored=True):
    dt, C, KS, act, table = case
    v, bound, pre = _dwg_full(dt, C, KS, act)
    src = dwg_source_pixels(table, DWG_B, DWG_HW * DWG_HW // 4, mut)
    return v[src], (bound if stored else pre)[src]


def dwg_f32(I, case):
    dt, C, KS, act, table = case
    c = _dw_conv(I["x"].float(), I["wt"].float(), I["bias"], KS, 1).reshape(-1, C)
    z = F.layer_norm(c, (C,), I["ln_w"], I["ln_b"], DWG_EPS)
    y = F.gelu(z) if act == ACT_GELU else F.relu(z) if act == ACT_RELU else z
    return y[dwg_source_pixels(table, DWG_B, DWG_HW * DWG_HW // 4)]


# ------------------------------------------------------------------------------------------------ registry
OPS = {o.name: o for o in [
    Op("gp_sn_stem", SN_STEM_CASES, sn_stem_inputs, sn_stem_ref, sn_stem_f32),
    Op("gp_sn_pointwise", SN_PW_CASES, sn_pw_inputs, sn_pw_ref, sn_pw_f32),
    Op("gp_sn_depthwise", SN_DW_CASES, sn_dw_inputs, sn_dw_ref, sn_dw_f32),
    Op("gp_sn_avgpool", SN_POOL_CASES, sn_pool_inputs, sn_pool_ref, sn_pool_f32),
    Op("gp_sn_se", SN_SE_CASES, sn_se_inputs, sn_se_ref, sn_se_f32),
    Op("gp_sn_head", SN_HEAD_CASES, sn_head_inputs, sn_head_ref, sn_head_f32),
    Op("gp_resnet_stem", RESNET_STEM_CASES, resnet_stem_inputs, resnet_stem_ref, resnet_stem_f32, functools.partial(resnet_stem_ref, stored=False)),
    Op("gp_maxpool3x3s2", MAXPOOL_CASES, maxpool_inputs, maxpool_ref, maxpool_f32),
    Op("gp_patchify_xyz", PATCHIFY_CASES, patchify_inputs, patchify_ref, patchify_f32),
    Op("gp_dwconv_ln_groups", DWG_CASES, dwg_inputs, dwg_ref, dwg_f32, functools.partial(dwg_ref, stored=False)),
]}

# the branch-coverage assertion is made per case where a case has at least this many values, and over the union of an operation's
# cases of one activation otherwise (a 1 x 1 map of 4 channels has 8 values)
BRANCH_MIN_VALUES = 32

# (operation, mutation, which cases must expose it)
MUTATIONS = [
    ("gp_sn_depthwise", "clamp_to_edge", lambda c: True),
    ("gp_resnet_stem", "clamp_to_edge", lambda c: True),
    ("gp_maxpool3x3s2", "zero_padding", lambda c: True),
    ("gp_sn_stem", "hs_no_upper_clamp", lambda c: True),
    ("gp_sn_stem", "hs_div_before_clamp", lambda c: True),
    ("gp_sn_pointwise", "hs_no_upper_clamp", lambda c: c[4] == 2 and c[0] * c[1] >= BRANCH_MIN_VALUES),
    ("gp_sn_pointwise", "hs_div_before_clamp", lambda c: c[4] == 2 and c[0] * c[1] >= BRANCH_MIN_VALUES),
    ("gp_sn_depthwise", "hs_no_upper_clamp", lambda c: c[6] == 2 and c[1] * c[2] * c[3] >= BRANCH_MIN_VALUES),
    ("gp_sn_depthwise", "hs_div_before_clamp", lambda c: c[6] == 2 and c[1] * c[2] * c[3] >= BRANCH_MIN_VALUES),
    ("gp_sn_pointwise", "res_before_act", lambda c: c[6] == 1 and c[4] != 0),
    ("gp_sn_pointwise", "se_row_plus_one", lambda c: c[5] == 1),
    ("gp_sn_avgpool", "padded_lane_divisor", lambda c: c[1] % 4 != 0),
    ("gp_sn_depthwise", "stride2_size_floor", lambda c: c[5] == 2 and (c[1] % 2 == 1 or c[2] % 2 == 1)),
    ("gp_sn_head", "one_hot_before_line1", lambda c: True),
    ("gp_sn_head", "roi_wh_not_scaled", lambda c: c[3] == 1),
    ("gp_sn_head", "use_hw0_reads_roi_wh", lambda c: c[3] == 0),
    ("gp_patchify_xyz", "writes_fourth_channel", lambda c: True),
    ("gp_patchify_xyz", "ky_kx_swapped", lambda c: True),
    ("gp_dwconv_ln_groups", "no_group_shift", lambda c: any(c[4])),
    ("gp_dwconv_ln_groups", "table_not_clamped", lambda c: c[4] == DWG_CLAMP_TABLE),
]


def case_dtype(case):
    """Storage type of a case's output (fp32 where the case names none)."""
    return next((x for x in case if isinstance(x, torch.dtype)), torch.float32)


def case_id(case):
    def one(x):
        if isinstance(x, torch.dtype):
            return "f16" if x == torch.float16 else "f32"
        if isinstance(x, tuple):
            return "t" + "".join(str(v) for v in x).replace("-", "m")
        return str(x)
    return "-".join(one(x) for x in case)
