"""Float64 references, per-element error bounds and the shared input sets of the small fp32 kernels that the network tests only reach
end to end: csrc/scalenet.hip (gp_sn_*), gp_resnet_stem / gp_maxpool3x3s2 / gp_patchify_xyz (csrc/misc.hip) and gp_dwconv_ln_groups
(csrc/norm.hip) -- and, in the second half, of the kernels at the network's entry and exits (gp_convnext_stem ... gp_groupnorm_apply_xyz).
No GPU here: tests/test_ops_reference_cpu.py checks this file against itself, tests/test_scalenet_ops_gpu.py,
tests/test_misc_ops_conformance.py and tests/test_head_ops_conformance_gpu.py hold the kernels against it.

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


# ================================================================================================ head entry and exit kernels
# gp_convnext_stem, gp_deconv_col2im, gp_xyz_out_layer, gp_pointwise_k3, the tiny-Cin 3x3 s2 convolutions, gp_pool_mmm, gp_size_head,
# gp_pose_tail(_rt), gp_attention64(_hd) (csrc/misc.hip) and gp_groupnorm_apply_xyz (csrc/norm.hip), held by
# tests/test_head_ops_conformance_gpu.py.  Where the kernel stores fp32 values computed from fp16 operands the case names the operand
# type as a string ("f16"), so that case_dtype() -- the type of the STORE -- stays fp32.
f16, f32 = torch.float16, torch.float32
DT = {"f16": f16, "f32": f32}
SPLIT = 2.0 ** -22


def cdiv(a, b):
    return (a + b - 1) // b


def split_err(a, sum_x, sum_w):
    """What the fp16 hi + lo split of both fp32 operands of an MFMA form adds to (n + 2) u a (stem_mfma_kernel,
    smallcin_conv3x3s2_mfma_kernel: x_hi w_hi + x_lo w_hi + x_hi w_lo in fp32).  hi = fp16(x), lo = fp16(x - hi), |x - hi| <= 2^-11 |x|:
      the dropped x_lo w_lo                       <= 2^-22 |x||w| per term
      the fp16 rounding of x_lo (times |w_hi|)    <= 2^-11 |x - hi| |w| <= 2^-22 |x||w|, or half a subnormal step 2^-25 |w| when x - hi lies
                                                   below fp16's normal range (|x| < 2^-3)
      the fp16 rounding of w_lo (times |x_hi|)    the same with x and w exchanged
    -> 3 x 2^-22 a + 2^-25 (sum |x| + sum |w|) over the terms of the output.  Nothing of order 2^-11 |x||w|: an operand that is only
    rounded to fp16 (a lo part left out) is outside this bound."""
    return 3 * SPLIT * a + 2.0 ** -25 * (sum_x + sum_w)


# ------------------------------------------------------------------------------------------------ gp_convnext_stem
STEM_C0 = 128
STEM_LARGE = (2, 512, 1024, f16, 1e-6)           # stem_mfma_kernel<4> starts at 256 workgroups: 8.4 M values, the one LARGE case
STEM_CASES = [(2, 8, 192, f32, 1e-6),             # stem_kernel<float>, PXB 16, three column blocks
              (1, 12, 256, f32, 1e-6),            # stem_kernel<float>, PXB 64
              (2, 8, 128, f16, 1e-6),             # stem_kernel<half>, PXB 16
              (2, 12, 256, f16, 0.25),            # stem_mfma_kernel<1>: H / 4 = 3 is no multiple of 4; eps 0.25
              (3, 16, 512, f16, 1e-6),            # stem_mfma_kernel<1>: H / 4 = 4 but 6 four-row workgroups; two column blocks
              STEM_LARGE]                         # stem_mfma_kernel<4>: 2 crops x 32 row groups x 4 column blocks = 256 workgroups
STEM_FORMS = {"stem<float,PXB 16>", "stem<float,PXB 64>", "stem<half,PXB 16>", "stem_mfma<1>", "stem_mfma<4>"}
STEM_ENV = ("GP_STEM_MFMA", "GP_STEM_RPW")


def stem_geometry(case):
    """(form, PXB, output rows per workgroup): gp_convnext_stem's routing restated, with GP_STEM_MFMA / GP_STEM_RPW unset."""
    B, H, W, dt, eps = case
    pxb = 64 if (W // 4) % 64 == 0 else 16
    if dt == f16 and pxb == 64:
        if (H // 4) % 4 == 0 and B * (H // 16) * (W // 4 // 64) >= 256:
            return "stem_mfma<4>", 64, 4
        return "stem_mfma<1>", 64, 1
    return f"stem<{'half' if dt == f16 else 'float'},PXB {pxb}>", pxb, 1


def stem_form(case):
    return stem_geometry(case)[0]


@functools.lru_cache(None)
def _stem_operands(B, H, W):
    g = _gen(1100 + 3 * H + W + 7 * B)
    off = torch.tensor([2.0, -2.0, 1.7]).view(1, 3, 1, 1)              # normalised crops: a per-channel offset of about +-2
    return dict(img=_rn(g, B, 3, H, W) + off, w=_rn(g, 48, STEM_C0, scale=48 ** -0.5), b=_rn(g, STEM_C0, scale=0.1),
                ln_w=1 + (torch.rand(STEM_C0, generator=g) * 2 - 1) * 0.3, ln_b=(torch.rand(STEM_C0, generator=g) * 2 - 1) * 0.3)


def stem_inputs(case):
    return _stem_operands(*case[:3])


def _stem_patches(img):
    """(B, 3, H, W) -> (B H/4 W/4, 48) with k = c 16 + kh 4 + kw, the row order of the (48, 128) tap matrix."""
    B, _, H, W = img.shape
    return img.reshape(B, 3, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(-1, 48)


def _stem_compute(case, mut=None):
    """conv 4x4 s4 (48 terms + bias) chained into the LayerNorm over the 128 channels (both forms are two-pass: mean, then centred
    squares), as norm_reference.dw_ref chains its depth-wise conv.  VALU forms: e_c = (48 + 2) u a.  MFMA forms: K is padded to 64 and
    three products are accumulated per term, 192 fp32 additions at most, e_c = (192 + 2) u a + split_err."""
    import norm_reference as NR
    B, H, W, dt, eps = case
    I = stem_inputs(case)
    form, pxb, rpw = stem_geometry(case)
    w, b, lw, lb = (_d(I[k]) for k in ("w", "b", "ln_w", "ln_b"))
    P = _stem_patches(I["img"].half().double() if mut == "x_lo_dropped" else _d(I["img"]))
    if mut == "w_lo_dropped":
        w = w.half().double()
    c = P @ w + b
    mu, sigma, yh, z = NR._ln(c, lw, lb, eps, "unbiased_variance" if mut == "variance_over_127" else None)
    if mut == "column_block_from_row_factor":
        # block index i = (b nh + row group) nwb + column block; the mutant takes its column block as (i / nwb) % nwb and writes where it should
        Ho, Wo = H // 4, W // 4
        nh, nwb = Ho // rpw, Wo // pxb
        bi, ho, wo = torch.arange(B).view(B, 1, 1), torch.arange(Ho).view(1, Ho, 1), torch.arange(Wo).view(1, 1, Wo)
        src = ((bi * nh + ho // rpw) % nwb) * pxb + wo % pxb
        return z.view(B, Ho, Wo, STEM_C0)[bi, ho, src].reshape(-1, STEM_C0), None, None
    if mut is not None:
        return z, None, None
    a = P.abs() @ w.abs() + b.abs()
    if form.startswith("stem_mfma"):
        e_c = (192 + 2) * U32 * a + split_err(a, P.abs().sum(1, keepdim=True), w.abs().sum(0))
    else:
        e_c = (48 + 2) * U32 * a
    pre = NR._ln_bound(c, e_c.max(1, keepdim=True).values, mu, sigma, yh, lw, lb, False)
    return z, pre + e_out(z, pre, dt), pre


_stem_small = functools.lru_cache(None)(_stem_compute)
_stem_large = functools.lru_cache(1)(_stem_compute)


def stem_ref(I, case, mut=None, stored=True):
    if mut is not None:
        return _stem_compute(case, mut)[0], None
    v, bound, pre = (_stem_large if case == STEM_LARGE else _stem_small)(case)
    return v, bound if stored else pre


def stem_f32(I, case):
    wc = I["w"].t().reshape(STEM_C0, 3, 4, 4)
    c = F.conv2d(I["img"], wc, I["b"], stride=4).permute(0, 2, 3, 1)
    return F.layer_norm(c, (STEM_C0,), I["ln_w"], I["ln_b"], case[4]).reshape(-1, STEM_C0)


# ------------------------------------------------------------------------------------------------ gp_deconv_col2im
# case: (B, H, W, C, output type, type of the column matrix)
COL2IM_CASES = [(B, H, W, C, odt, cdt) for (B, H, W, C) in [(2, 3, 5, 8), (1, 8, 8, 256)] for (odt, cdt) in [(f32, f32), (f16, f32), (f16, f16)]]
COL2IM_FORMS = {"col2im<float,float>", "col2im<half,float>", "col2im<half,half>"}


def col2im_form(case):
    n = {f16: "half", f32: "float"}
    return f"col2im<{n[case[4]]},{n[case[5]]}>"


@functools.lru_cache(None)
def _col2im_operands(B, H, W, C, cdt):
    return dict(cols=_rn(_gen(1200 + H + C), B * H * W, 9 * C).to(cdt))


def col2im_inputs(case):
    return _col2im_operands(*case[:4], case[5])


def col2im_sum(cols, case, mut=None):
    """(out (B, 2H, 2W, C), summands per output pixel (2H, 2W)) in cols' own type: out[b][2i-1+ky][2j-1+kx] += cols[(b, i, j)][ky 3 + kx]."""
    B, H, W, C = case[:4]
    c = cols.view(B, W, H, 9, C).transpose(1, 2) if mut == "h_w_swapped" else cols.view(B, H, W, 9, C)
    out = torch.zeros(B, 2 * H, 2 * W, C, dtype=cols.dtype)
    cnt = torch.zeros(2 * H, 2 * W, dtype=torch.long)
    i, j = torch.arange(H), torch.arange(W)
    for ky in range(3):
        mi = 2 * i - 1 + ky >= 0
        if mut == "last_row_clipped":                  # `i >= H - 1` for `i >= H`: the last input row never arrives
            mi = mi & (i < H - 1)
        for kx in range(3):
            mj = 2 * j - 1 + kx >= 0
            oy, ox = (2 * i - 1 + ky)[mi].view(-1, 1), (2 * j - 1 + kx)[mj].view(1, -1)
            out[:, oy, ox] += c[:, i[mi].view(-1, 1), j[mj].view(1, -1), ky * 3 + kx]
            cnt[oy, ox] += 1
    return out, cnt


def col2im_ref(I, case, mut=None, stored=True):
    """n = the summands that exist for the pixel (1, 2 or 4; fp16 columns: the rounded values), added in fp32 from 0: (n + 2) u a."""
    B, H, W, C, odt, cdt = case
    v, cnt = col2im_sum(_d(I["cols"]), case, mut)
    a, _ = col2im_sum(_d(I["cols"]).abs(), case)
    pre = ((cnt + 2).double() * U32).view(1, 2 * H, 2 * W, 1) * a
    v, pre = v.reshape(-1, C), pre.reshape(-1, C)
    return v, pre + e_out(v, pre, odt) if stored else pre


def col2im_f32(I, case):
    return col2im_sum(I["cols"].float(), case)[0].reshape(-1, case[3])


def col2im_summand_counts(case):
    """{summands: pixels}; odd output rows / columns but the last have two source rows / columns, every other one has one."""
    _, cnt = col2im_sum(torch.zeros(case[0] * case[1] * case[2], 9 * case[3], dtype=F64), case)
    return {int(n): int((cnt == n).sum()) for n in cnt.unique()}


# ------------------------------------------------------------------------------------------------ gp_xyz_out_layer
# case: (B, HW, C, operand type).  v is ONE flat buffer [NCHW (B, 3, HW) | (rows, 4) map whose 4th column is exactly 0].
XYZ_OUT_CASES = [(3, 35, 4, "f32"), (3, 35, 256, "f32"), (3, 35, 256, "f16"), (3, 35, 1024, "f16")]


def xyz_out_geometry(case):
    """(form, lanes per pixel, pixels per wave, trips of the chunk loop, rows in the last workgroup) of xyz_out_kernel."""
    B, HW, C, dts = case
    chunks = C // (8 if dts == "f16" else 4)
    lpp = min(chunks, 64)
    ppw = 64 // lpp
    return f"xyz_out<{dts}>", lpp, ppw, cdiv(chunks, lpp), (B * HW) % (4 * ppw)


@functools.lru_cache(None)
def _xyz_out_operands(B, HW, C, dts):
    g = _gen(1300 + C)
    return dict(x=_rn(g, B, HW, C).to(DT[dts]), w=_rn(g, 3, C, scale=C ** -0.5), b=_rn(g, 3))


def xyz_out_inputs(case):
    return _xyz_out_operands(*case)


def xyz_pack(y3, B, HW, mut=None):
    """(rows, 3) -> the flat [NCHW | (rows, 4)] buffer."""
    rows = B * HW
    if mut == "nchw_rows_for_hw":          # b = row / rows, pix = row - b rows: value c of row r lands at c rows + r
        nchw = y3.t().reshape(-1)
    else:
        nchw = y3.view(B, HW, 3).permute(0, 2, 1).reshape(-1)
    return torch.cat([nchw, torch.cat([y3, torch.zeros(rows, 1, dtype=y3.dtype)], 1).reshape(-1)])


def xyz_out_ref(I, case, mut=None):
    B, HW, C, dts = case
    x, w, b = _d(I["x"]).reshape(-1, C), _d(I["w"]), _d(I["b"])
    if mut == "chunk_loop_runs_once":      # 64 lanes x one 16-byte chunk: the channels behind them never arrive
        keep = min(C, 64 * (8 if dts == "f16" else 4))
        x = torch.cat([x[:, :keep], torch.zeros_like(x[:, keep:])], 1)
    y = x @ w.t() + b
    e = (C + 2) * U32 * (x.abs() @ w.abs().t() + b.abs()) + U32 * y.abs()
    return xyz_pack(y, B, HW, mut), xyz_pack(e, B, HW)


def xyz_out_f32(I, case):
    B, HW, C, dts = case
    return xyz_pack(I["x"].float().reshape(-1, C) @ I["w"].t() + I["b"], B, HW)


# ------------------------------------------------------------------------------------------------ gp_pointwise_k3
def _pk3_cases():
    out = []
    for Cout, dt in ((4, f32), (256, f32), (1024, f32), (256, f16)):
        pg = 256 // (Cout // (8 if dt == f16 else 4))
        out += [(rows, Cout, dt) for rows in (1, 8 * pg - 1, 8 * pg + 1)]
    return out


PK3_CASES = _pk3_cases()


def pk3_geometry(case):
    """(form, pixel groups per workgroup PG, workgroups, rows of the last workgroup) of pointwise_k3_kernel."""
    rows, Cout, dt = case
    pg = 256 // (Cout // (8 if dt == f16 else 4))
    return f"pointwise_k3<{'half' if dt == f16 else 'float'}>", pg, cdiv(rows, 8 * pg), rows % (8 * pg)


@functools.lru_cache(None)
def _pk3_operands(rows, Cout):
    g = _gen(1400 + Cout + rows)
    xyz4 = _rn(g, rows, 4)
    xyz4[:, 3] = 7.0                        # the map's 4th column is storage, not an operand
    return dict(xyz4=xyz4, w=_rn(g, Cout, 3), b=_rn(g, Cout))


def pk3_inputs(case):
    return _pk3_operands(*case[:2])


def pk3_ref(I, case, mut=None, stored=True):
    rows, Cout, dt = case
    x, w, b = _d(I["xyz4"])[:, :3], _d(I["w"]), _d(I["b"])
    if mut == "w_transposed":
        w = w.reshape(3, Cout).t()
    v = x @ w.t() + b
    if mut == "row_tail_dropped":
        v = v.clone()
        v[rows // (8 * pk3_geometry(case)[1]) * 8 * pk3_geometry(case)[1]:] = NAN
    pre = (3 + 2) * U32 * (x.abs() @ w.abs().t() + b.abs())
    return v, pre + e_out(v, pre, dt) if stored else pre


def pk3_f32(I, case):
    return I["xyz4"][:, :3] @ I["w"].t() + I["b"]


# ------------------------------------------------------------------------------------------------ tiny-Cin 3x3 s2 convolutions
# gp_xyz_conv3x3_s2 (CIN 3), gp_pnp_conv1 (CIN 5: + roi_coord_2d), gp_pnp_conv1_masked (CIN 5, x * mask before the conv).
# case: (B, R, Cout, output type)
SMALLCIN_CASES = [(B, R, Cout, dt) for (B, R, Cout) in [(3, 8, 4),          # both column edges in one pixel quad, 12 quads in a block of 256
                                                         (3, 24, 128), (1, 16, 256)] for dt in (f32, f16)] + \
                 [(2, 64, 128, f16), (2, 64, 256, f16)]                      # the MFMA form: fp16, R = 64
SMALLCIN_CIN = {"gp_xyz_conv3x3_s2": 3, "gp_pnp_conv1": 5, "gp_pnp_conv1_masked": 5}
SMALLCIN_ENV = ("GP_SMALLCIN_MFMA",)


def smallcin_form(name, case):
    B, R, Cout, dt = case
    cin = SMALLCIN_CIN[name]
    if dt == f16 and R == 64 and Cout in (128, 256):
        return f"smallcin_mfma<{cin},{Cout // 64}>"
    return f"smallcin<{'half' if dt == f16 else 'float'},{cin}>"


SMALLCIN_FORMS = {n: {f"smallcin<{t},{c}>" for t in ("half", "float")} | {f"smallcin_mfma<{c},{k}>" for k in (2, 4)} for n, c in SMALLCIN_CIN.items()}


@functools.lru_cache(None)
def _smallcin_operands(B, R, Cout, cin):
    g = _gen(1500 + R + Cout + cin)
    xyz4 = _rn(g, B * R * R, 4)
    xyz4[:, 3] = 7.0
    m = torch.rand(B, R, R, generator=g)
    m = torch.where(torch.rand(B, R, R, generator=g) < 0.15, torch.zeros_like(m), m.clamp(0.01, 0.99))      # soft, with exact zeros
    return dict(xyz4=xyz4, coord2d=_rn(g, B, 2, R, R), w=_rn(g, cin * 9, Cout, scale=(9 * cin) ** -0.5), mask=m)


def smallcin_inputs(name, case):
    return _smallcin_operands(*case[:3], SMALLCIN_CIN[name])


def _smallcin_x(I, name, case, dtype, mut=None):
    """The (B, CIN, R, R) operand of the convolution; masked: x * m rounded ONCE to fp32, as the kernels do before they convolve / split."""
    B, R = case[:2]
    x = I["xyz4"][:, :3].view(B, R, R, 3).permute(0, 3, 1, 2)
    if SMALLCIN_CIN[name] == 5:
        c2 = I["coord2d"].flip(1) if mut == "coord2d_swapped" else I["coord2d"]
        x = torch.cat([x, c2], 1)
    if name.endswith("masked"):
        m = I["mask"].view(B, 1, R, R)
        x = torch.cat([x[:, :3] * m, x[:, 3:]], 1) if mut == "mask_on_xyz_only" else x * m          # fp32 products
    return x.to(dtype)


def _smallcin_conv(x, w, Cout, mut=None):
    wc = w.t().reshape(Cout, -1, 3, 3)
    if mut == "window_one_column_right":
        # (an even R never reads the right padding: `padding 0 at the right edge` changes nothing.  The error that does is the window
        # anchored one column to the right, the zero column behind the right edge instead of in front of the left one.)
        return F.conv2d(F.pad(x, (0, 2, 1, 1)), wc, None, stride=2)[..., :x.shape[-1] // 2].permute(0, 2, 3, 1)
    return F.conv2d(x, wc, None, stride=2, padding=1).permute(0, 2, 3, 1)


def smallcin_ref(name, I, case, mut=None, stored=True):
    """27 / 45 terms from 0: (n + 2) u a.  MFMA form: K is padded to 96 and three products are accumulated per term, (288 + 2) u a + split_err."""
    B, R, Cout, dt = case
    cin = SMALLCIN_CIN[name]
    x, w = _smallcin_x(I, name, case, F64, mut), _d(I["w"])
    if mut == "x_lo_dropped":
        x = x.half().double()
    v = _smallcin_conv(x, w, Cout, mut).reshape(-1, Cout)
    xa = _smallcin_x(I, name, case, F64).abs()
    a = _smallcin_conv(xa, w.abs(), Cout).reshape(-1, Cout)
    if smallcin_form(name, case).startswith("smallcin_mfma"):
        sx = F.conv2d(xa, torch.ones(1, cin, 3, 3, dtype=F64), None, stride=2, padding=1).reshape(-1, 1)
        pre = (288 + 2) * U32 * a + split_err(a, sx, w.abs().sum(0))
    else:
        pre = (9 * cin + 2) * U32 * a
    return v, pre + e_out(v, pre, dt) if stored else pre


def smallcin_f32(name, I, case):
    return _smallcin_conv(_smallcin_x(I, name, case, f32), I["w"], case[2]).reshape(-1, case[2])


# ------------------------------------------------------------------------------------------------ gp_pool_mmm
# case: (k, C, HW, type), B = 3: out (B, k C) = [mean | max | min][:k] over the HW pixels
POOL_B = 3
POOL_CASES = [(k, C, HW, dt) for k in (1, 2, 3) for (C, dt) in [(8, f16), (128, f16), (512, f16), (4, f32), (256, f32)] for HW in (1, 3, 64, 67)]


def pool_geometry(case):
    """(form, pixel groups G of the workgroup, groups that see no pixel) of pool_mmm_kernel."""
    k, C, HW, dt = case
    G = 256 // (C // (8 if dt == f16 else 4))
    return f"pool_mmm<{'half' if dt == f16 else 'float'}>", G, max(G - HW, 0)


@functools.lru_cache(None)
def _pool_operands(C, HW, dt):
    x = _rn(_gen(1600 + C + HW), POOL_B, HW, C)
    x[..., 0] = -x[..., 0].abs() - 0.5        # one channel negative everywhere, one positive everywhere: an initial maximum
    x[..., 1] = x[..., 1].abs() + 0.5         # (minimum) of 0 is seen
    return dict(x=x.to(dt))


def pool_inputs(case):
    return _pool_operands(*case[1:])


def pool_ref(I, case, mut=None, stored=True):
    """Maximum and minimum are exact (bound 0: the operand's bits); the mean is a sum of HW terms, (HW + 2) u sum |x| / HW."""
    k, C, HW, dt = case
    x = _d(I["x"])
    mx, mn = x.max(1).values, x.min(1).values
    if mut == "max_initial_0":
        mx = mx.clamp_min(0)
    if mut == "min_initial_0":
        mn = mn.clamp_max(0)
    mean = x.sum(1) / HW
    pm = (HW + 2) * U32 * x.abs().sum(1) / HW
    z = torch.zeros_like(mx)
    v = torch.cat([mean, mx, mn][:k], 1)
    return v, torch.cat([pm + e_out(mean, pm, dt) if stored else pm, z, z][:k], 1)


def pool_f32(I, case):
    x = I["x"].float()
    return torch.cat([x.mean(1), x.max(1).values, x.min(1).values][:case[0]], 1)


# ------------------------------------------------------------------------------------------------ gp_size_head
# case: (B, HW, C, F, operand type): max over HW -> fc1 (C terms, BatchNorm folded, ReLU) -> fc2 (F terms) + mean_size / |mean_size|
SIZE_CASES = [(3, 1, 1024, 128, "f32"), (2, 64, 1024, 128, "f32"), (2, 64, 1024, 128, "f16"),
              (2, 5, 260, 16, "f32")]                # C 260: a second blockIdx.y block of size_pool_kernel with ONE live lane


def size_geometry(case):
    """(form, blockIdx.y blocks of the pool, live lanes of its last block, pixel quarters that see no pixel)."""
    B, HW, C, Fh, dts = case
    return f"size_pool<{dts}>", cdiv(C, 256), (C - (cdiv(C, 256) - 1) * 256) // 4, max(4 - HW, 0)


@functools.lru_cache(None)
def _size_operands(B, HW, C, Fh, dts):
    g = _gen(1700 + C + HW)
    feat = _rn(g, B, HW, C)
    feat[..., ::5] = -feat[..., ::5].abs() - 0.25                      # every fifth channel is negative everywhere
    ms = (torch.rand(B, 3, generator=g) + 0.2) * torch.tensor([0.3, 1.0, 2.5])[:B].view(B, 1)     # rows of different norms
    return dict(feat=feat.to(DT[dts]), w1=_rn(g, Fh, C, scale=C ** -0.5), b1=_rn(g, Fh, scale=0.3), w2=_rn(g, 3, Fh, scale=Fh ** -0.5),
                b2=_rn(g, 3, scale=0.3), mean_size=ms)


def size_inputs(case):
    return _size_operands(*case)


def size_ref(I, case, mut=None):
    """The pool is exact.  fc1 (C + 2) u a1; fc2 carries it through |w2| beside its own (F + 2) u a2 (chained layers).  r = ms / |ms|: sum of
    squares, sqrtf and the division, 2 u + u + u relative; then the two additions and the store."""
    B, HW, C, Fh, dts = case
    feat, w1, b1, w2, b2, ms = (_d(I[k]) for k in ("feat", "w1", "b1", "w2", "b2", "mean_size"))
    p = feat.max(1).values
    if mut == "max_initial_0":
        p = p.clamp_min(0)
    h = (p @ w1.t() + b1).clamp_min(0)
    e1 = (C + 2) * U32 * (p.abs() @ w1.abs().t() + b1.abs())
    y = h @ w2.t() + b2
    e2 = (Fh + 2) * U32 * ((h + e1) @ w2.abs().t() + b2.abs()) + e1 @ w2.abs().t()
    r = ms if mut == "mean_size_not_normalised" else ms / ms.norm(dim=1, keepdim=True)
    v = y + r
    return v, e2 + 4 * U32 * r.abs() + 2 * U32 * (y.abs() + r.abs()) + U32 * v.abs()


def size_f32(I, case):
    p = I["feat"].float().max(1).values
    h = F.relu(p @ I["w1"].t() + I["b1"])
    return h @ I["w2"].t() + I["b2"] + I["mean_size"] / I["mean_size"].norm(dim=1, keepdim=True)


# ------------------------------------------------------------------------------------------------ gp_attention64 / gp_attention64_hd
# case: (B, heads, head_dim, type): qkv (B, 64, 3 heads HD) -> softmax(q k^T HD^-0.5) v, (B, 64, heads HD)
ATT_CASES_HD = [(B, heads, HD, dt) for HD in (24, 32) for (B, heads) in [(1, 1), (3, 8)] for dt in (f32, f16)]
ATT_CASES_32 = [c for c in ATT_CASES_HD if c[2] == 32]
ATT_PEAK = 20.0
# expf: 1 ulp, the figure of the HIP math API's accuracy table for the single-precision exp (the build has no fast-math flag, so
# expf is the library function); 1 ulp = 2^-23 relative
EXPF_ULP = 1
EXPF_ERR = EXPF_ULP * 2.0 ** -23


def att_form(case):
    return f"attention64<{'half' if case[3] == f16 else 'float'},{case[2]}>"


@functools.lru_cache(None)
def _att_operands(B, heads, HD, dt):
    """Even query rows are PEAKED: q_i = tau k_t with t one of the 32 keys of the head that stand out most from the other keys, tau such that
    score t is 25 above every other one (ATT_PEAK = 20 is asserted on the rounded operands).  Odd rows are FLAT: q = 0.05 randn."""
    g = _gen(1800 + 3 * HD + heads)
    q, k, v = (_rn(g, B, 64, heads, HD) for _ in range(3))
    q = q * 0.05
    kh = k.double().permute(0, 2, 1, 3)                                                               # (B, heads, 64, HD)
    kk = kh @ kh.transpose(-1, -2) * HD ** -0.5
    diag = kk.diagonal(dim1=-2, dim2=-1)
    gap = diag - (kk - torch.diag_embed(torch.full_like(diag, float("inf")))).max(-1).values          # (B, heads, 64), per target key
    gap, t = gap.topk(32, -1)
    assert bool((gap > 0.5).all())
    q.permute(0, 2, 1, 3)[:, :, 0::2] = (kh.gather(2, t.unsqueeze(-1).expand(-1, -1, -1, HD)) * (25.0 / gap).unsqueeze(-1)).float()
    C = heads * HD
    return dict(qkv=torch.cat([q.reshape(B, 64, C), k.reshape(B, 64, C), v.reshape(B, 64, C)], -1).to(dt))


def att_inputs(case):
    return _att_operands(*case)


def _att_split(qkv, heads, HD):
    B = qkv.shape[0]
    return (t.reshape(B, 64, heads, HD).permute(0, 2, 1, 3) for t in qkv.chunk(3, -1))


def att_scores(I, case, mut=None):
    B, heads, HD, dt = case
    q, k, v = _att_split(_d(I["qkv"]), heads, HD)
    scale = (32 if mut == "scale_of_hd32" else 24 if mut == "scale_of_hd24" else HD) ** -0.5
    s, a = q @ k.transpose(-1, -2) * scale, q.abs() @ k.abs().transpose(-1, -2) * scale
    return (s.transpose(-1, -2) if mut == "scores_transposed" else s), a, v


def att_ref(I, case, mut=None, stored=True):
    """scores   s = sum q' k with q' = fl(q fl(HD^-0.5)): HD fmas from 0 and the two roundings of q': e_s = (HD + 4) u a_s
    exp      of t = fl(s' - max'): the shift cancels between numerator and denominator whatever its value, so the argument is off by
             d = e_s + u |s - max|; exp(t) (1 + EXPF_ERR).  Relative error of the numerator d (1 + d / 2 + ...) + EXPF_ERR
    sum      of 64 positive terms, each with its own relative error: their p-weighted mean, + (64 + 2) u;  inv = 1.0f / sum: u; p = e inv: u
             r = 1.01 (d + sum_l p_l d_l) + 2 EXPF_ERR + (64 + 4) u       (1.01: the second order of exp(d), d < 0.01)
    output   64 fmas from 0: sum_j p_j r_j |v_j| + (64 + 2) u sum_j p_j |v_j|."""
    B, heads, HD, dt = case
    s, a_s, v = att_scores(I, case, mut)
    p = torch.softmax(s, -1)
    if mut == "v_at_query_index":
        o = v.clone()
    else:
        o = p @ v
    d = (HD + 4) * U32 * a_s + U32 * (s - s.max(-1, keepdim=True).values).abs()
    r = 1.01 * (d + (p * d).sum(-1, keepdim=True)) + 2 * EXPF_ERR + (64 + 4) * U32
    pre = (p * r) @ v.abs() + (64 + 2) * U32 * (p @ v.abs())
    o, pre = (t.permute(0, 2, 1, 3).reshape(B * 64, heads * HD) for t in (o, pre))
    return o, pre + e_out(o, pre, dt) if stored else pre


def att_f32(I, case):
    B, heads, HD, dt = case
    q, k, v = _att_split(I["qkv"].float(), heads, HD)
    o = torch.softmax((q * HD ** -0.5) @ k.transpose(-1, -2), -1) @ v
    return o.permute(0, 2, 1, 3).reshape(B * 64, heads * HD)


def att_row_kinds(I, case):
    """(smallest lead of the top score over the rest on the even rows, largest probability on the odd rows)."""
    s, _, _ = att_scores(I, case)
    top = s.topk(2, -1).values
    return float((top[..., 0] - top[..., 1])[..., 0::2].min()), float(torch.softmax(s, -1)[..., 1::2, :].max())


# ------------------------------------------------------------------------------------------------ gp_pose_tail / gp_pose_tail_rt
# case: (rot_kind, rot_dim, is_allo, site, wild6d, ldh), B = 5.  v = [pred_rot (rot_dim) | pred_t (3)] per crop: three fc layers of 256 terms.
# The decode (rot_allo, rot_ego, trans) has no static bound: pose_decode() in float64 and float32, compared by the yardstick rule.
ROT_6D, ROT_6D_Y, ROT_6D_Z, ROT_QUAT, ROT_EULER = range(5)
ROT_NAMES = {ROT_6D: "rot6d", ROT_6D_Y: "rot6d_y", ROT_6D_Z: "rot6d_z", ROT_QUAT: "quat", ROT_EULER: "euler"}
POSE_B, POSE_ON_AXIS = 5, 2
POSE_CASES = [(kind, 4 if kind == ROT_QUAT else 6, allo, site, wild, ldh) for kind in range(5) for allo in (1, 0) for site in (1, 0) for wild in (0, 1)
              for ldh in (256, 260)]
POSE_GOLDEN_CALL = (ROT_6D, 6, 1, 1, 0, 256)       # what gp_pose_tail forwards


def pose_form(case):
    return f"pose_tail<{case[1]}>"


@functools.lru_cache(None)
def _pose_operands(RD, ldh):
    """Dense fc weights (logits of scale 1); fc_z's bias keeps the depth positive.  cam_K differs per crop (wild6d scales by crop 0's fx).
    Crop POSE_ON_AXIS has roi_wh = 0 and its bbox centre on the principal point: its ray is (0, 0, 1) exactly, whatever fc_t says."""
    g = _gen(1900 + RD + ldh)
    B = POSE_B
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = 577.5 + 31.0 * torch.arange(B)
    K[:, 1, 1] = 580.0 + 17.0 * torch.arange(B)
    K[:, 0, 2] = 319.5 + 3.0 * torch.arange(B)
    K[:, 1, 2] = 239.5 - 2.0 * torch.arange(B)
    K[:, 2, 2] = 1.0
    bbox = torch.stack([K[:, 0, 2] + 60.0 * (torch.arange(B) - 2.2), K[:, 1, 2] - 35.0 * (torch.arange(B) - 1.7)], 1)
    wh = torch.rand(B, 2, generator=g) * 80 + 40
    bbox[POSE_ON_AXIS], wh[POSE_ON_AXIS] = K[POSE_ON_AXIS, :2, 2], 0.0
    return dict(h=_rn(g, B, ldh), hz=_rn(g, B, ldh, scale=0.5), w_r=_rn(g, RD, 256, scale=1 / 16), b_r=_rn(g, RD, scale=0.1),
                w_t=_rn(g, 2, 256, scale=1 / 64), b_t=_rn(g, 2, scale=0.05), w_z=_rn(g, 1, 256, scale=1 / 64), b_z=torch.tensor([1.5]),
                cam_K=K.reshape(B, 9), bbox_center=bbox, resize_ratio=torch.rand(B, generator=g) + 0.8, roi_wh=wh)


def pose_inputs(case):
    return _pose_operands(case[1], case[5])


def pose_fc(I, case, dtype, mut=None):
    """(o (B, rot_dim + 3), the same on absolute values) in `dtype`."""
    RD, ldh = case[1], case[5]
    h, hz = I["h"].to(dtype), I["hz"].to(dtype)
    if mut == "ldh_taken_as_256":
        h, hz = (t.reshape(-1)[:POSE_B * 256].view(POSE_B, 256) for t in (h, hz))
    h, hz = h[:, :256], hz[:, :256]
    if mut == "fc_z_reads_h":
        hz = h
    wr, br, wt, bt, wz, bz = (I[k].to(dtype) for k in ("w_r", "b_r", "w_t", "b_t", "w_z", "b_z"))
    o = torch.cat([h @ wr.t() + br, h @ wt.t() + bt, hz @ wz.t() + bz], 1)
    a = torch.cat([h.abs() @ wr.abs().t() + br.abs(), h.abs() @ wt.abs().t() + bt.abs(), hz.abs() @ wz.abs().t() + bz.abs()], 1)
    return o, a


def pose_ref(I, case, mut=None):
    o, a = pose_fc(I, case, F64, mut)
    return o, (256 + 2) * U32 * a + U32 * o.abs()


def pose_f32(I, case):
    return pose_fc(I, case, f32)[0]


def _unit(v, cond):
    n = v.norm(dim=1, keepdim=True)
    cond.append(n)
    return v / n.clamp_min(1e-12)


def pose_decode(o, I, case, mut=None):
    """get_rot_mat, the centroid / depth back-projection and the allocentric -> egocentric turn in o's own type.
    -> dict(rot_allo (B, 9), rot_ego (B, 9), trans (B, 3)), and the norms in front of every normalisation + the ray's angle."""
    kind, RD, is_allo, site, wild, ldh = case
    B, dt = o.shape[0], o.dtype
    r, cond = o[:, :RD], []
    if kind == ROT_QUAT:
        w, x, y, z = _unit(r, cond).unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).view(B, 3, 3)
    elif kind == ROT_EULER:
        c1, s1, c2, s2, c3, s3 = r[:, 0].cos(), r[:, 0].sin(), r[:, 2].cos(), r[:, 2].sin(), r[:, 1].cos(), r[:, 1].sin()
        R = torch.stack([c2 * c3, -s2, c2 * s3, c1 * s2 * c3 + s1 * s3, c1 * c2, c1 * s2 * s3 - s1 * c3, s1 * s2 * c3 - c1 * s3, s1 * c2,
                         s1 * s2 * s3 + c1 * c3], 1).view(B, 3, 3)
    else:
        if kind == ROT_6D_Y:
            y = _unit(r[:, 3:], cond)
            z = _unit(torch.linalg.cross(y, r[:, :3]), cond)
            x = torch.linalg.cross(z, y)
            if mut == "fixed_y_columns_swapped":
                y, z = z, y
        elif kind == ROT_6D_Z:
            z = _unit(r[:, 3:], cond)
            x = _unit(torch.linalg.cross(z, r[:, :3]), cond)
            y = torch.linalg.cross(x, z)
        else:
            x = _unit(r[:, :3], cond)
            z = _unit(torch.linalg.cross(x, r[:, 3:]), cond)
            y = torch.linalg.cross(z, x)
        R = torch.stack([x, y, z], 2)
    K = I["cam_K"].to(dt).view(B, 3, 3)
    c = o[:, RD:RD + 2] if site else torch.zeros(B, 2, dtype=dt)
    cxy = c * I["roi_wh"].to(dt) + I["bbox_center"].to(dt)
    zz = o[:, RD + 2] * I["resize_ratio"].to(dt)
    if wild:
        zz = zz * (K[:, 0, 0] if mut == "wild6d_per_crop_fx" else K[0, 0, 0]) / 590.0
    tr = torch.stack([zz * (cxy[:, 0] - K[:, 0, 2]) / K[:, 0, 0], zz * (cxy[:, 1] - K[:, 1, 2]) / K[:, 1, 1], zz], 1)
    ray = tr / tr.norm(dim=1, keepdim=True)
    angle = torch.acos(ray[:, 2].clamp(-1, 1))
    ego = R
    if is_allo:
        ax = torch.stack([-ray[:, 1], ray[:, 0], torch.zeros(B, dtype=dt)], 1)
        ax = ax / ax.norm(dim=1, keepdim=True).clamp_min(1e-300 if dt == F64 else 1e-30)
        cs, sn = angle.cos(), angle.sin()
        Cc = 1 - cs
        x, y, z = ax.unbind(1)
        M = torch.stack([x * x * Cc + cs, x * y * Cc - z * sn, z * x * Cc + y * sn, x * y * Cc + z * sn, y * y * Cc + cs, y * z * Cc - x * sn,
                         z * x * Cc - y * sn, y * z * Cc + x * sn, z * z * Cc + cs], 1).view(B, 3, 3)
        if mut == "allo_to_ego_transposed":
            M = M.transpose(1, 2)
        ego = torch.where((angle > 0).view(B, 1, 1), M @ R, R)
    return dict(rot_allo=R.reshape(B, 9), rot_ego=ego.reshape(B, 9), trans=tr), (cond, angle)


POSE_DECODE_MUTATIONS = [("fixed_y_columns_swapped", lambda c: c[0] == ROT_6D_Y), ("wild6d_per_crop_fx", lambda c: c[4] == 1),
                         ("allo_to_ego_transposed", lambda c: c[2] == 1)]
U_FLOOR = 2.0 ** -24
YARDSTICK = 8.0            # tests/test_enc_backward_gpu.py::yardstick


def pose_decode_refs(I, case, mut=None):
    """(float64 decode of the float64 fc outputs, float32 decode of the float32 fc outputs)."""
    return pose_decode(pose_fc(I, case, F64)[0], I, case, mut)[0], pose_decode(pose_fc(I, case, f32)[0], I, case)[0]


def yardstick_figures(got, want, ref32):
    """{tensor: (max |got - f64| / max |f64|, the same figure of the float32 evaluation, floored at 2^-24)}."""
    out = {}
    for k, w in want.items():
        scale = float(w.abs().max())
        out[k] = (float((got[k].double().cpu() - w).abs().max()) / scale, max(float((ref32[k].double() - w).abs().max()) / scale, U_FLOOR))
    return out


# ------------------------------------------------------------------------------------------------ gp_groupnorm_apply_xyz
# case: (B, HW, C, operand type, packed16): GroupNorm (G 32, statistics from the caller's 64-row partial sums) + GELU + the 1x1 layer C -> 3;
# v is xyz_pack's flat [NCHW | (rows, 4)] buffer
GNXYZ_G, GNXYZ_ROWS, GNXYZ_EPS = 32, 64, 1e-5
GNXYZ_CASES = [(B, HW, C, dts, p16) for (C, dts, p16) in [(256, "f16", 0), (256, "f16", 1), (128, "f16", 0), (256, "f32", 0), (64, "f32", 0)]
               for (B, HW) in [(1, 64), (3, 1600)]]                # one statistics chunk; 25 chunks
GNXYZ_FORMS = {"gn_apply_xyz_mfma<true>", "gn_apply_xyz_mfma<false>", "gn_apply_xyz<half>", "gn_apply_xyz<float>"}
GNXYZ_ENV = ("GP_GNXYZ_MFMA", "GP_GELU16")


def gnxyz_form(case):
    B, HW, C, dts, p16 = case
    if dts == "f16" and C == 256:
        return "gn_apply_xyz_mfma<true>" if p16 else "gn_apply_xyz_mfma<false>"
    return "gn_apply_xyz<half>" if dts == "f16" else "gn_apply_xyz<float>"


@functools.lru_cache(None)
def _gnxyz_operands(B, HW, C, dts):
    g = _gen(2100 + C + HW)
    x = _rn(g, B, HW, C) * 1.5 + 0.3
    cpg = C // GNXYZ_G
    x[:, :, 3 * cpg:4 * cpg] = 20 + _rn(g, B, HW, cpg)                # group 3: |mean| = 20 std
    x = x.to(DT[dts])
    xc = x.double().view(B, HW // GNXYZ_ROWS, GNXYZ_ROWS, GNXYZ_G, cpg)
    part = torch.stack([xc.sum((2, 4)), (xc * xc).sum((2, 4))], -1).float().reshape(-1)       # as the producing conv leaves them: chunk sums in fp32
    u = lambda n, h: (torch.rand(n, generator=g) * 2 - 1) * h
    return dict(x=x, partial=part, gn_w=1 + u(C, 0.3), gn_b=u(C, 0.3), out_w=_rn(g, 3, C, scale=C ** -0.5), out_b=_rn(g, 3, scale=0.1))


def gnxyz_inputs(case):
    return _gnxyz_operands(*case[:4])


@functools.lru_cache(None)
def _gnxyz_norm(B, HW, C, dts, mut):
    """(y, e_y, x sc, sh): GroupNorm with the statistics of the supplied PARTIALS -- they are operands: S, Q = their float64 sums, exact for
    the reference.  The chain is norm_reference._gn_chain's (gn_finalize: mean = S fl(1 / N), var = Q fl(1 / N) - mean^2 and rstd in double,
    both rounded to fp32; sc = rstd w; sh = fma(-mean, sc, b) from that same sc; y = fma(x, sc, sh)) with no error of the sums themselves:
      d_mean = 2 u |mean|                      fl(1 / N), the fp32 store
      d_var  = u (Q / N + 2 mean^2)            fl(1 / N) on both terms of the cancelling difference: |mean| = 20 std makes it 800 u var
      r_sc   = d_var / (2 (var + eps)) + 2 u   rstd -> fp32, times w
      y' = (x - mean') sc' + b: |x - mean||sc| r_sc + d_mean |sc| + 2 u (|x sc| + |mean sc|) + 2 u (|sh| + |y|)
    (the last two: the roundings of the two products / fmas, of sh and of y; sh is made from the same sc', so sc's error multiplies x - mean)."""
    I = _gnxyz_operands(B, HW, C, dts)
    x, gw, gb = _d(I["x"]), _d(I["gn_w"]), _d(I["gn_b"])
    cpg = C // GNXYZ_G
    gidx = torch.arange(C) % GNXYZ_G if mut == "group_is_channel_mod_G" else torch.arange(C) // cpg
    SQ = _d(I["partial"]).view(B, HW // GNXYZ_ROWS, GNXYZ_G, 2).sum(1)
    N = HW * cpg
    mean = SQ[..., 0] / N
    var = (SQ[..., 1] / N - mean * mean).clamp_min(0)
    if mut == "unbiased_variance":
        var = var * N / (N - 1)
    sc = (1 / (var + GNXYZ_EPS).sqrt())[:, gidx] * gw
    mean_c = mean[:, gidx]
    sh = gb - mean_c * sc
    xs = x * sc[:, None, :]
    y = xs + sh[:, None, :]
    d_var = U32 * (SQ[..., 1] / N + 2 * mean * mean)
    r_sc = (d_var / (2 * (var + GNXYZ_EPS)) + 2 * U32)[:, gidx]
    e = ((x - mean_c[:, None, :]) * sc[:, None, :]).abs() * r_sc[:, None, :] + (2 * U32 * mean_c.abs() * sc.abs())[:, None, :] + \
        2 * U32 * (xs.abs() + (mean_c * sc).abs()[:, None, :]) + 2 * U32 * (sh.abs()[:, None, :] + y.abs())
    return y, e, xs, sh[:, None, :].expand_as(y)


def gnxyz_ref(I, case, mut=None):
    """g = GELU(y), out = g w^T + b.
      VALU forms      e_g = 1.13 e_y + the GELU form's error (gelu_poly2 / gelu_erf); out: (C + 2) u a
      MFMA form       the same e_g (gelu_poly2); g and w both split into fp16 hi + lo, three products per term: (3 C + 2) u a + split_err
      packed fp16     scale and shift rounded to fp16: 2^-11 (|x sc| + |sh|) + 2^-24 in front of the GELU; the v_pk_fma's own rounding of y is
                      the `x rounded to fp16` of gemm_reference's GELU_PK16 model, which also holds the fit and the fp16 Horner; the last
                      packed add rounds g: 2^-11 |g| + 2^-25.  g enters the MFMA as it stands against w's hi + lo: (2 C + 2) u a + split_err
    each chained into the 1x1 layer as sum |w| e_g beside the layer's own term, then the bias add and the store."""
    import norm_reference as NR
    B, HW, C, dts, p16 = case
    y, e_y, xs, sh = _gnxyz_norm(B, HW, C, dts, mut if mut in ("group_is_channel_mod_G", "unbiased_variance") else None)
    w, b = _d(I["out_w"]), _d(I["out_b"])
    g = gelu_exact(y).reshape(-1, C)
    out = g @ w.t() + b
    if mut is not None:
        return xyz_pack(out, B, HW, mut), None
    form = gnxyz_form(case)
    if p16:
        e_g = 1.13 * (e_y + U16 * (xs.abs() + sh.abs()) + 2.0 ** -24) + gelu_act_err(y, "pk16") + U16 * gelu_exact(y).abs() + 2.0 ** -25
        n_acc = 2 * C
    else:
        e_g = NR.act_bound(y, e_y, NR.ACT_GELU, DT[dts])
        n_acc = 3 * C if form.startswith("gn_apply_xyz_mfma") else C
    e_g = e_g.reshape(-1, C)
    a = (g.abs() + e_g) @ w.abs().t() + b.abs()
    e = (n_acc + 2) * U32 * a + e_g @ w.abs().t() + U32 * out.abs()
    if form.startswith("gn_apply_xyz_mfma"):
        e = e + split_err(a, (g.abs() + e_g).sum(1, keepdim=True), w.abs().sum(1))
    return xyz_pack(out, B, HW), xyz_pack(e, B, HW)


def gnxyz_f32(I, case):
    B, HW, C, dts, p16 = case
    y = F.group_norm(I["x"].float().permute(0, 2, 1), GNXYZ_G, I["gn_w"], I["gn_b"], GNXYZ_EPS).permute(0, 2, 1)
    return xyz_pack(F.gelu(y).reshape(-1, C) @ I["out_w"].t() + I["out_b"], B, HW)


def gnxyz_mean_over_std(I, case):
    """Largest |mean| / std over the groups of the case's images."""
    B, HW, C = case[:3]
    xg = _d(I["x"]).view(B, HW, GNXYZ_G, C // GNXYZ_G)
    return float((xg.mean((1, 3)).abs() / xg.std((1, 3), unbiased=False)).max())


# ------------------------------------------------------------------------------------------------ registry
def _named(fn, name):
    return functools.partial(fn, name)


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
    Op("gp_convnext_stem", STEM_CASES, stem_inputs, stem_ref, stem_f32, functools.partial(stem_ref, stored=False)),
    Op("gp_deconv_col2im", COL2IM_CASES, col2im_inputs, col2im_ref, col2im_f32, functools.partial(col2im_ref, stored=False)),
    Op("gp_xyz_out_layer", XYZ_OUT_CASES, xyz_out_inputs, xyz_out_ref, xyz_out_f32),
    Op("gp_pointwise_k3", PK3_CASES, pk3_inputs, pk3_ref, pk3_f32, functools.partial(pk3_ref, stored=False)),
] + [
    Op(n, SMALLCIN_CASES, _named(smallcin_inputs, n), _named(smallcin_ref, n), _named(smallcin_f32, n), functools.partial(smallcin_ref, n, stored=False))
    for n in SMALLCIN_CIN
] + [
    Op("gp_pool_mmm", POOL_CASES, pool_inputs, pool_ref, pool_f32, functools.partial(pool_ref, stored=False)),
    Op("gp_size_head", SIZE_CASES, size_inputs, size_ref, size_f32),
    Op("gp_attention64", ATT_CASES_32, att_inputs, att_ref, att_f32, functools.partial(att_ref, stored=False)),
    Op("gp_attention64_hd", ATT_CASES_HD, att_inputs, att_ref, att_f32, functools.partial(att_ref, stored=False)),
    Op("gp_pose_tail_rt", POSE_CASES, pose_inputs, pose_ref, pose_f32),
    Op("gp_groupnorm_apply_xyz", GNXYZ_CASES, gnxyz_inputs, gnxyz_ref, gnxyz_f32),
]}
HEAD_OPS = ["gp_convnext_stem", "gp_deconv_col2im", "gp_xyz_out_layer", "gp_pointwise_k3", *SMALLCIN_CIN, "gp_pool_mmm", "gp_size_head", "gp_attention64",
            "gp_attention64_hd", "gp_pose_tail_rt", "gp_groupnorm_apply_xyz"]

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
    # ---- head entry and exit kernels: the errors the one-shape relative-error tests let through
    ("gp_convnext_stem", "x_lo_dropped", lambda c: stem_form(c) == "stem_mfma<1>"),
    ("gp_convnext_stem", "w_lo_dropped", lambda c: stem_form(c) == "stem_mfma<1>"),
    ("gp_convnext_stem", "variance_over_127", lambda c: c != STEM_LARGE),
    ("gp_convnext_stem", "column_block_from_row_factor", lambda c: c[2] // 4 // stem_geometry(c)[1] > 1),
    ("gp_deconv_col2im", "h_w_swapped", lambda c: c[1] != c[2]),
    ("gp_deconv_col2im", "last_row_clipped", lambda c: True),
    ("gp_xyz_out_layer", "nchw_rows_for_hw", lambda c: True),
    ("gp_xyz_out_layer", "chunk_loop_runs_once", lambda c: xyz_out_geometry(c)[3] > 1),
    ("gp_pointwise_k3", "row_tail_dropped", lambda c: True),
    ("gp_pointwise_k3", "w_transposed", lambda c: True),
    ("gp_xyz_conv3x3_s2", "window_one_column_right", lambda c: True),
    ("gp_xyz_conv3x3_s2", "x_lo_dropped", lambda c: c[1] == 64),
    ("gp_pnp_conv1", "window_one_column_right", lambda c: True),
    ("gp_pnp_conv1", "coord2d_swapped", lambda c: True),
    ("gp_pnp_conv1", "x_lo_dropped", lambda c: c[1] == 64),
    ("gp_pnp_conv1_masked", "mask_on_xyz_only", lambda c: True),
    ("gp_pnp_conv1_masked", "coord2d_swapped", lambda c: True),
    ("gp_pnp_conv1_masked", "x_lo_dropped", lambda c: c[1] == 64),
    ("gp_pool_mmm", "max_initial_0", lambda c: c[0] >= 2),
    ("gp_pool_mmm", "min_initial_0", lambda c: c[0] == 3),
    ("gp_size_head", "max_initial_0", lambda c: True),
    ("gp_size_head", "mean_size_not_normalised", lambda c: True),
    ("gp_attention64", "scale_of_hd24", lambda c: True),
    ("gp_attention64", "v_at_query_index", lambda c: True),
    ("gp_attention64", "scores_transposed", lambda c: True),
    ("gp_attention64_hd", "scale_of_hd32", lambda c: c[2] == 24),
    ("gp_attention64_hd", "v_at_query_index", lambda c: True),
    ("gp_pose_tail_rt", "fc_z_reads_h", lambda c: True),
    ("gp_pose_tail_rt", "ldh_taken_as_256", lambda c: c[5] == 260),
    ("gp_groupnorm_apply_xyz", "group_is_channel_mod_G", lambda c: True),
    ("gp_groupnorm_apply_xyz", "unbiased_variance", lambda c: c[3] == "f32"),
    ("gp_groupnorm_apply_xyz", "nchw_rows_for_hw", lambda c: c[0] > 1),
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
