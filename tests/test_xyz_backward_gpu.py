"""GPU: the coordinate-head backward family (include/givepose_xyzgrad.h, gpx_*; givepose_amd/xyz_grad.py; PoseNet.xyz_head_backward and
PoseNet.head_grads_xyz) against float64.  The bounds and allowances are derived in tests/xyz_backward_ref.py.

Operator level.  Contractions: per element |got - ref| <= (K + 8) 2^-24 sum_k |a_k| |b_k|, K the number of terms that can exist in that
element's chain (counted by the same formula on all-ones operands).  Bilinear backward: the derived weight-formation + chain bound.
GroupNorm + GELU backward and the head end to end: 8 times the CPU float32 figure of the same inputs, per tensor, as
max|got - ref| / max|ref|; both figures are printed.

Measured on an MI355X (the ratio lines of that run are kept in profiles/xyz_head_backward.txt):

    operator level, largest error / bound over the shapes of each test:
        conv 3x3 s1     forward 0.10, dX 0.05, dW 0.09          transposed conv   forward 0.14, dX 0.03, dW 0.19
        conv 1x1        dX 0.24, dW 0.14, db 0.03               bilinear          backward 0.05, adjoint identity 0.004
    GroupNorm + GELU backward, device figure / CPU float32 figure over B = 1, 3 x (C, HW) = (64, 9), (256, 256), (256, 4096):
        dx 0.63 - 1.22, dgamma 0.69 - 1.56, dbeta 0.73 - 1.54
    the head, largest device figure / CPU float32 figure over the 31 saved tensors and 24 gradients of a case (8 allowed):
        (3, 512, 2) 1.59 (features.9.conv.weight)      (1, 1024, 8) 3.38 (pre6)      (2, 512, 8) 3.13 (features.10.conv.weight)

Why the two cases at H0 = 8 pass 2 (and (3, 512, 2) does not).  In the forward the ratio stays at 0.9 - 1.9 through the five layers at
16 x 16 and 32 x 32 (pre0 .. pre4, act0 .. act4, up0, up1) and steps to 2.8 - 3.4 at pre5, the first conv at 64 x 64 (pre5 3.30 / 2.87,
pre6 3.38 / 2.77, act5, act6, coor 2.02 / 1.74).  That is the layer at which the contraction stops being split: with B 4096 rows the GEMM
has 256 tiles or more and each element is ONE k-ordered chain of 2304 fmas, where the layers below (fewer than 256 tiles) are
cut into 4 or 8 chains of 576 or 288 merged in order, and torch's CPU convolution sums in blocks.  A sequential chain of 2304 collects more
rounding than blocked sums do -- the same finding as fc2 in tests/test_pnp_backward_gpu.py -- and it stays far inside its own bound
(conv 3x3 (1, 8, 256, 64) above: 0.10 of it).  At H0 = 2 the largest map is 16 x 16, every contraction is split, and no ratio passes
1.6.  The backward's ratios above 2 (features.7.norm.weight 3.31 / 2.72, features.10.conv.weight 2.36 / 3.13, the norm and conv
gradients of layers 4 - 10 at 2.0 - 2.5, features.1.bias 2.45, feat 2.02) inherit from those two layers: every gradient below the out
layer passes through the GroupNorm backward of layers 6 and 5, which differentiates at the saved pre6 / pre5, and through their dX
gathers, again single chains of 2304.  out_layer.bias (2.09 at (2, 512, 8)) is a sum of 8192 numbers against a CPU figure of 5.5e-08:
both are at the rounding level of one fp32 number.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import xyz_backward_ref as R

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SENTINEL = -7.25
U = 2.0 ** -24

class Guarded:
    """alloc hook of givepose_amd.xyz_grad: every buffer gets 64 sentinel elements on either side (the pattern of
    tests/test_pnp_backward_gpu.py); check() wants them untouched, every element of every output written, and everything finite."""

    def __init__(self):
        self.bufs = []

    def __call__(self, name, shape):
        n = int(np.prod(shape))
        whole = torch.full((n + 128,), SENTINEL, device="cuda", dtype=torch.float32)
        view = whole[64:64 + n].view(shape)
        assert view.data_ptr() % 256 == 0
        self.bufs.append((name, whole, view))
        return view

    def check(self):
        torch.cuda.synchronize()
        assert self.bufs
        for name, whole, view in self.bufs:
            assert torch.all(whole[:64] == SENTINEL) and torch.all(whole[-64:] == SENTINEL), name
            if name != "workspace":
                assert not torch.any(view == SENTINEL), name
                assert torch.all(torch.isfinite(view)), name


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[seed, 0x7B7]))


def normal(r, *shape):
    return r.standard_normal(shape).astype(np.float32)


def d64(a):
    return T(np.ascontiguousarray(a)).double()


def within(got, ref, rhs, what):
    """|got - ref| <= rhs per element; prints the largest ratio."""
    got, ref, rhs = (np.asarray(a.cpu() if torch.is_tensor(a) else a, np.float64) for a in (got, ref, rhs))
    assert got.shape == ref.shape == rhs.shape, (what, got.shape, ref.shape, rhs.shape)
    err = np.abs(got - ref)
    ratio = float(np.max(err / np.maximum(rhs, 1e-300)))
    print(f"{what}: max |got - ref| / bound = {ratio:.3f}")
    assert np.all(err <= rhs), (what, ratio)
    assert np.any(ref != 0)


def chain_bound(formula, *operands):
    """(K + 8) u sum |a| |b| per element: `formula` on absolute values, and on all-ones operands for K."""
    a = formula(*(o.abs() for o in operands))
    k = formula(*(torch.ones_like(o) for o in operands))
    return (k + 8) * U * a


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b, what):
    """Nested dicts / sequences of tensors (or plain numbers) are equal bit for bit."""
    if isinstance(a, dict):
        assert list(a) == list(b), what
        for k in a:
            same_bits(a[k], b[k], f"{what}[{k}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, f"{what}[{i}]")
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), what
    else:
        assert a == b or (a is None and b is None), what


# ------------------------------------------------------------------------------------------------ conv 3x3 stride 1
@pytest.mark.parametrize("B,Cin,Cout,H", [(1, 3, 5, 5), (2, 24, 40, 8), (1, 8, 256, 64), (3, 256, 256, 16)])
def test_conv3x3s1(B, Cin, Cout, H):
    from givepose_amd import xyz_grad
    r = rng(B * 1000 + Cin + H)
    dY, X, W = normal(r, B, Cout, H, H), normal(r, B, Cin, H, H), normal(r, Cout, Cin, 3, 3) / np.float32(np.sqrt(9 * Cin))
    guard = Guarded()
    Y = xyz_grad.conv3x3s1_forward(T(X).cuda(), T(W).cuda(), alloc=guard)
    out = xyz_grad.conv3x3s1_backward(T(dY).cuda(), T(X).cuda(), T(W).cuda(), alloc=guard)
    guard.check()
    dY, X, W = d64(dY), d64(X), d64(W)
    ref = F.conv2d(X, W, padding=1)
    assert float((ref - R.conv3x3_forward(X, W)).abs().max()) <= 1e-12 * float(ref.abs().max())
    within(Y, ref, chain_bound(R.conv3x3_forward, X, W), f"conv3x3 {B} {Cin} {Cout} {H} forward")
    dx, dw = R.conv3x3_backward(dY, X, W)
    bx, bw = chain_bound(lambda a, b, c: R.conv3x3_backward(a, b, c)[0], dY, X, W), chain_bound(lambda a, b, c: R.conv3x3_backward(a, b, c)[1], dY, X, W)
    within(out["dX"], dx, bx, f"conv3x3 {B} {Cin} {Cout} {H} dX")
    within(out["dW"], dw, bw, f"conv3x3 {B} {Cin} {Cout} {H} dW")


def test_conv3x3s1_dx_impulse_footprint():
    """One non-zero dY element reaches exactly the 3x3 input pixels around it that lie inside the map, with the taps' own weights."""
    from givepose_amd import xyz_grad
    r = rng(77)
    H, C = 5, 4
    W = normal(r, C, C, 3, 3)
    W = np.sign(W) * (np.abs(W) + 0.25)
    X = np.zeros((1, C, H, H), np.float32)
    for n, (oh, ow) in enumerate([(0, 0), (0, 4), (4, 0), (4, 4), (2, 3)]):
        dY = np.zeros((1, C, H, H), np.float32)
        co = n % C
        dY[0, co, oh, ow] = 1.5
        dX = xyz_grad.conv3x3s1_backward(T(dY).cuda(), T(X).cuda(), T(W).cuda())["dX"].cpu().numpy()
        for ih in range(H):
            for iw in range(H):
                kh, kw = ih - oh + 1, iw - ow + 1
                want = np.float32(1.5) * W[co, :, kh, kw] if 0 <= kh < 3 and 0 <= kw < 3 else np.zeros(C, np.float32)
                assert np.array_equal(dX[0, :, ih, iw], want), (oh, ow, ih, iw)


# ------------------------------------------------------------------------------------------------ transposed conv
@pytest.mark.parametrize("B,Cin,Cout,H", [(1, 5, 7, 3), (2, 512, 256, 8), (3, 64, 256, 2)])
def test_deconv3x3s2(B, Cin, Cout, H):
    from givepose_amd import xyz_grad
    r = rng(B * 1000 + Cin + H)
    dY, X, W = normal(r, B, Cout, 2 * H, 2 * H), normal(r, B, Cin, H, H), normal(r, Cin, Cout, 3, 3) / np.float32(np.sqrt(9 * Cin / 4))
    guard = Guarded()
    Y = xyz_grad.deconv3x3s2_forward(T(X).cuda(), T(W).cuda(), alloc=guard)
    out = xyz_grad.deconv3x3s2_backward(T(dY).cuda(), T(X).cuda(), T(W).cuda(), alloc=guard)
    guard.check()
    dY, X, W = d64(dY), d64(X), d64(W)
    ref = F.conv_transpose2d(X, W, None, stride=2, padding=1, output_padding=1)
    assert ref.shape == (B, Cout, 2 * H, 2 * H) and torch.all(ref[:, :, -1, :] != 0) and torch.all(ref[:, :, :, -1] != 0)
    within(Y, ref, chain_bound(R.deconv_forward, X, W), f"deconv {B} {Cin} {Cout} {H} forward")
    dx, dw = R.deconv_backward(dY, X, W)
    bx, bw = chain_bound(lambda a, b, c: R.deconv_backward(a, b, c)[0], dY, X, W), chain_bound(lambda a, b, c: R.deconv_backward(a, b, c)[1], dY, X, W)
    within(out["dX"], dx, bx, f"deconv {B} {Cin} {Cout} {H} dX")
    within(out["dW"], dw, bw, f"deconv {B} {Cin} {Cout} {H} dW")


# ------------------------------------------------------------------------------------------------ conv 1x1
@pytest.mark.parametrize("B,HW", [(1, 9), (3, 256), (2, 4096)])
def test_conv1x1_backward(B, HW):
    from givepose_amd import xyz_grad
    r = rng(B * 10000 + HW)
    S = int(np.sqrt(HW))
    dY, X, W = normal(r, B, 3, S, S), normal(r, B, 256, S, S), normal(r, 3, 256, 1, 1) / 16
    guard = Guarded()
    out = xyz_grad.conv1x1_backward(T(dY).cuda(), T(X).cuda(), T(W).cuda(), alloc=guard)
    guard.check()
    assert out["dW"].shape == (3, 256, 1, 1) and out["dX"].shape == (B, 256, S, S) and out["db"].shape == (3,)
    dY, X, W = d64(dY), d64(X), d64(W)
    ref = R.conv1x1_backward(dY, X, W)
    for i, k in enumerate(("dX", "dW", "db")):
        within(out[k], ref[i], chain_bound(lambda a, b, c: R.conv1x1_backward(a, b, c)[i], dY, X, W), f"conv1x1 B {B} HW {HW} {k}")


# ------------------------------------------------------------------------------------------------ bilinear x2
@pytest.mark.parametrize("H", [2, 3, 8, 32])
@pytest.mark.parametrize("B,C", [(1, 5), (3, 256)])
def test_upsample_bilinear2x_backward(B, C, H):
    from givepose_amd import xyz_grad
    r = rng(B * 1000 + C + H)
    x, g = normal(r, B, C, H, H), normal(r, B, C, 2 * H, 2 * H)
    guard = Guarded()
    y = xyz_grad.upsample_bilinear2x_forward(T(x).cuda(), alloc=guard)
    dx = xyz_grad.upsample_bilinear2x_backward(T(g).cuda(), alloc=guard)
    guard.check()
    within(dx, R.up_backward(d64(g)), R.up_backward_bound(g), f"bilinear backward B {B} C {C} H {H}")
    # the adjoint identity on the device's own forward: both directions use the same (i0, frac), so the weight formation cancels;
    # the forward rounds each term at most 6 times, the backward 26 (ref file): |<up x, g> - <x, up^T g>| <= 32 u <up |x|, |g|>
    a, b = float((y.double().cpu() * d64(g)).sum()), float((d64(x) * dx.double().cpu()).sum())
    rhs = 32 * U * float((R.up_forward(d64(x).abs()) * d64(g).abs()).sum())
    print(f"bilinear adjoint B {B} C {C} H {H}: |<up x, g> - <x, upT g>| / bound = {abs(a - b) / rhs:.3f}")
    assert abs(a - b) <= rhs
    # the forward itself against F.interpolate in float64: each product of two axis weights is off by at most 2 d + 2 u (ref file),
    # over at most 3 x 3 cells when fl(s) falls into the neighbouring cell, plus the 6 roundings of the evaluation
    ref = F.interpolate(d64(x), scale_factor=2, mode="bilinear", align_corners=True)
    d = (2 * (H - 1) + 1) * U
    assert float((y.double().cpu() - ref).abs().max()) <= (9 * (2 * d + 2 * U) + 6 * U) * float(np.abs(x).max())


# ------------------------------------------------------------------------------------------------ GroupNorm + GELU backward
@pytest.mark.parametrize("C,HW", [(64, 9), (256, 256), (256, 4096)])
@pytest.mark.parametrize("B", [1, 3])
def test_gn_gelu_backward(B, C, HW):
    from givepose_amd import xyz_grad
    r = rng(B * 100000 + C + HW)
    x = normal(r, B, C, HW) * (0.5 + r.random((1, C, 1)).astype(np.float32)) + normal(r, 1, C, 1)
    gamma, beta, dout = 2 * normal(r, C), normal(r, C) * 0.5, normal(r, B, C, HW)
    mean64, rstd64 = R.gn_stats(d64(x))
    mean, rstd = mean64.float().numpy(), rstd64.float().numpy()
    u = R.gn_gelu_forward(d64(x), d64(mean), d64(rstd), d64(gamma), d64(beta))[1]
    assert float(u.abs().max()) >= 6.0 and float((u.abs() < 1).double().mean()) > 0.2      # the tail and the bulk of the GELU
    guard = Guarded()
    got = xyz_grad.gn_gelu_backward(*(T(a).cuda() for a in (dout, x, mean, rstd, gamma, beta)), alloc=guard)
    guard.check()
    ref, f32 = (R.gn_gelu_backward(*(T(a).to(dt) for a in (dout, x, mean, rstd, gamma, beta))) for dt in (torch.float64, torch.float32))
    for i, k in enumerate(("dx", "dgamma", "dbeta")):
        want = ref[i].numpy()
        scale = np.max(np.abs(want))
        dev = np.max(np.abs(got[k].cpu().numpy().astype(np.float64) - want)) / scale
        cpu = np.max(np.abs(f32[i].numpy().astype(np.float64) - want)) / scale
        print(f"gn gelu backward B {B} C {C} HW {HW} {k}: device {dev:.2e}, CPU float32 {cpu:.2e}, ratio {dev / max(cpu, 1e-300):.2f}")
        assert dev <= 8 * cpu, (k, dev, cpu)


# ------------------------------------------------------------------------------------------------ the head
def device_params(Cin):
    return {k: T(v).cuda() for k, v in R.head_params(Cin).items()}


def run_head(case, g_scale=1.0, guard=None, crops=None):
    from givepose_amd import xyz_grad
    params, feat, g, _, _ = R.case_reference(case)
    sl = slice(None) if crops is None else crops
    f, gc = T(feat[sl]).cuda(), T(g[sl]).cuda() * g_scale
    P = device_params(case[1])
    saved = xyz_grad.xyz_forward_save(f, P, alloc=guard)
    grads, g_feat = xyz_grad.xyz_backward(P, saved, f, gc, alloc=guard)
    torch.cuda.synchronize()
    return {**grads, "feat": g_feat}, saved


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "B%d_Cin%d_H%d" % c)
def test_xyz_head_end_to_end(case):
    """gpx_xyz_forward_save and gpx_xyz_backward against the float64 restatement: every saved tensor, the 23 gradients and g_feat."""
    from givepose_amd import xyz_grad
    B, Cin, H0 = case
    _, _, _, fig32, r64 = R.case_reference(case)
    guard = Guarded()
    grads, saved = run_head(case, guard=guard)
    guard.check()
    names = [n for n, _, _ in guard.bufs]
    assert names.count("workspace") == 2 and len(names) == 31 + 24 + 2
    assert list(grads) == xyz_grad.PARAM_KEYS + ["feat"]
    for k, s in xyz_grad.param_shapes(Cin).items():
        assert tuple(grads[k].shape) == s and grads[k].is_contiguous(), k
    got = {**R.flatten_saved(saved), **{k: v.cpu().numpy() for k, v in grads.items()}}
    fig = R.rel_figures(got, {**r64["saved"], **r64["grads"]})
    assert set(fig) == set(fig32) and len(fig) == 31 + 24
    ratio = {k: fig[k] / fig32[k] if fig32[k] else float(fig[k] != 0) for k in fig}
    for k in fig:
        print(f"{case} {k}: device {fig[k]:.2e}, CPU float32 {fig32[k]:.2e}, ratio {ratio[k]:.2f}")
    worst = max(ratio, key=ratio.get)
    print(f"{case}: largest ratio {ratio[worst]:.2f} ({worst}); above 2: " + ", ".join(f"{k} {v:.2f}" for k, v in ratio.items() if v > 2))
    for k in fig:
        assert fig[k] <= 8 * fig32[k], (case, k, fig[k], fig32[k])


SMALL = R.CASES[0]


def test_equal_bits_exact_scaling_and_crop_independence():
    assert SMALL == (3, 512, 2)
    a, sa = run_head(SMALL)
    b, sb = run_head(SMALL)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k                          # two runs, equal bits
    for k, v in R.flatten_saved(sa).items():
        assert np.array_equal(v.view(np.int32), R.flatten_saved(sb)[k].view(np.int32)), k
    two, _ = run_head(SMALL, 2.0)
    for k in a:
        assert torch.equal(bits(two[k]), bits(a[k] * 2)) and torch.any(a[k] != 0), k      # linear in g_coor, bit for bit
    # a crop's g_feat does not depend on its batch.  Bit for bit: nothing sums over crops on the way to g_feat, and at this case's
    # sizes the split rule (a function of the tile count) cuts every contraction into the same 8 chunks at B = 1 and at B = 3
    for i in range(3):
        one, s1 = run_head(SMALL, crops=slice(i, i + 1))
        assert torch.equal(bits(one["feat"]), bits(a["feat"][i:i + 1])), i
        assert torch.equal(bits(s1["coor"]), bits(sa["coor"][i:i + 1])), i


@functools.lru_cache(maxsize=None)
def net_of(dtype=torch.float32):
    from givepose_amd import PoseNet, PoseNetConfig
    return PoseNet(PoseNetConfig(), seed=R.WEIGHT_SEED, dtype=dtype).cuda()


def test_posenet_xyz_head_backward_names_aliases_and_both_heads():
    """PoseNet.xyz_head_backward is the xyz_grad path on the state_dict's weights; all 35 names, a gn entry IS its norm entry."""
    from givepose_amd import xyz_grad
    net = net_of()
    _, feat, g, _, _ = R.case_reference(SMALL)
    res = net.xyz_head_backward("xyz_deform_head", T(feat), T(g), return_saved=True)
    torch.cuda.synchronize()
    assert list(res) == ["param_grads", "feat", "outputs", "saved"] and list(res["outputs"]) == ["coor"]
    pg = res["param_grads"]
    want = [k for k in net.state_dict() if k.startswith("xyz_deform_head.")]
    assert len(pg) == 35 and sorted(pg) == sorted(want)
    for alias, k in xyz_grad.ALIASES.items():
        assert pg["xyz_deform_head." + alias] is pg["xyz_deform_head." + k], alias
    assert len({id(v) for v in pg.values()}) == 23
    direct, saved = run_head(SMALL)
    for k in xyz_grad.PARAM_KEYS:
        assert torch.equal(bits(pg["xyz_deform_head." + k]), bits(direct[k])), k
    assert torch.equal(bits(res["feat"]), bits(direct["feat"])) and torch.equal(bits(res["outputs"]["coor"]), bits(saved["coor"]))
    # the other head: in_dim 1024
    f2, g2 = R.make_inputs(1, 1024, 2, seed=31)
    nocs = net.xyz_head_backward("xyz_nocs_head", T(f2), T(g2))
    torch.cuda.synchronize()
    assert len(nocs["param_grads"]) == 35 and nocs["feat"].shape == (1, 1024, 2, 2)
    assert nocs["param_grads"]["xyz_nocs_head.features.0.weight"].shape == (1024, 256, 3, 3)
    ref = R.head_run(R.head_params(1024), f2, g2)
    fig = R.rel_figures({k: nocs["param_grads"]["xyz_nocs_head." + k].cpu().numpy() for k in xyz_grad.PARAM_KEYS}, {k: ref["grads"][k] for k in xyz_grad.PARAM_KEYS})
    assert max(fig.values()) < 1e-4, fig


def test_in_place_parameter_update_is_seen():
    """The fp32 copies of the weights follow the parameters: after an in-place update of an fp16 network's parameter -- where the
    copies are real copies -- the next call differentiates the new value."""
    net = net_of(torch.float16)
    _, feat, g, _, _ = R.case_reference(SMALL)
    p = dict(net.named_parameters())["xyz_deform_head.out_layer.bias"]
    keep = p.detach().clone()
    before = net.xyz_head_backward("xyz_deform_head", T(feat), T(g))
    try:
        p.add_(1.0)
        after = net.xyz_head_backward("xyz_deform_head", T(feat), T(g))
    finally:
        p.copy_(keep)
    again = net.xyz_head_backward("xyz_deform_head", T(feat), T(g))
    torch.cuda.synchronize()
    assert torch.allclose(after["outputs"]["coor"], before["outputs"]["coor"] + 1.0, rtol=0, atol=1e-5)
    assert not torch.equal(after["outputs"]["coor"], before["outputs"]["coor"])
    assert torch.equal(bits(again["outputs"]["coor"]), bits(before["outputs"]["coor"]))
    assert torch.equal(bits(again["feat"]), bits(before["feat"]))


@pytest.mark.parametrize("key", ["features.0.weight", "features.6.conv.weight", "features.4.norm.weight", "out_layer.weight"])
def test_gradient_lies_under_its_parameters_index(key):
    """The element of largest reference gradient, perturbed in the float64 restatement: the central difference of <coor, g_coor> matches
    the device's gradient AT THAT INDEX.  Allowance 1e-4 max|grad|: the device's fp32 error is of the order 1e-6 max|grad| (yardstick),
    the central difference's (h = 1e-5, float64) below 1e-8; an element found under another index would be off by its own size."""
    params, feat, g, _, r64 = R.case_reference(SMALL)
    grads, _ = run_head(SMALL)
    ref = r64["grads"][key]
    idx = np.unravel_index(int(np.argmax(np.abs(ref))), ref.shape)
    f, gc = d64(feat), d64(g)
    val = []
    for sign in (1.0, -1.0):
        P = {k: d64(v) for k, v in params.items()}
        P[key][idx] += sign * 1e-5
        val.append(float((R.head_forward(P, f)["coor"] * gc).sum()))
    cd = (val[0] - val[1]) / 2e-5
    got = float(grads[key][idx])
    scale = float(np.max(np.abs(ref)))
    print(f"{key}{list(idx)}: device {got:.8e}, central difference {cd:.8e}, float64 formula {ref[idx]:.8e}")
    assert abs(cd - ref[idx]) <= 1e-6 * scale and abs(got - cd) <= 1e-4 * scale
    assert tuple(grads[key].shape) == ref.shape


# ------------------------------------------------------------------------------------------------ PoseNet.head_grads_xyz
@functools.lru_cache(maxsize=1)
def loss_batch():
    """The synthetic batch of tests/test_pnp_backward_gpu.py::test_head_grads_pnp."""
    import zlib

    import pose_loss_ref as PR
    from givepose_amd import synth
    z = np.load(PR.GOLDEN + "/pose_loss_e2e.npz")
    npb = synth.synth_batch(4, seed=int(z["batch_seed"]))
    r = np.random.Generator(np.random.Philox(key=[int(z["mask_seed"]), 4]))
    npb["roi_mask_deform"] = (r.random(npb["roi_mask"].shape) > 0.4).astype(np.float32)
    assert zlib.crc32(np.ascontiguousarray(npb["roi_img"]).tobytes()) == int(z["roi_img_crc"])
    _, gt = PR.make_inputs(B=4, P=256, seed=60)
    return {k: T(np.ascontiguousarray(v)) for k, v in {**npb, **gt}.items()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_head_grads_xyz(dtype):
    """head_grads_pnp's results bit for bit, plus xyz_head_backward on the forward's own feat_cat and the total d ivfc_coor."""
    import pose_loss_grad_ref as G
    from givepose_amd import PoseLoss
    data, net, pl, w = loss_batch(), net_of(dtype), PoseLoss(), T(G.make_gout())
    res = net.head_grads_xyz(data, pl, "cuda", gout=w)
    base = net.head_grads_pnp(data, pl, "cuda", gout=w)
    assert list(base) == ["loss", "output", "grads", "param_grads"] and len(base["param_grads"]) == 23
    assert list(res) == list(base) and list(res["grads"]) == list(base["grads"]) + ["feat_cat", "conv_feat256", "nocs_feat"]
    same_bits(res["loss"], base["loss"], "loss")
    same_bits(res["output"], base["output"], "output")
    for k in base["grads"]:
        assert torch.equal(bits(res["grads"][k]), bits(base["grads"][k])), k
    for k, v in base["param_grads"].items():
        assert k.startswith("pnp_net.") and torch.equal(bits(res["param_grads"][k]), bits(v)), k
    fwd = net.forward_device({**data, "roi_mask": data["roi_mask_deform"]}, "cuda")
    feat_cat = fwd["feat_cat"].permute(0, 3, 1, 2).float().contiguous()
    assert feat_cat.shape == (4, 512, 8, 8)
    back = net.xyz_head_backward("xyz_deform_head", feat_cat, base["grads"]["ivfc_coor"])
    torch.cuda.synchronize()
    assert len(res["param_grads"]) == 23 + 35 and len(back["param_grads"]) == 35
    for k, v in back["param_grads"].items():
        assert torch.equal(bits(res["param_grads"][k]), bits(v)) and torch.any(v != 0) and torch.all(torch.isfinite(v)), k
    fc = res["grads"]["feat_cat"]
    assert fc.shape == (4, 512, 8, 8) and torch.equal(bits(fc), bits(back["feat"])) and torch.any(fc != 0)
    for k, lo in (("conv_feat256", 0), ("nocs_feat", 256)):
        h = res["grads"][k]
        assert h.shape == (4, 256, 8, 8) and h.data_ptr() == fc[:, lo:lo + 256].data_ptr() and h.stride() == fc.stride(), k
        assert torch.equal(h, fc[:, lo:lo + 256])
    # the fp32 recompute of the head at the forward's own feature agrees with the map the forward emitted, to the forward's precision
    tol = 2e-2 if dtype == torch.float16 else 1e-4
    d = (back["outputs"]["coor"] - fwd["ivfc_coor"].float()).abs().max().item()
    print(f"head_grads_xyz {dtype}: fp32 recompute of ivfc_coor against the forward {d:.2e}")
    assert d <= tol * max(1.0, fwd["ivfc_coor"].float().abs().max().item())
