"""GPU: the pose-head backward family (include/givepose_headgrad.h, gph_*; givepose_amd/pnp_grad.py; PoseNet.pnp_backward and
PoseNet.head_grads_pnp) against float64.

Operator level.  Every contraction is an fp32 fma chain in the order of k (v_mfma_f32_32x32x2_f32 is one bit for bit), split into at
most 8 chains whose partial sums are merged in order, so per element |got - ref| <= (K + 8) 2^-24 sum_k |a_k| |b_k| (Higham, Accuracy
and Stability of Numerical Algorithms, section 3.1), K the contraction length, the 8 for the merges (at most 7), the rounding of the
LeakyReLU gate's 0.1 g or of the mask product, and the store.  The right-hand side is evaluated in float64 on absolute values.  For the
conv dX the chain holds the taps that exist, at most 4 x Cout terms; the absent ones contribute exact zeros.

GroupNorm + ReLU backward and end to end: the allowance is 8 times what the same formula (the same gated restatement) reaches in torch
float32 on the CPU on the same inputs, per tensor, as max|got - ref| / max|ref|; both figures are printed.  Measured on an MI355X:

    operator level, largest error / bound:  linear dX 0.16, dW 0.30, db 0.19; conv dX 0.003, dW 0.05; first conv dX 0.003, dW 0.0004
    GroupNorm + ReLU backward, device figure / CPU float32 figure over B = 1, 3 x HW = 64, 256, 1024:
        dx 0.63 - 1.17, dgamma 0.55 - 1.59, dbeta 0.75 - 1.12
    end to end, largest device figure / CPU float32 figure over the 24 tensors of a case:
        b1 1.00, b3 1.00, b5 1.49 (fc2_z.weight), b4_masked 2.15 (fc_t.weight; fc2.weight 1.84, fc2_z.weight 1.68, ivfc_coor 1.59)

Why b4_masked passes 2 (checked on the device's saved activations of that case, each against the float64 forward with the same gates;
device figure / torch float32 figure): conv and GroupNorm outputs 0.55 - 1.22, h1 1.23, h2 1.89 -- and fc_t.weight = g^T h2, a chain of
length B, carries h2's error on.  The step is fc2 (K = 1024, eight k-ordered chains of 128 merged in order).  From the device's own h1,
a CPU emulation of exactly those fma chains reproduces the device's h2 bit for bit (all 1024 values), so the kernel computes what it
is specified to compute and nothing else.  Against float64, on that same input: the k-ordered chains 9.1e-7, torch's blocked fp32 GEMM
5.3e-7, fc2 in float64 (the error h2 inherits from h1 alone) 5.7e-7.  The excess is the summation order of one layer, seen on a max
statistic: the order that makes the operator bounds derivable collects more rounding than a blocked one.  The operator-level figures
above show the same kernels well inside their own bounds.

Device gates that differ from the float64 forward's own signs: 0 of 1.7e5 B in every case (so none outside the layer's fp32 bound).
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pnp_backward_ref as R

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SENTINEL = -7.25
U = 2.0 ** -24


class Guarded:
    """alloc hook of givepose_amd.pnp_grad: every buffer gets 64 sentinel elements on either side (the `_guarded` pattern of
    tests/test_pose_loss_grad_gpu.py); check() wants them untouched and every element of every output written."""

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
    return np.random.Generator(np.random.Philox(key=[seed, 0x6A6]))


def normal(r, *shape):
    return r.standard_normal(shape).astype(np.float32)


def within(got, ref, rhs, what):
    """|got - ref| <= rhs per element; prints the largest ratio."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    ratio = float(np.max(err / np.maximum(rhs, 1e-300)))
    print(f"{what}: max |got - ref| / bound = {ratio:.3f}")
    assert got.shape == ref.shape and np.all(err <= rhs), (what, ratio)
    assert np.any(ref != 0)


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ linear backward
@pytest.mark.parametrize("M,N,K", [(1, 6, 256), (3, 256, 1024), (5, 2048, 8192), (17, 256, 1024)])
@pytest.mark.parametrize("gated", [False, True])
def test_linear_backward(M, N, K, gated):
    from givepose_amd import pnp_grad
    r = rng(M * 1000 + N + int(gated))
    dY, W, X = normal(r, M, N), normal(r, N, K) / np.sqrt(K, dtype=np.float32), normal(r, M, K)
    Y = None
    if gated:      # a saved LeakyReLU output: both signs and exact zeros (the gate at 0 is the slope, torch's convention)
        Y = normal(r, M, N)
        Y[r.random((M, N)) < 0.1] = 0.0
    guard = Guarded()
    out = pnp_grad.linear_backward(T(dY).cuda(), T(W).cuda(), T(X).cuda(), None if Y is None else T(Y).cuda(), alloc=guard)
    guard.check()
    g = dY.astype(np.float64)
    if gated:      # the kernel's slope is the fp32 value of 0.1
        g = g * np.where(Y > 0, 1.0, float(np.float32(0.1)))
    W64, X64 = W.astype(np.float64), X.astype(np.float64)
    within(out["dX"].cpu().numpy(), g @ W64, (N + 8) * U * (np.abs(g) @ np.abs(W64)), f"linear {M}x{N}x{K} dX")
    within(out["dW"].cpu().numpy(), g.T @ X64, (M + 8) * U * (np.abs(g).T @ np.abs(X64)), f"linear {M}x{N}x{K} dW")
    within(out["db"].cpu().numpy(), g.sum(0), (M + 8) * U * np.abs(g).sum(0), f"linear {M}x{N}x{K} db")


def test_linear_backward_accumulates_in_place():
    """accumulate: dX = what the buffer held + the fresh product, one fp32 addition per element (the two branches into the
    flattened feature are added this way)."""
    from givepose_amd import pnp_grad
    r = rng(5)
    dY, W, X, prior = (T(a).cuda() for a in (normal(r, 5, 1024), normal(r, 1024, 8192), normal(r, 5, 8192), normal(r, 5, 8192)))
    fresh = pnp_grad.linear_backward(dY, W, X)["dX"]
    acc = prior.clone()
    out = pnp_grad.linear_backward(dY, W, X, accumulate_into=acc)
    assert out["dX"] is acc and torch.equal(bits(acc), bits(prior + fresh))


# ------------------------------------------------------------------------------------------------ conv backward
def conv_ref(dY, X, W, cin_dx=None, mask=None):
    """float64 dX, dW of F.conv2d(X, W, stride=2, padding=1) by torch autograd, and the same on absolute values (the bound's sums)."""
    out = []
    for f in (lambda a: a, np.abs):
        x = T(f(X.astype(np.float64))).requires_grad_(True)
        w = T(f(W.astype(np.float64))).requires_grad_(True)
        F.conv2d(x, w, None, stride=2, padding=1).backward(T(f(dY.astype(np.float64))))
        dx = x.grad.numpy()[:, :cin_dx]
        if mask is not None:
            dx = dx * f(mask.astype(np.float64))
        out += [dx, w.grad.numpy()]
    return out


@pytest.mark.parametrize("H", [32, 16])
@pytest.mark.parametrize("B", [1, 3])
def test_conv_backward_128(B, H):
    from givepose_amd import pnp_grad
    r = rng(B * 100 + H)
    dY, X, W = normal(r, B, 128, H // 2, H // 2), normal(r, B, 128, H, H), normal(r, 128, 128, 3, 3) / 34
    guard = Guarded()
    out = pnp_grad.conv3x3s2_backward(T(dY).cuda(), T(X).cuda(), T(W).cuda(), alloc=guard)
    guard.check()
    dx, dw, adx, adw = conv_ref(dY, X, W)
    within(out["dX"].cpu().numpy(), dx, (4 * 128 + 8) * U * adx, f"conv B {B} H {H} dX")
    within(out["dW"].cpu().numpy(), dw, (B * (H // 2) ** 2 + 8) * U * adw, f"conv B {B} H {H} dW")


@pytest.mark.parametrize("masked", [False, True])
def test_first_conv_backward(masked):
    """5 -> 128 at 64 -> 32: all of dW (128,5,3,3); dX for the three ivfc channels only, times the mask."""
    from givepose_amd import pnp_grad
    r = rng(64 + int(masked))
    B = 2
    dY, X, W = normal(r, B, 128, 32, 32), normal(r, B, 5, 64, 64), normal(r, 128, 5, 3, 3) / 7
    mask = None
    if masked:
        mask = r.random((B, 1, 64, 64)).astype(np.float32)
        mask[:, :, 5:9, :] = 0.0
    guard = Guarded()
    out = pnp_grad.conv3x3s2_backward(T(dY).cuda(), T(X).cuda(), T(W).cuda(), mask=None if mask is None else T(mask).cuda(), cin_dx=3, alloc=guard)
    guard.check()
    assert out["dX"].shape == (B, 3, 64, 64) and out["dW"].shape == (128, 5, 3, 3)
    dx, dw, adx, adw = conv_ref(dY, X, W, cin_dx=3, mask=mask)
    within(out["dX"].cpu().numpy(), dx, (4 * 128 + 8) * U * adx, f"first conv masked {masked} dX")
    within(out["dW"].cpu().numpy(), dw, (B * 1024 + 8) * U * adw, f"first conv masked {masked} dW")
    if masked:
        assert torch.all(out["dX"][:, :, 5:9, :] == 0)


@pytest.mark.parametrize("H", [32, 16])
def test_conv_dx_impulse_footprint(H):
    """One non-zero dY element reaches exactly the input pixels of its 3x3 stride-2 footprint: rows 2 oh - 1 .. 2 oh + 1 inside the
    image (no bottom / right padding at even sizes: the last row and column get tap 2 only).  Everything else is an exact zero."""
    from givepose_amd import pnp_grad
    r = rng(H)
    Ho = H // 2
    W = normal(r, 128, 128, 3, 3)
    W = np.sign(W) * (np.abs(W) + 0.25)          # no zero weight: the footprint is full
    X = np.zeros((2, 128, H, H), np.float32)
    for n, (oh, ow) in enumerate([(0, 0), (0, Ho - 1), (Ho - 1, 0), (Ho - 1, Ho - 1), (Ho // 2 - 1, Ho // 2 + 1)]):
        dY = np.zeros((2, 128, Ho, Ho), np.float32)
        b, co = n % 2, 17 * n + 3
        dY[b, co, oh, ow] = 1.5
        dX = pnp_grad.conv3x3s2_backward(T(dY).cuda(), T(X).cuda(), T(W).cuda())["dX"].cpu().numpy()
        want = np.zeros((2, 128, H, H), bool)
        rows = [i for i in (2 * oh - 1, 2 * oh, 2 * oh + 1) if 0 <= i < H]
        cols = [i for i in (2 * ow - 1, 2 * ow, 2 * ow + 1) if 0 <= i < H]
        want[b][:, rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1] = True
        assert np.array_equal(dX != 0, want), (oh, ow)
        for ih in rows:          # and the values are the taps: dX[ci, ih, iw] = 1.5 W[co, ci, ih - 2 oh + 1, iw - 2 ow + 1]
            for iw in cols:
                assert np.array_equal(dX[b, :, ih, iw], np.float32(1.5) * W[co, :, ih - 2 * oh + 1, iw - 2 * ow + 1]), (oh, ow, ih, iw)


# ------------------------------------------------------------------------------------------------ GroupNorm + ReLU backward
def gn_formula(dout, out, x, mean, rstd, gamma, dtype):
    """The three-term backward of ReLU(GroupNorm) on the saved tensors, in torch `dtype` on the CPU."""
    c = lambda a: T(np.ascontiguousarray(a)).to(dtype)
    dout, out, x, mean, rstd, gamma = c(dout), c(out), c(x), c(mean), c(rstd), c(gamma)
    B, C = x.shape[:2]
    dy = torch.where(out > 0, dout, torch.zeros((), dtype=dtype)).reshape(B, C // 4, 4, -1)
    xh = (x.reshape(B, C // 4, 4, -1) - mean[:, :, None, None]) * rstd[:, :, None, None]
    dgamma, dbeta = (dy * xh).sum(dim=(0, 3)).reshape(C), dy.sum(dim=(0, 3)).reshape(C)
    dxh = dy * gamma.reshape(1, C // 4, 4, 1)
    dx = rstd[:, :, None, None] * (dxh - dxh.mean(dim=(2, 3), keepdim=True) - xh * (dxh * xh).mean(dim=(2, 3), keepdim=True))
    return {"dx": dx.reshape(x.shape).numpy(), "dgamma": dgamma.numpy(), "dbeta": dbeta.numpy()}


@pytest.mark.parametrize("HW", [64, 256, 1024])
@pytest.mark.parametrize("B", [1, 3])
def test_gn_relu_backward(B, HW):
    from givepose_amd import pnp_grad
    r = rng(B * 10000 + HW)
    S = int(np.sqrt(HW))
    x = normal(r, B, 128, S, S) * (0.5 + r.random((1, 128, 1, 1)).astype(np.float32)) + normal(r, 1, 128, 1, 1)
    gamma, beta, dout = normal(r, 128), normal(r, 128) * 0.5, normal(r, B, 128, S, S)
    x64 = T(x).double()
    var, mu = torch.var_mean(x64.reshape(B, 32, -1), dim=2, unbiased=False)
    mean, rstd = mu.float().numpy(), (var + 1e-5).rsqrt().float().numpy()
    out = F.relu(F.group_norm(x64, 32, T(gamma).double(), T(beta).double(), eps=1e-5)).float().numpy()
    assert 0.2 < (out > 0).mean() < 0.8
    guard = Guarded()
    got = pnp_grad.gn_relu_backward(*(T(a).cuda() for a in (dout, out, x, mean, rstd, gamma)), alloc=guard)
    guard.check()
    ref, f32 = (gn_formula(dout, out, x, mean, rstd, gamma, dt) for dt in (torch.float64, torch.float32))
    for k in ("dx", "dgamma", "dbeta"):
        scale = np.max(np.abs(ref[k]))
        dev, cpu = np.max(np.abs(got[k].cpu().numpy().astype(np.float64) - ref[k])) / scale, np.max(np.abs(f32[k].astype(np.float64) - ref[k])) / scale
        print(f"gn backward B {B} HW {HW} {k}: device {dev:.2e}, CPU float32 {cpu:.2e}, ratio {dev / max(cpu, 1e-300):.2f}")
        assert dev <= 8 * cpu, (k, dev, cpu)


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def net_of(masked=False, dtype=torch.float32):
    from givepose_amd import PoseNet, PoseNetConfig
    return PoseNet(PoseNetConfig(mask_attention_type="mul" if masked else "none"), seed=R.WEIGHT_SEED, dtype=dtype).cuda()


def device_gates(saved):
    g = {f"relu{li}": saved["act"][li] > 0 for li in range(3)}
    g.update(fc1=saved["h1"][:, :1024] > 0, fc1_z=saved["h1"][:, 1024:] > 0, fc2=saved["h2"] > 0, fc2_z=saved["h2z"] > 0)
    return {k: v.cpu().numpy() for k, v in g.items()}


def cuda_inputs(inp):
    return [None if a is None else T(a).cuda() for a in inp]


@pytest.mark.parametrize("name", list(R.CASES))
def test_pnp_backward_end_to_end(name):
    """PoseNet.pnp_backward against the gated float64 restatement, the gates taken from the device's saved outputs."""
    from givepose_amd import pnp_grad
    B, seed, masked = R.CASES[name]
    inp = R.make_inputs(B, seed, masked)
    ivfc, coord, mask, g_rot, g_t = cuda_inputs(inp)
    res = net_of(masked).pnp_backward(ivfc, coord, g_rot, g_t, mask=mask, return_saved=True)
    torch.cuda.synchronize()
    assert list(res) == ["param_grads", "ivfc_coor", "outputs", "saved"]
    params = R.head_params()
    assert list(res["param_grads"]) == [R.PREFIX + k for k in pnp_grad.PARAM_KEYS] and len(res["param_grads"]) == 23
    for k, v in res["param_grads"].items():
        assert v.dtype == torch.float32 and tuple(v.shape) == params[k].shape and v.is_contiguous(), k
    assert res["ivfc_coor"].shape == (B, 3, 64, 64)
    gates = device_gates(res["saved"])
    fig32, r64 = R.f32_figures(params, *inp, gates=gates)
    got = {**{k: v.cpu().numpy() for k, v in res["param_grads"].items()}, "ivfc_coor": res["ivfc_coor"].cpu().numpy()}
    fig = R.rel_figures(got, R.tensors_of(r64))
    worst = max(fig, key=lambda k: fig[k] / max(fig32[k], 1e-300) if fig[k] else 0.0)
    for k in fig:
        print(f"{name} {k}: device {fig[k]:.2e}, CPU float32 {fig32[k]:.2e}, ratio {fig[k] / fig32[k] if fig32[k] else float(fig[k] != 0):.2f}")
    print(f"{name}: largest ratio {fig[worst] / max(fig32[worst], 1e-300):.2f} ({worst})")
    for k in fig:
        assert fig[k] <= 8 * fig32[k], (name, k, fig[k], fig32[k])
    # the fp32 recompute's outputs, and the gates against the float64 forward's own signs
    for k in ("pred_rot", "pred_t"):
        assert np.max(np.abs(res["outputs"][k].cpu().numpy() - r64[k])) <= 1e-5 * np.max(np.abs(r64[k])), k
    n, bad, diff = R.gate_flips(gates, r64, R.forward_bounds(params, *inp[:3], r64))
    print(f"{name}: device gates that differ from the float64 forward's signs {diff} of {n}, outside the fp32 bound {bad}")
    assert bad == 0 and diff < 1e-4 * n, (name, bad, diff, n)
    if masked:
        assert torch.all(res["ivfc_coor"][:, :, :20, 30:] == 0)


def test_gradient_lies_under_its_state_dict_index():
    """Layout: with GroupNorm 7 passing channel 37 only, the flattened feature is non-zero in the NCHW flatten columns 37 * 64 + hw
    and fc1 / fc1_z's gradients lie in exactly those columns; with an input that is non-zero in one even pixel of ivfc channel 1, the
    first conv's gradient lies in input channel 1 at the centre tap and nowhere else."""
    net = net_of(False)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    mod = dict(sd)
    gw, gb = torch.zeros_like(sd["pnp_net.features.7.weight"]), torch.zeros_like(sd["pnp_net.features.7.bias"])
    gw[37], gb[37] = 1.0, 0.5
    mod["pnp_net.features.7.weight"], mod["pnp_net.features.7.bias"] = gw, gb
    ivfc = torch.zeros(2, 3, 64, 64)
    ivfc[0, 1, 10, 20], ivfc[1, 1, 10, 20] = 1.0, -2.0
    _, _, _, g_rot, g_t = R.make_inputs(2, seed=3)
    try:
        net.load_state_dict(mod)
        res = net.pnp_backward(ivfc, torch.zeros(2, 2, 64, 64), T(g_rot), T(g_t), return_saved=True)
        torch.cuda.synchronize()
    finally:
        net.load_state_dict(sd)
    flat = (res["saved"]["act"][2].reshape(2, 8192) != 0).any(0).cpu()
    assert flat[37 * 64:38 * 64].any() and int(flat.sum()) == int(flat[37 * 64:38 * 64].sum())
    for n in ("fc1", "fc1_z"):
        nz = (res["param_grads"][f"pnp_net.{n}.weight"] != 0).cpu()
        assert nz.shape == (1024, 8192) and torch.equal(nz.any(0), flat), n
    nz = (res["param_grads"]["pnp_net.features.0.weight"] != 0).cpu()
    assert nz.shape == (128, 5, 3, 3) and nz[:, 1, 1, 1].any() and int(nz.sum()) == int(nz[:, 1, 1, 1].sum())
    g7 = res["param_grads"]["pnp_net.features.7.weight"].cpu()
    assert g7[37] != 0 and tuple(res["param_grads"]["pnp_net.features.6.weight"].shape) == (128, 128, 3, 3)


# ------------------------------------------------------------------------------------------------ invariants
def run_head(g_scale=1.0, guard=None):
    from givepose_amd import pnp_grad
    B, seed, masked = R.CASES["b4_masked"]
    ivfc, coord, mask, g_rot, g_t = cuda_inputs(R.make_inputs(B, seed, masked))
    params = {k[len(R.PREFIX):]: T(v).cuda() for k, v in R.head_params().items()}
    saved = pnp_grad.pnp_forward_save(ivfc, coord, params, mask=mask, alloc=guard)
    grads, g_ivfc = pnp_grad.pnp_backward(params, saved, g_rot * g_scale, g_t * g_scale, mask=mask, alloc=guard)
    torch.cuda.synchronize()
    return {**grads, "ivfc_coor": g_ivfc}, saved


def test_equal_bits_exact_scaling_and_exact_zeros():
    a, sa = run_head()
    b, sb = run_head()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k                     # two calls, equal bits
    for k in ("h1", "h2", "h2z", "pred_rot", "pred_t", "x0"):
        assert torch.equal(bits(sa[k]), bits(sb[k])), k
    two, _ = run_head(2.0)
    for k in a:
        assert torch.equal(bits(two[k]), bits(a[k] * 2)) and torch.any(a[k] != 0), k      # linear in g, bit for bit
    zero, _ = run_head(0.0)
    for k in a:
        assert torch.all(zero[k] == 0), k


def test_sentinels_around_every_output_and_workspace_buffer():
    guard = Guarded()
    a, _ = run_head(guard=guard)
    guard.check()
    names = [n for n, _, _ in guard.bufs]
    assert names.count("workspace") == 2 and len(names) == 18 + 23 + 1 + 2
    plain, _ = run_head()
    for k in a:
        assert torch.equal(bits(a[k]), bits(plain[k])), k


# ------------------------------------------------------------------------------------------------ PoseNet.head_grads_pnp
@functools.lru_cache(maxsize=1)
def loss_batch():
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
def test_head_grads_pnp(dtype):
    """Bitwise the composition of head_grads() with pnp_backward on the forward's own ivfc_coor; the total is direct + head part;
    head_grads itself is unchanged."""
    import pose_loss_grad_ref as G
    from givepose_amd import PoseLoss
    data, net, pl, w = loss_batch(), net_of(False, dtype), PoseLoss(), T(G.make_gout())
    res = net.head_grads_pnp(data, pl, "cuda", gout=w)
    base = net.head_grads(data, pl, "cuda", gout=w)
    assert list(base) == ["loss", "output", "grads"] and list(base["grads"]) == ["rot6d", "pred_t", "size", "nocs_coor", "ivfc_coor"]
    assert list(res) == ["loss", "output", "grads", "param_grads"] and list(res["grads"]) == list(base["grads"]) + ["ivfc_coor_direct"]
    back = net.pnp_backward(base["output"]["ivfc_coor"], data["roi_coord_2d"], base["grads"]["rot6d"], base["grads"]["pred_t"],
                            mask=base["output"]["mask"])
    torch.cuda.synchronize()
    for k in ("rot6d", "pred_t", "size", "nocs_coor"):
        assert torch.equal(bits(res["grads"][k]), bits(base["grads"][k])), k
    assert torch.equal(bits(res["grads"]["ivfc_coor_direct"]), bits(base["grads"]["ivfc_coor"]))
    assert torch.equal(bits(res["grads"]["ivfc_coor"]), bits(base["grads"]["ivfc_coor"] + back["ivfc_coor"]))
    assert len(res["param_grads"]) == 23
    for k, v in back["param_grads"].items():
        assert torch.equal(bits(res["param_grads"][k]), bits(v)) and torch.any(v != 0) and torch.all(torch.isfinite(v)), k
    assert torch.any(back["ivfc_coor"] != 0)
    # the fp32 recompute of the head at the forward's own map agrees with what the forward emitted, to the forward's precision
    tol = 2e-2 if dtype == torch.float16 else 1e-4
    fwd = net.forward_device({**data, "roi_mask": data["roi_mask_deform"]}, "cuda")
    for k in ("pred_rot", "pred_t"):
        d = (back["outputs"][k] - fwd[k].float().reshape(back["outputs"][k].shape)).abs().max().item()
        print(f"head_grads_pnp {dtype} {k}: fp32 recompute against the forward {d:.2e}")
        assert d <= tol * max(1.0, fwd[k].float().abs().max().item()), k


def test_in_place_parameter_update_is_seen():
    """The fp32 copies of the weights follow the parameters: after an in-place update (an optimiser step) of an fp16 network's
    parameter -- where the copies are real copies -- the next call differentiates the new value."""
    net = net_of(False, torch.float16)
    ivfc, coord, _, g_rot, g_t = cuda_inputs(R.make_inputs(1, seed=2))
    p = dict(net.named_parameters())["pnp_net.fc_z.bias"]
    before = net.pnp_backward(ivfc, coord, g_rot, g_t)["outputs"]["pred_t"].clone()
    try:
        p.add_(1.0)
        after = net.pnp_backward(ivfc, coord, g_rot, g_t)["outputs"]["pred_t"].clone()
    finally:
        p.sub_(1.0)
    again = net.pnp_backward(ivfc, coord, g_rot, g_t)["outputs"]["pred_t"]
    assert torch.equal(after[:, :2], before[:, :2]) and torch.allclose(after[:, 2], before[:, 2] + 1.0, rtol=0, atol=1e-6)
    assert torch.equal(bits(again), bits(before))


def test_unsupported_configurations_refuse():
    net = net_of(False)
    cfg = net.cfg
    ivfc, coord, _, g_rot, g_t = cuda_inputs(R.make_inputs(1, seed=1))
    try:
        for flag, value in (("pnp_head", "att"), ("flat_op", "avg-max"), ("mask_attention_type", "concat")):
            net.cfg = dataclasses.replace(cfg, **{flag: value})
            with pytest.raises(NotImplementedError, match=flag):
                net.pnp_backward(ivfc, coord, g_rot, g_t)
            with pytest.raises(NotImplementedError, match=flag):
                net.head_grads_pnp(loss_batch(), None)
        net.cfg = dataclasses.replace(cfg, r_type="allo_rot6d_y")
        with pytest.raises(NotImplementedError, match="r_type"):
            net.head_grads_pnp(loss_batch(), None)
    finally:
        net.cfg = cfg
