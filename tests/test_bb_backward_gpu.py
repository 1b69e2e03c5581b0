"""GPU: the backbone backward family (include/givepose_bbgrad.h, gpb_*; givepose_amd/bb_grad.py; PoseNet.backbone_backward and
head_grads_backbone) against float64.  The bounds are derived in tests/bb_backward_ref.py.

Depth-wise 7x7 and the patch convs: per element |got - ref| <= (K + 8) 2^-24 sum_k |a_k| |b_k|, K counted on all-ones operands; a
tap that meets no pixel has the bound 0, so its d weight must be an exact 0.  LayerNorm, the block, the backbone and the chain: per
tensor max|got - ref| / max|ref| at most 8 times the CPU float32 figure of the same formulas on the same inputs (never less than
2^-24); both figures are printed.  The function is smooth: one float64 reference per case, computed once, serves every test.

Measured on an MI355X (the ratio lines of that run are kept in profiles/backbone_backward.txt):

    depth-wise 7x7, largest error / bound over the six shapes: forward 0.13, dX 0.14, dW 0.18, db 0.04
    patch convs, largest error / bound over the five shapes: forward 0.04, dX 0.01, dW 0.12, db 0.04
    device figure / CPU float32 figure: LayerNorm 0.00 - 1.91, the block 0.31 - 2.48
    the backbone, largest ratio over the gradients, d img and feat (8 allowed):
        A 1.52   B 1.13   C 1.10   D 1.29 (342 tensors)   E 1.72
    the chain (head_grads_backbone, depths (1,1,1,1), B = 2): 1.87 over the 54 new entries; the forward's feat 1.07

The ratios from 2 up, all of the block (2,16,16,512): h 2.21, mlp.fc1.weight 2.48 and mlp.fc2.weight 2.00.  At 512 rows x 2048 columns
fc1 has 256 tiles, the first size at which the shared GEMM stops splitting k (csrc/grad_gemm.hpp, gemm_split): each h element is ONE
k-ordered chain of 512 fmas where torch's CPU matmul sums in blocks, and d fc1.weight and d fc2.weight (256 tiles each, a single chain
over the 512 rows) read that h through GELU' and GELU.  It is the finding of tests/test_xyz_backward_gpu.py (the layer at which the
contraction stops being split) and stays far inside the chain bound.  (1,8,8,1024) and the smaller blocks have fewer tiles, are split,
and stay below 1.9.
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import bb_backward_ref as R
from test_enc_backward_gpu import cuda, yardstick
from test_xyz_backward_gpu import SENTINEL, Guarded, bits, chain_bound, d64, normal, rng, within

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def block_params(r, C):
    p = {"gamma": r.uniform(0.1, 0.3, C).astype(np.float32), "conv_dw.weight": normal(r, C, 1, 7, 7) / 7, "conv_dw.bias": normal(r, C) * np.float32(0.2),
         "norm.weight": 1 + normal(r, C) * np.float32(0.3), "norm.bias": normal(r, C) * np.float32(0.5),
         "mlp.fc1.weight": normal(r, 4 * C, C) / np.float32(np.sqrt(C)), "mlp.fc1.bias": normal(r, 4 * C) * np.float32(0.2),
         "mlp.fc2.weight": normal(r, C, 4 * C) / np.float32(np.sqrt(4 * C)), "mlp.fc2.bias": normal(r, C) * np.float32(0.2)}
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}


# ------------------------------------------------------------------------------------------------ depth-wise 7x7
@pytest.mark.parametrize("N,H,W,C", [(1, 1, 1, 128), (2, 3, 3, 64), (1, 7, 7, 192), (1, 12, 16, 128), (3, 8, 8, 1024), (2, 64, 64, 128)])
def test_dw7_forward_and_backward(N, H, W, C):
    from givepose_amd import bb_grad
    r = rng(N * 100000 + H * 1000 + W * 10 + C)
    x, w, b, dy = normal(r, N, H, W, C), normal(r, C, 1, 7, 7) / 7, normal(r, C) * np.float32(0.2), normal(r, N, H, W, C)
    guard = Guarded()
    y = bb_grad.dw7_forward(*cuda(x, w, b), alloc=guard)
    out = bb_grad.dw7_backward(*cuda(dy, x, w), alloc=guard)
    guard.check()
    assert out["dw"].shape == (C, 1, 7, 7) and out["dx"].shape == (N, H, W, C) and out["db"].shape == (C,)
    x, w, b, dy = d64(x), d64(w), d64(b), d64(dy)
    what = f"dw7 {N} {H} {W} {C}"
    within(y, R.dw7_forward(x, w, b), chain_bound(R.dw7_forward, x, w, b), what + " forward")
    ref = R.dw7_backward(dy, x, w)
    for i, k in enumerate(("dx", "dw", "db")):
        within(out[k], ref[i], chain_bound(lambda a, c, d: R.dw7_backward(a, c, d)[i], dy, x, w), f"{what} {k}")
    dead = R.dead_taps(H, W)
    assert dead.sum() == 49 - min(7, 2 * H - 1) * min(7, 2 * W - 1)
    got = out["dw"].cpu().numpy()[:, 0]
    assert np.all(got[:, dead] == 0) and np.all(got[:, ~dead] != 0)


# ------------------------------------------------------------------------------------------------ LayerNorm over channels
@pytest.mark.parametrize("rows,C", [(1, 128), (7, 64), (300, 1024), (8192, 128)])
def test_layernorm_forward_save_and_backward(rows, C):
    from givepose_amd import bb_grad
    r = rng(rows * 10 + C)
    x = normal(r, rows, C) * (np.float32(0.5) + r.random((1, C)).astype(np.float32)) + normal(r, 1, C)
    w, b, dy = 1 + normal(r, C) * np.float32(0.3), normal(r, C) * np.float32(0.5), normal(r, rows, C)
    guard = Guarded()
    fw = bb_grad.layernorm_forward_save(*cuda(x, w, b), alloc=guard)
    # the backward at the device's own statistics; the references differentiate at the same saved numbers
    bw = bb_grad.layernorm_backward(T(dy).cuda(), T(x).cuda(), fw["mean"], fw["rstd"], T(w).cuda(), alloc=guard)
    guard.check()
    mean, rstd = fw["mean"].cpu().numpy(), fw["rstd"].cpu().numpy()
    f64, f32 = ({**dict(zip(("y", "mean", "rstd"), R.ln_forward(*(T(a).to(dt) for a in (x, w, b))))),
                 **dict(zip(("dx", "dw", "db"), R.ln_backward(*(T(a).to(dt) for a in (dy, x, mean, rstd, w)))))}
                for dt in (torch.float64, torch.float32))
    yardstick({**fw, **bw}, f64, f32, f"layernorm {rows} {C}")


# ------------------------------------------------------------------------------------------------ the block
@pytest.mark.parametrize("N,H,W,C", [(1, 1, 1, 128), (2, 3, 3, 64), (1, 8, 8, 1024), (2, 16, 16, 512)])
def test_block_forward_save_and_backward(N, H, W, C):
    from givepose_amd import bb_grad
    r = rng(N * 100000 + H * 1000 + C + 1)
    P, x, g = block_params(r, C), normal(r, N, H, W, C), normal(r, N, H, W, C)
    guard = Guarded()
    Pd = {k: T(v).cuda() for k, v in P.items()}
    sv = bb_grad.block_forward_save(T(x).cuda(), Pd, alloc=guard)
    out = bb_grad.block_backward(T(g).cuda(), T(x).cuda(), Pd, sv, alloc=guard)
    guard.check()
    assert list(out) == ["dx"] + list(R.BLOCK_KEYS) and all(out[k].shape == Pd[k].shape for k in R.BLOCK_KEYS)
    ref = []
    for dt in (torch.float64, torch.float32):
        Pt, xt, gt = {k: T(v).to(dt) for k, v in P.items()}, T(x).to(dt), T(g).to(dt)
        s = R.block_forward(xt, Pt)
        ref.append({**s, **R.block_backward(gt, xt, Pt, s)})
    assert len(ref[0]) == 6 + 10
    yardstick({**sv, **out}, ref[0], ref[1], f"block {N} {H} {W} {C}")


# ------------------------------------------------------------------------------------------------ patch convs
@pytest.mark.parametrize("shape", [("stem", 1, 4, 64), ("stem", 2, 32, 128), ("down", 1, 2, 2, 64, 128), ("down", 3, 6, 6, 128, 256),
                                   ("down", 1, 16, 16, 512, 1024)], ids=lambda s: "-".join(str(v) for v in s))
def test_patch_conv(shape):
    from givepose_amd import bb_grad
    r = rng(sum(shape[1:]) * 7 + len(shape))
    if shape[0] == "stem":
        _, B, S, Cout = shape
        nchw, p, x, Cin = True, 4, normal(r, B, 3, S, S), 3
        rows = B * (S // 4) ** 2
    else:
        _, N, H, W, Cin, Cout = shape
        nchw, p, x = False, 2, normal(r, N, H, W, Cin)
        rows = N * (H // 2) * (W // 2)
    w, b, dy = normal(r, Cout, Cin, p, p) / np.float32(np.sqrt(Cin * p * p)), normal(r, Cout), normal(r, rows, Cout)
    guard = Guarded()
    y = bb_grad.patch_conv_forward(*cuda(x, w, b), nchw, alloc=guard)
    out = bb_grad.patch_conv_backward(*cuda(dy, x, w), nchw, alloc=guard)
    guard.check()
    assert out["dX"].shape == x.shape and out["dW"].shape == w.shape and out["db"].shape == (Cout,)
    x, w, b, dy = d64(x), d64(w), d64(b), d64(dy)
    what = "patch conv " + " ".join(str(v) for v in shape)
    within(y, R.patch_forward(x, w, b, nchw), chain_bound(lambda a, c, d: R.patch_forward(a, c, d, nchw), x, w, b), what + " forward")
    ref = R.patch_backward(dy, x, w, nchw)
    for i, k in enumerate(("dX", "dW", "db")):
        within(out[k], ref[i], chain_bound(lambda a, c, d: R.patch_backward(a, c, d, nchw)[i], dy, x, w), f"{what} {k}")


# ------------------------------------------------------------------------------------------------ the backbone
@functools.lru_cache(maxsize=None)
def device_params(dims, depths):
    return {k: T(v).cuda() for k, v in R.bb_params(dims, depths).items()}


def run_backbone(case, g_scale=1.0, guard=None, g_edit=None):
    from givepose_amd import bb_grad
    dims, depths, B, S = R.CASES[case]
    _, img, g = R.case_inputs(case)
    g = T(g).cuda() * g_scale
    if g_edit is not None:
        g_edit(g)
    P, img = device_params(dims, depths), T(img).cuda()
    saved, feat = bb_grad.backbone_forward_save(img, P, (dims, depths), alloc=guard)
    grads, d_img = bb_grad.backbone_backward(P, saved, img, g, (dims, depths), alloc=guard)
    torch.cuda.synchronize()
    return {**grads, "img": d_img, "feat": feat}


class GuardedNear(Guarded):
    """Guarded for tensors of millions of elements at scales above the sentinel: a true gradient can land ON the sentinel (case E:
    stages_3.downsample.1.weight holds -7.2499972 among 2 097 152 elements of up to 71.7, and a device rounding puts it at -7.25).  An
    element whose float64 reference lies within 1e-4 max|ref| of the sentinel -- five times what the yardstick lets the device differ by --
    is exempt from the was-it-written test; the yardstick holds it all the same."""

    def __init__(self, ref):
        super().__init__()
        self.ref = ref

    def check(self):
        torch.cuda.synchronize()
        assert self.bufs
        for name, whole, view in self.bufs:
            assert torch.all(whole[:64] == SENTINEL) and torch.all(whole[-64:] == SENTINEL), name
            if name != "workspace":
                hit = view == SENTINEL
                if name in self.ref:
                    r = np.asarray(self.ref[name])
                    hit &= T(np.abs(r - SENTINEL) > 1e-4 * np.abs(r).max()).to(hit.device)
                assert not torch.any(hit), name
                assert torch.all(torch.isfinite(view)), name


@pytest.mark.parametrize("case", list(R.CASES))
def test_backbone_end_to_end(case):
    """gpb_backbone_forward_save and gpb_backbone_backward against the float64 restatement: feat, d img and every parameter gradient,
    each in its parameter's shape, under its state_dict name and in state_dict order; the guarded allocator's sentinels stay intact."""
    from givepose_amd import bb_grad
    dims, depths, B, S = R.CASES[case]
    r64, r32 = R.reference(case)
    guard = GuardedNear(r64)
    got = run_backbone(case, guard=guard)
    guard.check()
    shapes = bb_grad.param_shapes((dims, depths))
    assert list(got) == bb_grad.PARAM_KEYS((dims, depths)) + ["img", "feat"] == list(r64)
    for k, s in shapes.items():
        assert tuple(got[k].shape) == s and got[k].is_contiguous(), k
    assert got["img"].shape == (B, 3, S, S) and got["feat"].shape == (B, dims[-1], S // 32, S // 32)
    worst = yardstick({k: v.cpu().numpy() for k, v in got.items()}, r64, r32, f"backbone {case}")
    print(f"backbone {case}: largest ratio {worst:.2f} over {len(got)} tensors")


@pytest.mark.parametrize("case", ["A", "E"])
def test_equal_bits_and_bitwise_linearity(case):
    """No atomic anywhere: two runs give equal bits, and g_feat x 2 gives every gradient x 2 bit for bit."""
    a, b, c = run_backbone(case), run_backbone(case), run_backbone(case, g_scale=2.0)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k
        assert torch.equal(bits(c[k]), bits(a[k] if k == "feat" else 2 * a[k])), k
        assert float(a[k].abs().max()) > 0, k


def test_a_crop_without_upstream_gradient_gets_none():
    """Case B with crop 1's g_feat set to zero: d img of crop 1 is exactly 0 and nonzero elsewhere."""
    def edit(g):
        g[1] = 0
    d = run_backbone("B", g_edit=edit)["img"]
    assert torch.all(d[1] == 0) and bool((d[0] != 0).any()) and bool((d[2] != 0).any())


def test_refusals_by_name():
    """A workspace smaller than the size query's answer, a dim that is not a multiple of 64 and the resnet34 backbone."""
    from givepose_amd import PoseNet, PoseNetConfig, _lib, bb_grad
    from givepose_amd.pnp_grad import _stream
    L = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    x, w, dy = (torch.zeros(s, device=dev) for s in ((2, 3, 3, 64), (64, 1, 7, 7), (2, 3, 3, 64)))
    dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty(64, device=dev)
    nbytes = L.gpb_dw7_backward_workspace(2, 3, 3, 64)
    ws = torch.empty(nbytes // 4, device=dev)
    args = (dy.data_ptr(), x.data_ptr(), w.data_ptr(), 2, 3, 3, 64, dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr())
    assert nbytes > 256 and L.gpb_dw7_backward(*args, nbytes, _stream(dev)) == 0
    with pytest.raises(_lib.GivePoseHipError, match="gpb_dw7_backward: workspace"):
        _lib.check(L.gpb_dw7_backward(*args, nbytes - 256, _stream(dev)), "gpb_dw7_backward")
    dims, depths, B, S = R.CASES["A"]
    cfg, P, img = (dims, depths), device_params(dims, depths), torch.zeros(B, 3, S, S, device=dev)
    saved = {k: torch.empty(s, device=dev) for k, s in bb_grad.saved_shapes(cfg, B, S).items()}
    pt, vt = bb_grad._table(P, bb_grad.param_shapes(cfg), dev, "params"), bb_grad._table(saved, bb_grad.saved_shapes(cfg, B, S), dev, "saved")
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    nbytes = L.gpb_backbone_forward_workspace(ints(dims), ints(depths), 4, B, S)
    ws, feat = torch.empty(nbytes // 4, device=dev), torch.empty(B, dims[-1], 1, 1, device=dev)
    with pytest.raises(_lib.GivePoseHipError, match="gpb_backbone_forward_save: workspace"):
        _lib.check(L.gpb_backbone_forward_save(img.data_ptr(), pt, ints(dims), ints(depths), 4, B, S, vt, feat.data_ptr(), ws.data_ptr(), nbytes - 256,
                                               _stream(dev)), "gpb_backbone_forward_save")
    with pytest.raises(_lib.GivePoseHipError, match=r"dims\[2\] = 500 is not a multiple of 64"):
        _lib.check(L.gpb_backbone_forward_save(img.data_ptr(), pt, ints((128, 256, 500, 1024)), ints(depths), 4, B, S, vt, feat.data_ptr(),
                                               ws.data_ptr(), nbytes, _stream(dev)), "gpb_backbone_forward_save")
    with pytest.raises(ValueError, match=r"dims\[1\] = 200 is not a multiple of 64"):
        bb_grad.backbone_forward_save(img, P, ((128, 200, 512, 1024), depths))
    with pytest.raises(ValueError, match="C = 96 is not a multiple of 64"):
        bb_grad.dw7_forward(torch.zeros(1, 2, 2, 96, device=dev), torch.zeros(96, 1, 7, 7, device=dev), torch.zeros(96, device=dev))
    with pytest.raises(ValueError, match="float32"):
        bb_grad.dw7_forward(x.double(), w, db)
    with pytest.raises(ValueError, match="not contiguous"):
        bb_grad.dw7_forward(torch.zeros(2, 3, 64, 3, device=dev).permute(0, 1, 3, 2), w, db)
    with pytest.raises(NotImplementedError, match="resnet34"):
        PoseNet(PoseNetConfig(main_backbone="resnet34")).backbone_backward(img, torch.zeros(B, 512, 1, 1, device=dev))


# ------------------------------------------------------------------------------------------------ PoseNet.head_grads_backbone
def test_head_grads_backbone_chain():
    """head_grads_backbone on a network of depths (1,1,1,1) at B = 2: head_grads_feat's entries bit for bit; the keys of param_grads are
    the network's parameters minus size_head.* and the never-applied dcnv3.bn.*; the new entries within the yardstick of the float64
    restatement run from data["roi_img"] and the device's own d feat; the recompute's feat and the forward's feat within the yardstick of
    the float64 feat."""
    import pose_loss_grad_ref as G
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, bb_grad
    from test_xyz_backward_gpu import loss_batch
    cfg = PoseNetConfig(convnext_depths=(1, 1, 1, 1))
    net = PoseNet(cfg, dtype=torch.float32, seed=R.WEIGHT_SEED).cuda()
    data = {k: v[:2] if v.dim() and v.shape[0] == 4 else v for k, v in loss_batch().items()}
    pl, w = PoseLoss(), T(G.make_gout())
    # head_grads_feat scatters d xp with fp32 atomics (include/givepose_encgrad.h): two calls of it agree bit for bit only outside what
    # follows a scatter.  So the shared entries are compared, all of them bit for bit, with what the head_grads_feat call INSIDE
    # head_grads_backbone returned (copied at its return), and with a second call bit for bit where no scatter feeds, else to rounding.
    seen, inner = {}, net.head_grads_feat

    def copied(v):
        return {k: copied(x) for k, x in v.items()} if isinstance(v, dict) else v.clone() if torch.is_tensor(v) else v

    def spy(*a, **k):
        r = inner(*a, **k)
        torch.cuda.synchronize()
        seen["res"] = copied(r)
        return r
    net.head_grads_feat = spy
    try:
        res = net.head_grads_backbone(data, pl, "cuda", gout=w)
    finally:
        del net.head_grads_feat
    base = net.head_grads_feat(data, pl, "cuda", gout=w)
    torch.cuda.synchronize()
    assert list(res) == list(base) and list(res["grads"]) == list(base["grads"]) + ["roi_img"]
    from givepose_amd import enc_grad
    from test_xyz_backward_gpu import same_bits
    for part in ("loss", "output"):
        same_bits(res[part], seen["res"][part], part)
        same_bits(res[part], base[part], part)
    after_scatter = {"nocs_coor", "nocs_coor_from_encoder", "feat_from_nocs_head", "feat"}
    for part, exact in (("grads", lambda k: k not in after_scatter),
                        ("param_grads", lambda k: k.split(".")[0] in ("pnp_net", "xyz_deform_head", "feat_reducer")
                         or k[len("nocs_encoder."):] in enc_grad.ATOMIC_FREE_KEYS)):
        assert list(seen["res"][part]) == list(base[part])
        for k, v in base[part].items():
            assert torch.equal(bits(res[part][k]), bits(seen["res"][part][k])), (part, k)
            if exact(k):
                assert torch.equal(bits(res[part][k]), bits(v)), (part, k)
            else:
                assert float((res[part][k] - v).abs().max()) <= 1e-4 * float(v.abs().max()), (part, k)
    # every name: a ConvModule's norm is registered under two names (.norm. / .gn.) and head_grads_feat reports both
    # (the never-applied BatchNorm of DCNv3_C is nocs_encoder.features.N.bn.*)
    names = [k for k, _ in net.named_parameters(remove_duplicate=False)
             if not k.startswith("size_head.") and not re.match(r"nocs_encoder\.features\.\d+\.bn\.", k)]
    assert set(res["param_grads"]) == set(names) and len(res["param_grads"]) == len(names)
    new = [k for k in res["param_grads"] if k not in base["param_grads"]]
    assert new == ["backbone." + k for k in bb_grad.PARAM_KEYS(cfg)] and len(new) == 4 + 12 + 36
    # the float64 restatement from the same image and the device's own d feat
    img, gf = data["roi_img"].float().numpy(), res["grads"]["feat"].cpu().numpy()
    params = {k[len("backbone."):]: v.detach().float().cpu().numpy() for k, v in net.state_dict().items() if k.startswith("backbone.") and k in new}
    r64, r32 = (R.flat(R.backbone_run(params, img, gf, cfg.convnext_dims, cfg.convnext_depths, dt)) for dt in (torch.float64, torch.float32))
    back = net.backbone_backward(data["roi_img"], res["grads"]["feat"])
    got = {**{k[len("backbone."):]: res["param_grads"][k] for k in new}, "img": res["grads"]["roi_img"], "feat": back["outputs"]["feat"]}
    for k in new:      # no atomic: the method alone gives the chain's bits
        assert torch.equal(bits(back["param_grads"][k]), bits(res["param_grads"][k])), k
    worst = yardstick(got, r64, r32, "chain")
    print(f"chain: largest ratio {worst:.2f} over the {len(got)} new entries")
    fwd = net.forward_device({**data, "roi_mask": data["roi_mask_deform"]}, "cuda")
    feat = fwd["feat"].permute(0, 3, 1, 2).float().contiguous()
    yardstick({"feat": feat}, {"feat": r64["feat"]}, {"feat": r32["feat"]}, "chain, the forward's feat")
