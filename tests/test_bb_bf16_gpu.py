"""GPU: the "bf16" precision of the backbone backward (include/givepose_bbgrad_bf16.h, gpbm_*; csrc/grad_gemm_bf16.hpp;
bb_grad.matmul_bf16 and precision="bf16"; PoseNet.set_backward_precision).

The kernel, per element.  The reference is float64 on the bf16-rounded operands, so what is left is the fp32 accumulation:
|got - ref| <= (K + 8) u sum_k |a_k| |b_k| with u = 2^-24, the project's chain bound.  Any fp32 accumulation with one rounding per add
meets it in any order; a kernel that does not round its operands misses it by four orders of magnitude.

The block, the backbone and PoseNet.  Per tensor, max|got - f64| / max|f64| of the device in bf16 mode is at most 8 times (the project's
yardstick factor) the same figure of the CPU float32 restatement with the bf16 rounding hook (tests/bb_bf16_ref.py); both against the
UNROUNDED float64 restatement on the same inputs, both printed.

Measured on an MI355X (the ratio lines of that run are kept in profiles/backbone_backward_bf16.txt):

    matmul_bf16, largest error / bound over the nine shapes: 0.036 (u = 2^-24 holds: the MFMA's adder needs no wider unit)
    device figure / CPU float32-with-hook figure, largest per test: the block 1.27 - 1.87; the backbone A 1.96, C 1.56; PoseNet 1.78
"""
import functools

import numpy as np
import pytest
import torch

import bb_backward_ref as R
import bb_bf16_ref as Q
from test_bb_backward_gpu import GuardedNear, block_params, device_params
from test_enc_backward_gpu import cuda, yardstick
from test_xyz_backward_gpu import Guarded, bits, chain_bound, normal, rng, within

pytestmark = pytest.mark.gpu
T = torch.from_numpy

# (M, N, K, trans_a, trans_b): the issue's seven, and two that the 128 x 128 tile does not split (k <= one step; 256 tiles)
MATMUL = [(1, 64, 64, 0, 0), (18, 256, 64, 0, 0), (65, 129, 33, 0, 0), (64, 4096, 1024, 0, 0), (512, 2048, 512, 0, 0),
          (256, 64, 4608, 1, 0), (130, 70, 40, 0, 1), (300, 200, 31, 1, 1), (2048, 2048, 96, 0, 0)]


@pytest.mark.parametrize("M,N,K,ta,tb", MATMUL, ids=lambda v: str(v))
def test_matmul_bf16_per_element(M, N, K, ta, tb):
    """bb_grad.matmul_bf16 under the guarded allocator against float64 on the rounded operands; equal bits between two calls; a x 2
    gives the result x 2 bit for bit."""
    from givepose_amd import bb_grad
    r = rng(M * 1000003 + N * 1009 + K * 7 + ta * 2 + tb)
    a, b = normal(r, *((K, M) if ta else (M, K))), normal(r, *((N, K) if tb else (K, N)))
    ar, br = Q.round_bf16(T(a)), Q.round_bf16(T(b))
    assert float((ar != T(a)).float().mean()) > 0.9 and float((br != T(b)).float().mean()) > 0.9      # not bf16-representable
    guard = Guarded()
    ad, bd = cuda(a, b)
    got = bb_grad.matmul_bf16(ad, bd, trans_a=ta, trans_b=tb, alloc=guard)
    guard.check()
    assert got.shape == (M, N)

    def product(x, y):
        return (x.T if ta else x) @ (y.T if tb else y)
    what = f"matmul_bf16 {M} {N} {K} trans {ta}{tb}"
    within(got, product(ar.double(), br.double()), chain_bound(product, ar.double(), br.double()), what)
    again = bb_grad.matmul_bf16(ad, bd, trans_a=ta, trans_b=tb)
    twice = bb_grad.matmul_bf16(2 * ad, bd, trans_a=ta, trans_b=tb)
    assert torch.equal(bits(got), bits(again)), what
    assert torch.equal(bits(twice), bits(2 * got)), what


def test_matmul_bf16_refusals():
    from givepose_amd import _lib, bb_grad
    from givepose_amd.pnp_grad import _stream
    dev = torch.device("cuda", torch.cuda.current_device())
    a, b = torch.zeros(4, 8, device=dev), torch.zeros(8, 4, device=dev)
    with pytest.raises(ValueError, match="do not contract"):
        bb_grad.matmul_bf16(a, a)
    with pytest.raises(ValueError, match="float32"):
        bb_grad.matmul_bf16(a.double(), b)
    L = _lib.load()
    big_a, big_b, c = torch.zeros(64, 1024, device=dev), torch.zeros(1024, 4096, device=dev), torch.empty(64, 4096, device=dev)
    nbytes = L.gpbm_matmul_bf16_workspace(64, 4096, 1024)
    ws = torch.empty(nbytes // 4, device=dev)
    args = (big_a.data_ptr(), big_b.data_ptr(), 64, 4096, 1024, 0, 0, c.data_ptr(), ws.data_ptr())
    assert L.gpbm_matmul_bf16(*args, nbytes, _stream(dev)) == 0
    with pytest.raises(_lib.GivePoseHipError, match="gpbm_matmul_bf16: workspace"):
        _lib.check(L.gpbm_matmul_bf16(*args, nbytes - 256, _stream(dev)), "gpbm_matmul_bf16")
    # an unknown precision is refused by name
    x = torch.zeros(1, 1, 1, 64, device=dev)
    P = {k: torch.zeros(s, device=dev) for k, s in bb_grad.block_shapes(64).items()}
    st = bb_grad._block_struct(P, 64, dev, "params")
    import ctypes
    out = [torch.empty(s, device=dev) for s in ((1, 64), (1,), (1,), (1, 256), (1, 64), (1, 64))]
    nb = L.gpbm_block_workspace(1, 1, 1, 64, 1)
    wsb = torch.empty(nb // 4, device=dev)
    with pytest.raises(_lib.GivePoseHipError, match="gpbm_block_forward_save: unknown precision 5"):
        _lib.check(L.gpbm_block_forward_save(x.data_ptr(), ctypes.byref(st), 1, 1, 1, 64, *(o.data_ptr() for o in out), wsb.data_ptr(), nb,
                                             _stream(dev), 5), "gpbm_block_forward_save")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the block
@pytest.mark.parametrize("N,H,W,C", [(1, 1, 1, 128), (2, 3, 3, 64), (1, 8, 8, 1024), (2, 16, 16, 512)])
def test_block_bf16(N, H, W, C):
    from givepose_amd import bb_grad
    r = rng(N * 100000 + H * 1000 + C + 1)
    P, x, g = block_params(r, C), normal(r, N, H, W, C), normal(r, N, H, W, C)
    guard = Guarded()
    Pd, xd, gd = {k: T(v).cuda() for k, v in P.items()}, T(x).cuda(), T(g).cuda()
    sv = bb_grad.block_forward_save(xd, Pd, alloc=guard, precision="bf16")
    out = bb_grad.block_backward(gd, xd, Pd, sv, alloc=guard, precision="bf16")
    guard.check()
    assert list(out) == ["dx"] + list(R.BLOCK_KEYS) and all(out[k].shape == Pd[k].shape for k in R.BLOCK_KEYS)
    P64, x64, g64 = {k: T(v).double() for k, v in P.items()}, T(x).double(), T(g).double()
    s64 = R.block_forward(x64, P64)
    ref64 = {**s64, **R.block_backward(g64, x64, P64, s64)}
    P32 = {k: T(v) for k, v in P.items()}
    s32 = Q.block_forward(T(x), P32, Q.round_bf16)
    ref32 = {**s32, **Q.block_backward(T(g), T(x), P32, s32, Q.round_bf16)}
    assert len(ref64) == len(ref32) == 6 + 10
    worst = yardstick({**sv, **out}, ref64, ref32, f"block bf16 {N} {H} {W} {C}")
    print(f"block bf16 {N} {H} {W} {C}: largest ratio {worst:.2f}")
    # precision="fp32" is the call without the keyword, bit for bit
    sa, sb = bb_grad.block_forward_save(xd, Pd), bb_grad.block_forward_save(xd, Pd, precision="fp32")
    oa, ob = bb_grad.block_backward(gd, xd, Pd, sa), bb_grad.block_backward(gd, xd, Pd, sb, precision="fp32")
    for k in sa:
        assert torch.equal(bits(sa[k]), bits(sb[k])), k
    for k in oa:
        assert torch.equal(bits(oa[k]), bits(ob[k])), k
    # the mode is in the arithmetic: the fc1 pre-activation differs from the fp32 mode's by about a bf16 rounding
    d = float((sv["h"] - sa["h"]).abs().max() / sa["h"].abs().max())
    assert 2.0 ** -14 < d < 2.0 ** -6, d


# ------------------------------------------------------------------------------------------------ the backbone
def run_backbone(case, g_scale=1.0, guard=None, forward="bf16", backward="bf16"):
    from givepose_amd import bb_grad
    dims, depths, B, S = R.CASES[case]
    _, img, g = R.case_inputs(case)
    g = T(g).cuda() * g_scale
    P, img = device_params(dims, depths), T(img).cuda()
    saved, feat = bb_grad.backbone_forward_save(img, P, (dims, depths), alloc=guard, precision=forward)
    grads, d_img = bb_grad.backbone_backward(P, saved, img, g, (dims, depths), alloc=guard, precision=backward)
    torch.cuda.synchronize()
    return {**grads, "img": d_img, "feat": feat}


@functools.lru_cache(maxsize=None)
def references(case):
    return R.reference(case)[0], Q.reference_bf16(case)


@pytest.mark.parametrize("case", ["A", "C"])
def test_backbone_bf16(case):
    """Every gradient, d img and feat within the yardstick; equal bits across two runs; a saved table written in one mode is accepted by
    the backward of the other."""
    from givepose_amd import bb_grad
    dims, depths, B, S = R.CASES[case]
    r64, r32 = references(case)
    guard = GuardedNear(r64)
    got = run_backbone(case, guard=guard)
    guard.check()
    assert list(got) == bb_grad.PARAM_KEYS((dims, depths)) + ["img", "feat"] == list(r64)
    worst = yardstick({k: v.cpu().numpy() for k, v in got.items()}, r64, r32, f"backbone bf16 {case}")
    print(f"backbone bf16 {case}: largest ratio {worst:.2f} over {len(got)} tensors")
    again = run_backbone(case)
    for k in got:
        assert torch.equal(bits(got[k]), bits(again[k])), k
    fp32 = run_backbone(case, forward="fp32", backward="fp32")
    assert not torch.equal(bits(fp32["feat"]), bits(got["feat"]))
    for fw, bw in (("fp32", "bf16"), ("bf16", "fp32")):
        mixed = run_backbone(case, forward=fw, backward=bw)
        assert torch.equal(bits(mixed["feat"]), bits((fp32 if fw == "fp32" else got)["feat"]))
        yardstick({k: v.cpu().numpy() for k, v in mixed.items()}, r64, r32, f"backbone {case}, forward {fw}, backward {bw}")


def test_backbone_bf16_bitwise_linearity():
    """Case A: g_feat x 2 gives every gradient x 2 bit for bit."""
    a, c = run_backbone("A"), run_backbone("A", g_scale=2.0)
    for k in a:
        assert torch.equal(bits(c[k]), bits(a[k] if k == "feat" else 2 * a[k])), k
        assert float(a[k].abs().max()) > 0, k


# ------------------------------------------------------------------------------------------------ PoseNet
def test_posenet_backward_precision():
    """depths (1,1,1,1), B = 2, as tests/test_bb_backward_gpu.py::test_head_grads_backbone_chain."""
    import pose_loss_grad_ref as G
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, Ranger, bb_grad
    from test_xyz_backward_gpu import loss_batch, same_bits
    cfg = PoseNetConfig(convnext_depths=(1, 1, 1, 1))
    net = PoseNet(cfg, dtype=torch.float32, seed=R.WEIGHT_SEED).cuda()
    assert net.backward_precision == "fp32"
    data = {k: v[:2] if v.dim() and v.shape[0] == 4 else v for k, v in loss_batch().items()}
    pl, w = PoseLoss(), T(G.make_gout())
    new = ["backbone." + k for k in bb_grad.PARAM_KEYS(cfg)]
    clone = lambda d: {k: v.clone() for k, v in d.items()}
    # the backbone alone has no atomic: its bits are recorded in fp32 mode, from the device's own d feat
    feat_res = net.head_grads_feat(data, pl, "cuda", gout=w)
    g_feat = feat_res["grads"]["feat"].clone()
    back32 = net.backbone_backward(data["roi_img"], g_feat)
    rec = {**clone(back32["param_grads"]), "img": back32["img"].clone(), "feat": back32["outputs"]["feat"].clone()}
    with pytest.raises(ValueError, match="expected 'fp32' or 'bf16'"):
        net.set_backward_precision("fp16")
    net.set_backward_precision("bf16")
    assert net.backward_precision == "bf16"
    # every entry head_grads_backbone shares with head_grads_feat has the bits it has in fp32 mode: those of the head_grads_feat call
    # inside it, whatever the mode (head_grads_feat scatters with atomics, so two calls of it are compared where no scatter feeds)
    seen, inner = {}, net.head_grads_feat

    def spy(*a, **k):
        r = inner(*a, **k)
        torch.cuda.synchronize()
        seen["res"] = {p: clone(r[p]) for p in ("grads", "param_grads")}
        return r
    net.head_grads_feat = spy
    try:
        res = net.head_grads_backbone(data, pl, "cuda", gout=w)
    finally:
        del net.head_grads_feat
    for part in ("loss", "output"):
        same_bits(res[part], feat_res[part], part)
    from givepose_amd import enc_grad
    after_scatter = {"nocs_coor", "nocs_coor_from_encoder", "feat_from_nocs_head", "feat"}
    for part, exact in (("grads", lambda k: k not in after_scatter),
                        ("param_grads", lambda k: k.split(".")[0] in ("pnp_net", "xyz_deform_head", "feat_reducer")
                         or k[len("nocs_encoder."):] in enc_grad.ATOMIC_FREE_KEYS)):
        assert list(seen["res"][part]) == list(feat_res[part])
        for k, v in seen["res"][part].items():
            assert torch.equal(bits(res[part][k]), bits(v)), (part, k)
            if exact(k):
                assert torch.equal(bits(v), bits(feat_res[part][k])), (part, k)
    assert [k for k in res["param_grads"] if k not in feat_res["param_grads"]] == new
    # the backbone gradients in bf16 mode, from the same d feat as the record: the yardstick
    back16 = net.backbone_backward(data["roi_img"], g_feat)
    img = data["roi_img"].float().numpy()
    params = {k[len("backbone."):]: v.detach().float().cpu().numpy() for k, v in net.state_dict().items() if k in new}
    r64 = R.flat(R.backbone_run(params, img, g_feat.cpu().numpy(), cfg.convnext_dims, cfg.convnext_depths, torch.float64))
    r32 = R.flat(Q.backbone_run(params, img, g_feat.cpu().numpy(), cfg.convnext_dims, cfg.convnext_depths))
    got = {**{k[len("backbone."):]: back16["param_grads"][k] for k in new}, "img": back16["img"], "feat": back16["outputs"]["feat"]}
    worst = yardstick(got, r64, r32, "PoseNet bf16")
    print(f"PoseNet bf16: largest ratio {worst:.2f} over {len(got)} tensors")
    assert not torch.equal(bits(got["feat"]), bits(rec["feat"]))
    # one train_step in bf16 mode; the forward after it is that of a fresh model with the updated parameters
    fdata = {**data, "roi_mask": data["roi_mask_deform"]}
    tensors = lambda out: {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    step = net.train_step(data, pl, Ranger(net), "cuda")
    assert set(step["param_grads"]) >= set(new) and all(bool(torch.isfinite(v).all()) for v in step["param_grads"].values())
    sd = net.state_dict()
    assert all(not torch.equal(sd[k], before[k]) for k in new)
    fwd = tensors(net.forward_device(fdata, "cuda"))
    fresh = PoseNet(cfg, dtype=torch.float32).cuda()
    fresh.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    same_bits(tensors(fresh.forward_device(fdata, "cuda")), fwd, "forward after the bf16 step")
    # back to fp32 at the parameters of the record: the recorded bits
    net.load_state_dict(before)
    net.set_backward_precision("fp32")
    assert net.backward_precision == "fp32"
    back = net.backbone_backward(data["roi_img"], g_feat)
    for k, v in {**back["param_grads"], "img": back["img"], "feat": back["outputs"]["feat"]}.items():
        assert torch.equal(bits(v), bits(rec[k])), k
