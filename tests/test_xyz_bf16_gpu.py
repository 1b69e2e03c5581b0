"""GPU: the "bf16" precision of the coordinate heads (include/givepose_xyzgrad_bf16.h, gpxm_*; csrc/xyz_conv_prec.hpp on
csrc/grad_gemm_bf16.hpp; xyz_grad's precision="bf16"; PoseNet.set_backward_precision(mode, xyz_heads="bf16")).

The contractions, per element.  The reference is float64 on the bf16-rounded operands, so what is left is the fp32 accumulation:
|got - ref| <= (K + 8) u sum_k |a_k| |b_k| with u = 2^-24, the project's chain bound, K the number of terms that exist in the element's
sum.  A kernel that does not round its operands, reads another element at a map edge or a crop boundary, or drops a term on ragged k
misses it by orders of magnitude.  The shapes are the smallest at which the staging of a window view can go wrong (see CONV / DECONV).

The head and PoseNet.  Per tensor, max|got - f64| / max|f64| of the device in bf16 mode is at most 8 times (the project's yardstick
factor) the same figure of the CPU float32 restatement with the bf16 rounding hook (tests/xyz_bf16_ref.py); both against the UNROUNDED
float64 restatement on the same inputs, both printed.

Measured on an MI355X (the ratio lines of that run are kept in profiles/xyz_backward_bf16.txt):

    contractions, largest error / bound: stride-1 conv 0.035 (forward of (2, 8, 256, 128)), transposed conv 0.134 (dW of (3, 64, 256, 2))
    device figure / CPU float32-with-hook figure, largest per case: the head 1.36 / 1.82 / 1.95 (the same with the saved table of the other
    mode); PoseNet 1.18 (xyz_deform_head), 1.13 .. 1.16 (xyz_nocs_head, over three runs); pre0 differs from the fp32 mode's by 2.3e-3 .. 2.7e-3 of its largest element

PoseNet.xyz_head_backward has no per-call precision keyword: tests/test_xyz_backward_cpu.py pins its signature, so the method reads
`xyz_backward_precision` and these tests switch the mode through the setter.
"""
import numpy as np
import pytest
import torch

import xyz_backward_ref as R
import xyz_bf16_ref as Q
from test_enc_backward_gpu import yardstick
from test_xyz_backward_gpu import Guarded, bits, chain_bound, normal, rng, within

pytestmark = pytest.mark.gpu
T = torch.from_numpy

# (B, Cin, Cout, H) of the stride-1 conv: H no multiple of 4 and HW = 25, so that a group of four k-neighbours crosses row and crop ends,
# K = 27 less than one k step, M and N less than a tile; M exactly one tile and K = 216 ragged against 32; 64 tiles: split k; the head's
# own channel count, K = 2304, split; 512 tiles: the unsplit path
CONV = [(1, 3, 5, 5), (2, 24, 40, 8), (1, 8, 256, 64), (3, 256, 256, 16), (2, 8, 256, 128)]
DECONV = [(1, 5, 7, 3), (2, 512, 256, 8), (3, 64, 256, 2)]


def rounded64(*arrays):
    """The bf16-rounded operands in float64, after asserting that most elements are not bf16-representable."""
    out = []
    for a in arrays:
        r = Q.round_bf16(T(a))
        assert float((r != T(a)).float().mean()) > 0.9
        out.append(r.double())
    return out


def per_element(what, fwd, bwd, ref_fwd, ref_bwd, dY, X, W):
    """forward, dX and dW in bf16 under the guarded allocator against float64 on the rounded operands; two calls agree bit for bit; the
    input x 2 gives the result x 2 bit for bit; precision="fp32" is the call without the keyword."""
    guard = Guarded()
    dYd, Xd, Wd = (T(a).cuda() for a in (dY, X, W))
    Y = fwd(Xd, Wd, alloc=guard, precision="bf16")
    out = bwd(dYd, Xd, Wd, alloc=guard, precision="bf16")
    guard.check()
    dY64, X64, W64 = rounded64(dY, X, W)
    within(Y, ref_fwd(X64, W64), chain_bound(ref_fwd, X64, W64), f"{what} forward")
    ref = ref_bwd(dY64, X64, W64)
    for i, k in enumerate(("dX", "dW")):
        within(out[k], ref[i], chain_bound(lambda a, b, c: ref_bwd(a, b, c)[i], dY64, X64, W64), f"{what} {k}")
    again, again_b = fwd(Xd, Wd, precision="bf16"), bwd(dYd, Xd, Wd, precision="bf16")
    twice, twice_b = fwd(2 * Xd, Wd, precision="bf16"), bwd(2 * dYd, Xd, Wd, precision="bf16")
    assert torch.equal(bits(Y), bits(again)) and torch.equal(bits(twice), bits(2 * Y)), what
    for k in ("dX", "dW"):
        assert torch.equal(bits(out[k]), bits(again_b[k])) and torch.equal(bits(twice_b[k]), bits(2 * out[k])), (what, k)
    plain, plain_b = fwd(Xd, Wd), bwd(dYd, Xd, Wd)
    named, named_b = fwd(Xd, Wd, precision="fp32"), bwd(dYd, Xd, Wd, precision="fp32")
    assert torch.equal(bits(plain), bits(named)) and not torch.equal(bits(plain), bits(Y)), what
    for k in ("dX", "dW"):
        assert torch.equal(bits(plain_b[k]), bits(named_b[k])), (what, k)


@pytest.mark.parametrize("B,Cin,Cout,H", CONV)
def test_conv3x3s1_bf16_per_element(B, Cin, Cout, H):
    from givepose_amd import xyz_grad
    r = rng(B * 1000 + Cin + H + 0xBF)
    dY, X, W = normal(r, B, Cout, H, H), normal(r, B, Cin, H, H), normal(r, Cout, Cin, 3, 3) / np.float32(np.sqrt(9 * Cin))
    per_element(f"conv3x3 bf16 {B} {Cin} {Cout} {H}", xyz_grad.conv3x3s1_forward, xyz_grad.conv3x3s1_backward, R.conv3x3_forward,
                R.conv3x3_backward, dY, X, W)


@pytest.mark.parametrize("B,Cin,Cout,H", DECONV)
def test_deconv3x3s2_bf16_per_element(B, Cin, Cout, H):
    from givepose_amd import xyz_grad
    r = rng(B * 1000 + Cin + H + 0xBF)
    dY, X, W = normal(r, B, Cout, 2 * H, 2 * H), normal(r, B, Cin, H, H), normal(r, Cin, Cout, 3, 3) / np.float32(np.sqrt(9 * Cin / 4))
    per_element(f"deconv bf16 {B} {Cin} {Cout} {H}", xyz_grad.deconv3x3s2_forward, xyz_grad.deconv3x3s2_backward, R.deconv_forward,
                R.deconv_backward, dY, X, W)


@pytest.mark.parametrize("H", [5, 8])
def test_conv3x3s1_bf16_dx_exact_edges(H):
    """bf16-representable weights and an impulse of 1.0 as dY: dX is the weights, flipped and clipped at the map, and an exact 0 everywhere
    else -- a single-term sum of representable values has no rounding.  Every corner, an edge centre and an interior pixel."""
    from givepose_amd import xyz_grad
    r = rng(77 + H)
    C = 4
    W = normal(r, C, C, 3, 3)
    W = Q.round_bf16(T(np.sign(W) * (np.abs(W) + np.float32(0.25)))).numpy()
    assert np.all(W != 0)
    X = np.zeros((2, C, H, H), np.float32)
    for n, (oh, ow) in enumerate([(0, 0), (0, H - 1), (H - 1, 0), (H - 1, H - 1), (0, H // 2), (H // 2, H - 1), (H // 2, H // 2 - 1)]):
        dY = np.zeros((2, C, H, H), np.float32)
        b, co = n % 2, n % C
        dY[b, co, oh, ow] = 1.0
        dX = xyz_grad.conv3x3s1_backward(T(dY).cuda(), T(X).cuda(), T(W).cuda(), precision="bf16")["dX"].cpu().numpy()
        want = np.zeros_like(dX)
        for ih in range(max(0, oh - 1), min(H, oh + 2)):
            for iw in range(max(0, ow - 1), min(H, ow + 2)):
                want[b, :, ih, iw] = W[co, :, ih - oh + 1, iw - ow + 1]
        assert np.array_equal(dX.view(np.int32), want.view(np.int32)), (H, oh, ow)
        assert np.count_nonzero(dX) == C * (min(H, oh + 2) - max(0, oh - 1)) * (min(H, ow + 2) - max(0, ow - 1))


# ------------------------------------------------------------------------------------------------ the head
def run_head(case, g_scale=1.0, guard=None, forward="bf16", backward="bf16"):
    from givepose_amd import xyz_grad
    params, feat, g, _, _ = R.case_reference(case)
    f, gc = T(feat).cuda(), T(g).cuda() * g_scale
    P = {k: T(v).cuda() for k, v in params.items()}
    saved = xyz_grad.xyz_forward_save(f, P, alloc=guard, precision=forward)
    grads, g_feat = xyz_grad.xyz_backward(P, saved, f, gc, alloc=guard, precision=backward)
    torch.cuda.synchronize()
    return {**R.flatten_saved(saved), **{k: v.cpu().numpy() for k, v in grads.items()}, "feat": g_feat.cpu().numpy()}


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "B%d_Cin%d_H%d" % c)
def test_xyz_head_bf16(case):
    """Every saved tensor (coor among them), the 23 gradients and d feat within the yardstick; equal bits across two runs; g_coor x 2
    gives every gradient x 2 bit for bit; a saved table written in one mode is accepted by the backward of the other; the mode is in the
    arithmetic.  (Bitwise independence of a crop from the others of its call is not a property of this mode: the k split depends on B.)"""
    from givepose_amd import xyz_grad
    r64, r32 = Q.flat(R.case_reference(case)[4]), Q.case_reference_bf16(case)
    assert len(r64) == len(r32) == 31 + 24
    guard = Guarded()
    got = run_head(case, guard=guard)
    guard.check()
    names = [n for n, _, _ in guard.bufs]
    assert names.count("workspace") == 2 and len(names) == 31 + 24 + 2
    assert list(got)[31:] == xyz_grad.PARAM_KEYS + ["feat"]
    worst = yardstick(got, r64, r32, f"head bf16 {case}")
    print(f"head bf16 {case}: largest ratio {worst:.2f} over {len(got)} tensors")
    again, two = run_head(case), run_head(case, g_scale=2.0)
    saved = set(list(got)[:31])      # the forward does not see g_coor
    for k, v in got.items():
        assert same(v, again[k]), k
        assert same(two[k], v if k in saved else 2 * v) and np.any(v != 0), k
    fp32 = run_head(case, forward="fp32", backward="fp32")
    d = float(np.max(np.abs(got["pre0"] - fp32["pre0"])) / np.max(np.abs(fp32["pre0"])))
    print(f"head bf16 {case}: pre0 differs from the fp32 mode's by {d:.2e} of its largest element")
    assert 2.0 ** -14 < d < 2.0 ** -6, d
    for fw, bw in (("fp32", "bf16"), ("bf16", "fp32")):
        mixed = run_head(case, forward=fw, backward=bw)
        for k in list(got)[:31]:
            assert same(mixed[k], (fp32 if fw == "fp32" else got)[k]), (fw, k)
        w = yardstick(mixed, r64, r32, f"head {case}, forward {fw}, backward {bw}")
        print(f"head {case}, forward {fw}, backward {bw}: largest ratio {w:.2f}")
    # the 1x1 output conv is fp32 code in both modes: on the same saved table its gradients have the fp32 mode's bits
    assert same(fp32["out_layer.bias"], got["out_layer.bias"])
    half = run_head(case, forward="fp32", backward="bf16")
    assert same(half["out_layer.weight"], fp32["out_layer.weight"]) and not same(half["features.10.conv.weight"], fp32["features.10.conv.weight"])


# ------------------------------------------------------------------------------------------------ PoseNet
def test_posenet_xyz_heads_precision():
    """depths (1,1,1,1), B = 2, as tests/test_bb_bf16_gpu.py::test_posenet_backward_precision."""
    import pose_loss_grad_ref as G
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, Ranger, xyz_grad
    from test_xyz_backward_gpu import loss_batch, same_bits
    cfg = PoseNetConfig(convnext_depths=(1, 1, 1, 1))
    net = PoseNet(cfg, dtype=torch.float32, seed=R.WEIGHT_SEED).cuda()
    assert (net.backward_precision, net.xyz_backward_precision) == ("fp32", "fp32")
    data = {k: v[:2] if v.dim() and v.shape[0] == 4 else v for k, v in loss_batch().items()}
    pl, w = PoseLoss(), T(G.make_gout())
    fdata = {**data, "roi_mask": data["roi_mask_deform"]}
    # the device's own inputs of the two heads: the forward's feat_cat / feat, and the loss gradients at the two coordinate maps
    fwd = net.forward_device(fdata, "cuda")
    base = net.head_grads_feat(data, pl, "cuda", gout=w)
    inputs = {"xyz_deform_head": (fwd["feat_cat"].permute(0, 3, 1, 2).float().contiguous(), base["grads"]["ivfc_coor"].clone()),
              "xyz_nocs_head": (fwd["feat"].permute(0, 3, 1, 2).float().contiguous(), base["grads"]["nocs_coor"].clone())}
    assert inputs["xyz_deform_head"][0].shape == (2, 512, 8, 8) and inputs["xyz_nocs_head"][0].shape == (2, 1024, 8, 8)

    def heads():
        out = {}
        for head, (feat, g) in inputs.items():
            res = net.xyz_head_backward(head, feat, g, return_saved=True)
            torch.cuda.synchronize()
            out[head] = {**R.flatten_saved(res["saved"]), **{k: res["param_grads"][f"{head}.{k}"].cpu().numpy() for k in xyz_grad.PARAM_KEYS},
                         "feat": res["feat"].cpu().numpy()}
        return out

    def equal(a, b):
        return all(same(a[h][k], b[h][k]) for h in a for k in a[h])
    rec = heads()
    with pytest.raises(ValueError, match="xyz_heads 'fp16', expected 'fp32' or 'bf16'"):
        net.set_backward_precision("bf16", xyz_heads="fp16")
    # the backbone's switch alone leaves the heads at their fp32 bits
    net.set_backward_precision("bf16")
    assert (net.backward_precision, net.xyz_backward_precision) == ("bf16", "fp32")
    assert equal(heads(), rec)
    # both: the yardstick against the hooked restatement on the device's own inputs
    net.set_backward_precision("bf16", xyz_heads="bf16")
    assert net.xyz_backward_precision == "bf16"
    got = heads()
    sd = net.state_dict()
    for head, (feat, g) in inputs.items():
        params = {k: sd[f"{head}.{k}"].detach().float().cpu().numpy() for k in xyz_grad.PARAM_KEYS}
        f, gc = feat.cpu().numpy(), g.float().cpu().numpy()
        worst = yardstick(got[head], Q.flat(R.head_run(params, f, gc, torch.float64)), Q.flat(Q.head_run(params, f, gc)), f"PoseNet bf16 {head}")
        print(f"PoseNet bf16 {head}: largest ratio {worst:.2f} over {len(got[head])} tensors")
        for k in xyz_grad.PARAM_KEYS + ["feat"]:
            if k != "out_layer.bias":      # the sum of g_coor: no contraction feeds it
                assert not same(got[head][k], rec[head][k]), (head, k)
    # one train_step with the backbone and the heads in bf16; the forward after it is that of a fresh model with the updated parameters
    tensors = lambda out: {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    step = net.train_step(data, pl, Ranger(net), "cuda")
    names = [k for k in step["param_grads"] if k.startswith(("xyz_nocs_head.", "xyz_deform_head."))]
    assert len(names) == 2 * 35 and all(bool(torch.isfinite(step["param_grads"][k]).all()) for k in names)
    sd = net.state_dict()
    assert all(not torch.equal(sd[k], before[k]) for k in names)
    after = tensors(net.forward_device(fdata, "cuda"))
    fresh = PoseNet(cfg, dtype=torch.float32).cuda()
    fresh.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    same_bits(tensors(fresh.forward_device(fdata, "cuda")), after, "forward after the bf16 step")
    # the heads alone
    net.load_state_dict(before)
    net.set_backward_precision("fp32", xyz_heads="bf16")
    assert (net.backward_precision, net.xyz_backward_precision) == ("fp32", "bf16")
    assert equal(heads(), got)
    # back to fp32 at the parameters of the record: the recorded bits
    net.set_backward_precision("fp32")
    assert (net.backward_precision, net.xyz_backward_precision) == ("fp32", "fp32")
    assert equal(heads(), rec)
