"""GPU: the map-encoder backward family (include/givepose_encgrad.h, gpe_*; givepose_amd/enc_grad.py; PoseNet.map_encoder_backward,
feat_reducer_backward and head_grads_feat) against float64.  The bounds are derived in tests/enc_backward_ref.py.

Contractions (Linear, conv1x1): per element |got - ref| <= (K + 8) 2^-24 sum_k |a_k| |b_k|, K counted on all-ones operands.
Everything else (depth-wise + LayerNorm + GELU, the DCNv3 core, GroupNorm + ReLU, the encoder and the chain): per tensor
max|got - ref| / max|ref| at most 8 times the CPU float32 figure of the same inputs (never less than 2^-24, one rounding of the
largest element); both figures are printed.  The encoder's float64 reference is the restatement evaluated at the DEVICE's gates (ReLU
masks and sampling cells read back from what the device saved), which may differ from float64's only inside the margin set.
The DCNv3 core once more PER ELEMENT, on odd non-square maps with taps exactly on the sampling edges, against tests/dcnv3_reference.py and
tests/dcnv3_backward_reference.py (test_dcnv3_core_per_element_at_the_sampling_edges; its ratio lines: profiles/dcnv3_backward_conformance.txt).

Measured on an MI355X (the ratio lines of that run are kept in profiles/enc_backward.txt):

    Linear and conv 1x1, largest error / bound over the shapes: forward 0.14, dX 0.07, dW 0.18, db 0.10
    device figure / CPU float32 figure: depth-wise + LayerNorm + GELU 0.30 - 1.39, the core 0.43 - 1.73, GroupNorm + ReLU 0.00 - 1.53
    the encoder, largest ratio over the 48 gradients, d coor and nocs_feat (8 allowed), and the gates:
        (1,16) 1.73   (3,16) 2.07   (5,16) 1.54   (2,64) 1.83   (5,16) as [2,3] 1.66
        the device's gates differ from float64's on no gate outside the margin set (6 / 19 / 33 / 445 / 45 gates lie inside it)
    the chain (head_grads_feat, B = 3, groups [1, 2]): 2.07 over the 89 new entries

The two ratios above 2.  (3,16) features.4.weight 2.07: over the four cases the device's figure for this tensor is 6.1e-6, 7.9e-6, 2.5e-6,
5.8e-6 and the CPU's 7.4e-6, 3.8e-6, 2.5e-6, 5.2e-6 (ratios 0.83, 2.07, 1.00, 1.12): each is the largest of 256 error samples and at (3,16) the
yardstick is the small one; the summation order was not emulated.  chain xyz_nocs_head.features.4.norm.weight 2.07: gpx_* code, the
finding of tests/test_xyz_backward_gpu.py (norm gradients of layers 4 - 10 at 2.0 - 2.5 behind the unsplit chains of the 64 x 64 convs).
"""
import functools

import numpy as np
import pytest
import torch

import dcnv3_backward_reference as DB
import dcnv3_reference as DR
import enc_backward_cases as C
import enc_backward_ref as R
from test_xyz_backward_gpu import Guarded, bits, chain_bound, d64, normal, rng, same_bits, within

pytestmark = pytest.mark.gpu
T = torch.from_numpy
U = 2.0 ** -24


def cuda(*arrays):
    return tuple(T(np.ascontiguousarray(a)).cuda() for a in arrays)


def yardstick(got, ref64, ref32, what, allow=8.0):
    """Per tensor: device figure <= allow x max(CPU float32 figure, 2^-24); prints both.  -> the largest ratio."""
    worst = 0.0
    for k, want in ref64.items():
        want = np.asarray(want.cpu() if torch.is_tensor(want) else want, np.float64)
        g = np.asarray(got[k].cpu() if torch.is_tensor(got[k]) else got[k], np.float64)
        c = np.asarray(ref32[k].cpu() if torch.is_tensor(ref32[k]) else ref32[k], np.float64)
        assert g.shape == want.shape, (what, k, g.shape, want.shape)
        scale = np.max(np.abs(want))
        assert scale > 0, (what, k)
        dev, cpu = np.max(np.abs(g - want)) / scale, max(np.max(np.abs(c - want)) / scale, U)
        print(f"{what} {k}: device {dev:.2e}, CPU float32 {cpu:.2e}, ratio {dev / cpu:.2f}")
        assert dev <= allow * cpu, (what, k, dev, cpu)
        worst = max(worst, dev / cpu)
    return worst


# ------------------------------------------------------------------------------------------------ Linear over rows
@pytest.mark.parametrize("rows,Cin,Cout", [(1, 3, 256), (7, 3, 256), (27, 256, 72), (27, 256, 36), (1024, 256, 256)])
def test_linear(rows, Cin, Cout):
    from givepose_amd import enc_grad
    r = rng(rows * 1000 + Cin + Cout)
    X, W, b, dY = normal(r, rows, Cin), normal(r, Cout, Cin) / np.float32(np.sqrt(Cin)), normal(r, Cout), normal(r, rows, Cout)
    guard = Guarded()
    Y = enc_grad.linear_forward(*cuda(X, W, b), alloc=guard)
    out = enc_grad.linear_backward(*cuda(dY, X, W), alloc=guard)
    guard.check()
    X, W, b, dY = d64(X), d64(W), d64(b), d64(dY)
    what = f"linear {rows} {Cin} {Cout}"
    within(Y, R.linear_forward(X, W, b), chain_bound(lambda x, w, c: R.linear_forward(x, w, c), X, W, b), what + " forward")
    ref = R.linear_backward(dY, X, W)
    for i, k in enumerate(("dX", "dW", "db")):
        within(out[k], ref[i], chain_bound(lambda a, x, w: R.linear_backward(a, x, w)[i], dY, X, W), f"{what} {k}")


# ------------------------------------------------------------------------------------------------ conv 1x1, NCHW, any Cout
@pytest.mark.parametrize("B,Cin,Cout,HW", [(1, 1024, 256, 64), (3, 512, 256, 4)])
def test_conv1x1_backward(B, Cin, Cout, HW):
    from givepose_amd import enc_grad
    r = rng(B * 10000 + Cin + HW)
    S = int(np.sqrt(HW))
    dY, X, W = normal(r, B, Cout, S, S), normal(r, B, Cin, S, S), normal(r, Cout, Cin, 1, 1) / np.float32(np.sqrt(Cin))
    guard = Guarded()
    out = enc_grad.conv1x1_backward(*cuda(dY, X, W), alloc=guard)
    guard.check()
    assert out["dW"].shape == (Cout, Cin, 1, 1) and out["dX"].shape == (B, Cin, S, S) and out["db"].shape == (Cout,)
    dY, X, W = d64(dY), d64(X), d64(W)
    ref = R.conv1x1_backward(dY, X, W)
    for i, k in enumerate(("dX", "dW", "db")):
        within(out[k], ref[i], chain_bound(lambda a, b, c: R.conv1x1_backward(a, b, c)[i], dY, X, W), f"conv1x1 {B} {Cin} {Cout} {HW} {k}")


# ------------------------------------------------------------------------------------------------ depth-wise 3x3 + LN + GELU on a prefix
def reach_of_prefix(N, H, W, n):
    """(N,H,W) bool: the pixels some prefix row's 3x3 window (inside the same image) holds."""
    pre = np.zeros(N * H * W, bool)
    pre[:n] = True
    pad = np.pad(pre.reshape(N, H, W), ((0, 0), (1, 1), (1, 1)))
    return np.any([pad[:, a:a + H, b:b + W] for a in range(3) for b in range(3)], axis=0)


@pytest.mark.parametrize("N,H,W,C,n", [(1, 2, 2, 256, 1), (3, 6, 6, 256, 27), (2, 4, 4, 256, 16), (5, 8, 8, 256, 80)])
def test_dwln_forward_save_and_backward(N, H, W, C, n):
    from givepose_amd import enc_grad
    r = rng(N * 1000 + H * 10 + n)
    xin, dw_w, dw_b = normal(r, N, H, W, C), normal(r, C, 1, 3, 3) / 3, normal(r, C) * 0.2
    ln_w, ln_b, dx1 = 1 + normal(r, C) * 0.3, normal(r, C) * 0.5, normal(r, n, C)
    guard = Guarded()
    sv = enc_grad.dwln_forward_save(*cuda(xin, dw_w, dw_b, ln_w, ln_b), n, alloc=guard)
    out = enc_grad.dwln_backward(T(dx1).cuda(), T(xin).cuda(), sv, *cuda(dw_w, ln_w, ln_b), alloc=guard)
    guard.check()
    f64, f32 = [], []
    for dt, dst in ((torch.float64, f64), (torch.float32, f32)):
        a = [T(v).to(dt) for v in (xin, dw_w, dw_b, ln_w, ln_b, dx1)]
        s = R.dwln_forward(a[0], a[1], a[2], a[3], a[4], n)
        dst.append({**s, **dict(zip(("dxin", "d_dw_w", "d_dw_b", "d_ln_w", "d_ln_b"), R.dwln_backward(a[5], a[0], s, a[1], a[3], a[4])))})
    yardstick({**sv, **out}, f64[0], f32[0], f"dwln {N} {H} {W} n {n}")
    # exact zeros where no prefix row reaches, and something everywhere else
    reach = reach_of_prefix(N, H, W, n)
    dx = out["dxin"].cpu().numpy()
    assert np.all(dx[~reach] == 0) and np.all(np.any(dx[reach] != 0, axis=-1))
    if (N, n) == (2, 16):      # the prefix ends at the image boundary: image 1 is untouched, image 0's last row has no lower neighbour
        assert not reach[1].any() and reach[0].all() and np.all(dx[1] == 0)


# ------------------------------------------------------------------------------------------------ the DCNv3 core
CORE_SEED = {(1, 2, 2): 1, (3, 4, 4): 1, (2, 16, 16): 5}
# a location is (2 o - 1) + (i + offset) with |location| < 64 at these sizes: three float32 roundings of numbers below 64, times 16
CORE_DELTA = 16 * 3 * 64 * U


def core_inputs(N, H, W):
    r = rng(CORE_SEED[(N, H, W)] * 7919 + N * 100 + H)
    rows = R.core_rows(N, H, W)
    return normal(r, N, H, W, 256), normal(r, rows, 72) * np.float32(1.5), normal(r, rows, 36), normal(r, rows, 256)


@pytest.mark.parametrize("N,H,W", list(CORE_SEED))
def test_dcnv3_core_forward_and_backward(N, H, W):
    from givepose_amd import enc_grad
    xp, off, logits, dy = core_inputs(N, H, W)
    lw, lh = R.core_locations(d64(off), N, H, W)
    for loc, size in ((lw, W), (lh, H)):      # the seed keeps every location away from the integers; taps leave the image on every side
        assert float((loc - torch.round(loc)).abs().min()) > CORE_DELTA
        assert bool((loc <= -1).any()) and bool((loc >= size).any())
    guard = Guarded()
    fw = enc_grad.dcnv3_core_forward(*cuda(xp, off, logits), alloc=guard)
    bw = enc_grad.dcnv3_core_backward(T(xp).cuda(), T(off).cuda(), fw["mask"], T(dy).cuda(), alloc=guard)
    guard.check()
    ref = []
    for dt in (torch.float64, torch.float32):
        a = [T(v).to(dt) for v in (xp, off, logits, dy)]
        m, y = R.core_forward(a[0], a[1], a[2])
        ref.append({"mask": m, "y": y, **dict(zip(("dxp", "doffset", "dmask_logits"), R.core_backward(a[0], a[1], m, a[3])))})
    cells64, cells32 = R.cells_of(d64(off), N, H, W), R.cells_of(T(off), N, H, W)
    assert all(torch.equal(cells64[k], cells32[k]) for k in cells64)
    yardstick({**fw, **bw}, ref[0], ref[1], f"core {N} {H} {W}")
    # a wholly invalid tap: exact zeros in d offset, and its d mask-logit is -m sum(m gm)
    dead = ~cells64["valid"].reshape(-1, 36)
    assert bool(dead.any()) and torch.all(bw["doffset"].cpu().reshape(-1, 36, 2)[dead] == 0)


def test_dcnv3_core_equal_logits_equal_gm():
    """One input pixel value everywhere and zero offsets at an interior output pixel: every tap samples the same value, gm is equal
    over the taps, and with equal logits m (gm - sum m gm) is zero to rounding: |d logit| <= 16 2^-24 m |gm|."""
    from givepose_amd import enc_grad
    N, H, W = 1, 8, 8
    rows = R.core_rows(N, H, W)
    xp = np.full((N, H, W, 256), 0.75, np.float32)
    off, logits = np.zeros((rows, 72), np.float32), np.full((rows, 36), 0.3, np.float32)
    dy = normal(rng(5), rows, 256)
    fw = enc_grad.dcnv3_core_forward(*cuda(xp, off, logits))
    bw = enc_grad.dcnv3_core_backward(T(xp).cuda(), T(off).cuda(), fw["mask"], T(dy).cuda())
    row = 2 * 4 + 2      # (ho, wo) = (2, 2): the window 3..5 lies inside the image
    gm = 0.75 * d64(dy)[row].reshape(4, 64).sum(1)
    dl = bw["dmask_logits"].cpu().double()[row].reshape(4, 9)
    assert torch.allclose(fw["mask"].cpu()[row], torch.full((36,), 1 / 9), rtol=0, atol=2 * U)
    assert torch.all(dl.abs() <= 16 * U * gm.abs()[:, None] / 9 + 64 * U * 0.75 * d64(dy)[row].abs().reshape(4, 64).sum(1)[:, None] / 9), dl


CORE_EDGE_CASES = [
    DR.mk("core-edges-N2-5x8", torch.float32, N=2, H=5, W=8, s=2, iset="edges", logits=True),      # 3 x 4 outputs, 864 taps: every pair of the edge tables
    DR.mk("core-c3-N1-7x4", torch.float32, N=1, H=7, W=4, s=2, logits=True),
]


@pytest.mark.parametrize("case", CORE_EDGE_CASES, ids=lambda c: c.name)
def test_dcnv3_core_per_element_at_the_sampling_edges(case):
    """gpe_dcnv3_core_forward / _backward on odd, non-square maps with taps exactly on the sampling edges, per element: y against
    dcnv3_reference.ref (the logits case); dxp and doffset against the bounds of dcnv3_backward_reference (the general backward at G 4,
    D 64, K 3, stride 2, pad 1, os 1, float32) evaluated on the mask the DEVICE saved; dmask_logits = m (gm - sum m gm) against the float64
    value on the same mask, its bound being grad_mask's pushed through the expression (dcnv3_backward_reference.dlogits_ref, derived in
    that module's docstring).  A bound of 0 -- every doffset slot of a tap outside the map, every dxp element nothing reaches, every y whose
    taps are all outside -- asks for an exact zero.  doffset and dmask_logits have one writer per element: equal bits on a second launch."""
    from givepose_amd import enc_grad
    c = case
    I = DR.inputs(c)
    rows = DR.n_rows(c)
    assert rows == R.core_rows(c.N, c.H, c.W) and (c.G, c.D, c.kh, c.kw, c.sh, c.ph, c.os, c.rc) == (4, 64, 3, 3, 2, 1, 1.0, 0)
    if c.iset == "edges":
        assert all(n > 0 for n in DR.classify(c, I).values())
    dy = DB.grad_output(c)
    xp, off, logits, dyd = I["x"].cuda(), I["off"].view(rows, 72).cuda(), I["mask"].view(rows, 36).cuda(), dy.cuda()
    guard = Guarded()
    fw = enc_grad.dcnv3_core_forward(xp, off, logits, alloc=guard)
    bw = enc_grad.dcnv3_core_backward(xp, off, fw["mask"], dyd, alloc=guard)
    again = enc_grad.dcnv3_core_backward(xp, off, fw["mask"], dyd, alloc=guard)
    guard.check()
    failures = []

    def hold(got, v, bound, what):
        zeros = what in ("dxp", "doffset") or (what == "y" and c.iset == "edges")      # the case must hold exact zeros there
        assert bool((bound > 0).any()) and (bool((bound == 0).any()) or not zeros), what
        ratio, msg = DR.check(got, v, bound, f"{c.name} {what}")
        print(f"GPU_RATIO {c.name} {what} {ratio:.4f}")
        if msg is not None:
            failures.append(msg)

    hold(fw["y"], *DR.ref(I, c), "y")
    saved = fw["mask"].cpu()
    cb = c._replace(logits=False, entry="any")
    r = DB.ref(dict(x=I["x"], off=I["off"], mask=saved.reshape(-1), gout=dy), cb)
    hold(bw["dxp"], *r["grad_input"], "dxp")
    hold(bw["doffset"], *r["grad_offset"], "doffset")
    hold(bw["dmask_logits"], *DB.dlogits_ref(saved.view(rows, 4, 9), *r["grad_mask"], 9), "dmask_logits")
    lh, lw, _ = DR.locations(c, I, torch.float32)
    outside = ~((lh > -1) & (lw > -1) & (lh < c.H) & (lw < c.W))
    assert bool(outside.any()) and bool((r["grad_offset"][1][outside] == 0).all())
    for k in ("doffset", "dmask_logits"):
        if not torch.equal(bits(bw[k]), bits(again[k])):
            failures.append(f"{c.name} {k}: a second launch gives other bits")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ GroupNorm + ReLU
@pytest.mark.parametrize("B,C,HW", [(1, 256, 1), (3, 256, 4), (2, 256, 64), (1, 256, 1024)])
def test_gn_relu_forward_and_backward(B, C, HW):
    from givepose_amd import enc_grad
    r = rng(B * 100000 + C + HW)
    x = normal(r, B, C, HW) * (0.5 + r.random((1, C, 1)).astype(np.float32)) + normal(r, 1, C, 1)
    gamma, beta, dout = 2 * normal(r, C), normal(r, C) * 0.5, normal(r, B, C, HW)
    guard = Guarded()
    fw = enc_grad.gn_relu_forward(*cuda(x, gamma, beta), alloc=guard)
    # the backward of the device's own statistics; the references differentiate at the same saved numbers
    mean, rstd = fw["mean"].cpu().numpy(), fw["rstd"].cpu().numpy()
    got = enc_grad.gn_relu_backward(T(dout).cuda(), T(x).cuda(), fw["mean"], fw["rstd"], *cuda(gamma, beta), alloc=guard)
    guard.check()
    m64, r64 = R.gn_stats(d64(x))
    yardstick(fw, {"mean": m64, "rstd": r64, "out": R.gn_relu_forward(d64(x), m64, r64, d64(gamma), d64(beta))[0]},
              {"mean": R.gn_stats(T(x))[0], "rstd": R.gn_stats(T(x))[1], "out": R.gn_relu_forward(T(x), *R.gn_stats(T(x)), T(gamma), T(beta))[0]},
              f"gn relu forward {B} {C} {HW}")
    u = R.gn_relu_forward(d64(x), d64(mean), d64(rstd), d64(gamma), d64(beta))[1]
    gate = u > 0
    assert torch.equal(gate, fw["out"].cpu() > 0) or float(u.abs()[gate != (fw["out"].cpu() > 0)].max()) < 1e-5
    ref, f32 = (dict(zip(("dx", "dgamma", "dbeta"), R.gn_relu_backward(*(T(a).to(dt) for a in (dout, x, mean, rstd, gamma, beta)), relu=gate)))
                for dt in (torch.float64, torch.float32))
    yardstick(got, ref, f32, f"gn relu backward {B} {C} {HW}")


# ------------------------------------------------------------------------------------------------ the encoder
@functools.lru_cache(maxsize=None)
def device_params():
    return {k: T(v).cuda() for k, v in R.enc_params().items()}


def run_encoder(case, groups=None, g_scale=1.0, guard=None, crops=None):
    from givepose_amd import enc_grad
    _, coor, g = R.case_inputs(case)
    sl = slice(None) if crops is None else crops
    c, gf = T(coor[sl]).cuda(), T(g[sl]).cuda() * g_scale
    saved = enc_grad.enc_forward_save(c, device_params(), groups=groups, alloc=guard)
    grads, g_coor = enc_grad.enc_backward(device_params(), saved, c, gf, alloc=guard)
    torch.cuda.synchronize()
    return {**grads, "coor": g_coor, "nocs_feat": torch.cat([s["act"][2] for s in saved])}, saved


def device_gates(saved, groups, R_):
    return [R.gates_of({k: [t.cpu() for t in v] for k, v in sv.items()}, N, R_) for sv, N in zip(saved, groups)]


@pytest.mark.parametrize("case,groups", [(c, None) for c in R.CASES] + [R.GROUPED], ids=lambda v: str(v).replace(" ", ""))
def test_encoder_end_to_end(case, groups):
    """gpe_map_encoder_forward_save and gpe_map_encoder_backward against the float64 restatement at the device's gates: the 48
    gradients, d coor and the result."""
    from givepose_amd import enc_grad
    B, R_ = case
    r64, _, fig32, margins = C.reference(case, groups)
    guard = Guarded()
    got, saved = run_encoder(case, groups, guard=guard)
    guard.check()
    glist = list(groups) if groups else [B]
    assert list(got) == enc_grad.PARAM_KEYS + ["coor", "nocs_feat"]
    for k, s in enc_grad.param_shapes().items():
        assert tuple(got[k].shape) == s and got[k].is_contiguous(), k
    gates = device_gates(saved, glist, R_)
    total, inside, bad = C.gate_disagreements(gates, r64, margins)
    print(f"{case} {groups}: the device's gates differ from float64's on {bad} gates outside the margin set ({inside} of {total} inside it)")
    assert bad == 0
    params, coor, g = R.case_inputs(case)
    ref = R.enc_run(params, coor, g, groups=groups, gates=gates)
    want = {**ref["grads"], "coor": ref["coor"], "nocs_feat": ref["nocs_feat"]}
    worst = yardstick({k: v.cpu().numpy() for k, v in got.items()}, want, {k: want[k] * (1 + fig32[k]) for k in want}, f"{case} {groups}")
    print(f"{case} {groups}: largest ratio {worst:.2f}")
    if groups:      # the same batches run alone and summed in order
        parts, i0 = [], 0
        for N in glist:
            parts.append(run_encoder(case, crops=slice(i0, i0 + N))[0])
            i0 += N
        for k in enc_grad.PARAM_KEYS:
            a, b = got[k], parts[0][k] + parts[1][k]
            tol = 16 * fig32[k] * float(np.max(np.abs(want[k])))
            assert float((a - b).abs().max()) <= tol, k
            if k in enc_grad.ATOMIC_FREE_KEYS:
                assert torch.equal(bits(a), bits(b)), k
        assert torch.equal(bits(got["nocs_feat"]), bits(torch.cat([p["nocs_feat"] for p in parts])))


SMALL = R.CASES[1]


def test_zero_gradient_repeatability_and_atomic_free_tensors():
    from givepose_amd import enc_grad
    assert SMALL == (3, 16)
    fig32 = C.reference(SMALL)[2]
    zero, _ = run_encoder(SMALL, g_scale=0.0)
    for k, v in zero.items():
        if k != "nocs_feat":
            assert torch.all(v == 0), k      # exact zeros, everywhere
    a, sa = run_encoder(SMALL)
    b, sb = run_encoder(SMALL)
    same_bits(sa, sb, "saved")               # the forward has no atomic
    for k in a:
        scale = float(a[k].abs().max())
        assert scale > 0 and float((a[k] - b[k]).abs().max()) <= 16 * fig32[k] * scale, k      # each within 8 x of the reference
        if k in enc_grad.ATOMIC_FREE_KEYS or k == "nocs_feat":
            assert torch.equal(bits(a[k]), bits(b[k])), k


@functools.lru_cache(maxsize=None)
def net_of(dtype=torch.float32):
    from givepose_amd import PoseNet, PoseNetConfig
    return PoseNet(PoseNetConfig(), seed=R.WEIGHT_SEED, dtype=dtype).cuda()


def test_posenet_map_encoder_backward_and_in_place_update():
    """PoseNet.map_encoder_backward is the enc_grad path on the state_dict's weights, with the forward's grouping rule; an in-place
    update of an fp16 network's parameter -- where the fp32 copies are real copies -- is seen at the next call."""
    from givepose_amd import PoseNet, PoseNetConfig, enc_grad
    net = net_of()
    _, coor, g = R.case_inputs(SMALL)
    res = net.map_encoder_backward(T(coor), T(g), groups=[1, 2], return_saved=True)
    torch.cuda.synchronize()
    assert list(res) == ["param_grads", "coor", "outputs", "saved"] and list(res["outputs"]) == ["nocs_feat"] and len(res["saved"]) == 2
    assert list(res["param_grads"]) == ["nocs_encoder." + k for k in enc_grad.PARAM_KEYS]
    assert not any(".bn." in k for k in res["param_grads"])
    direct, _ = run_encoder(SMALL, groups=[1, 2])
    for k in enc_grad.ATOMIC_FREE_KEYS:
        assert torch.equal(bits(res["param_grads"]["nocs_encoder." + k]), bits(direct[k])), k
    assert torch.equal(bits(res["outputs"]["nocs_feat"]), bits(direct["nocs_feat"]))
    # dcn_couple is the forward's rule when groups is None
    coupled = PoseNet(PoseNetConfig(), seed=R.WEIGHT_SEED, dtype=torch.float32, dcn_couple=1).cuda()
    c1 = coupled.map_encoder_backward(T(coor), T(g))
    assert torch.equal(bits(c1["outputs"]["nocs_feat"]), bits(run_encoder(SMALL, groups=[1, 1, 1])[0]["nocs_feat"]))
    assert not torch.equal(c1["outputs"]["nocs_feat"][1:], res["outputs"]["nocs_feat"][1:])
    net16 = net_of(torch.float16)
    p = dict(net16.named_parameters())["nocs_encoder.features.7.bias"]
    keep = p.detach().clone()
    before = net16.map_encoder_backward(T(coor), T(g))
    try:
        p.add_(0.5)
        after = net16.map_encoder_backward(T(coor), T(g))
    finally:
        p.copy_(keep)
    again = net16.map_encoder_backward(T(coor), T(g))
    torch.cuda.synchronize()
    a, b = after["outputs"]["nocs_feat"], before["outputs"]["nocs_feat"]
    assert torch.allclose(a[b > 0], b[b > 0] + 0.5, rtol=0, atol=1e-5) and not torch.equal(a, b)      # ReLU(u + 0.5) where u > 0
    assert torch.equal(bits(again["outputs"]["nocs_feat"]), bits(before["outputs"]["nocs_feat"]))


# ------------------------------------------------------------------------------------------------ PoseNet.head_grads_feat
def test_head_grads_feat_chain():
    """head_grads_feat at B = 3 with groups = [1, 2]: head_grads_xyz's entries bit for bit; the sums are the sums of the returned parts;
    every new entry within 8 x the CPU float32 figure of the float64 chain restated from the forward's own tensors; and the grouping
    is honoured."""
    import pose_loss_grad_ref as G
    import xyz_backward_ref as X
    from givepose_amd import PoseLoss, enc_grad, xyz_grad
    from test_xyz_backward_gpu import loss_batch
    data = {k: v[:3] if v.dim() and v.shape[0] == 4 else v for k, v in loss_batch().items()}
    net, pl, w, groups = net_of(), PoseLoss(), T(G.make_gout()), [1, 2]
    res = net.head_grads_feat(data, pl, "cuda", gout=w, groups=groups)
    base = net.head_grads_xyz(data, pl, "cuda", gout=w, groups=groups)
    torch.cuda.synchronize()
    g = res["grads"]
    assert list(res) == list(base)
    assert list(g) == list(base["grads"]) + ["nocs_coor_direct", "nocs_coor_from_encoder", "feat_from_reducer", "feat_from_nocs_head", "feat"]
    same_bits(res["loss"], base["loss"], "loss")
    same_bits(res["output"], base["output"], "output")
    for k, v in base["grads"].items():
        assert torch.equal(bits(g["nocs_coor_direct" if k == "nocs_coor" else k]), bits(v)), k
    for k, v in base["param_grads"].items():
        assert torch.equal(bits(res["param_grads"][k]), bits(v)), k
    new = set(res["param_grads"]) - set(base["param_grads"])
    assert len(new) == 2 + 48 + 35 and len(res["param_grads"]) == 23 + 35 + 85
    assert {k.split(".")[0] for k in new} == {"feat_reducer", "nocs_encoder", "xyz_nocs_head"}
    # the forward's own tensors
    fwd = net.forward_device({**data, "roi_mask": data["roi_mask_deform"]}, "cuda", groups=groups)
    nocs = fwd["nocs_coor"].float().clone()
    feat = fwd["feat"].permute(0, 3, 1, 2).float().contiguous()
    assert feat.shape == (3, 1024, 8, 8) and g["feat"].shape == feat.shape
    enc = net.map_encoder_backward(nocs, g["nocs_feat"], groups=groups, return_saved=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(g["nocs_coor"]), bits(g["nocs_coor_direct"] + g["nocs_coor_from_encoder"]))
    assert torch.equal(bits(g["feat"]), bits(g["feat_from_reducer"] + g["feat_from_nocs_head"]))
    # the float64 chain, at the device's gates, and its float32 yardstick (autograd for the encoder, the restatements for the rest)
    P = R.enc_params()
    gates = device_gates(enc["saved"], groups, 64)
    gnf, nc = g["nocs_feat"].cpu().numpy(), nocs.cpu().numpy()
    ref = R.enc_run(P, nc, gnf, groups=groups, gates=gates)
    o64, o32 = (C.oracle_run(P, nc, gnf, dt, groups) for dt in (torch.float64, torch.float32))
    fig_enc = R.rel_figures({**o32["grads"], "coor": o32["coor"]}, {**o64["grads"], "coor": o64["coor"]})
    r32 = R.enc_run(P, nc, gnf, groups=groups, gates=gates, dtype=torch.float32)      # held at the same gates: no flipped gate inflates it
    held = R.rel_figures({**r32["grads"], "coor": r32["coor"]}, {**ref["grads"], "coor": ref["coor"]})
    fig_enc = {k: min(v, held[k]) for k, v in fig_enc.items()}
    want = {"nocs_encoder." + k: v for k, v in ref["grads"].items()}
    f32 = {"nocs_encoder." + k: v * (1 + fig_enc[k]) for k, v in ref["grads"].items()}
    direct = g["nocs_coor_direct"].cpu().numpy().astype(np.float64)
    want["nocs_coor"], f32["nocs_coor"] = direct + ref["coor"], direct + ref["coor"] * (1 + fig_enc["coor"])
    fr_w = net.state_dict()["feat_reducer.weight"].float().cpu()
    gc = g["conv_feat256"].cpu()
    # the float32 chain feeds its head the float32 encoder's d coor: the float64 total plus the float32 autograd's own error
    total32 = want["nocs_coor"] + (o32["coor"].astype(np.float64) - o64["coor"])
    for dt, dst, tot in ((torch.float64, want, want["nocs_coor"]), (torch.float32, f32, total32)):
        dX, dW, db = R.conv1x1_backward(gc.to(dt), feat.cpu().to(dt), fr_w.to(dt))
        dst.update({"feat_reducer.weight": dW.numpy(), "feat_reducer.bias": db.numpy(), "feat_from_reducer": dX.numpy()})
        total = torch.from_numpy(tot).to(dt)
        h = X.head_run(X.head_params(1024), feat.cpu().numpy(), total.numpy(), dtype=dt)
        dst.update({"xyz_nocs_head." + k: h["grads"][k] for k in xyz_grad.PARAM_KEYS})
        dst["feat_from_nocs_head"] = h["grads"]["feat"]
        dst["feat"] = np.asarray(dst["feat_from_reducer"], np.float64) + np.asarray(dst["feat_from_nocs_head"], np.float64)
    got = {**{k: v for k, v in res["param_grads"].items() if k in want}, **{k: g[k] for k in ("nocs_coor", "feat_from_reducer", "feat_from_nocs_head", "feat")}}
    assert set(got) == set(want)
    worst = yardstick(got, want, f32, "chain")
    print(f"chain: largest ratio {worst:.2f}")
    # without the groups the encoder's gradient is another: the coupling is honoured
    one = net.head_grads_feat(data, pl, "cuda", gout=w)
    k = "nocs_encoder.features.6.dcnv3.output_proj.weight"
    assert float((one["param_grads"][k] - res["param_grads"][k]).abs().max()) > 1e-3 * float(res["param_grads"][k].abs().max())
