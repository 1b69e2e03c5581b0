"""GPU: the train-mode size head (include/givepose_sizegrad.h, gps_*; givepose_amd/size_grad.py; PoseNet.size_head_backward and the
size_head= keyword of head_grads_feat / head_grads_backbone / train_step) against the float64 run of tests/size_head_ref.py.

The rule is the project's `yardstick` (tests/test_enc_backward_gpu.py): per tensor, max|got - ref64| / max|ref64| is at most 8 times the
figure of the same restatement in float32 on the CPU, which counts as at least 2^-24; both are printed.  conv1.bias is the exception:
its gradient db1 = sum_b dh is analytically zero, so |db1 - ref64| is measured against max_f sum_b |dh_ref64[b,f]|, the size of the
terms that are summed, with the same factor of 8 over the CPU float32 figure (`db1_rule`).

Every operator call here puts its outputs, saved tensors and workspace into `Guarded` buffers (tests/test_xyz_backward_gpu.py): every
element of every output must be written and no sentinel touched.

Measured on an MI355X, largest device / CPU float32 ratio (8 allowed; every line is in profiles/size_head_train.txt):

    operator, 5 shapes x 2 weight scales x 3 layouts: 3.09 (conv2.bias at (5, 256, 64, 32), 1.8e-7 against 6e-8); the layouts agree bit for bit
    goldens of the reference's module: b5 3.09, b2 2.34;  chain 1.01;  train_step twice 1.00

With the per-channel statistics in fp32 the golden b2 missed the rule by 56 x on d feat (1.84e-4 against 3.27e-6): torch's CPU BatchNorm
accumulates float32 input in double, and the case has a channel of variance 26 eps.  They are formed in fp64 since.
"""
import re

import numpy as np
import pytest
import torch

import size_head_ref as R
from test_enc_backward_gpu import yardstick
from test_xyz_backward_gpu import Guarded, bits

pytestmark = pytest.mark.gpu
T = torch.from_numpy
U = 2.0 ** -24
LAYOUTS = ("nchw", "nhwc32", "nhwc16")


def hw_of(HW):
    return {64: (8, 8), 4: (2, 2), 1: (1, 1)}[HW]


def device_feat(feat, layout):
    """feat (B,C,HW) numpy -> (device tensor in the layout, nhwc flag)."""
    B, C, HW = feat.shape
    H, W = hw_of(HW)
    t = T(np.ascontiguousarray(feat))
    if layout == "nchw":
        return t.view(B, C, H, W).cuda(), False
    t = t.permute(0, 2, 1).contiguous().view(B, H, W, C).cuda()
    return (t.half() if layout == "nhwc16" else t), True


def run_device(case, layout, alloc=None, seed=None):
    from givepose_amd import size_grad
    B, C, HW = case["feat"].shape
    feat, nhwc = device_feat(case["feat"], layout)
    P = {k: T(v).cuda() for k, v in case["params"].items()}
    saved = size_grad.size_forward_save(feat, P, keep=None if seed is not None else T(case["keep"]).cuda(), seed=seed, nhwc=nhwc, alloc=alloc)
    grads, dfeat = size_grad.size_backward(P, saved, T(case["g_out"]).cuda(), (B, C) + hw_of(HW), alloc=alloc)
    torch.cuda.synchronize()
    return saved, grads, dfeat


def db1_rule(got, ref64, ref32, what):
    scale = float(ref64["dh"].abs().sum(0).max())
    want = ref64["conv1.bias"]
    dev = float((got.double().cpu() - want).abs().max()) / scale
    cpu = max(float((ref32["conv1.bias"].double() - want).abs().max()) / scale, U)
    print(f"{what} conv1.bias (of max_f sum_b |dh|): device {dev:.2e}, CPU float32 {cpu:.2e}, ratio {dev / cpu:.2f}")
    assert dev <= 8 * cpu, (what, dev, cpu)
    return dev / cpu


def against(ref64, ref32, saved, grads, dfeat, what):
    """Every output, statistic and gradient within the rule.  -> the largest ratio."""
    B, C = saved["pooled"].shape
    got = {"out": saved["out"], "pooled": saved["pooled"], "mean": saved["mean"], "var_unbiased": saved["var_unbiased"], "feat": dfeat.view(B, C, -1),
           **{k: grads[k] for k in R.PARAM_KEYS if k != "conv1.bias"}}
    worst = yardstick(got, {k: ref64[k] for k in got}, {k: ref32[k] for k in got}, what)
    assert torch.equal(saved["arg"].cpu().long(), ref64["arg"]), what
    assert torch.equal(saved["pooled"].cpu().double(), ref64["pooled"]), (what, "a maximum is exact")
    return max(worst, db1_rule(grads["conv1.bias"], ref64, ref32, what))


# ------------------------------------------------------------------------------------------------ the operator against float64
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_operator_against_float64(shape, scale, layout):
    case, r64, r32 = R.cached_reference(shape, scale)
    assert not R.has_ties(case["feat"]) and R.gate_margin(r64) > R.GATE_MARGIN
    guard = Guarded()
    saved, grads, dfeat = run_device(case, layout, alloc=guard)
    guard.check()
    worst = against(r64, r32, saved, grads, dfeat, f"size head {shape} {scale} {layout}")
    assert torch.equal(saved["keep"].cpu(), T(case["keep"]))               # the forward returns the mask it used
    print(f"size head {shape} {scale} {layout}: largest device / CPU float32 ratio {worst:.2f}")


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_goldens_of_the_reference_module(name):
    """The reference's own SizeHead in .train(), float64 run as the reference and float32 run as the CPU figure, with the mask it drew."""
    import os

    from givepose_amd import size_grad
    gold = np.load(os.path.join(R.GOLDEN, f"size_head_train_{name}.npz"))
    case = R.golden_case(name)
    assert int(gold["input_crc"]) == R.case_crc(case)
    case["keep"] = gold["keep"]
    B, C, HW = case["feat"].shape
    dh64 = R.reference(case, torch.float64)["dh"]
    assert R.gate_margin(R.reference(case, torch.float64)) > R.GATE_MARGIN
    worst = 0.0
    for layout in LAYOUTS:
        guard = Guarded()
        saved, grads, dfeat = run_device(case, layout, alloc=guard)
        guard.check()
        arg = T(gold["f64_feat_arg"].astype(np.int64))
        assert torch.equal(saved["arg"].cpu().long(), arg)
        dense = dfeat.view(B, C, HW).cpu()
        assert int((dense != 0).sum()) <= B * C
        got = {"out": saved["out"], "feat_values": dense.gather(2, arg[:, :, None]).squeeze(2), **{k: grads[k] for k in R.PARAM_KEYS if k != "conv1.bias"}}
        what = f"golden {name} {layout}"
        worst = max(worst, yardstick(got, {k: gold["f64_" + k] for k in got}, {k: gold["f32_" + k] for k in got}, what))
        worst = max(worst, db1_rule(grads["conv1.bias"], {"dh": dh64, "conv1.bias": T(gold["f64_conv1.bias"])}, {"conv1.bias": T(gold["f32_conv1.bias"])}, what))
        # the running statistics after one and after two calls, from a fresh BatchNorm1d's buffers
        rm, rv, nbt = torch.zeros(saved["mean"].numel(), device="cuda"), torch.ones(saved["mean"].numel(), device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")
        for calls in (1, 2):
            size_grad.bn_running_update(rm, rv, nbt, saved["mean"], saved["var_unbiased"])
            k = {"running_mean": rm, "running_var": rv}
            worst = max(worst, yardstick(k, {n: gold[f"f64_{n}_{calls}"] for n in k}, {n: gold[f"f32_{n}_{calls}"] for n in k}, f"{what} call {calls}"))
            assert int(nbt) == calls
    print(f"golden {name}: largest device / CPU float32 ratio {worst:.2f}")


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("B,C,HW,F", [(3, 128, 64, 16), (2, 64, 4, 16), (2, 64, 1, 16)])
def test_ties_take_the_lowest_index_and_d_feat_has_one_entry_per_map(B, C, HW, F):
    """feat of few distinct fp16 values: most maps attain their maximum several times.  arg is the lowest such index in every layout,
    d feat holds dpooled there and +0.0 (all bits zero) everywhere else, and the three layouts agree bit for bit."""
    r = R.rng(B * 100 + HW)
    case = R.make_case(B, C, HW, F, "sqrt", seed=5)
    case["feat"] = (r.integers(-4, 5, size=(B, C, HW)) / 8).astype(np.float32)
    if HW > 1:
        assert R.has_ties(case["feat"]) and ((case["feat"] == case["feat"].max(-1, keepdims=True)).sum(-1) > 1).mean() > 0.2
    want = T(case["feat"].argmax(-1))             # numpy: the first occurrence
    first = None
    for layout in LAYOUTS:
        guard = Guarded()
        saved, grads, dfeat = run_device(case, layout, alloc=guard)
        guard.check()
        assert torch.equal(saved["arg"].cpu().long(), want), layout
        assert torch.equal(saved["pooled"].cpu(), T(case["feat"].max(-1))), layout
        dense = dfeat.view(B, C, HW).cpu()
        dp = dense.gather(2, want[:, :, None])
        rest = dense.clone().scatter_(2, want[:, :, None], 0.0)
        assert not bits(rest).any(), (layout, "a non-zero or a -0.0 beside the maximum")
        assert int((dense != 0).sum()) == int((dp != 0).sum()) and int((dp != 0).sum()) > 0.9 * B * C, layout
        res = {"dp": dp, **{k: v.cpu() for k, v in grads.items()}, **{k: v.cpu() for k, v in saved.items()}}
        if first is None:
            first = res
        else:
            for k in first:
                assert torch.equal(first[k].view(torch.uint8), res[k].view(torch.uint8)), (layout, k)


# ------------------------------------------------------------------------------------------------ the seeded mask
@pytest.mark.parametrize("shape", [(5, 256, 64, 32), (65, 512, 64, 128)], ids=lambda s: "x".join(map(str, s)))
def test_seeded_mask_equals_the_numpy_restatement(shape):
    case, _, _ = R.cached_reference(shape, "sqrt")
    B, F = shape[0], shape[3]
    masks = []
    for seed in (7, 0xFEDCBA9876543210):
        saved, grads, dfeat = run_device(case, "nhwc16", seed=seed)
        want = R.keep_mask(seed, B, F)
        assert saved["keep"].dtype == torch.uint8 and np.array_equal(saved["keep"].cpu().numpy(), want), hex(seed)
        masks.append(want)
        # the seeded call is the explicit call with that mask, bit for bit
        s2, g2, d2 = run_device({**case, "keep": want}, "nhwc16")
        for a, b in [(saved[k], s2[k]) for k in saved] + [(grads[k], g2[k]) for k in grads] + [(dfeat, d2)]:
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert (masks[0] != masks[1]).mean() > 0.2


# ------------------------------------------------------------------------------------------------ determinism
def test_two_calls_give_equal_bits_wherever_the_buffers_lie():
    case, _, _ = R.cached_reference((65, 512, 64, 128), "sqrt")
    runs = [run_device(case, "nhwc32"), run_device(case, "nhwc32"), run_device(case, "nhwc32", alloc=Guarded())]
    s0, g0, d0 = runs[0]
    for s, g, d in runs[1:]:
        for a, b in [(s0[k], s[k]) for k in s0] + [(g0[k], g[k]) for k in g0] + [(d0, d)]:
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # and the layouts: the pooled maxima are the same numbers, so everything behind them is the same bits
    for layout in ("nchw", "nhwc16"):
        s, g, d = run_device(case, layout)
        for a, b in [(s0[k], s[k]) for k in s0] + [(g0[k], g[k]) for k in g0] + [(d0, d)]:
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), layout


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_by_name():
    from givepose_amd import PoseNet, PoseNetConfig, _lib, size_grad
    for (B, C, HW, F), match in (((1, 64, 4, 16), "B = 1"), ((2, 64, 4, 8), "F = 8"), ((2, 96, 4, 16), "C = 96")):
        case = R.make_case(B, C, HW, F, "sqrt", seed=3)
        with pytest.raises(_lib.GivePoseHipError, match=match):
            run_device(case, "nchw")
    case = R.make_case(2, 64, 4, 16, "sqrt", seed=3)
    feat, _ = device_feat(case["feat"], "nchw")
    P = {k: T(v).cuda() for k, v in case["params"].items()}
    keep = T(case["keep"]).cuda()
    with pytest.raises(ValueError, match="exactly one of keep and seed"):
        size_grad.size_forward_save(feat, P, keep=keep, seed=7)
    with pytest.raises(ValueError, match="exactly one of keep and seed"):
        size_grad.size_forward_save(feat, P)
    with pytest.raises(ValueError, match="keep.*expected \\(B,F\\)"):
        size_grad.size_forward_save(feat, P, keep=keep[:, :8])
    with pytest.raises(ValueError, match="float32"):
        size_grad.size_forward_save(feat.half(), P, seed=7)                  # NCHW is float32 only
    net = PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1)), dtype=torch.float32, seed=3).cuda()
    f = torch.randn(2, 1024, 8, 8, device="cuda")
    g = torch.randn(2, 3, device="cuda")
    with pytest.raises(ValueError, match="exactly one of keep and seed"):
        net.size_head_backward(f, g)
    with pytest.raises(ValueError, match="exactly one of keep and seed"):
        net.size_head_backward(f, g, keep=torch.ones(2, 128, dtype=torch.uint8), seed=1)
    with pytest.raises(_lib.GivePoseHipError, match="B = 1"):
        net.size_head_backward(f[:1], g[:1], seed=1)
    # the module-level entry point: names, shapes, and the operator's bits
    res = net.size_head_backward(f, g, seed=11, return_saved=True)
    assert list(res) == ["param_grads", "feat", "outputs", "stats", "saved"] and list(res["outputs"]) == ["size_raw", "keep"] and list(res["stats"]) == ["mean", "var_unbiased"]
    sd = net.state_dict()
    assert list(res["param_grads"]) == ["size_head." + k for k in size_grad.PARAM_KEYS]
    assert all(v.shape == sd[k].shape for k, v in res["param_grads"].items()) and res["feat"].shape == f.shape
    assert res["outputs"]["size_raw"].shape == (2, 3) and np.array_equal(res["outputs"]["keep"].cpu().numpy(), R.keep_mask(11, 2, 128))
    # parameters come from _module_params_f32: an in-place update is seen at the next call
    with torch.no_grad():
        net.size_head.conv2.bias.add_(1.0)
    again = net.size_head_backward(f, g, seed=11)
    assert torch.allclose(again["outputs"]["size_raw"], res["outputs"]["size_raw"] + 1.0, atol=1e-5)


# ------------------------------------------------------------------------------------------------ the chain
def small_net_and_batch():
    import bb_backward_ref as B
    from givepose_amd import PoseNet, PoseNetConfig
    from test_xyz_backward_gpu import loss_batch
    cfg = PoseNetConfig(convnext_depths=(1, 1, 1, 1))
    net = PoseNet(cfg, dtype=torch.float32, seed=B.WEIGHT_SEED).cuda()
    data = {k: v[:2] if v.dim() and v.shape[0] == 4 else v for k, v in loss_batch().items()}
    return cfg, net, data


def restate_on_device_feat(net, data, seed, g_size):
    """The float64 / float32 restatement on the device's own feat (the forward is deterministic) and the given d size."""
    from givepose_amd import size_grad
    raw = net._forward_do_loss(data, "cuda", None)[1]
    feat = raw["feat"].float().cpu()                     # (B,8,8,C)
    B, C = feat.shape[0], feat.shape[3]
    sd = net.state_dict()
    case = {"feat": np.ascontiguousarray(feat.view(B, 64, C).permute(0, 2, 1).numpy()),
            "params": {k: sd["size_head." + k].detach().float().cpu().numpy() for k in size_grad.PARAM_KEYS},
            "keep": R.keep_mask(seed, B, sd["size_head.bn1.weight"].numel()), "g_out": g_size.detach().float().cpu().numpy()}
    r64, r32 = R.reference(case, torch.float64), R.reference(case, torch.float32)
    assert not R.has_ties(case["feat"]) and R.gate_margin(r64) > R.GATE_MARGIN
    return case, r64, r32


def test_chain_with_and_without_the_size_head():
    """size_head=None: the keyword changes nothing -- the atomic-free entries are the bits of a call without it, the entries behind the
    encoder's atomic scatter agree to rounding (1e-4 of the largest magnitude, the bound tests/test_bb_backward_gpu.py uses between two
    calls: there is no float64 restatement of the whole chain to hold a yardstick against).
    size_head={"seed": 7}: param_grads covers every parameter but the never-applied bn.*; grads["feat"] is, bit for bit,
    (feat_from_reducer + feat_from_nocs_head) + feat_from_size_head in float32 -- so grads["feat"] - (feat_from_reducer +
    feat_from_nocs_head) is feat_from_size_head exactly wherever that is zero, all but B C elements, and to one rounding of the sum at
    the B C others (a float32 subtraction does not undo an addition bit for bit) --; the six gradients and feat_from_size_head are within
    the yardstick of the float64 restatement on the device's own feat and grads["size"].  Fails without the feature: the keyword does
    not exist."""
    from givepose_amd import PoseLoss, enc_grad, size_grad
    from test_xyz_backward_gpu import same_bits
    cfg, net, data = small_net_and_batch()
    pl = PoseLoss()
    base = net.head_grads_backbone(data, pl, "cuda")
    none = net.head_grads_backbone(data, pl, "cuda", size_head=None)
    torch.cuda.synchronize()
    assert list(none) == list(base) == ["loss", "output", "grads", "param_grads"] and "feat_from_size_head" not in none["grads"]
    assert not [k for k in none["param_grads"] if k.startswith("size_head.")]
    same_bits(none["loss"], base["loss"], "loss")
    same_bits(none["output"], base["output"], "output")
    after_scatter = {"nocs_coor", "nocs_coor_from_encoder", "feat_from_nocs_head", "feat", "roi_img"}
    for part, exact in (("grads", lambda k: k not in after_scatter),
                        ("param_grads", lambda k: k.split(".")[0] in ("pnp_net", "xyz_deform_head", "feat_reducer")
                         or (k.startswith("nocs_encoder.") and k[len("nocs_encoder."):] in enc_grad.ATOMIC_FREE_KEYS))):
        assert list(none[part]) == list(base[part])
        for k, v in base[part].items():
            if exact(k):
                assert torch.equal(bits(none[part][k]), bits(v)), (part, k)
            else:
                assert float((none[part][k] - v).abs().max()) <= 1e-4 * float(v.abs().max()), (part, k)
    # ---- with the train-mode head
    res = net.head_grads_backbone(data, pl, "cuda", size_head={"seed": 7})
    torch.cuda.synchronize()
    assert list(res) == ["loss", "output", "grads", "size_head", "param_grads"]
    names = [k for k, _ in net.named_parameters(remove_duplicate=False) if not re.match(r"nocs_encoder\.features\.\d+\.bn\.", k)]
    assert set(res["param_grads"]) == set(names) and len(res["param_grads"]) == len(names)
    assert sorted(set(res["param_grads"]) - set(base["param_grads"])) == sorted("size_head." + k for k in size_grad.PARAM_KEYS)
    g = res["grads"]
    assert list(g) == list(base["grads"])[:-1] + ["feat_from_size_head", "roi_img"]
    partial = g["feat_from_reducer"] + g["feat_from_nocs_head"]
    assert torch.equal(bits(g["feat"]), bits(partial + g["feat_from_size_head"]))
    diff, fs = g["feat"] - partial, g["feat_from_size_head"]
    zero = fs == 0
    B, C = fs.shape[:2]
    assert int((~zero).sum()) <= B * C and int((~zero).sum()) > 0 and not bits(diff[zero]).any() and not bits(fs[zero]).any()
    assert float((diff - fs)[~zero].abs().max()) <= 2.0 ** -23 * float(g["feat"].abs().max())
    # the loss saw the train-mode prediction
    case, r64, r32 = restate_on_device_feat(net, data, 7, g["size"])
    ms = data["mean_size"].double()
    nm = ms / ms.norm(dim=1, keepdim=True)
    yardstick({"size": res["output"]["size"], "size_raw": res["size_head"]["outputs"]["size_raw"]}, {"size": r64["out"] + nm, "size_raw": r64["out"]},
              {"size": r32["out"] + nm.float(), "size_raw": r32["out"]}, "chain")
    assert np.array_equal(res["size_head"]["outputs"]["keep"].cpu().numpy(), case["keep"])
    assert not torch.equal(res["output"]["size"], base["output"]["size"]) and float(res["loss"]["Size"]) != float(base["loss"]["Size"])
    got = {**{k: res["param_grads"]["size_head." + k] for k in R.PARAM_KEYS if k != "conv1.bias"}, "feat": fs.view(B, C, -1),
           "mean": res["size_head"]["stats"]["mean"], "var_unbiased": res["size_head"]["stats"]["var_unbiased"]}
    worst = yardstick(got, {k: r64[k] for k in got}, {k: r32[k] for k in got}, "chain")
    worst = max(worst, db1_rule(res["param_grads"]["size_head.conv1.bias"], r64, r32, "chain"))
    for k in R.PARAM_KEYS:
        assert res["param_grads"]["size_head." + k].shape == net.state_dict()["size_head." + k].shape, k
    print(f"chain: largest device / CPU float32 ratio over the size head's entries {worst:.2f}")


# ------------------------------------------------------------------------------------------------ PoseNet.train_step
def test_train_step_twice_with_the_size_head():
    """Two train_steps with size_head={"seed": 7}: size_head.* follows ranger_ref in float64 within the rule of tests/test_optim_gpu.py (the
    clip coefficient is that of all gradients of the step); bn1's running statistics equal the restatement's two-step values within the
    yardstick and num_batches_tracked advanced by 2; the eval-mode forward after the steps equals, bit for bit, that of a fresh PoseNet
    loaded with the updated state_dict."""
    import ranger_ref as RR
    from givepose_amd import PoseLoss, PoseNet, Ranger, size_grad
    from test_optim_gpu import rule
    from test_xyz_backward_gpu import same_bits
    cfg, net, data = small_net_and_batch()
    fdata = {**data, "roi_mask": data["roi_mask_deform"]}
    tensors = lambda out: {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    opt = Ranger(net)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    fwd0 = tensors(net.forward_device(fdata, "cuda"))
    size_names = ["size_head." + k for k in size_grad.PARAM_KEYS]
    refs, run = None, {dt: {k: before["size_head.bn1." + k].cpu().to(dt) for k in ("running_mean", "running_var")} for dt in (torch.float64, torch.float32)}
    worst = 0.0
    for step in (1, 2):
        _, r64, r32 = restate_on_device_feat(net, data, 7, torch.zeros(2, 3))        # the statistics of this step's feat
        res = net.train_step(data, PoseLoss(), opt, "cuda", size_head={"seed": 7})
        torch.cuda.synchronize()
        names = [n for n in opt.param_names if n in res["param_grads"]]
        assert set(size_names) <= set(names)
        if refs is None:
            refs = [RR.RangerRef({n: before[n].cpu().to(dt) for n in names}) for dt in (torch.float64, torch.float32)]
        for dt, ref in zip((torch.float64, torch.float32), refs):
            ref.step({n: res["param_grads"][n].cpu().to(dt) for n in names}, clip_norm=5.0)
        sd = net.state_dict()
        worst = max(worst, rule({n: sd[n] for n in size_names}, {n: refs[0].p[n] for n in size_names}, {n: refs[1].p[n] for n in size_names}, f"train_step {step}"))
        for dt, r in ((torch.float64, r64), (torch.float32, r32)):
            m = torch.tensor(R.BN_MOMENTUM, dtype=dt)
            run[dt]["running_mean"] = (1 - m) * run[dt]["running_mean"] + m * r["mean"]
            run[dt]["running_var"] = (1 - m) * run[dt]["running_var"] + m * r["var_unbiased"]
        got = {k: sd["size_head.bn1." + k] for k in ("running_mean", "running_var")}
        worst = max(worst, yardstick(got, run[torch.float64], run[torch.float32], f"train_step {step}"))
        assert int(sd["size_head.bn1.num_batches_tracked"]) == int(before["size_head.bn1.num_batches_tracked"]) + step
        assert all(opt.steps[opt._index[n]] == step for n in size_names)
        for n in size_names + ["size_head.bn1.running_mean", "size_head.bn1.running_var"]:
            if n != "size_head.conv1.bias":          # its gradient is analytically zero: whether a bit of it moves says nothing
                assert not torch.equal(sd[n], before[n]), n
    print(f"train_step with the size head: largest device / CPU float32 ratio {worst:.2f}")
    sd = net.state_dict()
    fwd1 = tensors(net.forward_device(fdata, "cuda"))
    assert not torch.equal(fwd0["size"], fwd1["size"])
    fresh = PoseNet(cfg, dtype=torch.float32).cuda()
    fresh.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    same_bits(tensors(fresh.forward_device(fdata, "cuda")), fwd1, "forward after the steps")
    for k, v in net._module_params_f32("size_head", size_grad.PARAM_KEYS, "cuda").items():
        assert torch.equal(bits(v), bits(sd["size_head." + k])), k
