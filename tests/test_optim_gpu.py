"""GPU: the optimiser family (include/givepose_optim.h, gpo_*; givepose_amd/optim.py; PoseNet.train_step) against the float64 run of
tests/ranger_ref.py on the seeded cases of that file (13 steps: 1-5 unrectified, 6 the first rectified and first Lookahead step, 12 the
second Lookahead; the clip coefficient is exactly 1 on the even steps and far below 1 on the odd ones; one tensor has no gradient on
steps 3 and 9), each with seeded parameters at lr 1e-3 and with parameters 0 at lr 0.1, where p is the accumulated update itself.

The rule is that of tests/test_bb_backward_gpu.py (`yardstick`): after every step, per tensor and for each of p, exp_avg, exp_avg_sq and
slow_buffer, max|got - ref64| / max|ref64| is at most 8 times the figure of ranger_ref in float32 on the CPU on the same inputs, and that
figure counts as at least 2^-24; both are printed.  A tensor whose float64 reference is all zeros (the centralised (5,1) tensor's
moments) must be all zeros on the device.  The ratio lines of a run on an MI355X are kept in profiles/optim_step.txt.

Measured on an MI355X, largest device / CPU float32 ratio over steps, tensors and states (8 allowed):

    seeded parameters, lr 1e-3:  gc 2.24   nogc 2.24   gc_conv_only 2.24   weight decay 2.42
    parameters 0, lr 0.1:        gc 4.47   nogc 3.82   gc_conv_only 3.82   weight decay 2.74
    the norm 0.75 - 1.46; clip_grad_norm_ 0.69; train_step 0.92 over the 171 updated tensors

The largest, 4.47, is p of the 1-element tensor in the second run at step 13 (device 2.7e-7, CPU float32 6e-8): p is there the sum of
updates that largely cancel (1.2e-6 is left after step 12), so a rounding of one term weighs far more than one of p itself.
"""
import io

import numpy as np
import pytest
import torch

import ranger_ref as R
from test_enc_backward_gpu import yardstick
from test_xyz_backward_gpu import SENTINEL, Guarded, bits

pytestmark = pytest.mark.gpu
T = torch.from_numpy
KEYS = R.STATE_KEYS


class CaseNet(torch.nn.Module):
    """The case's tensors as the parameters of a module; alloc(name, shape) supplies their storage (guard bands, odd alignment)."""

    def __init__(self, arrays, alloc=None, alias=False):
        super().__init__()
        for n, a in arrays.items():
            t = T(a).cuda() if alloc is None else alloc("param." + n, a.shape).copy_(T(a))
            self.register_parameter(n, torch.nn.Parameter(t, requires_grad=False))
        if alias:        # one Parameter under two names, as ConvModule's .gn / .norm
            self.twin = torch.nn.Module()
            self.twin.register_parameter("conv", self.conv)
        self.updated = 0

    def params_updated(self):
        self.updated += 1


def shifted(name, shape):
    """Storage that starts 4 bytes past a 16-byte boundary: every quad of it moves as four 4-byte accesses."""
    whole = torch.zeros(int(np.prod(shape)) + 1, device="cuda")
    assert whole.data_ptr() % 16 == 0
    return whole[1:].view(shape)


def device_state(opt, net):
    """{name: {key: tensor}} of the optimiser's current state (views, not copies)."""
    idx = {n: opt._index[n] for n in R.SHAPES}
    return {n: {"p": getattr(net, n).data, **{k: opt._view(k, i) for k in KEYS[1:]}} for n, i in idx.items()}


def rule(got, ref64, ref32, what):
    """yardstick where the float64 reference is not all zeros; exact zeros where it is.  -> the largest ratio."""
    zero = [k for k, v in ref64.items() if not v.any()]
    for k in zero:
        assert not got[k].any(), (what, k, "the reference is an exact 0")
    live = [k for k in ref64 if k not in zero]
    return yardstick({k: got[k] for k in live}, {k: ref64[k] for k in live}, {k: ref32[k] for k in live}, what) if live else 0.0


def flat(states):
    return {f"{n}.{k}": v for n, s in states.items() for k, v in s.items()}


def grads_cuda(step, alloc=None):
    g = R.case_grads(step)
    return {n: T(a).cuda() if alloc is None else alloc("grad." + n, a.shape).copy_(T(a)) for n, a in g.items()}


def snapshot(states):
    return {n: {k: v.clone() for k, v in s.items()} for n, s in states.items()}


def same_states(a, b, what):
    for n in a:
        for k in KEYS:
            assert torch.equal(bits(a[n][k]), bits(b[n][k])), (what, n, k)


def run_device(variant, run, steps=R.STEPS, alloc=None, galloc=None, on_step=None, **kw):
    from givepose_amd import Ranger
    net = CaseNet(R.case_params(run), alloc)
    opt = Ranger(net, lr=R.RUNS[run], alloc=alloc if isinstance(alloc, Guarded) else None, **{**R.VARIANTS[variant], **kw})
    for step in range(1, steps + 1):
        opt.step(grads_cuda(step, galloc), clip_norm=R.CLIP)
        if on_step:
            on_step(step, opt, net)
    return opt, net


# ------------------------------------------------------------------------------------------------ the device against ranger_ref
@pytest.mark.parametrize("run", list(R.RUNS))
@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_ranger_against_float64(variant, run):
    guard = Guarded()
    refs = {dt: R.RangerRef({n: T(a).to(dt) for n, a in R.case_params(run).items()}, lr=R.RUNS[run], **R.VARIANTS[variant])
            for dt in (torch.float64, torch.float32)}
    start = {n: T(a) for n, a in R.case_params(run).items()}
    worst, before = [0.0], {}

    def check(step, opt, net):
        for dt, ref in refs.items():
            ref.step({n: T(g).to(dt) for n, g in R.case_grads(step).items()}, clip_norm=R.CLIP)
        r64, r32 = (flat({n: ref.tensors(n) for n in R.SHAPES}) for ref in refs.values())
        dev = device_state(opt, net)
        worst[0] = max(worst[0], rule(flat(dev), r64, r32, f"ranger {variant} {run} step {step}"))
        # the norm and the coefficient of this step
        norm, coef = opt.scalars.tolist()
        rule({"norm": np.float64(norm)}, {"norm": refs[torch.float64].norm.numpy()}, {"norm": refs[torch.float32].norm.numpy()},
             f"ranger {variant} {run} step {step}")
        assert (coef == 1.0) == (step % 2 == 0) and (coef == 1.0 or coef < 0.1)
        # the centralised tensor of row length 1: its gradient is an exact 0
        if refs[torch.float64].centralised(start["w51"]):
            assert not bits(dev["w51"]["exp_avg_sq"]).any()
            if refs[torch.float64].wd == 0:
                assert not bits(dev["w51"]["exp_avg"]).any()
                assert torch.equal(bits(dev["w51"]["p"]), bits(start["w51"].cuda())) and torch.equal(bits(dev["w51"]["slow_buffer"]), bits(start["w51"].cuda()))
        # the tensor without a gradient keeps every bit, and its step count
        if step in R.SKIP_STEPS["skip"]:
            for k in KEYS:
                assert torch.equal(bits(dev["skip"][k]), bits(before["skip"][k])), (step, k)
        before.update(snapshot({"skip": dev["skip"]}))
        assert net.updated == step

    opt, net = run_device(variant, run, alloc=guard, galloc=guard, on_step=check)
    guard.check()
    assert opt.steps[opt._index["skip"]] == R.STEPS - 2 and opt.steps[opt._index["w51"]] == R.STEPS
    print(f"ranger {variant} {run}: largest device / CPU float32 ratio over {R.STEPS} steps {worst[0]:.2f}")


# ------------------------------------------------------------------------------------------------ clipping
def test_clip_grad_norm():
    from givepose_amd import clip_grad_norm_
    for step in (1, 2):              # far above the threshold; below it
        guard = Guarded()
        g = grads_cuda(step, guard)
        g["conv_again"] = g["conv"]              # one tensor under two names counts once and is scaled once
        norm = clip_grad_norm_(g, R.CLIP, alloc=guard)
        guard.check()
        assert norm.device.type == "cuda" and norm.dim() == 0
        cpu = R.case_grads(step)
        ref = {}
        for dt in (torch.float64, torch.float32):
            gs = [T(a).to(dt) for a in cpu.values()]
            n = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(x) for x in gs]))
            c = torch.clamp(R.CLIP / (n + 1e-6), max=1.0)
            ref[dt] = {"norm": n, **{k: x * c for k, x in zip(cpu, gs)}}
        got = {"norm": norm, **{k: g[k] for k in cpu}}
        rule(got, ref[torch.float64], ref[torch.float32], f"clip_grad_norm_ step {step}")
        if step == 2:                # the coefficient is exactly 1: no bit of any gradient moves
            assert float(norm) < R.CLIP and all(torch.equal(bits(g[k]), bits(T(cpu[k]).cuda())) for k in cpu)
        else:
            assert float(norm) > 20 * R.CLIP
    for bad, match in (({"x": torch.ones(4, 4, device="cuda").t()}, "x.*not contiguous"), ({"x": torch.ones(4, device="cuda", dtype=torch.float16)}, "x.*float16"),
                       ({"x": torch.ones(4)}, "x.*HIP device")):
        with pytest.raises(ValueError, match=match):
            clip_grad_norm_(bad, 5.0)
    with pytest.raises(ValueError, match="max_norm"):
        clip_grad_norm_({"x": torch.ones(4, device="cuda")}, 0)


def test_fused_clip_agrees_with_clip_then_step():
    from givepose_amd import Ranger, clip_grad_norm_
    refs = {dt: R.run_case("gc", "seeded", dt, steps=0) for dt in (torch.float64, torch.float32)}
    nets = [CaseNet(R.case_params("seeded")) for _ in range(2)]
    fused, apart = (Ranger(n, lr=R.RUNS["seeded"]) for n in nets)
    for step in (1, 2):
        for dt, ref in refs.items():
            ref.step({n: T(g).to(dt) for n, g in R.case_grads(step).items()}, clip_norm=R.CLIP)
        fused.step(grads_cuda(step), clip_norm=R.CLIP)
        g = grads_cuda(step)
        clip_grad_norm_(g, R.CLIP)
        apart.step(g)
        assert float(apart.scalars[1]) == 1.0        # no second clip
        r64, r32 = (flat({n: ref.tensors(n) for n in R.SHAPES}) for ref in refs.values())
        a, b = device_state(fused, nets[0]), device_state(apart, nets[1])
        rule(flat(a), r64, r32, f"fused clip, step {step}")
        rule(flat(b), r64, r32, f"clip then step, step {step}")
        if step == 2:                # the coefficient is exactly 1 either way, and step 1 left rounding-level differences only
            assert float(fused.scalars[1]) == 1.0


# ------------------------------------------------------------------------------------------------ determinism, alignment, resuming
def test_two_runs_give_equal_bits_wherever_the_buffers_lie():
    a = device_state(*run_device("gc", "seeded"))
    b = device_state(*run_device("gc", "seeded"))
    same_states(a, b, "second run")
    c = device_state(*run_device("gc", "seeded", alloc=shifted, galloc=shifted))      # parameters and gradients off the 16-byte grid
    same_states(a, c, "4-byte aligned buffers")


def test_resuming_from_a_saved_state_dict_continues_bit_for_bit():
    from givepose_amd import Ranger
    whole = device_state(*run_device("gc", "seeded", steps=10))
    opt, net = run_device("gc", "seeded", steps=7)
    buf = io.BytesIO()
    torch.save({"optimizer": opt.state_dict(), "model": net.state_dict()}, buf)
    buf.seek(0)
    ckpt = torch.load(buf)
    assert sorted(ckpt["optimizer"]["state"]) == list(range(len(R.SHAPES))) and ckpt["optimizer"]["state"][opt._index["skip"]]["step"] == 6
    net2 = CaseNet({n: np.zeros(s, np.float32) for n, s in R.SHAPES.items()})
    net2.load_state_dict(ckpt["model"])
    opt2 = Ranger(net2, lr=0.5, k=3)          # the loaded group overrides these
    opt2.load_state_dict(ckpt["optimizer"])
    assert opt2.lr == R.RUNS["seeded"] and opt2.k == 6 and opt2.steps == opt.steps
    for step in (8, 9, 10):
        opt2.step(grads_cuda(step), clip_norm=R.CLIP)
    same_states(whole, device_state(opt2, net2), "resumed run")


def test_refusals_and_options():
    from givepose_amd import Ranger
    net = CaseNet(R.case_params("seeded"), alias=True)
    opt = Ranger(net)
    assert len(opt.params) == len(R.SHAPES) and opt._index["twin.conv"] == opt._index["conv"]
    g = grads_cuda(1)
    for bad, match in (({"odd": g["odd"].t().contiguous().t()}, "odd.*not contiguous"), ({"odd": g["odd"].half()}, "odd.*float16"),
                       ({"odd": g["odd"].cpu()}, "odd.*cpu"), ({"odd": g["long"]}, "odd.*expected contiguous float32 \\(3, 1031\\)"),
                       ({"nope": g["odd"]}, "no parameter of that name"), ({"conv": g["conv"], "twin.conv": 2 * g["conv"]}, "different gradients")):
        with pytest.raises(ValueError, match=match):
            opt.step(bad)
    assert opt.steps == [0] * len(R.SHAPES) and net.updated == 0          # a refused step changes nothing
    with pytest.raises(ValueError, match="clip_norm"):
        opt.step(g, clip_norm=0)
    # both names of one parameter with one gradient: a single update; per-call lr
    p0 = net.conv.detach().clone()
    opt.step({"conv": g["conv"], "twin.conv": g["conv"]}, lr=0.25)
    ref = R.RangerRef({"conv": p0.double().cpu()}, lr=0.25)
    ref.step({"conv": g["conv"].double().cpu()})
    ref32 = R.RangerRef({"conv": p0.cpu()}, lr=0.25)
    ref32.step({"conv": g["conv"].cpu()})
    rule({"p": net.conv.data}, {"p": ref.p["conv"]}, {"p": ref32.p["conv"]}, "aliased names, lr per call")
    assert opt.steps[opt._index["conv"]] == 1 and sum(opt.steps) == 1 and float(opt.scalars[1]) == 1.0


# ------------------------------------------------------------------------------------------------ PoseNet.train_step
def test_train_step():
    """train_step on a network of depths (1,1,1,1) at B = 2: (a) the updated parameters within the rule of ranger_ref in float64 applied to
    the param_grads the step itself returns (it leaves them unscaled); (b) size_head.* and the never-applied bn.* keep their bits and
    have no state; (c) a forward after the step differs from the one before and equals, bit for bit, the forward of a fresh PoseNet loaded
    with the updated state_dict; (d) the fp32 parameter copies of the backward equal the parameters bit for bit."""
    import re

    import bb_backward_ref as B
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, Ranger, bb_grad, enc_grad
    from test_xyz_backward_gpu import loss_batch, same_bits
    cfg = PoseNetConfig(convnext_depths=(1, 1, 1, 1))
    net = PoseNet(cfg, dtype=torch.float32, seed=B.WEIGHT_SEED).cuda()
    data = {k: v[:2] if v.dim() and v.shape[0] == 4 else v for k, v in loss_batch().items()}
    fdata = {**data, "roi_mask": data["roi_mask_deform"]}
    tensors = lambda out: {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    opt = Ranger(net)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    fwd0 = tensors(net.forward_device(fdata, "cuda"))
    res = net.train_step(data, PoseLoss(), opt, "cuda")
    assert list(res["loss"]) and set(res) >= {"loss", "grads", "param_grads", "output"}
    norm, coef = opt.scalars.tolist()
    assert norm > 0 and 0 < coef <= 1
    # (a)
    names = [n for n in opt.param_names if n in res["param_grads"]]
    frozen = [n for n in opt.param_names if n not in res["param_grads"]]
    assert frozen and all(n.startswith("size_head.") or re.match(r"nocs_encoder\.features\.\d+\.bn\.", n) for n in frozen)
    refs = []
    for dt in (torch.float64, torch.float32):
        ref = R.RangerRef({n: before[n].cpu().to(dt) for n in names})
        ref.step({n: res["param_grads"][n].cpu().to(dt) for n in names}, clip_norm=5.0)
        refs.append(ref)
    sd = net.state_dict()
    worst = rule({n: sd[n] for n in names}, refs[0].p, refs[1].p, "train_step")
    rule({"norm": np.float64(norm)}, {"norm": refs[0].norm.numpy()}, {"norm": refs[1].norm.numpy()}, "train_step")
    print(f"train_step: largest device / CPU float32 ratio over the {len(names)} updated tensors {worst:.2f}")
    # (b)
    state = opt.state_dict()["state"]
    for n in frozen:
        assert torch.equal(bits(sd[n]), bits(before[n])) and opt._index[n] not in state and opt.steps[opt._index[n]] == 0, n
    assert sorted(state) == sorted(opt._index[n] for n in names) and all(s["step"] == 1 for s in state.values())
    for n, v in sd.items():            # aliases and buffers: .gn follows .norm, the running statistics stay
        if n not in opt._index:
            assert torch.equal(v, before[n]), n
    # (c)
    fwd1 = tensors(net.forward_device(fdata, "cuda"))
    assert any(not torch.equal(fwd0[k], fwd1[k]) for k in fwd0)
    fresh = PoseNet(cfg, dtype=torch.float32).cuda()
    fresh.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    same_bits(tensors(fresh.forward_device(fdata, "cuda")), fwd1, "forward after the step")
    # (d)
    for module, keys in (("backbone", bb_grad.PARAM_KEYS(cfg)), ("nocs_encoder", enc_grad.PARAM_KEYS), ("feat_reducer", ("weight", "bias"))):
        for k, v in net._module_params_f32(module, keys, "cuda").items():
            assert torch.equal(bits(v), bits(sd[f"{module}.{k}"])), (module, k)
    with pytest.raises(ValueError, match="built over this model"):
        fresh.train_step(data, PoseLoss(), opt, "cuda")
