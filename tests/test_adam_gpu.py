"""GPU: Adam and AdamW (include/givepose_adam.h, gpad_*; givepose_amd/optim.py; PoseNet.train_step) on the cases of tests/ranger_ref.py
plus two flat tensors of exactly GPO_CHUNK and GPO_CHUNK + 1 elements (tests/adam_ref.py): 13 steps; the clip coefficient is exactly 1 on
the even steps and far below 1 on the odd ones; one tensor has no gradient on steps 3 and 9; seeded parameters at lr 1e-3 and parameters
0 at lr 0.1, where p is the accumulated update itself.  The variants are Adam wd 0, AdamW wd 1e-2, Adam wd 1e-2 and AdamW with amsgrad.
Every buffer comes from a guard-band allocator, once on the 16-byte grid and once 4 bytes off it.

Two yardsticks.  (1) Bits: after every step p, exp_avg, exp_avg_sq and max_exp_avg_sq equal, bit for bit, the numpy float32 restatement of
the header's contract (adam_ref.AdamRef) fed the device's own clip coefficient.  (2) DESIGN.md 1e's rule against torch itself: per tensor
and state, max|got - ref64| / max|ref64| is at most 8 times the figure of torch's float32 CPU run, which counts as at least 2^-24, where
ref64 is torch.optim.Adam / AdamW (foreach=False) in float64 after torch.nn.utils.clip_grad_norm_.

Measured on an MI355X: 0 elements differ from the restatement in every variant, run, step and placement.  Largest device / torch float32
ratio over steps, tensors and states (8 allowed): 2.64 in both runs of adam, adamw and adamw_ams, 1.94 / 3.00 (seeded / zero) with adam_wd;
the accumulated AdamW 3.45; train_step 1.43 over the 171 updated tensors.  The ratio lines are kept in profiles/adam_step.txt.
"""
import functools
import io

import numpy as np
import pytest
import torch

import adam_ref as A

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SENTINEL = -7.25


class Guard:
    """alloc(name, shape): every buffer has at least 64 sentinel elements on either side; with shift = 1 it starts 4 bytes past a 16-byte
    boundary, so that every quad of it moves as four 4-byte accesses (the workspace stays 256-byte aligned, as its contract asks).
    check() wants every element outside the buffers untouched, every element of a buffer written, and everything finite."""

    def __init__(self, shift=0):
        self.shift, self.bufs = shift, []

    def __call__(self, name, shape):
        n = int(np.prod(shape))
        whole = torch.full((n + 132,), SENTINEL, device="cuda", dtype=torch.float32)
        off = 64 + (0 if name == "workspace" else self.shift)
        view = whole[off:off + n].view(shape)
        assert view.data_ptr() % 256 == 4 * (off - 64)
        self.bufs.append((name, whole, off, n))
        return view

    def check(self):
        torch.cuda.synchronize()
        assert self.bufs
        for name, whole, off, n in self.bufs:
            assert torch.all(whole[:off] == SENTINEL) and torch.all(whole[off + n:] == SENTINEL), name
            if name != "workspace":
                assert not torch.any(whole[off:off + n] == SENTINEL) and torch.all(torch.isfinite(whole[off:off + n])), name


class CaseNet(torch.nn.Module):
    """The case's tensors as the parameters of a module; alloc(name, shape) supplies their storage."""

    def __init__(self, arrays, alloc):
        super().__init__()
        for n, a in arrays.items():
            self.register_parameter(n, torch.nn.Parameter(alloc("param." + n, a.shape).copy_(T(a)), requires_grad=False))
        self.updated = 0

    def params_updated(self):
        self.updated += 1


def plain(name, shape):
    return torch.empty(shape, device="cuda", dtype=torch.float32)


def make(variant, run, alloc, **kw):
    import givepose_amd
    cls, args = A.VARIANTS[variant]
    net = CaseNet(A.case_params(run), alloc)
    return getattr(givepose_amd, cls)(net, lr=A.RUNS[run], alloc=alloc, **{**args, **kw}), net


def grads_cuda(step, alloc=plain, scale=None):
    return {n: alloc("grad." + n, a.shape).copy_(T(a if scale is None else a * np.float32(scale))) for n, a in A.case_grads(step).items()}


def device_state(opt, net, names=None):
    """{name: {key: array}} of the optimiser's current state, copied to the host."""
    keys = A.STATE_KEYS[1:] if opt.amsgrad else A.STATE_KEYS[1:3]
    return {n: {"p": getattr(net, n).detach().cpu().numpy(), **{k: opt._view(k, opt._index[n]).cpu().numpy() for k in keys}} for n in names or A.SHAPES}


def same_bits(a, b, what):
    for n in a:
        assert set(a[n]) == set(b[n]), (what, n)
        for k in a[n]:
            x, y = np.ascontiguousarray(a[n][k]), np.ascontiguousarray(b[n][k])
            assert x.dtype == y.dtype == np.float32 and x.shape == y.shape, (what, n, k)
            diff = x.view(np.int32) != y.view(np.int32)
            assert not diff.any(), (what, n, k, int(diff.sum()), "of", diff.size, "elements differ")


@functools.lru_cache(maxsize=None)
def torch_runs(variant, run, steps=A.STEPS):
    """torch's own optimiser after clip_grad_norm_ on the CPU, in float64 and float32: per step ({name: state} x 2, norm x 2).  Computed
    once per (variant, run) and shared."""
    amsgrad = A.VARIANTS[variant][1].get("amsgrad", False)
    runs = [A.make_torch(variant, A.case_params(run), A.RUNS[run], dt) for dt in (torch.float64, torch.float32)]
    out = []
    for step in range(1, steps + 1):
        grads = A.case_grads(step)
        norms = [A.torch_step(o, ps, grads).numpy().astype(np.float64) for o, ps in runs]
        out.append(tuple({n: A.torch_tensors(o, ps, n, amsgrad) for n in A.SHAPES} for o, ps in runs) + tuple(norms))
    return out


def flat(states):
    return {f"{n}.{k}": v for n, s in states.items() for k, v in s.items()}


# ------------------------------------------------------------------------------------------------ bits, float64 rule, norm, invariants
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off_grid"])
@pytest.mark.parametrize("run", list(A.RUNS))
@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_adam_bits_and_float64(variant, run, shift):
    from givepose_amd import clip_grad_norm_
    guard = Guard(shift)
    opt, net = make(variant, run, guard)
    ref = A.make_ref(variant, A.case_params(run), A.RUNS[run])
    refs = torch_runs(variant, run)
    worst, before = 0.0, None
    for step in range(1, A.STEPS + 1):
        g = grads_cuda(step, guard)
        kept = {n: t.clone() for n, t in g.items()}
        opt.step(g, clip_norm=A.CLIP)
        norm, coef = opt.scalars.cpu().numpy()
        assert norm.dtype == np.float32 and (coef == 1.0) == (step % 2 == 0) and (coef == 1.0 or coef < 0.1)
        for n in g:                                  # the gradients are read, not scaled
            assert torch.equal(g[n], kept[n]), n
        # (1) the restatement, fed the device's coefficient: every bit
        ref.step(A.case_grads(step), coef)
        dev = device_state(opt, net)
        same_bits(dev, {n: ref.tensors(n) for n in A.SHAPES}, f"{variant} {run} step {step}")
        # (2) torch in float64
        r64, r32, n64, n32 = refs[step - 1]
        worst = max(worst, A.rule(flat(dev), flat(r64), flat(r32), f"{variant} {run} step {step}", quiet=True))
        A.rule({"norm": np.float64(norm)}, {"norm": n64}, {"norm": n32}, f"{variant} {run} step {step}", quiet=True)
        # the norm has the bits of the library's clip_grad_norm_ on the same gradients
        clipped = clip_grad_norm_(kept, A.CLIP)
        assert clipped.cpu().numpy().view(np.int32) == norm.view(np.int32), (step, float(clipped), float(norm))
        # the tensor without a gradient keeps every bit, and its step count
        if step in A.SKIP_STEPS["skip"]:
            same_bits({"skip": dev["skip"]}, {"skip": before["skip"]}, f"skipped at step {step}")
        before = dev
        assert net.updated == step
    guard.check()
    assert opt.steps[opt._index["skip"]] == A.STEPS - 2 and opt.steps[opt._index["chunk1"]] == A.STEPS
    print(f"{variant} {run} {'off grid' if shift else 'aligned'}: largest device / torch float32 ratio over {A.STEPS} steps {worst:.2f}")


def test_two_runs_give_equal_bits_wherever_the_buffers_lie():
    runs = []
    for alloc, galloc in ((plain, plain), (Guard(0), plain), (Guard(1), Guard(1)), (plain, Guard(1))):
        opt, net = make("adamw_ams", "seeded", alloc)
        for step in range(1, 8):
            opt.step(grads_cuda(step, galloc), clip_norm=A.CLIP)
        runs.append((device_state(opt, net), opt.scalars.cpu().numpy()))
    for other, sc in runs[1:]:
        same_bits(runs[0][0], other, "another placement")
        assert np.array_equal(sc.view(np.int32), runs[0][1].view(np.int32))


# ------------------------------------------------------------------------------------------------ clipping
def test_fused_clip_agrees_with_clip_then_step():
    from givepose_amd import clip_grad_norm_
    refs = torch_runs("adamw", "seeded")
    (fused, fnet), (apart, anet) = (make("adamw", "seeded", plain) for _ in range(2))
    for step in (1, 2):
        fused.step(grads_cuda(step), clip_norm=A.CLIP)
        g = grads_cuda(step)
        clip_grad_norm_(g, A.CLIP)
        apart.step(g)
        assert float(apart.scalars[1]) == 1.0        # no second clip
        r64, r32 = refs[step - 1][:2]
        A.rule(flat(device_state(fused, fnet)), flat(r64), flat(r32), f"fused clip, step {step}", quiet=True)
        A.rule(flat(device_state(apart, anet)), flat(r64), flat(r32), f"clip then step, step {step}", quiet=True)
        if step == 2:                # the coefficient is exactly 1 either way
            assert float(fused.scalars[1]) == 1.0


# ------------------------------------------------------------------------------------------------ resuming
def test_resuming_from_a_saved_state_dict_continues_bit_for_bit():
    from givepose_amd import AdamW

    def run(lo, hi, opt, net):
        for step in range(lo, hi + 1):
            opt.step(grads_cuda(step), clip_norm=A.CLIP)
        return opt, net
    whole = device_state(*run(1, 10, *make("adamw_ams", "seeded", plain)))
    opt, net = run(1, 7, *make("adamw_ams", "seeded", plain))
    buf = io.BytesIO()
    torch.save({"optimizer": opt.state_dict(), "model": net.state_dict()}, buf)
    buf.seek(0)
    ckpt = torch.load(buf)
    state = ckpt["optimizer"]["state"]
    assert sorted(state) == list(range(len(A.SHAPES))) and float(state[opt._index["skip"]]["step"]) == 6 and state[0]["step"].dtype == torch.float32
    assert set(state[0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    net2 = CaseNet({n: np.zeros(s, np.float32) for n, s in A.SHAPES.items()}, plain)
    net2.load_state_dict(ckpt["model"])
    opt2 = AdamW(net2, lr=0.5, weight_decay=0.3, amsgrad=True)          # the loaded group overrides these
    opt2.load_state_dict(ckpt["optimizer"])
    assert opt2.lr == A.RUNS["seeded"] and opt2.weight_decay == 1e-2 and opt2.steps == opt.steps
    same_bits(whole, device_state(*run(8, 10, opt2, net2)), "resumed run")
    # and torch's own class takes the same checkpoint
    topt = torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu()) for p in net.parameters()], amsgrad=True)
    topt.load_state_dict(ckpt["optimizer"])
    assert topt.param_groups[0]["lr"] == A.RUNS["seeded"] and len(topt.state) == len(A.SHAPES)


# ------------------------------------------------------------------------------------------------ refusals and options
def test_refusals_and_options():
    opt, net = make("adamw", "seeded", plain)
    g = grads_cuda(1)
    for bad, match in (({"odd": g["odd"].t().contiguous().t()}, "odd.*not contiguous"), ({"odd": g["odd"].half()}, "odd.*float16"),
                       ({"odd": g["odd"].cpu()}, "odd.*cpu"), ({"odd": g["long"]}, "odd.*expected contiguous float32 \\(3, 1031\\)"),
                       ({"nope": g["odd"]}, "no parameter of that name")):
        with pytest.raises(ValueError, match=match):
            opt.step(bad)
    assert opt.steps == [0] * len(A.SHAPES) and net.updated == 0          # a refused step changes nothing
    # one tensor alone, per-call lr, no clip: the restatement's bits
    p0 = net.conv.detach().cpu().numpy()
    opt.step({"conv": g["conv"]}, lr=0.25)
    ref = A.make_ref("adamw", {"conv": p0}, 0.25)
    ref.step({"conv": A.case_grads(1)["conv"]}, 1.0)
    same_bits(device_state(opt, net, ["conv"]), {"conv": ref.tensors("conv")}, "lr per call")
    assert opt.steps[opt._index["conv"]] == 1 and sum(opt.steps) == 1 and float(opt.scalars[1]) == 1.0 and net.updated == 1


# ------------------------------------------------------------------------------------------------ accumulation
def test_accumulation_with_adamw_against_the_loop_in_float64():
    """GradAccumulator over AdamW, accumulate = 2, four micro-steps, against a float64 torch replay of engine/train.py:117-131: the loss is
    divided by accumulate, so every backward adds g / accumulate to .grad; clip_grad_norm_(., 5) clips the ACCUMULATED gradients in place
    on every micro-step; when global_step % accumulate == 0 (global_step starts at 0) the optimiser steps and the gradients are dropped."""
    from givepose_amd import GradAccumulator
    accumulate, guard = 2, Guard(0)
    opt, net = make("adamw", "seeded", guard)
    acc = GradAccumulator(opt, alloc=guard)
    runs = [A.make_torch("adamw", A.case_params("seeded"), A.RUNS["seeded"], dt) for dt in (torch.float64, torch.float32)]
    stepped = 0
    for i in range(4):
        grads = A.case_grads(i + 1)
        acc.add(grads_cuda(i + 1, guard), scale=1.0 / accumulate, clip_norm=A.CLIP)
        if i % accumulate == 0:
            opt.step(acc.grads, clip_norm=None)
            acc.zero()
            stepped += 1
        for o, ps in runs:
            for n, a in grads.items():
                gs = T(a).to(ps[n].dtype) / accumulate
                ps[n].grad = gs if ps[n].grad is None else ps[n].grad + gs
            torch.nn.utils.clip_grad_norm_([p for p in ps.values() if p.grad is not None], A.CLIP)
            if i % accumulate == 0:
                o.step()
                o.zero_grad(set_to_none=True)
        r64, r32 = ({n: A.torch_tensors(o, ps, n, False) for n in A.SHAPES} for o, ps in runs)
        worst = A.rule(flat(device_state(opt, net)), flat(r64), flat(r32), f"accumulate {accumulate}, micro-step {i}", quiet=True)
        print(f"accumulated AdamW, micro-step {i}: largest device / torch float32 ratio {worst:.2f}")
    guard.check()
    assert stepped == 2 and net.updated == 2 and opt.steps[opt._index["skip"]] == 2 and float(opt.scalars[1]) == 1.0


# ------------------------------------------------------------------------------------------------ PoseNet.train_step
def test_train_step_with_adamw():
    """train_step with AdamW on the network of depths (1,1,1,1) at B = 2 (that of test_optim_gpu.py::test_train_step): (a) every updated
    tensor within the float64 rule against torch.optim.AdamW fed the param_grads the step itself returns, after clip_grad_norm_(., 5);
    (b) the tensors without a gradient keep their bits and have no state; (c) the forward after the step equals, bit for bit, the forward
    of a fresh PoseNet loaded with the updated state dict."""
    import bb_backward_ref as B
    from givepose_amd import AdamW, PoseLoss, PoseNet, PoseNetConfig, build_optimizer
    from test_xyz_backward_gpu import loss_batch, same_bits as same_tensors
    cfg = PoseNetConfig(convnext_depths=(1, 1, 1, 1))
    net = PoseNet(cfg, dtype=torch.float32, seed=B.WEIGHT_SEED).cuda()
    data = {k: v[:2] if v.dim() and v.shape[0] == 4 else v for k, v in loss_batch().items()}
    fdata = {**data, "roi_mask": data["roi_mask_deform"]}
    tensors = lambda out: {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    opt = build_optimizer(net, "AdamW", 1e-3)
    assert type(opt) is AdamW and opt.model is net
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    fwd0 = tensors(net.forward_device(fdata, "cuda"))
    res = net.train_step(data, PoseLoss(), opt, "cuda")
    norm, coef = opt.scalars.tolist()
    assert list(res["loss"]) and norm > 0 and 0 < coef <= 1
    # (a)
    names = [n for n in opt.param_names if n in res["param_grads"]]
    frozen = [n for n in opt.param_names if n not in res["param_grads"]]
    assert names and frozen
    grads = {n: res["param_grads"][n].cpu().numpy() for n in names}
    runs = [A.make_torch("adamw", {n: before[n].cpu().numpy() for n in names}, 1e-3, dt) for dt in (torch.float64, torch.float32)]
    norms = [A.torch_step(o, ps, grads, clip=5.0) for o, ps in runs]
    sd = net.state_dict()
    worst = A.rule({n: sd[n] for n in names}, *({n: ps[n].detach() for n in names} for _, ps in runs), "train_step", quiet=True)
    A.rule({"norm": np.float64(norm)}, {"norm": norms[0].numpy()}, {"norm": norms[1].numpy()}, "train_step")
    print(f"train_step with AdamW: largest device / torch float32 ratio over the {len(names)} updated tensors {worst:.2f}")
    # (b)
    state = opt.state_dict()["state"]
    for n in frozen:
        assert torch.equal(sd[n].view(torch.int32), before[n].view(torch.int32)) and opt._index[n] not in state and opt.steps[opt._index[n]] == 0, n
    assert sorted(state) == sorted(opt._index[n] for n in names) and all(float(s["step"]) == 1 for s in state.values())
    # (c)
    fwd1 = tensors(net.forward_device(fdata, "cuda"))
    assert any(not torch.equal(fwd0[k], fwd1[k]) for k in fwd0)
    fresh = PoseNet(cfg, dtype=torch.float32).cuda()
    fresh.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    same_tensors(tensors(fresh.forward_device(fdata, "cuda")), fwd1, "forward after the step")
    with pytest.raises(ValueError, match="built over this model"):
        fresh.train_step(data, PoseLoss(), opt, "cuda")
