"""GPU: the gradient-accumulation family (include/givepose_accum.h, gpc_*; givepose_amd.optim.GradAccumulator; the accumulator keywords of
PoseNet.train_step) against the float64 run of tests/grad_accum_ref.py on the seeded cases of tests/ranger_ref.py.

The rule is `rule` of tests/test_optim_gpu.py (`yardstick` of tests/test_enc_backward_gpu.py): per tensor, max|got - ref64| / max|ref64|
is at most 8 times the figure of the same arithmetic in float32 on the CPU, which counts as at least 2^-24; a reference that is all
zeros demands exact zeros.  Both figures are printed.  The ratio lines of a run on an MI355X are kept in profiles/grad_accum.txt.

Measured on an MI355X, largest device / CPU float32 ratio (8 allowed):

    test_window_against_float64                  1.74 over 7 micro-steps (grads, the norm, and the four states on the stepping ones)
    test_two_ranks_with_different_gradients      1.80 (exp_avg of the 7-element tensor; p, exp_avg and the norm of the last add)
    test_train_step_accumulates                  1.53 over the 171 updated tensors at micro-steps 0 and 2
    the norm alone: 0.01 - 1.52

The other tests compare bits.  test_train_step_without_the_keywords_is_the_parent_body feeds the twin's step the gradients that
train_step returned: the map encoder's backward adds with atomics, so two runs of the backward chain differ in the last bits.

The two-rank tests run both ranks on the one GPU of the box over gloo; the one-rank RCCL test proves that the flat buffer goes through
RCCL's all_reduce on this code's stream.  Multi-GPU RCCL behaviour over xGMI stays unmeasured here.
"""
import multiprocessing as mp
import socket

import numpy as np
import pytest
import torch

import grad_accum_ref as A
import ranger_ref as R
from test_optim_gpu import CaseNet, device_state, flat, grads_cuda, rule, same_states, shifted
from test_xyz_backward_gpu import SENTINEL, Guarded, bits

pytestmark = pytest.mark.gpu
T = torch.from_numpy
LR = R.RUNS["seeded"]
ACCUMULATE, MICRO_STEPS = 3, 7               # the window: steps fall at micro-steps 0, 3 and 6; micro-step i is fed case_grads(i + 1)


def off_grid(name, shape):
    """`shifted` for everything but the workspace, which the library wants 256-byte aligned."""
    return torch.empty(int(np.prod(shape)), device="cuda").view(shape) if name == "workspace" else shifted(name, shape)


def run_window(alloc=None, galloc=None, on_micro_step=None, accumulate=ACCUMULATE, micro_steps=MICRO_STEPS):
    """The reference's loop over the seeded cases on the device.  -> (accumulator, optimiser, net, the grads after every micro-step)."""
    from givepose_amd import GradAccumulator, Ranger
    net = CaseNet(R.case_params("seeded"), alloc)
    opt = Ranger(net, lr=LR, alloc=alloc if alloc is not shifted else off_grid)
    acc = GradAccumulator(opt, alloc=alloc if alloc is not shifted else off_grid)
    seen = []
    for i in range(micro_steps):
        acc.add(grads_cuda(i + 1, galloc), scale=1.0 / accumulate, clip_norm=R.CLIP)
        stepped = i % accumulate == 0
        if stepped:
            opt.step(acc.grads, clip_norm=None)
        seen.append(({n: g.clone() for n, g in acc.grads.items()}, acc.scalars.clone()))
        if on_micro_step:
            on_micro_step(i, acc, opt, net, stepped)
        if stepped:
            acc.zero()
    return acc, opt, net, seen


def padding_of(acc):
    """The elements of acc.flat between the tensors."""
    o, sizes = acc._offsets, [p.numel() for p in acc.optimizer.params]
    return torch.cat([acc.flat[int(o[i]) + n:int(o[i + 1])] for i, n in enumerate(sizes)])


# ------------------------------------------------------------------------------------------------ 1. a window against float64
def reference_window(dtype, accumulate=ACCUMULATE, micro_steps=MICRO_STEPS):
    """Per micro-step: {"grads", "norm", "coef", "stepped", "state" (on stepping micro-steps)} of loop_ref in `dtype`."""
    out = []

    def keep(i, acc, opt, stepped):
        out.append({"grads": dict(acc.acc), "norm": acc.norm, "coef": float(acc.coef), "stepped": stepped,
                    "state": flat({n: dict(opt.tensors(n)) for n in R.SHAPES}) if stepped else None})
    A.loop_ref(R.case_params("seeded"), [R.case_grads(i + 1) for i in range(micro_steps)], accumulate, R.CLIP, LR, dtype, on_micro_step=keep)
    return out


def test_window_against_float64():
    guard = Guarded()
    r64, r32 = reference_window(torch.float64), reference_window(torch.float32)
    worst = [0.0]

    def check(i, acc, opt, net, stepped):
        what = f"window micro-step {i}"
        assert stepped == r64[i]["stepped"] == (i in (0, 3, 6))
        got = acc.grads
        assert set(got) == set(r64[i]["grads"]) and acc.live == list(got)
        assert ("skip" in R.case_grads(i + 1)) == (i != 2) and "skip" in got          # live at micro-step 2 without a gradient there
        worst[0] = max(worst[0], rule(got, r64[i]["grads"], r32[i]["grads"], what + " grads"))
        norm, coef = acc.scalars.tolist()
        worst[0] = max(worst[0], rule({"norm": np.float64(norm)}, {"norm": r64[i]["norm"].numpy()}, {"norm": r32[i]["norm"].numpy()}, what))
        # odd cases are far above the threshold; an even one stays below it unless it adds to what is left of an odd one
        assert (coef == 1.0) == (r64[i]["coef"] == 1.0) and (coef < 0.2) == (i % 2 == 0)
        if stepped:
            worst[0] = max(worst[0], rule(flat(device_state(opt, net)), r64[i]["state"], r32[i]["state"], what + " state"))
            assert float(opt.scalars[1]) == 1.0          # the step itself does not clip again

    acc, opt, net, _ = run_window(alloc=guard, galloc=guard, on_micro_step=check)
    guard.check()
    assert {r["coef"] == 1.0 for r in r64} == {True, False}
    assert not bits(padding_of(acc)).any() and padding_of(acc).numel() > 0          # the padding of flat: never written
    assert opt.steps == [3] * len(R.SHAPES) and net.updated == 3 and acc.live == []
    print(f"window: largest device / CPU float32 ratio over {MICRO_STEPS} micro-steps {worst[0]:.2f}")


# ------------------------------------------------------------------------------------------------ 2. exact identities
def fresh_accumulator(alloc=None):
    from givepose_amd import GradAccumulator, Ranger
    net = CaseNet(R.case_params("seeded"))
    return GradAccumulator(Ranger(net, lr=LR), alloc=alloc)


def test_exact_identities():
    from givepose_amd import clip_grad_norm_
    g = grads_cuda(1)
    # overwrite with scale 1 and no clip: the bits of g, and the norm with coefficient exactly 1
    acc = fresh_accumulator()
    acc.add(g)
    assert all(torch.equal(bits(acc.grads[n]), bits(g[n])) for n in g) and float(acc.scalars[1]) == 1.0 and float(acc.scalars[0]) > 20 * R.CLIP
    # scale 0.5 added twice from the same g: g
    acc = fresh_accumulator()
    acc.add(g, scale=0.5)
    assert all(torch.equal(bits(acc.grads[n]), bits(0.5 * g[n])) for n in g)
    acc.add(g, scale=0.5)
    assert all(torch.equal(bits(acc.grads[n]), bits(g[n])) for n in g)
    # overwrite, scale 1, clip: the bits of clip_grad_norm_ on a clone -- data, norm and coefficient
    for step in (1, 2):              # clipped hard; coefficient exactly 1, no bit moves
        g = grads_cuda(step)
        clone, kept = {n: t.clone() for n, t in g.items()}, {}

        def keep(name, shape):
            kept[name] = torch.empty(shape, device="cuda")
            return kept[name]
        clip_grad_norm_(clone, R.CLIP, alloc=keep)
        acc = fresh_accumulator()
        acc.add(g, scale=1.0, clip_norm=R.CLIP)
        assert torch.equal(bits(acc.scalars), bits(kept["scalars"])), (step, acc.scalars.tolist(), kept["scalars"].tolist())
        assert all(torch.equal(bits(acc.grads[n]), bits(clone[n])) for n in g), step
        assert (float(acc.scalars[1]) == 1.0) == (step == 2)
        if step == 2:
            assert all(torch.equal(bits(acc.grads[n]), bits(g[n])) for n in g)
    # a live tensor with a null g is counted in the norm and scaled by the coefficient: exactly what a gradient of zeros gives
    small, big = grads_cuda(2), grads_cuda(3)
    assert "skip" in small and "skip" not in big
    acc, twin = fresh_accumulator(), fresh_accumulator()
    for a in (acc, twin):
        a.add({n: 100.0 * t for n, t in small.items()})
    before = acc.grads["skip"].clone()
    total = sum(float((acc.grads[n].double() + (big[n].double() if n in big else 0.0)).square().sum()) for n in R.SHAPES)
    counted, left_out = np.sqrt(total), np.sqrt(total - float(before.double().square().sum()))
    acc.add(big, clip_norm=R.CLIP)
    assert abs(float(acc.scalars[0]) - counted) <= 1e-5 * counted < abs(float(acc.scalars[0]) - left_out)
    twin.add({**big, "skip": torch.zeros_like(before)}, clip_norm=R.CLIP)
    coef = acc.scalars[1]
    assert float(coef) < 0.1 and torch.equal(bits(acc.scalars), bits(twin.scalars))
    assert torch.equal(bits(acc.grads["skip"]), bits(before * coef)) and "skip" in acc.live
    assert all(torch.equal(bits(acc.grads[n]), bits(twin.grads[n])) for n in R.SHAPES)
    # a parameter that was never added keeps its sentinel and is absent from grads
    acc = fresh_accumulator()
    acc.flat.fill_(SENTINEL)
    acc.add(big, clip_norm=R.CLIP)
    assert "skip" not in acc.grads and "skip" not in acc.live and len(acc.grads) == len(R.SHAPES) - 1
    assert torch.all(acc._view(acc.optimizer._index["skip"]) == SENTINEL) and torch.all(padding_of(acc) == SENTINEL)
    assert all(not torch.any(v == SENTINEL) for v in acc.grads.values())


# ------------------------------------------------------------------------------------------------ 3. determinism and alignment
def test_two_runs_give_equal_bits_wherever_the_buffers_lie():
    def same(x, y, what):
        for i, ((ga, sa), (gb, sb)) in enumerate(zip(x[3], y[3])):
            assert list(ga) == list(gb) and torch.equal(bits(sa), bits(sb)), (what, i, "scalars")
            for n in ga:
                assert torch.equal(bits(ga[n]), bits(gb[n])), (what, i, n)
        same_states(device_state(x[1], x[2]), device_state(y[1], y[2]), what)
    a, b = run_window(), run_window()
    same(a, b, "second run")
    c = run_window(alloc=shifted, galloc=shifted)          # flat, the gradients, the parameters and the state off the 16-byte grid
    assert c[0].flat.data_ptr() % 16 == 4 and c[1]._flat["exp_avg"].data_ptr() % 16 == 4 and c[2].conv.data_ptr() % 16 == 4
    same(a, c, "4-byte aligned buffers")


# ------------------------------------------------------------------------------------------------ 4. A = 1 through the accumulator
def test_accumulate_1_equals_clip_then_step():
    from givepose_amd import GradAccumulator, Ranger, clip_grad_norm_
    nets = [CaseNet(R.case_params("seeded")) for _ in range(2)]
    through, apart = (Ranger(n, lr=LR) for n in nets)
    acc = GradAccumulator(through)
    for step in (1, 2, 3):
        acc.add(grads_cuda(step), 1.0, R.CLIP)
        through.step(acc.grads)
        acc.zero()
        g = grads_cuda(step)
        clip_grad_norm_(g, R.CLIP)
        apart.step(g)
        same_states(device_state(through, nets[0]), device_state(apart, nets[1]), f"step {step}")
    assert through.steps == apart.steps and through.steps[through._index["skip"]] == 2


# ------------------------------------------------------------------------------------------------ 5. two ranks, 6. one rank on RCCL
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(world, backend, grads_of_rank, accumulate):
    """`world` fresh processes of optim.rank_accum_selfcheck from the fork server.  -> {rank: (parameters, exp_avg, scalars)}."""
    from givepose_amd.optim import rank_accum_selfcheck
    ctx = mp.get_context("forkserver")        # server started in conftest.pytest_configure, before any GPU call
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=rank_accum_selfcheck, args=(r, world, port, q, backend, R.case_params("seeded"), grads_of_rank(r), accumulate, R.CLIP, LR))
          for r in range(world)]
    [p.start() for p in ps]
    res = {}
    try:
        for _ in ps:
            rank, status, p, m, scalars = q.get(timeout=240)
            assert status == "ok", (rank, status)
            res[rank] = (p, m, scalars)
    finally:
        [p.join(30) for p in ps]
        [p.kill() for p in ps if p.is_alive()]
    return res


def one_rank(grads_per_micro_step, accumulate):
    """The same micro-steps in this process without a group.  -> (parameters, exp_avg, scalars) as numpy arrays."""
    from givepose_amd import GradAccumulator, Ranger
    net = CaseNet(R.case_params("seeded"))
    opt = Ranger(net, lr=LR)
    acc = GradAccumulator(opt)
    for i, g in enumerate(grads_per_micro_step):
        acc.add({n: T(a).cuda() for n, a in g.items()}, scale=1.0 / accumulate, clip_norm=R.CLIP)
        if i % accumulate == 0:
            opt.step(acc.grads, clip_norm=None, lr=LR)
            acc.zero()
    return ({n: getattr(net, n).detach().cpu().numpy() for n in R.SHAPES}, {n: opt._view("exp_avg", opt._index[n]).cpu().numpy() for n in R.SHAPES},
            acc.scalars.cpu().numpy())


def same_arrays(a, b, what):
    for x, y, part in zip(a, b, ("p", "exp_avg")):
        assert list(x) == list(y), (what, part)
        for n in x:
            assert np.array_equal(x[n].view(np.int32), y[n].view(np.int32)), (what, part, n)
    assert np.array_equal(np.asarray(a[2], np.float32).view(np.int32), np.asarray(b[2], np.float32).view(np.int32)), (what, "scalars")


@pytest.mark.timeout(300)
def test_two_ranks_with_identical_gradients_equal_one_rank():
    """world = 2, both ranks fed case_grads(1..4) with A = 2: 0.5 g + 0.5 g is exact and the chunking is that of the one-rank path, so
    every returned array has the bits of the run without a group.  `skip` is live without a gradient at micro-step 2."""
    grads = [R.case_grads(i + 1) for i in range(4)]
    res = run_ranks(2, "gloo", lambda r: grads, 2)
    alone = one_rank(grads, 2)
    for r in range(2):
        same_arrays(res[r], alone, f"rank {r}")
    assert not np.array_equal(alone[0]["conv"], R.case_params("seeded")["conv"])


def rank_grads(r):
    """Rank r's gradients of micro-steps 0..2: case_grads(2 i + r + 1).  Every rank must pass the same names (GradAccumulator.add), and
    case_grads(3) has no `skip` where case_grads(4) has one: rank 0 contributes a gradient of zeros there, which is what DDP contributes
    for a parameter that a rank's loss did not reach."""
    out = [dict(R.case_grads(2 * i + r + 1)) for i in range(3)]
    for g in out:
        g.setdefault("skip", np.zeros(R.SHAPES["skip"], np.float32))
    return out


@pytest.mark.timeout(300)
def test_two_ranks_with_different_gradients():
    res = run_ranks(2, "gloo", rank_grads, 2)
    same_arrays(res[0], res[1], "rank 0 against rank 1")
    per_step = [[rank_grads(0)[i], rank_grads(1)[i]] for i in range(3)]
    assert not np.array_equal(per_step[0][0]["conv"], per_step[0][1]["conv"])
    refs = [A.loop_ref(R.case_params("seeded"), per_step, 2, R.CLIP, LR, dt) for dt in (torch.float64, torch.float32)]
    (o64, a64), (o32, a32) = refs
    worst = rule({n: T(res[0][0][n]) for n in R.SHAPES}, o64.p, o32.p, "two ranks p")
    worst = max(worst, rule({n: T(res[0][1][n]) for n in R.SHAPES}, {n: o64.state[n]["exp_avg"] for n in R.SHAPES},
                            {n: o32.state[n]["exp_avg"] for n in R.SHAPES}, "two ranks exp_avg"))
    worst = max(worst, rule({"norm": np.float64(res[0][2][0])}, {"norm": a64.norm.numpy()}, {"norm": a32.norm.numpy()}, "two ranks"))
    print(f"two ranks: largest device / CPU float32 ratio {worst:.2f}")


@pytest.mark.timeout(300)
def test_one_rank_on_rccl_equals_no_group():
    """The worker with backend "nccl" and world 1 (the one-rank communicator of dist.init_from_env(force=True), as
    tests/test_rccl_single_rank.py): stage goes through RCCL's all_reduce on this code's stream and comes back as it was, so the results
    have the bits of the run without a group.  Multi-GPU RCCL behaviour stays unmeasured here."""
    grads = [R.case_grads(i + 1) for i in range(4)]
    res = run_ranks(1, "nccl", lambda r: grads, 2)
    same_arrays(res[0], one_rank(grads, 2), "one rank on RCCL")


# ------------------------------------------------------------------------------------------------ 7. PoseNet.train_step
def train_setup():
    import bb_backward_ref as B
    from givepose_amd import GradAccumulator, PoseNet, PoseNetConfig, Ranger
    from test_xyz_backward_gpu import loss_batch
    cfg = PoseNetConfig(convnext_depths=(1, 1, 1, 1))
    net = PoseNet(cfg, dtype=torch.float32, seed=B.WEIGHT_SEED).cuda()
    data = {k: v[:2] if v.dim() and v.shape[0] == 4 else v for k, v in loss_batch().items()}
    opt = Ranger(net)
    return cfg, net, data, {**data, "roi_mask": data["roi_mask_deform"]}, opt, GradAccumulator(opt)


def tensors(out):
    return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}


def params_of(net, opt):
    sd = net.state_dict()
    return {n: sd[n].detach().clone() for n in opt.param_names}


def test_train_step_accumulates():
    """A = 2 over micro-steps 0, 1, 2 at B = 2: steps at 0 and 2, none at 1."""
    from givepose_amd import PoseLoss, PoseNet
    from test_xyz_backward_gpu import same_bits
    cfg, net, data, fdata, opt, acc = train_setup()
    pl = PoseLoss()
    start = params_of(net, opt)
    got, grads = [], []
    for i in range(3):
        if i == 1:
            fwd_before = tensors(net.forward_device(fdata, "cuda"))
        res = net.train_step(data, pl, opt, "cuda", accumulator=acc, accumulate=2, micro_step=i)
        assert res["stepped"] == (i != 1) and (set(acc.live) >= set(res["param_grads"]) if i == 1 else acc.live == [])
        grads.append({n: res["param_grads"][n].detach().clone().cpu() for n in opt.param_names if n in res["param_grads"]})
        got.append(params_of(net, opt))
        if i == 1:                   # no parameter moved, and the forward is the forward before it
            assert all(torch.equal(bits(got[1][n]), bits(got[0][n])) for n in opt.param_names)
            same_bits(tensors(net.forward_device(fdata, "cuda")), fwd_before, "forward after the micro-step without a step")
            assert 0 < float(acc.scalars[0])
    names = list(grads[0])
    assert names == list(grads[1]) == list(grads[2]) and len(names) < len(opt.param_names)
    assert any(not torch.equal(got[0][n], start[n]) for n in names)
    refs = []
    for dt in (torch.float64, torch.float32):
        kept = []
        A.loop_ref({n: start[n].cpu() for n in names}, grads, 2, 5.0, opt.lr, dt, on_micro_step=lambda i, a, o, s: kept.append(dict(o.p)))
        refs.append(kept)
    worst = rule({n: got[0][n] for n in names}, refs[0][0], refs[1][0], "train_step micro-step 0")
    worst = max(worst, rule({n: got[2][n] for n in names}, refs[0][2], refs[1][2], "train_step micro-step 2"))
    print(f"train_step with A = 2: largest device / CPU float32 ratio over the {len(names)} updated tensors {worst:.2f}")
    assert opt.steps[opt._index[names[0]]] == 2
    fwd_after = tensors(net.forward_device(fdata, "cuda"))
    assert any(not torch.equal(fwd_before[k], fwd_after[k]) for k in fwd_before)
    fresh = PoseNet(cfg, dtype=torch.float32).cuda()
    fresh.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    same_bits(tensors(fresh.forward_device(fdata, "cuda")), fwd_after, "forward after the step")


def test_train_step_accumulates_with_the_size_head():
    from givepose_amd import PoseLoss
    cfg, net, data, fdata, opt, acc = train_setup()
    pl = PoseLoss()
    before, mean0 = params_of(net, opt), net.state_dict()["size_head.bn1.running_mean"].clone()
    res = net.train_step(data, pl, opt, "cuda", accumulator=acc, accumulate=2, micro_step=1, size_head={"seed": 11})
    assert res["stepped"] is False and any(n.startswith("size_head.") for n in acc.live)
    mean1 = net.state_dict()["size_head.bn1.running_mean"].clone()
    assert not torch.equal(mean1, mean0)                          # the running statistics move on every micro-step
    after = params_of(net, opt)
    assert all(torch.equal(bits(after[n]), bits(before[n])) for n in before) and sum(opt.steps) == 0
    res = net.train_step(data, pl, opt, "cuda", accumulator=acc, accumulate=2, micro_step=2, size_head={"seed": 12})
    assert res["stepped"] is True and acc.live == []
    assert not torch.equal(net.state_dict()["size_head.bn1.running_mean"], mean1)
    state = opt.state_dict()["state"]
    size = [n for n in opt.param_names if n.startswith("size_head.")]
    assert len(size) == 6 and all(opt._index[n] in state and state[opt._index[n]]["step"] == 1 for n in size)
    moved = params_of(net, opt)
    # (conv1.bias feeds a BatchNorm on batch statistics: its gradient is 0 up to rounding, so not every one of the six has to move)
    assert any(not torch.equal(moved[n], before[n]) for n in size) and not torch.equal(moved["size_head.conv2.bias"], before["size_head.conv2.bias"])


def test_train_step_without_the_keywords_is_the_parent_body():
    """train_step without the new keywords against its body before them, inlined on a twin net: head_grads_backbone, then the fused
    clip + step.  The map encoder's d xp scatter adds with atomics (csrc/encgrad.hip), so two runs of the backward chain need not give
    equal bits: the twin's chain is run and must return the same names, and its step is then fed the gradients that train_step
    returned (it leaves them as computed), which makes every bit of the two updates comparable."""
    from givepose_amd import PoseLoss
    pl = PoseLoss()
    _, net_a, data, _, opt_a, _ = train_setup()
    _, net_b, _, _, opt_b, _ = train_setup()
    a, b = params_of(net_a, opt_a), params_of(net_b, opt_b)
    assert all(torch.equal(bits(a[n]), bits(b[n])) for n in a)          # twins
    res_a = net_a.train_step(data, pl, opt_a, "cuda")
    res_b = net_b.head_grads_backbone(data, pl, "cuda", groups=None)
    assert "stepped" not in res_a and list(res_a) == list(res_b) and list(res_a["param_grads"]) == list(res_b["param_grads"])
    opt_b.step({n: g.clone() for n, g in res_a["param_grads"].items()}, clip_norm=5.0, lr=None)
    assert torch.equal(bits(opt_a.scalars), bits(opt_b.scalars)) and opt_a.steps == opt_b.steps and sum(opt_a.steps) > 0
    a, b = params_of(net_a, opt_a), params_of(net_b, opt_b)
    assert all(torch.equal(bits(a[n]), bits(b[n])) for n in a)
    for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
        assert torch.equal(bits(opt_a._flat[key]), bits(opt_b._flat[key])), key
