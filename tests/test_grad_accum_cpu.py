"""CPU: the gradient-accumulation family (include/givepose_accum.h, gpc_*; givepose_amd.optim.GradAccumulator; the accumulator keywords of
PoseNet.train_step) -- the model of the reference's loop in tests/grad_accum_ref.py against that loop run literally on a torch.nn module
in float64, the family's registration, its size queries, and the accumulator's bookkeeping built on the host.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import grad_accum_ref as A
import ranger_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


# ------------------------------------------------------------------------------------------------ the model of the loop
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b, self.side = torch.nn.Linear(4, 3), torch.nn.Linear(3, 2), torch.nn.Linear(4, 2)

    def forward(self, x, use_side):
        y = self.b(torch.tanh(self.a(x)))
        return y + self.side(x) if use_side else y


class _SgdRef:
    """torch.optim.SGD(momentum) in the interface loop_ref asks of an optimiser: a parameter without a gradient is skipped."""

    def __init__(self, params, momentum):
        self.p, self.buf, self.momentum = {n: t.clone() for n, t in params.items()}, {}, momentum

    def step(self, grads, lr):
        for n, g in grads.items():
            self.buf[n] = g.clone() if n not in self.buf else self.momentum * self.buf[n] + g
            self.p[n] = self.p[n] - lr * self.buf[n]


def test_accum_ref_is_the_reference_loop():
    """engine/train.py:117-131 literally -- loss / A, backward(), clip_grad_norm_ on every micro-step, step and zero_grad on
    global_step % A == 0 -- for A = 3 over micro-steps 0..6 in float64.  `side` is not reached by the loss on micro-step 2, where it has
    an accumulated gradient (it is still counted and scaled), and on micro-step 4, the first of its window, where it has none.  The
    scale of the inputs makes both clip branches happen."""
    accumulate, clip, lr, momentum, steps = 3, 5.0, 0.05, 0.9, 7
    torch.manual_seed(7)
    net = _Net().double()
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    opt = torch.optim.SGD(net.parameters(), lr=lr, momentum=momentum)
    opt.zero_grad()
    xs = [torch.randn(5, 4, dtype=torch.float64) * (40.0 if i % 2 else 0.5) for i in range(steps)]
    unused = {2, 4}
    micro_grads, seen, coefs = [], [], []
    acc = A.AccumRef()
    for global_step in range(steps):
        use_side = global_step not in unused
        # this micro-step's own gradient, unscaled: what a backward chain that accumulates nothing returns
        loss = net(xs[global_step], use_side).square().sum()
        names = [n for n, _ in net.named_parameters() if use_side or not n.startswith("side.")]
        g = dict(zip(names, torch.autograd.grad(loss, [p for n, p in net.named_parameters() if n in names])))
        micro_grads.append({n: t.clone() for n, t in g.items()})
        acc.add(g, 1.0 / accumulate, clip)
        coefs.append(float(acc.coef))
        # the loop
        total_loss = net(xs[global_step], use_side).square().sum()
        total_loss = total_loss / accumulate
        total_loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), clip)
        have = {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
        assert set(have) == set(acc.acc), global_step
        for n, want in have.items():
            assert float((acc.acc[n] - want).abs().max()) <= TOL * float(want.abs().max()), (global_step, n)
        seen.append(set(have))
        if global_step % accumulate == 0:
            opt.step()
            opt.zero_grad()
            acc.zero()
    assert "side.weight" in seen[2] and "side.weight" not in seen[4] and "side.weight" in seen[5]
    assert any(c == 1.0 for c in coefs) and any(c < 0.5 for c in coefs)
    ref, _ = A.loop_ref(start, micro_grads, accumulate, clip, lr, torch.float64, optimizer=lambda p: _SgdRef(p, momentum))
    for n, p in net.named_parameters():
        assert float((ref.p[n] - p.detach()).abs().max()) <= TOL * float(p.detach().abs().max()), n
        assert not torch.equal(p.detach(), start[n])


def test_loop_ref_with_one_rank_list_equals_the_dict_form():
    grads = [R.case_grads(s) for s in (1, 2, 3)]
    a, _ = A.loop_ref(R.case_params("seeded"), grads, 2, R.CLIP, 1e-3, torch.float64)
    b, _ = A.loop_ref(R.case_params("seeded"), [[g, g] for g in grads], 2, R.CLIP, 1e-3, torch.float64)
    for n in R.SHAPES:
        assert torch.equal(a.p[n], b.p[n]), n


# ------------------------------------------------------------------------------------------------ header, prototypes, exports
def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build
    hdr = _header("givepose_accum.h")
    declared = set(re.findall(r"\b(gpc_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.ACCUM_PROTOTYPES) and len(declared) == 2
    for other in (_lib.PROTOTYPES, _lib.ALIGN_PROTOTYPES, _lib.LOSS_PROTOTYPES, _lib.HEADGRAD_PROTOTYPES, _lib.GRAD_PROTOTYPES,
                  _lib.XYZGRAD_PROTOTYPES, _lib.ENCGRAD_PROTOTYPES, _lib.BBGRAD_PROTOTYPES, _lib.OPTIM_PROTOTYPES, _lib.SIZEGRAD_PROTOTYPES):
        assert not set(_lib.ACCUM_PROTOTYPES) & set(other)
        assert not any(name.startswith("gpc_") for name in other)
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gpc_[a-z0-9_]+)", out)) == declared
    assert "accum.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "givepose_amd", "csrc", "accum.hip")).read()
    shared = open(os.path.join(ROOT, "givepose_amd", "csrc", "flat_tensors.hpp")).read()
    assert '#include "flat_tensors.hpp"' in src and not re.search(r"\batomic\w*\s*\(", src + shared, flags=re.I)                    # no atomic in the family
    entry = src.split("int gpc_grad_accumulate(")[1].split('}  // extern "C"')[0]
    assert len(re.findall(r"hipLaunchKernelGGL", entry)) == _lib.GPC_ACCUM_LAUNCHES == 3
    consts = {k: int(v) for k, v in re.findall(r"#define (GPC_[A-Z_]+) (\d+)", hdr)}
    assert consts == {"GPC_ACCUM_LAUNCHES": _lib.GPC_ACCUM_LAUNCHES, "GPC_FLAG_OVERWRITE": _lib.GPC_FLAG_OVERWRITE}
    assert not _lib.GPC_FLAG_OVERWRITE & (_lib.GPO_FLAG_RECTIFIED | _lib.GPO_FLAG_LOOKAHEAD)


def test_size_queries_answer_on_the_host():
    from givepose_amd import _lib, optim
    lib = _lib.load()
    tab = np.zeros(3, optim._TENSOR)
    tab["p"], tab["g"] = 4096, [8192, 0, 8192]
    tab["n"] = [10, 2 * 4099, 5]
    tab["flags"] = [_lib.GPC_FLAG_OVERWRITE, 0, 0]                # a null g without OVERWRITE: a live tensor that is only normed
    # chunks: 1 + 3 + 1.  Tables 3 x 24 + 5 x 16 bytes, then the chunks' sums of squares and the scalars, each rounded up to 256 bytes
    assert lib.gpc_grad_accumulate_workspace(optim._table_ptr(tab), 3) == 256 + 256 + 256
    assert lib.gpc_grad_accumulate_workspace(optim._table_ptr(tab), 0) == 0 and lib.gpc_grad_accumulate_workspace(None, 3) == 0
    for field, value in (("n", 0), ("n", -3), ("p", 0), ("p", 4098), ("g", 8194), ("flags", _lib.GPC_FLAG_OVERWRITE), ("flags", 1)):
        bad = tab.copy()
        bad[field][1] = value
        assert lib.gpc_grad_accumulate_workspace(optim._table_ptr(bad), 3) == 0, (field, value)
        assert b"tensor 1" in lib.gp_last_error()
    # the entry point refuses what the query refuses, before it touches the device
    bad = tab.copy()
    bad["flags"][1] = _lib.GPC_FLAG_OVERWRITE
    assert lib.gpc_grad_accumulate(optim._table_ptr(bad), 3, 1.0, 5.0, None, None, 0, None) < 0
    assert b"GPC_FLAG_OVERWRITE without a gradient" in lib.gp_last_error()
    assert lib.gpc_grad_accumulate(optim._table_ptr(tab), 3, float("nan"), 5.0, None, None, 0, None) < 0
    assert lib.gpc_grad_accumulate(optim._table_ptr(tab), 3, 1.0, 5.0, None, None, 0, None) < 0 and b"workspace" in lib.gp_last_error()


# ------------------------------------------------------------------------------------------------ GradAccumulator on the host
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 3)
        self.norm = torch.nn.GroupNorm(2, 4)
        self.gn = torch.nn.GroupNorm(2, 4)
        self.gn.weight, self.gn.bias = self.norm.weight, self.norm.bias          # one Parameter under two names
        self.fc = torch.nn.Linear(4, 2)


def _host_ranger():
    from givepose_amd.optim import Ranger

    class HostRanger(Ranger):        # the table and the layout on the host; the launches themselves need the device
        _require_device = False
    return HostRanger


def test_accumulator_layout_and_aliases():
    import givepose_amd
    from givepose_amd.optim import GradAccumulator
    assert givepose_amd.GradAccumulator is GradAccumulator
    net = _Tiny()
    opt = _host_ranger()(net)
    acc = GradAccumulator(opt)
    assert acc.optimizer is opt and acc._offsets is opt._offsets and acc.flat.numel() == int(opt._offsets[-1]) and not acc.flat.any()
    assert acc.flat.dtype == torch.float32 and acc.scalars.shape == (2,) and acc.stage is None
    assert (acc._static["p"] == acc.flat.data_ptr() + 4 * opt._offsets[:-1]).all() and (acc._static["n"] == [p.numel() for p in opt.params]).all()
    assert acc.live == [] and acc.grads == {}
    acc._live = {2, 4}
    assert acc.live == ["norm.weight", "gn.weight", "fc.weight"]
    g = acc.grads
    assert list(g) == acc.live and g["gn.weight"].data_ptr() == g["norm.weight"].data_ptr() == acc.flat.data_ptr() + 4 * int(opt._offsets[2])
    assert g["fc.weight"].shape == net.fc.weight.shape and g["fc.weight"].is_contiguous()
    assert sorted(opt._collect(g)) == [2, 4]                     # what Ranger.step makes of them: one entry per parameter
    acc.zero()
    assert acc.live == [] and acc.grads == {}
    with pytest.raises(ValueError, match="Ranger is expected"):
        GradAccumulator(torch.optim.SGD(net.parameters(), lr=0.1))


def test_accumulator_live_and_overwrite_bookkeeping():
    """The tables of a window of the seeded cases, built on the host: `skip` has no gradient at case_grads(3)."""
    from givepose_amd import _lib
    from givepose_amd.optim import GradAccumulator
    net = torch.nn.Module()
    for n, a in R.case_params("seeded").items():
        net.register_parameter(n, torch.nn.Parameter(torch.from_numpy(a), requires_grad=False))
    opt = _host_ranger()(net)
    acc = GradAccumulator(opt)
    skip = opt._index["skip"]
    T = lambda step: {n: torch.from_numpy(a) for n, a in R.case_grads(step).items()}
    g2 = T(2)
    entries, tab, grads = acc._table(g2)
    assert entries == list(range(len(R.SHAPES))) and (tab["flags"] == _lib.GPC_FLAG_OVERWRITE).all()          # nothing is live: all overwritten
    assert tab["g"].tolist() == [g2[n].data_ptr() for n in R.SHAPES] and (tab["p"] == acc._static["p"]).all()
    assert acc.live == []                                        # building a table changes nothing
    acc._live.update(grads)
    g3 = T(3)
    entries, tab, grads = acc._table(g3)
    assert skip not in grads and entries == list(range(len(R.SHAPES)))            # live but absent: in the table with a null g
    assert tab["g"][skip] == 0 and (tab["flags"] == 0).all() and (np.delete(tab["g"], skip) != 0).all()
    acc.zero()
    entries, tab, grads = acc._table(g3)
    assert skip not in entries and len(entries) == len(R.SHAPES) - 1 and (tab["flags"] == _lib.GPC_FLAG_OVERWRITE).all()
    acc._live.update(grads)
    entries, tab, grads = acc._table(T(4))                        # skip joins a window the others already belong to
    assert tab["flags"].tolist() == [_lib.GPC_FLAG_OVERWRITE if i == skip else 0 for i in entries]
    assert _lib.load().gpc_grad_accumulate_workspace(__import__("givepose_amd").optim._table_ptr(tab), len(tab)) > 0


def test_accumulator_refusals_change_nothing():
    from givepose_amd.optim import GradAccumulator
    net = _Tiny()
    opt = _host_ranger()(net)
    acc = GradAccumulator(opt)
    ones = {n: torch.ones_like(p) for n, p in net.named_parameters(remove_duplicate=False)}
    for bad, match in (({"fc.weight": torch.ones(2, 4).t()}, "fc.weight.*expected contiguous float32 \\(2, 4\\)"),
                       ({"fc.weight": torch.ones(2, 4, dtype=torch.float16)}, "fc.weight.*float16"),
                       ({"fc.weight": torch.ones(4, 2).t()}, "fc.weight.*not contiguous"), ({"nope": torch.ones(1)}, "no parameter of that name"),
                       ({**ones, "gn.weight": 2 * ones["norm.weight"]}, "gn.weight.*norm.weight.*different gradients")):
        with pytest.raises(ValueError, match=match):
            acc.add(bad)
    with pytest.raises(ValueError, match="clip_norm"):
        acc.add(ones, clip_norm=0)
    with pytest.raises(ValueError, match="scale"):
        acc.add(ones, scale=float("inf"))
    assert acc.live == [] and not acc.flat.any() and acc.stage is None and acc._ws is None
    acc.add({})                                                   # nothing live and nothing given: nothing to do


def test_train_step_keyword_refusals():
    from givepose_amd import GradAccumulator, PoseNet, PoseNetConfig
    net = PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1)), dtype=torch.float32)
    opt = _host_ranger()(net)
    for kw in (dict(accumulate=2), dict(micro_step=1), dict(group=object())):
        with pytest.raises(ValueError, match="need accumulator"):
            net.train_step({}, None, opt, "cuda", **kw)
    other = _host_ranger()(net)
    with pytest.raises(ValueError, match="built over this optimizer"):
        net.train_step({}, None, opt, "cuda", accumulator=GradAccumulator(other))
    acc = GradAccumulator(opt)
    for kw in (dict(accumulate=0), dict(accumulate=1.5), dict(micro_step=-1)):
        with pytest.raises(ValueError, match="accumulate .* micro_step"):
            net.train_step({}, None, opt, "cuda", accumulator=acc, **kw)
    twin = PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1)), dtype=torch.float32)
    with pytest.raises(ValueError, match="built over this model"):
        twin.train_step({}, None, opt, "cuda", accumulator=acc)
