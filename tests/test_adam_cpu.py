"""CPU: Adam and AdamW (include/givepose_adam.h, gpad_*; givepose_amd/optim.py) -- the family's registration, the host scalars, the
state-dict exchange with torch.optim.Adam / AdamW in both directions, the refusals, build_optimizer, and the numpy float32 restatement
tests/adam_ref.py (what tests/test_adam_gpu.py asks the device to reproduce bit for bit) against torch itself.

The restatement's rule is DESIGN.md 1e's: on the cases of tests/ranger_ref.py plus two chunk-sized tensors, after torch.nn.utils.
clip_grad_norm_(., 5), per tensor and state and after every one of 13 steps, max|got - ref64| / max|ref64| is at most 8 times the figure
of torch's own float32 CPU run on the same inputs, which counts as at least 2^-24; ref64 is torch.optim.Adam / AdamW (foreach=False) on
float64 parameters.  Largest ratio (seeded / zero run): adam 2.45 / 2.83, adamw 2.45 / 2.45, adam_wd 1.94 / 2.60, adamw_ams 2.45 / 2.45.
"""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import adam_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _table(n=3):
    from givepose_amd import optim
    tab = np.zeros(n, optim._ADAM_TENSOR)
    for f in ("p", "g", "m", "v", "vmax"):
        tab[f] = 4096
    tab["n"], tab["step_size"], tab["bc2_sqrt"], tab["decay"] = [10, 2 * 4096 + 1, 5][:n], 1e-3, 0.5, 1.0
    return tab


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build, optim
    hdr = _header("givepose_adam.h")
    declared = set(re.findall(r"\b(gpad_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.ADAM_PROTOTYPES) and len(declared) == 2
    for other in (_lib.PROTOTYPES, _lib.OPTIM_PROTOTYPES, _lib.ACCUM_PROTOTYPES, _lib.REPACK_PROTOTYPES, _lib.SIZEGRAD_PROTOTYPES, _lib.BBGRAD_PROTOTYPES):
        assert not set(_lib.ADAM_PROTOTYPES) & set(other)
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gpad_[a-z0-9_]+)", out)) == declared
    assert "adam.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "givepose_amd", "csrc", "adam.hip")).read()
    shared = open(os.path.join(ROOT, "givepose_amd", "csrc", "flat_tensors.hpp")).read()          # the family's other half
    assert '#include "flat_tensors.hpp"' in src
    assert not re.search(r"\batomic\w*\s*\(", src + shared)                    # no atomic in the family
    body = src.split("int gpad_adam_step(")[1]
    assert len(re.findall(r"hipLaunchKernelGGL", body)) == _lib.GPAD_STEP_LAUNCHES == 3
    for text in (src, shared):
        assert "hipMalloc" not in text and "Synchronize" not in text and "DeviceToHost" not in text
    # one copy per step: none in adam.hip, one in the header, inside send_tables, which the step calls once
    assert src.count("hipMemcpyAsync") == 0 and shared.count("hipMemcpyAsync") == 1
    assert shared.split("int send_tables(")[1].split("\n}\n")[0].count("hipMemcpyAsync(") == 1
    assert len(re.findall(r"\bsend_tables\s*\(", body)) == 1 and len(re.findall(r"\bsend_tables\s*\(", src)) == 1
    consts = {k: int(v) for k, v in re.findall(r"#define (GPAD_[A-Z_]+) (\d+)", hdr)}
    assert consts == {"GPAD_STEP_LAUNCHES": _lib.GPAD_STEP_LAUNCHES, "GPAD_MAX_TENSORS": _lib.GPAD_MAX_TENSORS, "GPAD_MODE_ADAM": _lib.GPAD_MODE_ADAM,
                      "GPAD_MODE_ADAMW": _lib.GPAD_MODE_ADAMW}
    assert A.CHUNK == _lib.GPO_CHUNK and '#include "givepose_optim.h"' in hdr          # the chunk is the optimiser family's
    assert ctypes.sizeof(_lib.AdamTensor) == optim._ADAM_TENSOR.itemsize == 64 and ctypes.sizeof(_lib.AdamHyper) == 48
    for f, _ in _lib.AdamTensor._fields_:
        assert getattr(_lib.AdamTensor, f).offset == optim._ADAM_TENSOR.fields[f][1], f


def test_the_size_query_answers_on_the_host_and_refuses_by_name():
    from givepose_amd import _lib, optim
    lib = _lib.load()
    hyper = lambda **kw: ctypes.byref(_lib.AdamHyper(**{**dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=5.0, mode=0, amsgrad=1), **kw}))
    tab = _table()
    ptr = optim._adam_table_ptr(tab)
    # chunks 1 + 3 + 1; tables 3 x 64 + 5 x 16 bytes, then the chunks' sums of squares and the scalars, each rounded up to 256 bytes
    assert lib.gpad_adam_step_workspace(ptr, 3, hyper()) == 512 + 256 + 256
    assert lib.gpad_adam_step_workspace(ptr, 0, hyper()) == 0 and lib.gpad_adam_step_workspace(None, 3, hyper()) == 0
    assert lib.gpad_adam_step_workspace(ptr, 3, None) == 0 and b"null hyper" in lib.gp_last_error()
    for field, value in (("n", 0), ("g", 0), ("g", 4098), ("p", 0), ("m", 2), ("v", 0), ("vmax", 0), ("bc2_sqrt", 0.0), ("step_size", np.nan)):
        bad = tab.copy()
        bad[field][1] = value
        assert lib.gpad_adam_step_workspace(optim._adam_table_ptr(bad), 3, hyper()) == 0, (field, value)
        assert b"tensor 1" in lib.gp_last_error(), (field, value)
    bad = tab.copy()
    bad["vmax"] = 0                                # vmax is read under amsgrad only
    assert lib.gpad_adam_step_workspace(optim._adam_table_ptr(bad), 3, hyper(amsgrad=0)) > 0
    for kw, match in ((dict(beta1=1.0), b"betas"), (dict(beta2=-0.1), b"betas"), (dict(eps=-1.0), b"eps"), (dict(weight_decay=-1.0), b"weight_decay"),
                      (dict(mode=2), b"mode 2"), (dict(amsgrad=2), b"amsgrad 2")):
        assert lib.gpad_adam_step_workspace(ptr, 3, hyper(**kw)) == 0 and match in lib.gp_last_error(), kw
    # the entry point refuses the same tables before anything is sent to a device
    sc = hyper(amsgrad=3)
    assert lib.gpad_adam_step(ptr, 3, sc, None, None, 0, None) != 0 and b"gpad_adam_step: amsgrad 3" in lib.gp_last_error()
    assert lib.gpad_adam_step(ptr, 3, hyper(), None, None, 0, None) != 0 and b"workspace of 1024 bytes" in lib.gp_last_error()


def test_host_scalars_are_torchs_python_float_expressions():
    from givepose_amd.optim import adam_step_scalars
    for lr, b1, b2, wd in ((1e-3, 0.9, 0.999, 0.0), (0.1, 0.9, 0.999, 1e-2), (3e-4, 0.8, 0.99, 0.1)):
        for step in range(1, A.STEPS + 1):
            step_f = float(step)                   # torch: step = _get_value(step_t), a Python float
            want = (lr / (1 - b1 ** step_f), (1 - b2 ** step_f) ** 0.5, 1 - lr * wd)
            assert adam_step_scalars(step, lr, b1, b2, wd) == want == A.step_scalars(step, lr, b1, b2, wd), (lr, step)


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 3)
        self.norm = torch.nn.GroupNorm(2, 4)
        self.gn = torch.nn.GroupNorm(2, 4)
        self.gn.weight, self.gn.bias = self.norm.weight, self.norm.bias          # one Parameter under two names
        self.fc = torch.nn.Linear(4, 2)


def _host(cls):
    """The class with the table and the layout on the host; the step itself needs the device."""
    return type("Host" + cls.__name__, (cls,), {"_require_device": False})


def _torch_steps(opt, params, seed, steps, skip=None):
    r = np.random.default_rng(seed)
    for _ in range(steps):
        for i, p in enumerate(params):
            g = T(r.standard_normal(tuple(p.shape)).astype(np.float32))
            p.grad = None if i == skip else g
        opt.step()


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_state_dict_round_trips_with_torch_in_both_directions(name, amsgrad):
    import givepose_amd
    ours_cls, torch_cls = _host(getattr(givepose_amd, name)), getattr(torch.optim, name)
    torch.manual_seed(3)
    net = _Tiny()
    names = [n for n, _ in net.named_parameters()]
    opt = ours_cls(net, lr=2e-3, amsgrad=amsgrad)
    assert opt.param_names == names == ["conv.weight", "conv.bias", "norm.weight", "norm.bias", "fc.weight", "fc.bias"]
    assert opt._index["gn.weight"] == opt._index["norm.weight"] == 2 and len(opt._index) == 8 and all(o % 64 == 0 for o in opt._offsets)
    assert all(a is b for a, b in zip(opt.params, net.parameters())) and opt.steps == [0] * 6 and opt.model is net
    fresh, torch_fresh = opt.state_dict(), torch_cls(net.parameters(), lr=2e-3, amsgrad=amsgrad).state_dict()
    assert fresh["state"] == {} and set(fresh["param_groups"][0]) == set(torch_fresh["param_groups"][0]) | {"param_names"}
    for k, v in torch_fresh["param_groups"][0].items():          # torch's keys with torch's values
        assert fresh["param_groups"][0][k] == v, k
    # torch -> ours: three steps of torch's optimiser, the last parameter without a gradient
    tnet = _Tiny()
    tnet.load_state_dict(net.state_dict())
    saved_from = torch_cls(tnet.parameters(), lr=5e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.03, amsgrad=amsgrad)
    _torch_steps(saved_from, list(tnet.parameters()), 11, 3, skip=5)
    buf = io.BytesIO()
    torch.save(saved_from.state_dict(), buf)
    buf.seek(0)
    opt.load_state_dict(torch.load(buf))
    assert opt.steps == [3, 3, 3, 3, 3, 0] and (opt.lr, opt.betas, opt.eps, opt.weight_decay) == (5e-4, (0.8, 0.99), 1e-6, 0.03)
    keys = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ())
    for i, p in enumerate(tnet.parameters()):
        for key in keys:
            assert torch.equal(opt._view(key, i), saved_from.state[p][key] if i < 5 else torch.zeros_like(p)), (i, key)
    as_int = saved_from.state_dict()               # (its state entries are the optimiser's own dicts: build new ones)
    as_int = {**as_int, "state": {i: {**s, "step": int(s["step"])} for i, s in as_int["state"].items()}}       # the layout of torch < 1.12
    opt.load_state_dict(as_int)
    assert opt.steps == [3, 3, 3, 3, 3, 0]
    # ours -> torch: the dict we save has torch's layout, loads into torch's class, and that optimiser continues exactly as the one the
    # state came from
    sd = opt.state_dict()
    want = saved_from.state_dict()
    assert sorted(sd["state"]) == sorted(want["state"]) == [0, 1, 2, 3, 4]
    for i, s in sd["state"].items():
        assert set(s) == set(want["state"][i]) == {"step", *keys}
        assert torch.is_tensor(s["step"]) and s["step"].dtype == torch.float32 and s["step"].dim() == 0 and torch.equal(s["step"], want["state"][i]["step"])
        assert all(torch.equal(s[key], want["state"][i][key]) and s[key].shape == want["state"][i][key].shape for key in keys)
    assert {k: v for k, v in sd["param_groups"][0].items() if k != "param_names"} == want["param_groups"][0]
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    cnet = _Tiny()
    cnet.load_state_dict(tnet.state_dict())
    cont = torch_cls(cnet.parameters(), amsgrad=amsgrad)
    cont.load_state_dict(torch.load(buf))
    _torch_steps(saved_from, list(tnet.parameters()), 12, 2)
    _torch_steps(cont, list(cnet.parameters()), 12, 2)
    for a, b in zip(tnet.parameters(), cnet.parameters()):
        assert torch.equal(a, b)
    assert [int(cont.state[p]["step"]) for p in cnet.parameters()] == [5, 5, 5, 5, 5, 2]
    # and ours -> ours
    new = ours_cls(net, amsgrad=amsgrad)
    new.load_state_dict(sd)
    assert new.steps == opt.steps and new.lr == 5e-4 and all(torch.equal(new._flat[k], opt._flat[k]) for k in keys)
    renamed = {**sd, "param_groups": [{**sd["param_groups"][0], "param_names": ["x"] + names[1:]}]}
    with pytest.raises(ValueError, match="names differ"):
        new.load_state_dict(renamed)


def test_refusals_by_name():
    from givepose_amd import Adam, AdamW, GradAccumulator, Ranger
    net = _Tiny()
    for cls in (Adam, AdamW):
        with pytest.raises(ValueError, match=f"{cls.__name__}: parameter conv.weight.*HIP device"):
            cls(net)
        for key in ("maximize", "capturable", "differentiable", "fused"):
            with pytest.raises(NotImplementedError, match=f"{cls.__name__}: {key}=True is not built"):
                _host(cls)(net, **{key: True})
            _host(cls)(net, **{key: False})
        _host(cls)(net, foreach=True)
        for bad, match in ((dict(lr=-1e-3), "Invalid learning rate"), (dict(eps=-1.0), "Invalid epsilon"), (dict(betas=(1.0, 0.9)), "beta parameter at index 0"),
                           (dict(betas=(0.9, 1.0)), "beta parameter at index 1"), (dict(weight_decay=-1), "Invalid weight_decay"),
                           (dict(lr=torch.tensor(1e-3)), "tensor lr")):
            with pytest.raises((ValueError, NotImplementedError), match=match):
                _host(cls)(net, **bad)
    adam, adamw = _host(Adam)(net), _host(AdamW)(net)
    assert (adam.lr, adam.betas, adam.eps, adam.weight_decay, adam.amsgrad) == (1e-3, (0.9, 0.999), 1e-8, 0.0, False)
    assert (adamw.lr, adamw.betas, adamw.eps, adamw.weight_decay, adamw.amsgrad) == (1e-3, (0.9, 0.999), 1e-8, 1e-2, False)
    assert isinstance(adamw, Adam) and not isinstance(adam, AdamW) and not isinstance(adam, Ranger)
    with pytest.raises(ValueError, match="AdamW.load_state_dict: the saved group has decoupled_weight_decay=False \\(Adam\\)"):
        adamw.load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="Adam.load_state_dict: the saved group has amsgrad=True"):
        adam.load_state_dict(_host(Adam)(net, amsgrad=True).state_dict())
    sd = adam.state_dict()
    sd["param_groups"][0]["maximize"] = True
    with pytest.raises(NotImplementedError, match="maximize=True"):
        adam.load_state_dict(sd)
    with pytest.raises(ValueError, match="one parameter group over 6"):
        adam.load_state_dict({"state": {}, "param_groups": [{**sd["param_groups"][0], "params": [0, 1]}]})
    # _collect is Ranger's: aliases merged, a parameter without a gradient skipped, refusals by name
    g = {n: torch.ones_like(p) for n, p in net.named_parameters(remove_duplicate=False)}
    assert sorted(adam._collect(g)) == list(range(6))
    del g["gn.weight"], g["fc.bias"]
    assert sorted(adam._collect(g)) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="no parameter of that name"):
        adam._collect({"nope": torch.ones(1)})
    with pytest.raises(ValueError, match="fc.weight.*float16"):
        adam._collect({"fc.weight": torch.ones(2, 4, dtype=torch.float16)})
    with pytest.raises(ValueError, match="clip_norm"):
        adam.step(g, clip_norm=0)
    # the accumulator takes the two classes next to Ranger, and nothing else
    host_alloc = lambda name, shape: torch.empty(shape)
    for opt in (adam, adamw):
        acc = GradAccumulator(opt, alloc=host_alloc)
        assert acc.optimizer is opt and acc.flat.numel() == int(opt._offsets[-1])
    with pytest.raises(ValueError, match="Ranger is expected"):
        GradAccumulator(torch.optim.AdamW(net.parameters()))


def test_build_optimizer_restates_the_loops_three_branches(monkeypatch):
    from givepose_amd import Adam, AdamW, Ranger, build_optimizer, optim
    for cls in ("Ranger", "Adam", "AdamW"):
        monkeypatch.setattr(getattr(optim, cls), "_require_device", False)
    net = _Tiny()
    r, w, a, other = (build_optimizer(net, t, 3e-4) for t in ("Ranger", "AdamW", "Adam", "sgd"))
    assert type(r) is Ranger and r.lr == 3e-4 and r.betas == (0.95, 0.999)
    assert type(w) is AdamW and w.lr == 3e-4 and w.weight_decay == 1e-2
    assert type(a) is Adam and type(other) is Adam and a.lr == other.lr == 1e-3 and a.weight_decay == 0.0      # torch's default rate, as the reference
    assert all(o.model is net for o in (r, w, a, other))


@pytest.mark.parametrize("run", list(A.RUNS))
@pytest.mark.parametrize("variant", list(A.VARIANTS))
def test_the_restatement_against_torch_in_float64(variant, run):
    amsgrad = A.VARIANTS[variant][1].get("amsgrad", False)
    params, lr = A.case_params(run), A.RUNS[run]
    ref = A.make_ref(variant, params, lr)
    (o64, p64), (o32, p32) = (A.make_torch(variant, params, lr, dt) for dt in (torch.float64, torch.float32))
    worst = 0.0
    for step in range(1, A.STEPS + 1):
        grads = A.case_grads(step)
        A.torch_step(o64, p64, grads)
        norm32 = A.torch_step(o32, p32, grads)
        coef = torch.clamp(A.CLIP / (norm32 + 1e-6), max=1.0)          # clip_grad_norm_'s own float32 coefficient
        assert norm32.dtype == torch.float32 and (float(coef) == 1.0) == (step % 2 == 0)
        ref.step(grads, coef.numpy())
        for n in A.SHAPES:
            got, r64, r32 = ref.tensors(n), A.torch_tensors(o64, p64, n, amsgrad), A.torch_tensors(o32, p32, n, amsgrad)
            assert r64["p"].dtype == np.float64 and r32["p"].dtype == np.float32 and set(got) == set(r64)
            if step in A.SKIP_STEPS.get(n, ()):
                assert all(np.array_equal(got[k], before[n][k]) for k in got), (n, step)
            worst = max(worst, A.rule(got, r64, r32, f"{variant} {run} step {step} {n}", quiet=True))
        before = {n: {k: v.copy() for k, v in ref.tensors(n).items()} for n in A.SHAPES}
    assert ref.state["skip"]["step"] == A.STEPS - 2 and ref.state["chunk1"]["step"] == A.STEPS
    print(f"{variant} {run}: largest restatement / torch float32 ratio over {A.STEPS} steps {worst:.2f} (8 allowed)")
