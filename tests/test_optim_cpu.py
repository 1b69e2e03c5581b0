"""CPU: the optimiser family (include/givepose_optim.h, gpo_*; givepose_amd/optim.py) -- the float64 restatement tests/ranger_ref.py
against the reference's own Ranger after clip_grad_norm_ (tests/golden/ranger_*.npz, scripts/gen_golden_ranger.py), flat_and_anneal_lr
against the reference's scheduler (tests/golden/flat_and_anneal.npz), the family's registration, the state-dict layout and the
deduplication of parameters registered under two names.

ranger_ref in float64 and the golden float64 run evaluate the same formulas in the same precision: they differ by the summation order of
the norm and of the row means only, so every stored figure is asked to 1e-12 -- per tensor, |got - golden| <= 1e-12 max|golden| at the
sampled elements, and 1e-12 sum|golden| for the tensor's sum over all its elements.
"""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ranger_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-12


@pytest.mark.parametrize("variant,run", R.GOLDEN, ids=lambda v: v)
def test_ranger_ref_float64_reproduces_the_reference(variant, run):
    gold = np.load(os.path.join(GOLD, f"ranger_{variant}_{run}.npz"))
    assert int(gold["input_crc"]) == R.input_crc(run), "the seeded inputs changed: regenerate with scripts/gen_golden_ranger.py"
    idx = R.sample_index()
    bounds = np.cumsum([0] + [len(idx[n]) for n in R.SHAPES])
    worst = [0.0]

    def check(step, ref):
        s = R.summarise(ref.tensors)
        for key in R.STATE_KEYS:
            want, wsum, wabs = (gold[f"f64_{key}{suffix}"][step - 1] for suffix in ("", "_sum", "_abs"))
            got, gsum, _ = s[key]
            for t, name in enumerate(R.SHAPES):
                a, b = got[bounds[t]:bounds[t + 1]], want[bounds[t]:bounds[t + 1]]
                scale = np.abs(b).max()
                assert np.abs(a - b).max() <= TOL * scale, (variant, run, step, key, name)
                assert abs(gsum[t] - wsum[t]) <= TOL * wabs[t], (variant, run, step, key, name, "sum")
                if scale > 0:
                    worst[0] = max(worst[0], np.abs(a - b).max() / scale)
        assert abs(float(ref.norm) - gold["norm"][step - 1]) <= TOL * gold["norm"][step - 1]
        assert abs(float(ref.coef) - gold["coef"][step - 1]) <= TOL
        assert (float(ref.coef) == 1.0) == (step % 2 == 0)          # both clip branches: the even steps' norm is below the threshold

    ref = R.run_case(variant, run, torch.float64, on_step=check)
    print(f"{variant} {run}: largest |ranger_ref - reference| / max|reference| over steps, states and tensors {worst[0]:.2e}")
    assert ref.state["skip"]["step"] == R.STEPS - 2 and ref.state["w51"]["step"] == R.STEPS
    if variant in ("gc", "wd"):       # (5,1) is centralised with row length 1: its gradient is an exact 0
        assert not ref.state["w51"]["exp_avg_sq"].any()
    if variant == "gc":               # and without weight decay neither exp_avg nor the parameter ever moves
        assert not ref.state["w51"]["exp_avg"].any()
        assert torch.equal(ref.p["w51"], torch.from_numpy(R.case_params(run)["w51"]).double())


def test_the_cases_cover_the_branches():
    from givepose_amd.optim import radam_step_size
    rect = [radam_step_size(t, 0.95, 0.999, 5)[0] for t in range(1, R.STEPS + 1)]
    assert rect == [False] * 5 + [True] * 8           # steps 1-5 unrectified, step 6 the first rectified one and the first Lookahead step
    norms = [np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in R.case_grads(s).values())) for s in range(1, R.STEPS + 1)]
    assert all((n < R.CLIP) == (s % 2 == 0) for s, n in zip(range(1, R.STEPS + 1), norms)) and max(norms) > 20 * R.CLIP
    assert "skip" not in R.case_grads(3) and "skip" not in R.case_grads(9) and "skip" in R.case_grads(4)


def test_flat_and_anneal_lr_matches_the_reference_scheduler():
    from givepose_amd import flat_and_anneal_lr
    gold = np.load(os.path.join(GOLD, "flat_and_anneal.npz"))
    total, warm, wf, ap, target, power, gamma, s0, s1 = gold["settings"]
    n = 0
    for key in gold.files:
        if key == "settings":
            continue
        anneal, method = key.split("__")
        got = np.array([flat_and_anneal_lr(it, int(total), warmup_iters=int(warm), warmup_factor=wf, warmup_method=method, anneal_point=ap,
                                           anneal_method=anneal, target_lr_factor=target, poly_power=power, step_gamma=gamma, steps=(s0, s1))
                        for it in range(int(total))])
        assert got.shape == gold[key].shape and np.abs(got - gold[key]).max() <= TOL, key
        n += 1
    assert n == 12
    assert flat_and_anneal_lr(0, 100) == 1 and flat_and_anneal_lr(100, 100) == pytest.approx(0.0, abs=1e-15)       # the defaults: no warm-up, cosine to 0
    for bad, match in ((dict(warmup_method="exp"), "warmup_method"), (dict(anneal_method="sqrt"), "anneal_method"),
                       (dict(anneal_method="step", steps=(0.5, 1.5)), "error in steps"), (dict(anneal_method="step", steps=(0.9, 0.5)), "ascending"),
                       (dict(anneal_method="step", steps=(0.05, 0.5), warmup_iters=10), "error in steps"), (dict(anneal_point=1.5), "anneal_point"),
                       (dict(anneal_point=-0.1), "anneal_point")):
        with pytest.raises(ValueError, match=match):
            flat_and_anneal_lr(3, 100, **bad)


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build, optim
    hdr = _header("givepose_optim.h")
    declared = set(re.findall(r"\b(gpo_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.OPTIM_PROTOTYPES) and len(declared) == 4
    for other in (_lib.PROTOTYPES, _lib.HEADGRAD_PROTOTYPES, _lib.GRAD_PROTOTYPES, _lib.XYZGRAD_PROTOTYPES, _lib.ENCGRAD_PROTOTYPES, _lib.BBGRAD_PROTOTYPES):
        assert not set(_lib.OPTIM_PROTOTYPES) & set(other)
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gpo_[a-z0-9_]+)", out)) == declared
    assert "optim.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "givepose_amd", "csrc", "optim.hip")).read()
    shared = open(os.path.join(ROOT, "givepose_amd", "csrc", "flat_tensors.hpp")).read()
    assert '#include "flat_tensors.hpp"' in src and not re.search(r"\batomic\w*\s*\(", src + shared)                    # no atomic in the family
    assert len(re.findall(r"hipLaunchKernelGGL", src.split("int gpo_ranger_step(")[1].split("long long gpo_clip")[0])) == _lib.GPO_STEP_LAUNCHES
    consts = {k: int(v) for k, v in re.findall(r"#define (GPO_[A-Z_]+) (\d+)", hdr)}
    assert consts == {"GPO_CHUNK": _lib.GPO_CHUNK, "GPO_STEP_LAUNCHES": _lib.GPO_STEP_LAUNCHES, "GPO_CLIP_LAUNCHES": _lib.GPO_CLIP_LAUNCHES,
                      "GPO_MAX_TENSORS": _lib.GPO_MAX_TENSORS, "GPO_FLAG_RECTIFIED": _lib.GPO_FLAG_RECTIFIED, "GPO_FLAG_LOOKAHEAD": _lib.GPO_FLAG_LOOKAHEAD}
    assert ctypes.sizeof(_lib.OptTensor) == optim._TENSOR.itemsize == 64 and ctypes.sizeof(_lib.OptHyper) == 48
    for f, _ in _lib.OptTensor._fields_:
        assert getattr(_lib.OptTensor, f).offset == optim._TENSOR.fields[f][1], f
    # the size queries answer on the host (they read no device memory); a table the entry point refuses has no workspace
    lib = _lib.load()
    tab = np.zeros(3, optim._TENSOR)
    for f in ("p", "g", "m", "v", "slow"):
        tab[f] = 4096
    tab["n"], tab["rows"], tab["row_len"] = [10, 2 * 4099, 5], [0, 2, 5], [0, 4099, 1]
    ptr = optim._table_ptr(tab)
    # chunks: 1 flat, 2 rows x 2 segments, 1 run of rows -> 6; row partials: 4 + 5.  Tables 3 x 80 + 6 x 16 bytes, then the chunks' sums
    # of squares, the row partials and the scalars, each rounded up to 256 bytes
    assert lib.gpo_ranger_step_workspace(ptr, 3) == 512 + 256 + 256 + 256 and lib.gpo_clip_grad_norm_workspace(ptr, 3) > 0
    assert lib.gpo_ranger_step_workspace(ptr, 0) == 0 and lib.gpo_ranger_step_workspace(None, 3) == 0
    for field, value in (("n", 0), ("rows", 3), ("row_len", 0), ("g", 0), ("g", 4098), ("slow", 0), ("flags", 4), ("rows", -1)):
        bad = tab.copy()
        bad[field][1] = value
        assert lib.gpo_ranger_step_workspace(optim._table_ptr(bad), 3) == 0, (field, value)
    assert b"tensor 1" in lib.gp_last_error()


def test_the_flat_tensor_families_share_one_text():
    """What the gpo_*, gpc_* and gpad_* families have in common -- the reductions, the quad moves, the finalize kernel, the chunk record
    -- is defined in csrc/flat_tensors.hpp and in none of the three files: the norm's bits are equal across them by construction."""
    from givepose_amd import build
    csrc = os.path.join(ROOT, "givepose_amd", "csrc")
    shared = open(os.path.join(csrc, "flat_tensors.hpp")).read()
    family = {f: open(os.path.join(csrc, f)).read() for f in ("optim.hip", "accum.hip", "adam.hip")}
    definitions = [r"\bfloat\s+wave_sum\s*\(", r"\bfloat\s+wg_sum\s*\(", r"\bf32x4\s+load_quad\s*\(", r"\bvoid\s+store_quad\s*\(", r"\bbool\s+al16\s*\(",
                   r"\blong long\s+up256\s*\(", r"\bstruct\s+Chunk\b", r"\bvoid\s+\w*finalize_kernel\s*\(", r"\bfloat\s+sq_add\s*\(",
                   r"\bint\s+send_tables\s*\(", r"\bstruct\s+Plan\b"]
    for d in definitions:
        assert len(re.findall(d, shared)) == 1, d
        for f, text in family.items():
            assert not re.search(d, text), (d, f)
    for f, text in family.items():
        assert text.count('#include "flat_tensors.hpp"') == 1, f
        assert "finalize_kernel" in text and not re.search(r"\b\w+_finalize_kernel\b", text), f          # each launches the one definition
        assert not re.search(r"__fmul_rn\((\w+(?:\[\w+\])?), \1\)", text) and "__builtin_fmaf" not in text and "sq_add(" in text, f      # one way to square
        assert not re.search(r"#define\s+GP\w+_CHECK\b", text), f
    assert "__builtin_fmaf(x, x, sq)" in shared and len(re.findall(r"#define\s+FLAT_CHECK\b", shared)) == 1
    # included by exactly the three, and a dependency of the build
    users = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp")) and '"flat_tensors.hpp"' in open(os.path.join(csrc, f)).read())
    assert users == ["accum.hip", "adam.hip", "optim.hip"]
    assert "flat_tensors.hpp" in open(build.__file__).read()


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

    class HostRanger(Ranger):        # the table and the layout on the host; the step itself needs the device
        _require_device = False
    return HostRanger


def test_state_dict_has_the_layout_of_torch_optimizers_and_round_trips():
    from givepose_amd import Ranger
    net = _Tiny()
    with pytest.raises(ValueError, match="conv.weight.*HIP device"):
        Ranger(net)
    with pytest.raises(NotImplementedError, match="gc_loc=False"):
        Ranger(net, gc_loc=False)
    for bad, match in ((dict(alpha=1.5), "slow update rate"), (dict(k=0), "lookahead steps"), (dict(lr=0), "Learning Rate"), (dict(eps=0), "eps")):
        with pytest.raises(ValueError, match=match):
            Ranger(net, **bad)
    opt = _host_ranger()(net, lr=2e-3, k=5)
    names = [n for n, _ in net.named_parameters()]
    assert opt.param_names == names == ["conv.weight", "conv.bias", "norm.weight", "norm.bias", "fc.weight", "fc.bias"]
    assert all(a is b for a, b in zip(opt.params, net.parameters()))
    sd = opt.state_dict()
    torch_sd = torch.optim.Adam(net.parameters()).state_dict()
    assert set(sd) == set(torch_sd) == {"state", "param_groups"} and sd["state"] == {}
    assert sd["param_groups"][0]["params"] == torch_sd["param_groups"][0]["params"] == list(range(6))
    assert sd["param_groups"][0]["param_names"] == names
    assert {"lr", "alpha", "k", "step_counter", "betas", "N_sma_threshhold", "eps", "weight_decay"} <= set(sd["param_groups"][0])
    # state for the stepped parameters only, in the parameters' shapes
    opt.steps[0], opt.steps[4] = 3, 2
    for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
        opt._flat[key].copy_(torch.arange(opt._flat[key].numel(), dtype=torch.float32))
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 4] and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "slow_buffer"}
    assert sd["state"][0]["step"] == 3 and sd["state"][4]["exp_avg"].shape == net.fc.weight.shape
    assert all(o % 64 == 0 for o in opt._offsets) and sd["state"][4]["exp_avg"][0, 0] == float(opt._offsets[4])
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    new = _host_ranger()(net)
    new.load_state_dict(torch.load(buf))
    assert new.steps == opt.steps and new.lr == 2e-3 and new.k == 5
    for i in (0, 4):
        for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
            assert torch.equal(new._view(key, i), opt._view(key, i))
    assert not new._view("exp_avg", 1).any()
    renamed = {**sd, "param_groups": [{**sd["param_groups"][0], "param_names": ["x"] + names[1:]}]}
    with pytest.raises(ValueError, match="names differ"):
        new.load_state_dict(renamed)


def test_parameters_under_two_names_are_one_entry():
    Host = _host_ranger()
    net = _Tiny()
    opt = Host(net)
    assert opt._index["gn.weight"] == opt._index["norm.weight"] == 2 and opt._index["gn.bias"] == opt._index["norm.bias"] == 3
    assert len(opt._index) == 8 and len(opt.params) == 6
    assert [tuple(r) for r in opt._static[["rows", "row_len"]].tolist()] == [(4, 27), (0, 0), (0, 0), (0, 0), (2, 4), (0, 0)]
    assert [tuple(r) for r in Host(net, gc_conv_only=True)._static[["rows", "row_len"]].tolist()] == [(4, 27)] + [(0, 0)] * 5
    assert not Host(net, use_gc=False)._static["rows"].any()
    g = {n: torch.ones_like(p) for n, p in net.named_parameters(remove_duplicate=False)}
    assert sorted(opt._collect(g)) == list(range(6))
    g["gn.weight"] = g["norm.weight"].clone()                 # equal but distinct: accepted
    assert sorted(opt._collect(g)) == list(range(6))
    g["gn.weight"] = 2 * g["norm.weight"]
    with pytest.raises(ValueError, match="gn.weight.*norm.weight.*different gradients"):
        opt._collect(g)
    del g["gn.weight"], g["fc.bias"]
    assert sorted(opt._collect(g)) == [0, 1, 2, 3, 4]          # a parameter without a gradient is skipped
    for bad, match in (({"fc.weight": torch.ones(2, 4).t()}, "fc.weight.*expected contiguous float32 \\(2, 4\\)"),
                       ({"fc.weight": torch.ones(2, 4, dtype=torch.float16)}, "fc.weight.*float16"),
                       ({"fc.weight": torch.ones(4, 2).t()}, "fc.weight.*not contiguous"), ({"nope": torch.ones(1)}, "no parameter of that name")):
        with pytest.raises(ValueError, match=match):
            opt._collect(bad)


def test_posenet_aliases_and_parameter_order():
    """The 35 names of a coordinate head are 23 tensors, and the index order of the state dict is model.parameters() order: the
    non-backbone names in the order the reference's state dict lists them (tests/golden/state_dict_manifest.json)."""
    import json
    from givepose_amd import PoseNet, PoseNetConfig
    net = PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1)), dtype=torch.float32)
    opt = _host_ranger()(net)
    assert len(opt.params) == len(list(net.parameters())) and opt.param_names == [n for n, _ in net.named_parameters()]
    head = [n for n in opt._index if n.startswith("xyz_nocs_head.")]
    assert len(head) == 35 and len({opt._index[n] for n in head}) == 23
    assert all(opt._index[n] == opt._index[n.replace(".gn.", ".norm.")] for n in head)
    manifest = json.load(open(os.path.join(GOLD, "state_dict_manifest.json")))["non_backbone_from_reference"]
    want = [n for n in manifest if ".gn." not in n and not n.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert [n for n in opt.param_names if not n.startswith("backbone.")] == want
    assert opt.param_names[0].startswith("backbone.") and hasattr(net, "params_updated") and hasattr(net, "train_step")
