#!/usr/bin/env python3
"""Generate tests/golden/ranger_<variant>_<run>.npz and tests/golden/flat_and_anneal.npz from the REFERENCE's own
tools/torch_utils/solver/ranger2020.py:Ranger (after torch.nn.utils.clip_grad_norm_(params, 5), as engine/train.py:117-126 calls the
two) and tools/torch_utils/solver/lr_scheduler.py:flat_and_anneal_lr_scheduler.

Run:  python scripts/gen_golden_ranger.py [REFERENCE_ROOT]       (build container only: needs the reference checkout, never a GPU)

Only the reference's OUTPUTS are stored; the inputs are the seeded arrays of tests/ranger_ref.py (case_params, case_grads), recorded by
a CRC.  Per file, after every one of the 13 steps and for p, exp_avg, exp_avg_sq and slow_buffer:
  * "f64_<state>" (13, S): the float64 run at the sampled elements of every tensor (ranger_ref.sample_index, concatenated in SHAPES order),
    "f64_<state>_sum" / "_abs" (13, T): each tensor's sum and sum of |.| over ALL its elements;
  * "f32_<state>" (13, S): the float32 run at the same elements;
  * "norm", "coef" (13,): the float64 total norm clip_grad_norm_ returned and the coefficient it applied.
The full tensors (21 k elements x 4 states x 13 steps x 2 precisions, 13 MB per case) are not stored: the samples pin the elements,
the sums every element.

The float64 run.  ranger2020.py:149-154 casts the gradient and the parameter with .float(), so run as written on float64 tensors it
would still compute in float32.  For the float64 run the generator maps Tensor.float to Tensor.double while Ranger.step runs -- the
reference's own statements, evaluated in float64; the float32 run is the reference untouched.
The generator asserts that both clip branches occur (coefficient exactly 1 on the even steps, below 0.1 on the odd ones) and prints
how far the float32 run is from the float64 one.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_shim  # noqa: E402

if len(sys.argv) > 1:
    ref_shim.REFERENCE_ROOT = os.path.abspath(sys.argv[1])
ref_shim.install()
import torch  # noqa: E402

import ranger_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def save(name, **arrs):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    size = os.path.getsize(path)
    print(f"  wrote {name}.npz ({size / 1024:.1f} KB)")
    assert size < 200 * 1024


class _Float64:
    """While active, Tensor.float() returns a float64 tensor (see the module docstring)."""

    def __enter__(self):
        self.keep = torch.Tensor.float
        torch.Tensor.float = lambda t, *a, **k: t.double()

    def __exit__(self, *exc):
        torch.Tensor.float = self.keep


def reference_run(Ranger, variant, run, dtype):
    params = {n: torch.nn.Parameter(torch.from_numpy(a).to(dtype)) for n, a in R.case_params(run).items()}
    opt = Ranger(list(params.values()), lr=R.RUNS[run], **R.VARIANTS[variant])
    per_step, norms, coefs = [], [], []
    for step in range(1, R.STEPS + 1):
        grads = R.case_grads(step)
        for n, p in params.items():
            p.grad = torch.from_numpy(grads[n]).to(dtype) if n in grads else None
        norm = torch.nn.utils.clip_grad_norm_(list(params.values()), R.CLIP)
        first = next(n for n in params if n in grads)
        coefs.append(float((params[first].grad.double().reshape(-1)[0] / float(torch.from_numpy(grads[first]).to(dtype).double().reshape(-1)[0]))))
        norms.append(float(norm))
        if dtype == torch.float64:
            with _Float64():
                opt.step()
        else:
            opt.step()
        for n, p in params.items():
            assert p.dtype == dtype and all(opt.state[p][k].dtype == dtype for k in R.STATE_KEYS[1:]), (n, "the run left its precision")
        per_step.append(R.summarise(lambda n: {"p": params[n].data, **{k: opt.state[params[n]][k] for k in R.STATE_KEYS[1:]}}))
    return per_step, np.array(norms), np.array(coefs)


def gen_ranger():
    from tools.torch_utils.solver.ranger2020 import Ranger
    print("clip_grad_norm_ + Ranger.step")
    for variant, run in R.GOLDEN:
        s64, norm, coef = reference_run(Ranger, variant, run, torch.float64)
        s32, _, _ = reference_run(Ranger, variant, run, torch.float32)
        small = [s for s in range(1, R.STEPS + 1) if norm[s - 1] < R.CLIP]
        assert small == [s for s in range(1, R.STEPS + 1) if s % 2 == 0], small
        assert all(coef[s - 1] == 1.0 for s in small) and all(coef[s - 1] < 0.1 for s in range(1, R.STEPS + 1) if s not in small), coef
        arrs = {"input_crc": R.input_crc(run), "norm": norm, "coef": coef}
        for key in R.STATE_KEYS:
            arrs["f64_" + key] = np.stack([s[key][0] for s in s64])
            arrs["f64_" + key + "_sum"] = np.stack([s[key][1] for s in s64])
            arrs["f64_" + key + "_abs"] = np.stack([s[key][2] for s in s64])
            arrs["f32_" + key] = np.stack([s[key][0] for s in s32]).astype(np.float32)
            scale = np.abs(arrs["f64_" + key]).max()
            print(f"  {variant:8s} {run:6s} {key:11s} float32 run against float64 at the samples: {np.abs(arrs['f32_' + key] - arrs['f64_' + key]).max() / scale:.2e} of max|.|")
        save(f"ranger_{variant}_{run}", **arrs)


SCHED = dict(total_iters=200, warmup_iters=20, warmup_factor=0.1, anneal_point=0.72, target_lr_factor=0.05, poly_power=2.0, step_gamma=0.1,
             steps=[2 / 3.0, 8 / 9.0])


def gen_scheduler():
    from tools.torch_utils.solver.lr_scheduler import flat_and_anneal_lr_scheduler
    print("flat_and_anneal_lr_scheduler")
    arrs = {}
    for anneal in ("cosine", "linear", "poly", "exp", "step", "none"):
        for warm in ("linear", "constant"):
            opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
            sched = flat_and_anneal_lr_scheduler(opt, warmup_method=warm, anneal_method=anneal, **SCHED)
            f = sched.lr_lambdas[0]
            arrs[f"{anneal}__{warm}"] = np.array([float(f(it)) for it in range(SCHED["total_iters"])], np.float64)
    arrs["settings"] = np.array([SCHED["total_iters"], SCHED["warmup_iters"], SCHED["warmup_factor"], SCHED["anneal_point"], SCHED["target_lr_factor"],
                                 SCHED["poly_power"], SCHED["step_gamma"], *SCHED["steps"]], np.float64)
    save("flat_and_anneal", **arrs)


if __name__ == "__main__":
    gen_ranger()
    gen_scheduler()
    print("done")
