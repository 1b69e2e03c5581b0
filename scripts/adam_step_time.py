#!/usr/bin/env python3
"""Time one clip + AdamW step over the full model's tensor list next to this tree's clip + Ranger step and to what the reference would
run, torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW at torch's defaults, on the same GPU and tensors.  The set-up is
scripts/optim_step_time.py's: the ConvNeXt-Base configuration, seeded gradients for the 459 tensors that have one, no forward.

    python scripts/adam_step_time.py [--rounds 3] [--seconds 1] [--settle 2] [--out FILE]    the three steps in alternating rounds
    python scripts/adam_step_time.py --kernel-count [--out FILE]                              kernels of one step from rocprofv3 --kernel-trace
    python scripts/adam_step_time.py --train-step [--out FILE]                                train_step with AdamW against Ranger

Times are host clocks around steps that end in ONE device synchronise (the host's table build is inside), in rounds of about `--seconds`
each that run the three in turn after `--settle` seconds of the same; per step the median round with min .. max.  The condition: the Adam
step moves a subset of Ranger's bytes (no slow buffer, no row sums), so it must not be slower than Ranger's by more than the spread of
Ranger's rounds.  Bytes per step are what the algorithm needs: the gradient twice (norm pass, update), p, exp_avg and exp_avg_sq read and
written.

--kernel-count starts two child processes under rocprofv3 (1 step and 4 steps after the same warm-up) and reports the difference of
their kernel counts over 3, the launches of a steady-state step whatever launched them; it must equal GPAD_STEP_LAUNCHES.
--train-step: PoseNet.train_step (ConvNeXt-Base, B = 64, float32 network, device repack) with AdamW and with Ranger over the same model,
in alternating rounds of 5 steps.
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import optim_step_time as base  # noqa: E402  (setup, timed, HBM_PEAK)


def window(fn, seconds):
    """ms per call over about `seconds`: a short calibration, then one host-timed run of that many calls ending in a synchronise."""
    n = max(int(seconds / max(base.timed(fn, 3), 1e-5)), 3)
    return base.timed(fn, n) * 1e3


def alternate(fns, rounds, settle, seconds):
    """{name: fn} -> {name: (median, min, max) ms per call} over `rounds` rounds that run the names in turn."""
    for fn in fns.values():
        window(fn, settle / len(fns))
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(window(fn, seconds))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def verdict(res, new, old, what):
    extra, spread = res[new][0] - res[old][0], res[old][2] - res[old][1]
    return (f"{what}: {new} is {extra:+.3f} ms against {old} ({res[old][0] / res[new][0]:.2f}x), the spread of the {old} rounds is {spread:.3f} ms"
            + ("" if extra <= spread else f": SLOWER than {old} by more than the spread"))


def child(steps, warmup):
    import torch

    from givepose_amd import AdamW
    net, grads = base.setup()
    net.params_updated = lambda: None         # the step's kernels only
    opt = AdamW(net)
    for _ in range(warmup + steps):
        opt.step(grads, clip_norm=5.0)
    torch.cuda.synchronize()


def kernel_count(say):
    counts = {}
    for steps in (1, 4):
        with tempfile.TemporaryDirectory() as d:
            subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--child", str(steps)], check=True, stdout=subprocess.DEVNULL)
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                rows += list(csv.DictReader(open(f)))
            names = [r.get("Kernel_Name", "") for r in rows]
            copies = sum("__amd_rocclr_" in n for n in names)       # the runtime's own copy kernels, where the trace lists them
            counts[steps] = (len(names) - copies, copies)
            mine = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows
                          if "adam_" in r.get("Kernel_Name", "") or "finalize_kernel" in r.get("Kernel_Name", ""))[-9:]
            if steps == 4 and len(mine) == 9:
                per = {}
                for a, b, n in mine:
                    key = next(k for k in ("adam_reduce_kernel", "finalize_kernel", "adam_update_kernel") if k in n)
                    per[key] = per.get(key, 0.0) + (b - a) / 3e3
                say("kernel time per step (mean of the last three steps under the tracer): "
                    + ", ".join(f"{k} {v:.1f} us" for k, v in per.items()) + f"; sum {sum(per.values()):.1f} us")
    per_step, copies = (counts[4][0] - counts[1][0]) / 3, (counts[4][1] - counts[1][1]) / 3
    from givepose_amd import _lib
    say(f"kernels per steady-state AdamW step (rocprofv3 --kernel-trace, all kernels of the process, (4 steps - 1 step) / 3): {per_step:g}; "
        f"documented constant GPAD_STEP_LAUNCHES = {_lib.GPAD_STEP_LAUNCHES}; copy kernels of the runtime per step: {copies:g}")
    say(f"    kernels traced: {counts[1][0]} with 1 step, {counts[4][0]} with 4 steps, after 2 warm-up steps")
    if per_step != _lib.GPAD_STEP_LAUNCHES:
        raise SystemExit(f"a step launched {per_step:g} kernels, not {_lib.GPAD_STEP_LAUNCHES}")


def step_times(args, say):
    import torch

    from givepose_amd import AdamW, Ranger
    net, grads = base.setup()
    net.params_updated = lambda: None         # the steps' kernels only: the repack is scripts/repack_time.py's
    ranger, adamw = Ranger(net), AdamW(net)
    idx = sorted({adamw._index[n] for n in grads})
    n_elem = sum(adamw.params[i].numel() for i in idx)
    say(f"device: {torch.cuda.get_device_name(0)}; {len(idx)} tensors with a gradient of {len(adamw.params)}, {n_elem / 1e6:.1f} M elements")
    # what the reference would run: torch's own AdamW over copies of the same tensors, the gradients in .grad
    tparams = [torch.nn.Parameter(adamw.params[i].detach().clone()) for i in idx]
    for p, i in zip(tparams, idx):
        p.grad = grads[adamw.param_names[i]].clone()
    topt = torch.optim.AdamW(tparams)

    def torch_step():
        torch.nn.utils.clip_grad_norm_(tparams, 5.0)
        topt.step()
    fns = {"AdamW": lambda: adamw.step(grads, clip_norm=5.0), "Ranger": lambda: ranger.step(grads, clip_norm=5.0), "torch AdamW": torch_step}
    res = alternate(fns, args.rounds, args.settle, args.seconds)
    say(f"ms per step, host clock around steps ending in one synchronise, host table build included: median of {args.rounds} alternating "
        f"{args.seconds:g} s rounds (min .. max) after {args.settle:g} s of the same")
    nbytes = {"AdamW": n_elem * 4 * (2 + 3 + 3), "Ranger": n_elem * 4 * (2 + 3 + 3 + 2 / ranger.k)}
    for k, (med, lo, hi) in res.items():
        line = f"  {k:12s} {med:8.3f} ({lo:.3f} .. {hi:.3f})"
        if k in nbytes:
            line += (f"   {nbytes[k] / 1e9:.2f} GB per step needed -> {nbytes[k] / (med * 1e-3) / 1e12:.2f} TB/s, "
                     f"{nbytes[k] / (med * 1e-3) / base.HBM_PEAK:.2f} of the {base.HBM_PEAK / 1e12:g} TB/s BASELINE.md uses")
        else:
            line += f"   clip_grad_norm_ + torch.optim.AdamW at torch's defaults: {med / res['AdamW'][0]:.1f} x the AdamW step"
        say(line)
    say("  " + verdict(res, "AdamW", "Ranger", "the step"))


def train_step_times(say, rounds=3, steps=5):
    import numpy as np
    import torch

    import pose_loss_ref as PR
    from givepose_amd import AdamW, PoseLoss, PoseNet, PoseNetConfig, Ranger, synth
    B = 64
    net = PoseNet(PoseNetConfig(), dtype=torch.float32, seed=3).cuda().set_repack("device")
    npb = synth.synth_batch(B, seed=11)
    npb["roi_mask_deform"] = npb["roi_mask"]
    _, gt = PR.make_inputs(B=B, P=256, seed=60)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**npb, **gt}.items()}
    opts, pl = {"AdamW": AdamW(net), "Ranger": Ranger(net)}, PoseLoss()
    runs = {m: [] for m in opts}
    for _ in range(rounds):
        for m, opt in opts.items():
            net.train_step(data, pl, opt, "cuda")
            torch.cuda.synchronize()
            t = []
            for _ in range(steps):
                t0 = time.perf_counter()
                net.train_step(data, pl, opt, "cuda")
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            runs[m].append(sorted(t)[len(t) // 2])
    res = {m: (sorted(v)[len(v) // 2], min(v), max(v)) for m, v in runs.items()}
    say(f"train_step, ConvNeXt-Base, B = {B}, float32 network, set_repack('device'), size_head=None: ms per step, median of {rounds} alternating "
        f"rounds of {steps} steps (min .. max of the rounds' medians)")
    for m in opts:
        say(f"  {m:8s} {res[m][0]:8.1f} ({res[m][1]:.1f} .. {res[m][2]:.1f})")
    say("  " + verdict(res, "AdamW", "Ranger", "train_step"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--settle", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-count", action="store_true")
    ap.add_argument("--train-step", action="store_true")
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args.child, 2)
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if args.kernel_count:
        return kernel_count(say)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("adam_step_time.py needs the GPU: a time from anywhere else says nothing")
    if args.train_step:
        return train_step_times(say)
    step_times(args, say)


if __name__ == "__main__":
    main()
