#!/usr/bin/env python3
"""Time one clip + Ranger step over the full model's tensor list (ConvNeXt-Base configuration, seeded gradients of the parameters'
shapes; no forward is run) on the device, next to tests/ranger_ref.py in float32 on the same GPU over the same tensors.

    python scripts/optim_step_time.py [--steps 240] [--warmup 6] [--out FILE]     timings, bytes / time, the host repack
    python scripts/optim_step_time.py --kernel-count [--out FILE]                 kernels of one step from rocprofv3 --kernel-trace

Times are host clocks around work that ends in a device synchronise, over `--steps` steps after `--warmup` (the warm-up covers the
first step, which creates the state, and steps 6 and 12, the Lookahead steps).  Every parameter outside size_head and the never-applied
dcnv3.bn.* has a gradient, as in PoseNet.head_grads_backbone.  Bytes per step are what the algorithm needs: the gradient twice (norm
pass, update), p, exp_avg and exp_avg_sq read and written; slow_buffer read and written on every k-th step.

--kernel-count starts two child processes under rocprofv3 (1 step and 4 steps after the same warm-up) and reports the difference of
their kernel counts over 3: the launches of a steady-state step, whatever launched them.
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
HBM_PEAK = 8e12      # bytes / s, the figure BASELINE.md uses


def setup(seed=0):
    import re

    import torch

    from givepose_amd import PoseNet, PoseNetConfig
    net = PoseNet(PoseNetConfig(), dtype=torch.float32, seed=seed).cuda()
    gen = torch.Generator(device="cuda").manual_seed(1234)
    grads = {}
    for name, p in net.named_parameters(remove_duplicate=False):
        if name.startswith("size_head.") or re.match(r"nocs_encoder\.features\.\d+\.bn\.", name):
            continue
        twin = name.replace(".gn.", ".norm.")
        grads[name] = grads[twin] if twin in grads else 1e-3 * torch.randn(p.shape, device="cuda", generator=gen)
    return net, grads


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def child(steps, warmup):
    import torch

    from givepose_amd import Ranger
    net, grads = setup()
    net.params_updated = lambda: None         # the step's kernels only: the repack is timed on its own
    opt = Ranger(net)
    for _ in range(warmup + steps):
        opt.step(grads, clip_norm=5.0)
    torch.cuda.synchronize()


def kernel_count(args, say):
    counts = {}
    for steps in (1, 4):
        with tempfile.TemporaryDirectory() as d:
            subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--child", str(steps), "--warmup", "2"], check=True, stdout=subprocess.DEVNULL)
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                rows += list(csv.DictReader(open(f)))
            names = [r.get("Kernel_Name", "") for r in rows]
            copies = sum("__amd_rocclr_" in n for n in names)       # the runtime's own copy kernels, where the trace lists them
            counts[steps] = (len(names) - copies, copies)
            # the family's own kernels of the last three steps, in launch order: their time on the device
            mine = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows
                          if "DevTensor" in r.get("Kernel_Name", "") or "finalize_kernel" in r.get("Kernel_Name", ""))[-9:]
            if steps == 4 and len(mine) == 9:
                per = {}
                for a, b, n in mine:
                    key = next(k for k in ("reduce_kernel", "finalize_kernel", "update_kernel") if k in n)
                    per[key] = per.get(key, 0.0) + (b - a) / 3e3
                say("kernel time per step (mean of the last three steps under the tracer): "
                    + ", ".join(f"{k} {v:.1f} us" for k, v in per.items()) + f"; sum {sum(per.values()):.1f} us")
    per_step, copies = (counts[4][0] - counts[1][0]) / 3, (counts[4][1] - counts[1][1]) / 3
    from givepose_amd import _lib
    say(f"kernels per steady-state step (rocprofv3 --kernel-trace, all kernels of the process, (4 steps - 1 step) / 3): {per_step:g}; "
        f"documented constant GPO_STEP_LAUNCHES = {_lib.GPO_STEP_LAUNCHES}; copy kernels of the runtime per step: {copies:g}")
    say(f"    kernels traced: {counts[1][0]} with 1 step, {counts[4][0]} with 4 steps, after 2 warm-up steps")
    if per_step != _lib.GPO_STEP_LAUNCHES:
        raise SystemExit(f"a step launched {per_step:g} kernels, not {_lib.GPO_STEP_LAUNCHES}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-count", action="store_true")
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.warmup)
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if args.kernel_count:
        return kernel_count(args, say)

    import torch

    import ranger_ref as R
    from givepose_amd import Ranger
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_time.py needs the GPU: a time from anywhere else says nothing")
    net, grads = setup()
    repack = [0]
    net.params_updated = lambda: repack.__setitem__(0, repack[0] + 1)      # the step's kernels only: the repack is timed below
    opt = Ranger(net)
    n_elem = sum(p.numel() for i, p in enumerate(opt.params) if opt.param_names[i] in grads)
    n_tensors = len({opt._index[n] for n in grads})
    say(f"device: {torch.cuda.get_device_name(0)}; {n_tensors} tensors with a gradient of {len(opt.params)}, {n_elem / 1e6:.1f} M elements")
    for _ in range(args.warmup):
        opt.step(grads, clip_norm=5.0)
    t_dev = timed(lambda: opt.step(grads, clip_norm=5.0), args.steps)
    look = sum(1 for s in range(args.warmup + 1, args.warmup + args.steps + 1) if s % opt.k == 0) / args.steps
    nbytes = n_elem * 4 * (2 + 3 + 3 + 2 * look)
    say(f"device step (gpo_ranger_step, clip fused, host table build included): {t_dev * 1e3:.3f} ms per step over {args.steps} steps")
    say(f"    {nbytes / 1e9:.2f} GB per step needed ({look:.2f} of the steps are Lookahead steps) -> {nbytes / t_dev / 1e12:.2f} TB/s, "
        f"{nbytes / t_dev / HBM_PEAK:.2f} of the {HBM_PEAK / 1e12:g} TB/s BASELINE.md uses")
    # the baseline: the same step in plain torch ops, float32, on this GPU
    names = [opt.param_names[i] for i in sorted({opt._index[n] for n in grads})]
    ref = R.RangerRef({n: net.state_dict()[n].detach().clone() for n in names})
    g = {n: grads[n] for n in names}
    for _ in range(args.warmup):
        ref.step(g, clip_norm=5.0)
    t_ref = timed(lambda: ref.step(g, clip_norm=5.0), max(args.steps // 3, 3))
    say(f"ranger_ref in float32 on the same GPU, same tensors: {t_ref * 1e3:.3f} ms per step ({t_ref / t_dev:.1f} x the device step)")
    # what the next forward pays: the host repack of the updated weights
    dev = torch.device("cuda")
    net._reset_plans()
    t_pack = timed(lambda: net._pack(dev), 2)
    say(f"host repack of the fp32 parity model (PoseNet._pack, what the first forward after a step pays): {t_pack * 1e3:.0f} ms")
    say(f"    params_updated() was called {repack[0]} times by {args.warmup + args.steps} steps")


if __name__ == "__main__":
    main()
