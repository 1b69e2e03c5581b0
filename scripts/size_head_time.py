#!/usr/bin/env python3
"""Time the train-mode size head (gps_size_forward_save + gps_size_backward) on the device, next to the same function written in torch
ops on the same GPU, and PoseNet.train_step with and without size_head=.

    python scripts/size_head_time.py [--out FILE]                   the operator at B = 64, C = 1024, HW = 64, F = 128
    python scripts/size_head_time.py --train-step small|base [--out FILE]
                                                                    train_step, size_head=None against size_head={"seed": s}
    python scripts/size_head_time.py --kernel-count [--out FILE]    kernels of one forward-and-save and one backward (rocprofv3)

Method (the guide's): a 2 s settle of the same work, then the median of `--windows` windows of `--reps` calls each between device
events; the spread is the windows' min .. max.  The torch baseline is nn.BatchNorm1d in train mode, F.conv1d, an explicit mask and
autograd, float32, on the NHWC float16 feature converted and transposed as torch needs it (that conversion is inside its time).
size_head=None runs the code of the commit before this feature unchanged, so the first train_step line is that commit's figure on the
same box in the same process.
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
SHAPE = (64, 1024, 64, 128)


def windows(fn, reps, n, settle=2.0):
    import torch
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < settle:
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def operator_inputs():
    import numpy as np
    import torch

    import size_head_ref as R
    B, C, HW, F = SHAPE
    case = R.make_case(B, C, HW, F, "sqrt", seed=384)
    feat = torch.from_numpy(np.ascontiguousarray(case["feat"])).permute(0, 2, 1).contiguous().view(B, 8, 8, C).cuda().half()
    P = {k: torch.from_numpy(v).cuda() for k, v in case["params"].items()}
    return case, feat, P, torch.from_numpy(case["keep"]).cuda(), torch.from_numpy(case["g_out"]).cuda()


def operator(args, say):
    import torch
    import torch.nn.functional as Fn

    from givepose_amd import _lib, size_grad
    B, C, HW, F = SHAPE
    _, feat, P, keep, g = operator_inputs()
    say(f"device: {torch.cuda.get_device_name(0)}; B = {B}, C = {C}, HW = {HW}, F = {F}; feat NHWC float16; explicit mask")

    def fwd():
        return size_grad.size_forward_save(feat, P, keep=keep, nhwc=True)
    saved = fwd()

    def bwd():
        return size_grad.size_backward(P, saved, g, (B, C, 8, 8))

    def both():
        size_grad.size_backward(P, fwd(), g, (B, C, 8, 8))
    for name, fn in (("forward-and-save", fwd), ("backward", bwd), ("forward-and-save + backward", both)):
        med, lo, hi = windows(fn, args.reps, args.windows)
        say(f"{name}: median {med * 1e3:.1f} us per call ({lo * 1e3:.1f} .. {hi * 1e3:.1f} over {args.windows} windows of {args.reps} calls; host "
            f"wrapper and buffer allocation included)")
    say(f"launches: forward-and-save {_lib.GPS_FORWARD_LAUNCHES}, backward {_lib.GPS_BACKWARD_LAUNCHES}, whatever B (--kernel-count traces them)")
    bn = torch.nn.BatchNorm1d(F).cuda().train()
    params = {k: v.clone().requires_grad_() for k, v in P.items()}
    with torch.no_grad():
        bn.weight.copy_(P["bn1.weight"]), bn.bias.copy_(P["bn1.bias"])
    kf = keep.float()[:, :, None]

    def torch_both():
        x = feat.permute(0, 3, 1, 2).float().flatten(2).requires_grad_()
        pooled = x.max(dim=-1, keepdim=True).values
        y = bn(Fn.conv1d(pooled, params["conv1.weight"], params["conv1.bias"]))
        out = Fn.conv1d(Fn.relu(y) * kf / 0.8, params["conv2.weight"], params["conv2.bias"]).squeeze(2)
        torch.autograd.grad(out, [x, bn.weight, bn.bias, *[params[k] for k in size_grad.PARAM_KEYS[:4]]], g)
    med, lo, hi = windows(torch_both, args.reps, args.windows)
    say(f"the same function in torch ops + autograd, float32, same GPU: median {med * 1e3:.1f} us per call ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")


def train_step(args, say):
    import torch

    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, Ranger, synth
    import pose_loss_ref as PR
    small = args.train_step == "small"
    B = 2 if small else 64
    cfg = PoseNetConfig(convnext_depths=(1, 1, 1, 1)) if small else PoseNetConfig()
    net = PoseNet(cfg, dtype=torch.float32, seed=3).cuda()
    npb = synth.synth_batch(B, seed=11)
    npb["roi_mask_deform"] = npb["roi_mask"]
    _, gt = PR.make_inputs(B=B, P=256, seed=60)
    data = {k: torch.from_numpy(__import__("numpy").ascontiguousarray(v)) for k, v in {**npb, **gt}.items()}
    opt, pl = Ranger(net), PoseLoss()
    say(f"device: {torch.cuda.get_device_name(0)}; train_step, {'depths (1,1,1,1)' if small else 'ConvNeXt-Base'}, B = {B}, float32; each step ends "
        f"with params_updated(), so each includes the host repack of the next forward")
    seed = [0]

    def with_head():
        seed[0] += 1
        net.train_step(data, pl, opt, "cuda", size_head={"seed": seed[0]})
    runs = []
    for rnd in range(args.rounds):          # alternate, so that drift of the box lands on both
        for name, fn in (("size_head=None", lambda: net.train_step(data, pl, opt, "cuda")), ("size_head={'seed': s}", with_head)):
            fn()
            torch.cuda.synchronize()
            t = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            t.sort()
            runs.append((name, t[len(t) // 2]))
            say(f"round {rnd + 1} {name}: median {t[len(t) // 2]:.1f} ms per step ({t[0]:.1f} .. {t[-1]:.1f} over {args.steps} steps)")
    a, b = [t for n, t in runs if n == "size_head=None"], [t for n, t in runs if n != "size_head=None"]
    say(f"size_head=None medians {min(a):.1f} .. {max(a):.1f} ms; with the size head {min(b):.1f} .. {max(b):.1f} ms; difference of the means "
        f"{sum(b) / len(b) - sum(a) / len(a):+.2f} ms against a spread of {max(a) - min(a):.2f} ms of the size_head=None rounds")


def child():
    import torch

    from givepose_amd import size_grad
    B, C, HW, F = SHAPE
    _, feat, P, keep, g = operator_inputs()
    torch.cuda.synchronize()
    saved = size_grad.size_forward_save(feat, P, keep=keep, nhwc=True)
    size_grad.size_backward(P, saved, g, (B, C, 8, 8))
    torch.cuda.synchronize()


def kernel_count(say):
    from givepose_amd import _lib
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child"],
                       check=True, stdout=subprocess.DEVNULL)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    mine = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows
                  if any(k in r.get("Kernel_Name", "") for k in ("pool_kernel", "hidden_kernel", "out_kernel", "chan_kernel", "dw1_kernel", "dfeat_kernel")))
    for a, b, n in mine:
        say(f"    {(b - a) / 1e3:8.1f} us  {n[:100]}")
    fwd = sum(1 for _, _, n in mine if any(k in n for k in ("pool_kernel", "hidden_kernel", "out_kernel")))
    say(f"kernels of one forward-and-save: {fwd} (GPS_FORWARD_LAUNCHES = {_lib.GPS_FORWARD_LAUNCHES}); of one backward: {len(mine) - fwd} "
        f"(GPS_BACKWARD_LAUNCHES = {_lib.GPS_BACKWARD_LAUNCHES}); device time of the six {sum(b - a for a, b, _ in mine) / 1e3:.1f} us")
    if fwd != _lib.GPS_FORWARD_LAUNCHES or len(mine) - fwd != _lib.GPS_BACKWARD_LAUNCHES:
        raise SystemExit("the launch counts are not the documented constants")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--train-step", choices=("small", "base"), default=None)
    ap.add_argument("--kernel-count", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child()
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("size_head_time.py needs the GPU: a time from anywhere else says nothing")
    if args.kernel_count:
        return kernel_count(say)
    if args.train_step:
        return train_step(args, say)
    operator(args, say)


if __name__ == "__main__":
    main()
