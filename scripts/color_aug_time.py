#!/usr/bin/env python3
"""Time givepose_amd.ColorAugmenter on B = 64 frames of 480 x 640: seeded 'new' plans, and plans with every operation forced on.

    python scripts/color_aug_time.py [--out FILE] [--windows 7] [--calls 20] [--no-train-step] [--no-trace]      writes profiles/color_aug.txt

  device time per call   hip events around `--calls` calls (the host's draws, table build and upload are inside; where the host is the
                         slower side the figure holds its gaps), median of `--windows` windows with min .. max, after a warm-up
  kernel time            one `rocprofv3 --kernel-trace --stats` run of a child process of its own (--child): each operation alone on all
                         frames, a copy, then the forced and the seeded plans; the launches are told apart by their order, which the
                         parent recomputes from the plans
  bytes                  what the stage needs from the shapes: 6 H W per frame that takes part in an apply launch (read + write),
                         3 H W per Contrast frame of a reduction; over kernel time, next to HBM_PEAK (8 TB/s spec; MI355X_MICROARCH.md
                         gives 6.3 TB/s as what a float4 copy reaches)
  share of a train_step  PoseNet.train_step at B = 64 (ConvNeXt-Base, float32, device repack, Ranger), median of 5 steps, same process
  host figure            Pillow on the same forced plans on 8 frames where Pillow is importable: a CPU number of the box, one core
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, H, W = 64, 480, 640
HBM_PEAK = 8e12
CHILD_CALLS = 5
SINGLE = (("sharpness", 1, 1.5), ("contrast", 2, 1.3), ("brightness", 3, 0.8), ("color", 4, 2.0))


def forced_plan(seed):
    """Every operation on, in a drawn order, factors in the ranges of 'new'."""
    from givepose_amd.color_aug import NEW_CHILDREN
    r = np.random.Generator(np.random.Philox(key=[seed, 0x6363]))
    order = np.argsort(r.random((B, 4)), axis=1)
    lo, hi = (np.array([c[2][i] for c in NEW_CHILDREN]) for i in (0, 1))
    fac = (lo + (hi - lo) * r.random((B, 4))).astype(np.float32)
    return {"ops": (order + 1).astype(np.int32), "factors": np.take_along_axis(fac, order, 1)}


def child_plans():
    """(label, plan) of every call the traced child makes, CHILD_CALLS times each, in order."""
    from givepose_amd import color_aug_draws
    plans = [(name, {"ops": np.full((B, 1), code, np.int32), "factors": np.full((B, 1), f, np.float32)}) for name, code, f in SINGLE]
    plans.append(("copy", {"ops": np.zeros((B, 1), np.int32), "factors": np.ones((B, 1), np.float32)}))
    plans.append(("forced", forced_plan(0)))
    plans.append(("seeded", color_aug_draws(0, B)))
    return plans


def launches_of(plan):
    """[(kernel, frames taking part)] in launch order, from the plan alone."""
    from givepose_amd import _lib
    from givepose_amd.color_aug import stage_tables
    rows, _ = stage_tables(plan["ops"], plan["factors"])
    seq = []
    for t in rows:
        nc = int((t[:, 0] == _lib.GPCA_OP_CONTRAST).sum())
        if nc:
            seq.append(("luma", nc))
        seq.append(("apply", int((t[:, 0] != _lib.GPCA_OP_SKIP).sum())))
    return seq


def make_frames():
    import torch
    g = torch.Generator(device="cuda").manual_seed(1)
    return torch.randint(0, 256, (B, H, W, 3), device="cuda", dtype=torch.uint8, generator=g)


def child():
    import torch
    from givepose_amd import ColorAugmenter
    frames, aug = make_frames(), ColorAugmenter(H, W, "cuda")
    out = torch.empty_like(frames)
    aug(frames, plan=forced_plan(1), out=out)            # warm-up: code objects, buffers
    torch.cuda.synchronize()
    for _, plan in child_plans():
        for _ in range(CHILD_CALLS):
            aug(frames, plan=plan, out=out)
        torch.cuda.synchronize()


def traced(say):
    expect = []
    for label, plan in child_plans():
        expect += [(label, k, n) for k, n in launches_of(plan)] * CHILD_CALLS
    warm = len(launches_of(forced_plan(1)))
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                        "--child"], check=True, stdout=subprocess.DEVNULL)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    mine = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows if "coloraug_" in r.get("Kernel_Name", ""))
    mine = mine[warm:]
    if len(mine) != len(expect):
        raise SystemExit(f"the trace holds {len(mine)} coloraug launches after the warm-up, the plans say {len(expect)}")
    acc = {}
    for (a, b, name), (label, kind, n) in zip(mine, expect):
        assert ("luma" in name) == (kind == "luma"), (name, label, kind)
        e = acc.setdefault((label, kind), [0.0, 0, 0])
        e[0] += (b - a) * 1e-3
        e[1] += 1
        e[2] += n
    say(f"kernel time, rocprofv3 --kernel-trace --stats, a run of its own, {CHILD_CALLS} calls per plan after a warm-up call; bytes from the shapes")
    say(f"  {'plan':10s} {'kernel':6s} {'launches/call':>13s} {'us/launch':>10s} {'frames/launch':>13s} {'MB/launch':>10s} {'TB/s':>6s} {'of 8 TB/s':>9s}")
    per_call = {}
    for (label, kind), (us, cnt, n) in acc.items():
        nbytes = n / cnt * H * W * (3 if kind == "luma" else 6)
        t = us / cnt
        per_call[label] = per_call.get(label, 0.0) + us / CHILD_CALLS
        say(f"  {label:10s} {kind:6s} {cnt / CHILD_CALLS:13.1f} {t:10.1f} {n / cnt:13.1f} {nbytes / 1e6:10.1f} {nbytes / t / 1e6:6.2f} {nbytes / (t * 1e-6) / HBM_PEAK:9.2f}")
    say("  kernel time per call: " + ", ".join(f"{k} {v:.1f} us" for k, v in per_call.items()))
    return per_call


def windows(fn, n_windows, calls):
    import torch
    for _ in range(calls):
        fn(0)
    torch.cuda.synchronize()
    t = []
    for w in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(calls):
            fn(w * calls + i)
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) / calls)
    return sorted(t)[len(t) // 2], min(t), max(t)


def train_step_ms():
    import torch

    import pose_loss_ref as PR
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, Ranger, synth
    net = PoseNet(PoseNetConfig(), dtype=torch.float32, seed=3).cuda().set_repack("device")
    npb = synth.synth_batch(B, seed=11)
    npb["roi_mask_deform"] = npb["roi_mask"]
    _, gt = PR.make_inputs(B=B, P=256, seed=60)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**npb, **gt}.items()}
    opt, pl = Ranger(net), PoseLoss()
    for _ in range(2):
        net.train_step(data, pl, opt, "cuda")
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        net.train_step(data, pl, opt, "cuda")
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return sorted(t)[2], min(t), max(t)


def pillow_ms(plan, frames, n=8):
    try:
        from PIL import Image, ImageEnhance
    except ImportError:
        return None
    enh = {1: ImageEnhance.Sharpness, 2: ImageEnhance.Contrast, 3: ImageEnhance.Brightness, 4: ImageEnhance.Color}
    t0 = time.perf_counter()
    for i in range(n):
        im = Image.fromarray(frames[i])
        for code, f in zip(plan["ops"][i], plan["factors"][i]):
            if code:
                im = enh[int(code)](im).enhance(float(f))
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_aug.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("color_aug_time.py needs the GPU: a time from anywhere else says nothing")
    out = open(args.out, "w") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    from givepose_amd import ColorAugmenter, color_aug_draws
    say(f"device: {torch.cuda.get_device_name(0)}; ColorAugmenter on B = {B} frames of {H} x {W} x 3 uint8 ({B * H * W * 3 / 1e6:.1f} MB)")
    if not args.no_trace:
        traced(say)
    frames, aug = make_frames(), ColorAugmenter(H, W, "cuda")
    dst = torch.empty_like(frames)
    forced = [forced_plan(s) for s in range(8)]
    res = {"seeded 'new' plans (prob 0.8)": windows(lambda i: aug(frames, seed=i, out=dst), args.windows, args.calls),
           "every operation forced on": windows(lambda i: aug(frames, plan=forced[i % 8], out=dst), args.windows, args.calls)}
    say(f"device time per call, hip events around {args.calls} calls (host draws, table build and upload inside), median of {args.windows} "
        f"windows (min .. max) after {args.calls} warm-up calls")
    for k, (med, lo, hi) in res.items():
        say(f"  {k:32s} {med * 1e3:8.1f} us ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")
    ops = np.concatenate([color_aug_draws(s, B)["ops"] for s in range(args.windows * args.calls)])
    say(f"  the seeded plans of those calls hold {np.mean((ops != 0).sum(1)):.2f} operations per frame on average, "
        f"{np.mean([len(launches_of(color_aug_draws(s, B))) for s in range(20)]):.1f} launches per call")
    host = pillow_ms(forced[0], frames[:8].cpu().numpy())
    if host is None:
        say("host figure: Pillow is not importable here: not measured")
    else:
        import PIL
        say(f"host figure: Pillow {PIL.__version__} on the forced plans, one core of this box (a CPU number): {host:.1f} ms per frame, "
            f"{host * B:.0f} ms per {B} frames")
    if not args.no_train_step:
        del frames, dst, aug
        torch.cuda.empty_cache()
        med, lo, hi = train_step_ms()
        say(f"train_step, ConvNeXt-Base, B = {B}, float32 network, set_repack('device'), Ranger: {med:.1f} ms (median of 5 steps, {lo:.1f} .. {hi:.1f})")
        for k, (m, _, _) in res.items():
            say(f"  a call with {k} is {100 * m / med:.2f} % of it")


if __name__ == "__main__":
    main()
