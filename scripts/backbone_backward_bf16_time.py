#!/usr/bin/env python3
"""Time the backbone's forward_save + backward in both precisions on one MI355X and write profiles/backbone_backward_bf16.txt.

Run on the GPU box:  python scripts/backbone_backward_bf16_time.py [--out profiles/backbone_backward_bf16.txt] [--no-profile]
                                                                   [--no-train-step] [--deviations FILE]

The sibling of scripts/backbone_backward_time.py for PoseNet.set_backward_precision (include/givepose_bbgrad_bf16.h).  The fp32 mode
of this tree is the code of before, so it is the baseline.  ConvNeXt-Base at 256 x 256, B = 4 and B = 64, preallocated buffers, one
saved table shared by both modes (its shapes and dtypes do not depend on the mode).  Discipline: two seconds of back-to-back pairs to
settle, then three rounds that alternate the modes on the one box, each a window of at least one second between device events; per
mode the median round, with the spread.  bf16 has to beat fp32 by more than the spread of the fp32 rounds.

The per-kernel split comes from one `rocprofv3 --kernel-trace --stats` run of its own at B = 64 in bf16 mode (a fresh child process,
started before this process touches the device).  train_step (ConvNeXt-Base, B = 64, float32 network, device repack) is timed in
alternating rounds too.  --deviations: the `-s` output of tests/test_bb_bf16_gpu.py, whose ratio lines are appended.
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import backbone_backward_time as base  # noqa: E402  (window, the rocprofv3 run and its table)

S_NET = base.S_NET
MODES = ("fp32", "bf16")


def setup(B, first="fp32"):
    """`first`: the precision of the run that allocates.
    -> {mode: one forward_save + backward pair on preallocated buffers}, what keeps them alive, (workspace bytes per mode, saved bytes)."""
    import numpy as np
    import torch
    import bb_backward_ref as R
    from givepose_amd import PoseNetConfig, _lib, bb_grad
    cfg = PoseNetConfig()
    dims, depths = cfg.convnext_dims, cfg.convnext_depths
    L = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    params = {k: torch.from_numpy(v).cuda() for k, v in R.bb_params(dims, depths).items()}
    r = np.random.Generator(np.random.Philox(key=[90 + B, 0xBB]))
    img = torch.from_numpy(r.standard_normal((B, 3, S_NET, S_NET)).astype(np.float32)).cuda()
    g = torch.from_numpy(r.standard_normal((B, dims[-1], S_NET // 32, S_NET // 32)).astype(np.float32)).cuda()
    saved, feat = bb_grad.backbone_forward_save(img, params, cfg, precision=first)
    grads, d_img = bb_grad.backbone_backward(params, saved, img, g, cfg, precision=first)
    shapes = bb_grad.param_shapes(cfg)
    pt, gt = bb_grad._table(params, shapes, dev, "params"), bb_grad._table(grads, shapes, dev, "grads")
    vt = bb_grad._table(saved, bb_grad.saved_shapes(cfg, B, S_NET), dev, "saved")
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    di, de, n = ints(dims), ints(depths), len(dims)
    keep, pairs, sizes = [params, img, g, saved, feat, grads, d_img, pt, gt, vt], {}, {}
    for mode in MODES:
        prec = bb_grad.PRECISIONS[mode]
        nf, nb = L.gpbm_backbone_forward_workspace(di, de, n, B, S_NET, prec), L.gpbm_backbone_backward_workspace(di, de, n, B, S_NET, prec)
        wf, wb = torch.empty(nf // 4 + 64, device=dev), torch.empty(nb // 4 + 64, device=dev)
        keep += [wf, wb]
        sizes[mode] = (nf, nb)

        def pair(prec=prec, nf=nf, nb=nb, wf=wf, wb=wb):
            _lib.check(L.gpbm_backbone_forward_save(img.data_ptr(), pt, di, de, n, B, S_NET, vt, feat.data_ptr(), wf.data_ptr(), nf, stream(), prec),
                       "gpbm_backbone_forward_save")
            _lib.check(L.gpbm_backbone_backward(pt, vt, img.data_ptr(), g.data_ptr(), di, de, n, B, S_NET, gt, d_img.data_ptr(), wb.data_ptr(), nb,
                                                stream(), prec), "gpbm_backbone_backward")
        pairs[mode] = pair
    return pairs, keep, (sizes, bb_grad.saved_bytes(cfg, B, S_NET))


def alternate(fns, rounds=3, settle=2.0, seconds=1.0):
    """{name: fn} -> {name: (median, min, max) ms per call} over `rounds` rounds that run the names in turn."""
    for fn in fns.values():
        base.window(fn, settle / len(fns))
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(base.window(fn, seconds))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def verdict(res, what):
    gain, spread = res["fp32"][0] - res["bf16"][0], res["fp32"][2] - res["fp32"][1]
    return (f"{what}: bf16 is {gain:+.3f} ms ({res['fp32'][0] / res['bf16'][0]:.2f}x) against a spread of {spread:.3f} ms of the fp32 rounds"
            + ("" if gain > spread else ": NOT beyond the spread"))


def profile_child():
    """What the rocprofv3 run executes: three forward_save + backward pairs at B = 64 in bf16 mode (setup's own, then two)."""
    import torch
    pairs, keep, _ = setup(64, first="bf16")
    pairs["bf16"]()
    pairs["bf16"]()
    torch.cuda.synchronize()


def train_step_times(say, rounds=3, steps=5):
    import numpy as np
    import torch
    import pose_loss_ref as PR
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, Ranger, synth
    B = 64
    net = PoseNet(PoseNetConfig(), dtype=torch.float32, seed=3).cuda().set_repack("device")
    npb = synth.synth_batch(B, seed=11)
    npb["roi_mask_deform"] = npb["roi_mask"]
    _, gt = PR.make_inputs(B=B, P=256, seed=60)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**npb, **gt}.items()}
    opt, pl = Ranger(net), PoseLoss()
    runs = {m: [] for m in MODES}
    for rnd in range(rounds):
        for mode in MODES:
            net.set_backward_precision(mode)
            net.train_step(data, pl, opt, "cuda")
            torch.cuda.synchronize()
            t = []
            for _ in range(steps):
                t0 = time.perf_counter()
                net.train_step(data, pl, opt, "cuda")
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            runs[mode].append(sorted(t)[len(t) // 2])
    res = {m: (sorted(v)[len(v) // 2], min(v), max(v)) for m, v in runs.items()}
    say(f"train_step, ConvNeXt-Base, B = {B}, float32 network, set_repack('device'), size_head=None: ms per step, median of {rounds} alternating "
        f"rounds of {steps} steps (min .. max of the rounds' medians)")
    for m in MODES:
        say(f"  set_backward_precision({m!r}): {res[m][0]:8.1f} ({res[m][1]:.1f} .. {res[m][2]:.1f})")
    say("  " + verdict(res, "train_step"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backbone_backward_bf16.txt"))
    ap.add_argument("--deviations", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    a = ap.parse_args()
    if a.profile_child:
        return profile_child()
    base.__file__ = os.path.abspath(__file__)      # the rocprofv3 run starts this script's child
    breakdown = [] if a.no_profile else base.kernel_breakdown(pairs=3)      # first: the child runs before this process opens the device
    import torch
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
    say(f"backbone forward_save + backward (ConvNeXt-Base, {S_NET} x {S_NET}) in both precisions, milliseconds per pair: median of three "
        f"alternating 1 s rounds (min .. max) ({torch.cuda.get_device_name(0)})")
    say("   B   fp32 (the code of before)        bf16                             saved MB   workspace MB forward / backward: fp32, bf16")
    f = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    verdicts = []
    for B in (4, 64):
        pairs, keep, (sizes, ns) = setup(B)
        res = alternate(pairs)
        say(f"{B:4d}   {f(res['fp32'])}   {f(res['bf16'])}   {ns / 1e6:.1f}   " + ", ".join(f"{sizes[m][0] / 1e6:.1f} / {sizes[m][1] / 1e6:.1f}" for m in MODES))
        verdicts.append(verdict(res, f"B = {B}"))
        del pairs, keep
        torch.cuda.empty_cache()
    for v in verdicts:
        say(v)
    say("")
    if not a.no_train_step:
        train_step_times(say)
        say("")
    for ln in breakdown:
        say(ln)
    if a.deviations and os.path.exists(a.deviations):
        say("")
        say("ratios printed by tests/test_bb_bf16_gpu.py (error / bound of the kernel; device figure / CPU float32-with-bf16-hook figure):")
        with open(a.deviations) as fh:
            for ln in fh:
                if "largest ratio" in ln or "/ bound" in ln:
                    say("  " + ln.strip().lstrip("."))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
