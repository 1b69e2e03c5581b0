#!/usr/bin/env python3
"""Time the coordinate head's forward_save + backward in both precisions on one MI355X and write profiles/xyz_backward_bf16.txt.

Run on the GPU box:  python scripts/xyz_backward_bf16_time.py [--out profiles/xyz_backward_bf16.txt] [--no-profile] [--no-train-step]
                                                              [--deviations FILE]

The sibling of scripts/xyz_head_backward_time.py for PoseNet.set_backward_precision(mode, xyz_heads=) (include/givepose_xyzgrad_bf16.h).
The fp32 mode of this tree is the code of before, so it is the baseline.  One head at Cin 512, H0 8 (xyz_deform_head at the network's
size), B = 4 and B = 64, preallocated buffers, one saved table shared by both modes.  Discipline: two seconds of back-to-back calls to
settle, then three rounds that alternate the modes on the one box, each a window of at least one second between device events; per
mode the median round, with the spread.  bf16 has to beat fp32 by more than the spread of the fp32 rounds.

The staging specialisations of the bf16 kernel (csrc/grad_gemm_bf16.hpp: Bf16Wide for Tr<Nchw> as A, Bf16Rows for the stride-1 window
as A) are timed against an investigation build that switches them off, when that library lies next to the product library:
    GP_BUILD_TAG=wide0 GP_EXTRA_HIPCC_FLAGS=-DGP_BF16_WIDE_MASK=0 python -m givepose_amd.build
on dW (the first), forward and dX (the second) of the stride-1 conv at the head's three resolutions, alternating in this one process;
the results of the two builds are compared bit for bit.  Without that library the section says "not measured".

The per-kernel split comes from one `rocprofv3 --kernel-trace --stats` run of its own at B = 64 in bf16 mode (a fresh child process,
started before this process touches the device).  train_step (ConvNeXt-Base, B = 64, float32 network, device repack) is timed in
alternating rounds in three settings.  --deviations: the `-s` output of tests/test_xyz_bf16_gpu.py, whose ratio lines are appended.
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

import xyz_head_backward_time as base  # noqa: E402  (window, the rocprofv3 run and its table)

CIN, H0 = base.CIN, base.H0
MODES = ("fp32", "bf16")


def setup(B, first="fp32"):
    """-> {mode: {"forward_save", "backward", "both": calls on preallocated buffers}}, what keeps them alive, {mode: workspace bytes}."""
    import torch
    import xyz_backward_ref as R
    from givepose_amd import _lib, xyz_grad
    L = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    params = {k: torch.from_numpy(v).cuda() for k, v in R.head_params(CIN).items()}
    feat, g = (torch.from_numpy(x).cuda() for x in R.make_inputs(B, CIN, H0, seed=90 + B))
    saved = xyz_grad.xyz_forward_save(feat, params, precision=first)
    grads, g_feat = xyz_grad.xyz_backward(params, saved, feat, g, precision=first)
    pw, sv = xyz_grad._params_struct(params, CIN, "params"), xyz_grad._saved_struct(saved, B, CIN, H0)
    pg = xyz_grad._params_struct(grads, CIN, "grads")
    keep, calls, sizes = [params, feat, g, saved, grads, g_feat, pw, sv, pg], {}, {}
    for mode in MODES:
        prec = xyz_grad.PRECISIONS[mode]
        nf, nb = L.gpxm_xyz_forward_workspace(B, CIN, H0, prec), L.gpxm_xyz_backward_workspace(B, CIN, H0, prec)
        wf, wb = torch.empty(nf // 4 + 64, device=dev), torch.empty(nb // 4 + 64, device=dev)
        keep += [wf, wb]
        sizes[mode] = (nf, nb)

        def fwd(prec=prec, nf=nf, wf=wf):
            _lib.check(L.gpxm_xyz_forward_save(feat.data_ptr(), ctypes.byref(pw), B, CIN, H0, ctypes.byref(sv), wf.data_ptr(), nf, stream(), prec),
                       "gpxm_xyz_forward_save")

        def bwd(prec=prec, nb=nb, wb=wb):
            _lib.check(L.gpxm_xyz_backward(ctypes.byref(pw), ctypes.byref(sv), feat.data_ptr(), g.data_ptr(), B, CIN, H0, ctypes.byref(pg),
                                           g_feat.data_ptr(), wb.data_ptr(), nb, stream(), prec), "gpxm_xyz_backward")

        def both(fwd=fwd, bwd=bwd):
            fwd()
            bwd()
        calls[mode] = {"forward_save": fwd, "backward": bwd, "both": both}
    return calls, keep, sizes


def alternate(fns, rounds=3, settle=2.0, seconds=1.0):
    """{name: fn} -> {name: (median, min, max) ms per call} over `rounds` rounds that run the names in turn."""
    for fn in fns.values():
        base.window(fn, settle / len(fns))
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(base.window(fn, seconds))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def verdict(res, what, a="fp32", b="bf16"):
    gain, spread = res[a][0] - res[b][0], res[a][2] - res[a][1]
    return (f"{what}: {b} is {gain:+.3f} ms ({res[a][0] / res[b][0]:.2f}x) against a spread of {spread:.3f} ms of the {a} rounds"
            + ("" if gain > spread else ": NOT beyond the spread"))


def profile_child():
    """What the rocprofv3 run executes: eight forward_save + backward pairs at B = 64 in bf16 mode (setup's own, then seven)."""
    import torch
    calls, keep, _ = setup(64, first="bf16")
    for _ in range(7):
        calls["bf16"]["both"]()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the staging specialisations
GENERIC = "generic fetch (GP_BF16_WIDE_MASK=0)"
SPECIAL = "this tree"


def staging_ab(say, B=64):
    import numpy as np
    import torch
    from givepose_amd import _lib
    path = os.path.join(ROOT, "givepose_amd", "libgivepose_hip_wide0.so")
    if not os.path.exists(path):
        say(f"staging specialisations: not measured ({os.path.basename(path)} is not built; see this script's docstring)")
        return
    generic = ctypes.CDLL(path)
    for name in ("gpxm_conv3x3s1_workspace", "gpxm_conv3x3s1_forward", "gpxm_conv3x3s1_backward"):
        getattr(generic, name).argtypes, getattr(generic, name).restype = _lib.XYZGRAD_BF16_PROTOTYPES[name]
    libs = {GENERIC: generic, SPECIAL: _lib.load()}
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    say(f"staging specialisations of gemm_bf16_kernel on the three contractions of the 3x3 stride-1 conv (256 -> 256 channels, B = {B}, bf16), this "
        "tree against a build with the element-wise fetch only: ms per call, median of three alternating 1 s rounds (min .. max); the two "
        "builds give equal bits")
    say("  dW = <Tr<Nchw>, WindowS1, EpRow>: Tr<Nchw> as A, four pixels of a channel in one 16-byte load")
    say("  forward = <WindowS1, MatCol, EpNchw>, dX = <WindowS1, WeightDx, EpNchw>: the window as A, tap mask and pixel address formed once per thread")
    for H in (16, 32, 64):
        r = np.random.Generator(np.random.Philox(key=[H, 0xAB]))
        dY, X = (torch.from_numpy(r.standard_normal((B, 256, H, H)).astype(np.float32)).cuda() for _ in range(2))
        Wt = torch.from_numpy(r.standard_normal((256, 256, 3, 3)).astype(np.float32) / 48).cuda()
        for what in ("dW", "forward", "dX"):
            fns, outs, keep = {}, {}, []
            for label, lib in libs.items():
                nb = lib.gpxm_conv3x3s1_workspace(B, 256, 256, H, 1)
                ws = torch.empty(nb // 4 + 64, device=dev)
                out = torch.empty((256, 256, 3, 3) if what == "dW" else (B, 256, H, H), device=dev)
                keep.append(ws)
                outs[label] = out

                def fn(lib=lib, nb=nb, ws=ws, out=out):
                    if what == "forward":
                        rc = lib.gpxm_conv3x3s1_forward(X.data_ptr(), Wt.data_ptr(), B, 256, 256, H, out.data_ptr(), ws.data_ptr(), nb, stream(), 1)
                    elif what == "dW":
                        rc = lib.gpxm_conv3x3s1_backward(dY.data_ptr(), X.data_ptr(), None, B, 256, 256, H, None, out.data_ptr(), ws.data_ptr(), nb,
                                                         stream(), 1)
                    else:
                        rc = lib.gpxm_conv3x3s1_backward(dY.data_ptr(), None, Wt.data_ptr(), B, 256, 256, H, out.data_ptr(), None, ws.data_ptr(), nb,
                                                         stream(), 1)
                    assert rc == 0, rc
                fns[label] = fn
            res = alternate(fns)
            torch.cuda.synchronize()
            assert torch.equal(outs[GENERIC].view(torch.int32), outs[SPECIAL].view(torch.int32)) and bool(outs[SPECIAL].abs().max() > 0)
            say(f"  H = {H:2d} {what:8s}" + "; ".join(f"{k} {v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})" for k, v in res.items()))
            say("    " + verdict(res, f"H = {H} {what}", a=GENERIC, b=SPECIAL))
            del fns, outs, keep
        del dY, X, Wt
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ train_step
SETTINGS = (("all fp32", ("fp32", "fp32")), ("backbone bf16", ("bf16", "fp32")), ("backbone + heads bf16", ("bf16", "bf16")))


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
    runs = {k: [] for k, _ in SETTINGS}
    for rnd in range(rounds):
        for name, (mode, heads) in SETTINGS:
            net.set_backward_precision(mode, xyz_heads=heads)
            net.train_step(data, pl, opt, "cuda")
            torch.cuda.synchronize()
            t = []
            for _ in range(steps):
                t0 = time.perf_counter()
                net.train_step(data, pl, opt, "cuda")
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            runs[name].append(sorted(t)[len(t) // 2])
    res = {m: (sorted(v)[len(v) // 2], min(v), max(v)) for m, v in runs.items()}
    say(f"train_step, ConvNeXt-Base, B = {B}, float32 network, set_repack('device'), size_head=None: ms per step, median of {rounds} alternating "
        f"rounds of {steps} steps (min .. max of the rounds' medians)")
    for name, (mode, heads) in SETTINGS:
        say(f"  set_backward_precision({mode!r}, xyz_heads={heads!r}) ({name}): {res[name][0]:8.1f} ({res[name][1]:.1f} .. {res[name][2]:.1f})")
    say("  " + verdict(res, "train_step", a="backbone bf16", b="backbone + heads bf16"))
    say("  " + verdict(res, "train_step", a="all fp32", b="backbone + heads bf16"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xyz_backward_bf16.txt"))
    ap.add_argument("--deviations", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    a = ap.parse_args()
    if a.profile_child:
        return profile_child()
    base.__file__ = os.path.abspath(__file__)      # the rocprofv3 run starts this script's child
    breakdown = [] if a.no_profile else base.kernel_breakdown(pairs=8)      # first: the child runs before this process opens the device
    import torch
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
    say(f"coordinate head forward_save + backward (Cin {CIN}, H0 {H0}) in both precisions, milliseconds per call: median of three alternating "
        f"1 s rounds (min .. max) ({torch.cuda.get_device_name(0)}; buffers resident on the device)")
    f = lambda t: f"{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    verdicts = []
    for B in (4, 64):
        calls, keep, sizes = setup(B)
        say(f"B = {B}   workspace MB forward / backward: " + ", ".join(f"{m} {sizes[m][0] / 1e6:.1f} / {sizes[m][1] / 1e6:.1f}" for m in MODES))
        for what in ("forward_save", "backward", "both"):
            res = alternate({m: calls[m][what] for m in MODES})
            say(f"  {what:13s} fp32 (the code of before) {f(res['fp32'])}   bf16 {f(res['bf16'])}")
            verdicts.append(verdict(res, f"B = {B} {what}"))
        del calls, keep
        torch.cuda.empty_cache()
    for v in verdicts:
        say(v)
    say("")
    staging_ab(say)
    say("")
    if not a.no_train_step:
        train_step_times(say)
        say("")
    for ln in breakdown:
        say(ln.replace("at B = 64 (", "at B = 64 in bf16 mode ("))
    if a.deviations and os.path.exists(a.deviations):
        say("")
        say("ratios printed by tests/test_xyz_bf16_gpu.py (error / bound of the contractions; device figure / CPU float32-with-bf16-hook figure):")
        with open(a.deviations) as fh:
            for ln in fh:
                if "largest ratio" in ln or "/ bound" in ln or "pre0 differs" in ln:
                    say("  " + ln.strip().lstrip("."))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
