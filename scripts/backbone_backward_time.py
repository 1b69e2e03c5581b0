#!/usr/bin/env python3
"""Time the backbone backward (gpb_backbone_forward_save + gpb_backbone_backward) on one MI355X and write profiles/backbone_backward.txt.

Run on the GPU box:  python scripts/backbone_backward_time.py [--out profiles/backbone_backward.txt] [--deviations FILE] [--no-profile]

Milliseconds per call at B = 4 and B = 64 for the full network (ConvNeXt-Base, 256 x 256), fp32, on preallocated buffers (what a
training step would issue).  Discipline, as scripts/enc_backward_time.py: about two seconds of back-to-back calls first, then three
windows of at least one second each between device events; the median window is reported, with the spread.

Next to each figure stands the contraction floor: the FLOPs of fc1, fc2 and the patch convs (the forward's once, the backward's dX and
dW twice) at the 157.3 TFLOP/s fp32 matrix peak.  No threshold is asserted: this is the untuned baseline a later change has to beat.

The per-kernel breakdown comes from one `rocprofv3 --kernel-trace --stats` run of its own at B = 64 (a fresh child process, started
before this process touches the device).  --deviations: a text file (the `-s` output of tests/test_bb_backward_gpu.py) whose ratio
lines are appended.
"""
import argparse
import csv
import ctypes
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MATRIX_FP32_FLOPS = 157.3e12
S_NET = 256


def contraction_flop_forward(cfg):
    """FLOP of one crop's contractions in the forward (the backward has dX and dW: twice this)."""
    dims, depths = cfg.convnext_dims, cfg.convnext_depths
    f = 2 * (S_NET // 4) ** 2 * 48 * dims[0]
    for s, (C, n) in enumerate(zip(dims, depths)):
        rows = (S_NET // (4 << s)) ** 2
        if s:
            f += 2 * rows * 4 * dims[s - 1] * C
        f += n * 2 * 2 * rows * C * 4 * C
    return f


def setup(B):
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
    saved, feat = bb_grad.backbone_forward_save(img, params, cfg)
    grads, d_img = bb_grad.backbone_backward(params, saved, img, g, cfg)
    shapes = bb_grad.param_shapes(cfg)
    pt, gt = bb_grad._table(params, shapes, dev, "params"), bb_grad._table(grads, shapes, dev, "grads")
    vt = bb_grad._table(saved, bb_grad.saved_shapes(cfg, B, S_NET), dev, "saved")
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    di, de, n = ints(dims), ints(depths), len(dims)
    nf, nb = L.gpb_backbone_forward_workspace(di, de, n, B, S_NET), L.gpb_backbone_backward_workspace(di, de, n, B, S_NET)
    wf, wb = torch.empty(nf // 4 + 64, device=dev), torch.empty(nb // 4 + 64, device=dev)
    keep = (params, img, g, saved, feat, grads, d_img, wf, wb, pt, gt, vt)

    def fwd():
        _lib.check(L.gpb_backbone_forward_save(img.data_ptr(), pt, di, de, n, B, S_NET, vt, feat.data_ptr(), wf.data_ptr(), nf, stream()),
                   "gpb_backbone_forward_save")

    def bwd():
        _lib.check(L.gpb_backbone_backward(pt, vt, img.data_ptr(), g.data_ptr(), di, de, n, B, S_NET, gt, d_img.data_ptr(), wb.data_ptr(), nb,
                                           stream()), "gpb_backbone_backward")
    return fwd, bwd, keep, (nf, nb, bb_grad.saved_bytes(cfg, B, S_NET))


def window(fn, seconds):
    """Calls of fn between two device events until `seconds` of host time have passed -> milliseconds per call."""
    import time

    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, t0 = 0, time.perf_counter()
    a.record()
    while time.perf_counter() - t0 < seconds:
        fn()
        n += 1
        torch.cuda.synchronize()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def measure(fn):
    window(fn, 2.0)                                  # settle
    w = sorted(window(fn, 1.0) for _ in range(3))
    return w[1], w[0], w[2]


def profile_child():
    """What the rocprofv3 run executes: two forward_save + backward pairs at B = 64 (setup's own, then one)."""
    import torch
    fwd, bwd, keep, _ = setup(64)
    fwd()
    bwd()
    torch.cuda.synchronize()


def kernel_breakdown(pairs=2):
    """One rocprofv3 --kernel-trace --stats run of a fresh child -> lines (kernel, calls, total ms per pair, share)."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--profile-child"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return [f"per-kernel breakdown: not measured (rocprofv3 exit {r.returncode}, {len(files)} stats files): {r.stderr.strip()[-300:]}"]
        rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda x: -float(x["TotalDurationNs"]))
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    out = [f"per-kernel breakdown at B = 64 (rocprofv3 --kernel-trace --stats, a run of its own: {pairs} forward_save + backward pairs; "
           f"ms are per pair; sum of kernel time {total / pairs * 1e-6:.2f} ms per pair)",
           "     ms/pair   share   calls/pair   kernel"]
    for x in rows:
        name = x["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
        t = float(x["TotalDurationNs"])
        if t / total < 0.002:
            continue
        out.append(f"  {t / pairs * 1e-6:9.3f}   {100 * t / total:5.1f}%   {int(x['Calls']) / pairs:8.1f}     {name[:150]}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backbone_backward.txt"))
    ap.add_argument("--deviations", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    a = ap.parse_args()
    if a.profile_child:
        return profile_child()
    breakdown = [] if a.no_profile else kernel_breakdown()      # first: the child runs before this process opens the device
    import torch
    from givepose_amd import PoseNetConfig
    ff = contraction_flop_forward(PoseNetConfig())
    fl = ff / MATRIX_FP32_FLOPS * 1e3      # ms per crop
    lines = [f"backbone backward (ConvNeXt-Base, {S_NET} x {S_NET}), milliseconds per call, median of three 1 s windows (min .. max) "
             f"({torch.cuda.get_device_name(0)}; fp32)",
             f"floor per crop: contractions {ff * 1e-9:.2f} GFLOP forward, twice that backward, at {MATRIX_FP32_FLOPS * 1e-12:.1f} TFLOP/s = "
             f"{fl:.4f} / {2 * fl:.4f} ms",
             "   B   gpb_backbone_forward_save (floor)   gpb_backbone_backward (floor)   saved MB   workspace MB forward / backward"]
    f = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    for B in (4, 64):
        fwd, bwd, keep, (nf, nb, ns) = setup(B)
        tf, tb = measure(fwd), measure(bwd)
        lines.append(f"{B:4d}   {f(tf)} ({B * fl:.3f}, {tf[0] / (B * fl):.1f}x)   {f(tb)} ({2 * B * fl:.3f}, {tb[0] / (2 * B * fl):.1f}x)   "
                     f"{ns / 1e6:.1f}   {nf / 1e6:.1f} / {nb / 1e6:.1f}")
        del fwd, bwd, keep
        torch.cuda.empty_cache()
    lines += [""] + breakdown
    if a.deviations and os.path.exists(a.deviations):
        lines += ["", "ratios printed by tests/test_bb_backward_gpu.py (device figure / CPU float32 figure, or error / bound):"]
        with open(a.deviations) as fh:
            lines += ["  " + ln.strip().lstrip(".") for ln in fh if "largest ratio" in ln or "/ bound" in ln]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
