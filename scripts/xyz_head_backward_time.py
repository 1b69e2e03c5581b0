#!/usr/bin/env python3
"""Time the coordinate-head backward (gpx_xyz_forward_save + gpx_xyz_backward) on one MI355X, and write profiles/xyz_head_backward.txt.

Run on the GPU box:  python scripts/xyz_head_backward_time.py [--out profiles/xyz_head_backward.txt] [--deviations FILE] [--no-profile]

Milliseconds per call at B = 4 and B = 64 for H0 = 8 and Cin = 512 (xyz_deform_head at the network's size), every input and buffer
resident on the device (the raw C entry points on preallocated buffers: what a training step would issue).  Discipline, as
scripts/pnp_backward_time.py: about two seconds of back-to-back calls first, so that the clock settles and every code object is
loaded, then three windows of at least one second each between device events; the median window is reported, with the spread.

Next to each figure stands the contraction floor: the six 3x3 convs are 12.7 GFLOP per crop and pass (2 x 256 x 2304 x (2 x 256 + 2 x
1024 + 2 x 4096); the transposed conv's 0.15 GFLOP of existing taps are left out), the forward is one pass and the backward two (dX and
dW); at the 157.3 TFLOP/s fp32 matrix peak that is 0.081 ms per crop and pass, 0.24 ms per crop for the three.  A time over its floor is
a whole-call figure, not a kernel's share of peak.

The per-kernel breakdown comes from one `rocprofv3 --kernel-trace --stats` run of its own at B = 64 (a fresh child process that runs
eight forward_save + backward pairs, the first of them through givepose_amd.xyz_grad; started before this process touches the device).  For context only, the
time of torch autograd on the device over oracle.posenet_ref.xyz_head_ref (forward + backward, B = 4) is appended.

No threshold is asserted: these are the figures a later change has to beat.
--deviations: a text file (the `-s` output of tests/test_xyz_backward_gpu.py) whose ratio lines are appended.
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
CIN, H0 = 512, 8
PASS_FLOP = 2 * 256 * 2304 * (2 * 256 + 2 * 1024 + 2 * 4096)      # the six 3x3 convs of one crop, one pass


def setup(B):
    import torch
    import xyz_backward_ref as R
    from givepose_amd import _lib, xyz_grad
    L = _lib.load()
    dev = torch.device("cuda")
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    params = {k: torch.from_numpy(v).cuda() for k, v in R.head_params(CIN).items()}
    feat, g = (torch.from_numpy(x).cuda() for x in R.make_inputs(B, CIN, H0, seed=90 + B))
    saved = xyz_grad.xyz_forward_save(feat, params)
    grads, g_feat = xyz_grad.xyz_backward(params, saved, feat, g)
    pw, sv = xyz_grad._params_struct(params, CIN, "params"), xyz_grad._saved_struct(saved, B, CIN, H0)
    pg = xyz_grad._params_struct(grads, CIN, "grads")
    nf, nb = L.gpx_xyz_forward_workspace(B, CIN, H0), L.gpx_xyz_backward_workspace(B, CIN, H0)
    wf, wb = torch.empty(nf // 4 + 64, device=dev), torch.empty(nb // 4 + 64, device=dev)
    keep = (params, feat, g, saved, grads, g_feat, wf, wb)

    def fwd():
        _lib.check(L.gpx_xyz_forward_save(feat.data_ptr(), ctypes.byref(pw), B, CIN, H0, ctypes.byref(sv), wf.data_ptr(), nf, stream()),
                   "gpx_xyz_forward_save")

    def bwd():
        _lib.check(L.gpx_xyz_backward(ctypes.byref(pw), ctypes.byref(sv), feat.data_ptr(), g.data_ptr(), B, CIN, H0, ctypes.byref(pg),
                                      g_feat.data_ptr(), wb.data_ptr(), nb, stream()), "gpx_xyz_backward")
    return fwd, bwd, keep


def window(fn, seconds):
    """Calls of fn between two device events until `seconds` of host time have passed -> milliseconds per call."""
    import time

    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, t0 = 0, time.perf_counter()
    a.record()
    while time.perf_counter() - t0 < seconds:
        for _ in range(4):
            fn()
        n += 4
        torch.cuda.synchronize()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def measure(fn):
    window(fn, 2.0)                                  # settle
    w = sorted(window(fn, 1.0) for _ in range(3))
    return w[1], w[0], w[2]


def profile_child():
    """What the rocprofv3 run executes: eight forward_save + backward pairs at B = 64 (setup's own, then seven)."""
    import torch
    fwd, bwd, keep = setup(64)
    for _ in range(7):
        fwd()
        bwd()
    torch.cuda.synchronize()


def kernel_breakdown(pairs=8):
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


def autograd_time(B):
    import torch
    import xyz_backward_ref as R
    from oracle import posenet_ref
    prefix = R.HEAD_OF[CIN] + "."
    P = {prefix + k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in R.head_params(CIN).items()}
    feat, g = (torch.from_numpy(x).cuda() for x in R.make_inputs(B, CIN, H0, seed=90 + B))
    feat.requires_grad_(True)

    def step():
        with torch.enable_grad():
            out = posenet_ref.xyz_head_ref(P, feat, prefix)
        torch.autograd.grad(out, [feat] + list(P.values()), g)
    return measure(step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xyz_head_backward.txt"))
    ap.add_argument("--deviations", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    a = ap.parse_args()
    if a.profile_child:
        return profile_child()
    breakdown = [] if a.no_profile else kernel_breakdown()      # first: the child runs before this process opens the device
    import torch
    floor = PASS_FLOP / MATRIX_FP32_FLOPS * 1e3      # ms per crop and pass
    lines = [f"coordinate-head backward (Cin {CIN}, H0 {H0}), milliseconds per call, median of three 1 s windows (min .. max) "
             f"({torch.cuda.get_device_name(0)}; fp32; buffers resident on the device)",
             f"contraction floor: {PASS_FLOP * 1e-9:.2f} GFLOP per crop and pass at {MATRIX_FP32_FLOPS * 1e-12:.1f} TFLOP/s = {floor:.4f} ms; forward 1 pass, "
             "backward 2, both 3",
             "   B   forward_save (floor, x floor)              backward (floor, x floor)                  both (floor, x floor)"]
    f = lambda t, fl: f"{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f}) ({fl:.3f}, {t[0] / fl:.1f}x)"
    for B in (4, 64):
        fwd, bwd, keep = setup(B)

        def both():
            fwd()
            bwd()
        tf, tb, tt = measure(fwd), measure(bwd), measure(both)
        lines.append(f"{B:4d}   {f(tf, B * floor)}   {f(tb, 2 * B * floor)}   {f(tt, 3 * B * floor)}")
        del fwd, bwd, both, keep
        torch.cuda.empty_cache()
    ta = autograd_time(4)
    lines += ["", f"for context: torch autograd on the device over xyz_head_ref, forward + backward, B = 4: {ta[0]:.3f} ms ({ta[1]:.3f} .. {ta[2]:.3f})", ""]
    lines += breakdown
    if a.deviations and os.path.exists(a.deviations):
        lines += ["", "ratios printed by tests/test_xyz_backward_gpu.py (device figure / CPU float32 figure, or error / bound):"]
        with open(a.deviations) as fh:
            lines += ["  " + ln.strip().lstrip(".") for ln in fh if "largest ratio" in ln or "/ bound" in ln or "gn gelu backward" in ln]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
