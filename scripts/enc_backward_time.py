#!/usr/bin/env python3
"""Time the map-encoder backward (gpe_map_encoder_forward_save + gpe_map_encoder_backward, PoseNet.map_encoder_backward) and the whole
chain PoseNet.head_grads_feat on one MI355X, and write profiles/enc_backward.txt.

Run on the GPU box:  python scripts/enc_backward_time.py [--out profiles/enc_backward.txt] [--deviations FILE] [--no-profile]

Milliseconds per call at B = 4 and B = 64 at the network's sizes (R = 64, one coupling batch), fp32.  The two entry points are timed
on preallocated buffers (what a training step would issue); map_encoder_backward and head_grads_feat are timed as the Python calls
they are, allocations included.  Discipline, as scripts/xyz_head_backward_time.py: about two seconds of back-to-back calls first,
then three windows of at least one second each between device events; the median window is reported, with the spread.

Two floors stand next to the entry points' figures:
  * the contraction FLOPs of the Linears (conv1x1, input_proj, offset, mask, output_proj over the three layers: 1.13 GFLOP per crop in
    the forward, twice that in the backward) at the 157.3 TFLOP/s fp32 matrix peak;
  * the bytes of the d xp scatter: rows x 4 groups x 9 taps x 4 corners x 64 channels x 4 B = 37.7 + 9.4 + 2.4 MB per crop over the three
    layers, at the 1.3 TB/s chip-wide rate of fp32 global atomics.  That rate is an estimate taken from the microarchitecture notes this
    project works from, not a measurement on this code; taps outside the image add nothing, so the true byte count is lower.
No threshold is asserted: this is the untuned baseline a later change has to beat.

The per-kernel breakdown comes from one `rocprofv3 --kernel-trace --stats` run of its own at B = 64 (a fresh child process, started
before this process touches the device).  --deviations: a text file (the `-s` output of tests/test_enc_backward_gpu.py) whose ratio
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
ATOMIC_BYTES_PER_S = 1.3e12
R_NET = 64


def linear_flop_forward():
    """FLOP of one crop's Linears in the forward (the backward has dX and dW: twice this)."""
    f = 0
    for l, cin in enumerate((3, 256, 256)):
        rows = (R_NET >> l) ** 2
        n = rows // 4
        f += 2 * (rows * cin * 256 + rows * 256 * 256 + n * 256 * (72 + 36) + n * 256 * 256)
    return f


def scatter_bytes():
    return sum(((R_NET >> l) ** 2 // 4) * 4 * 9 * 4 * 64 * 4 for l in range(3))


def setup(B):
    import torch
    import enc_backward_ref as R
    from givepose_amd import _lib, enc_grad
    L = _lib.load()
    dev = torch.device("cuda")
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    params = {k: torch.from_numpy(v).cuda() for k, v in R.enc_params().items()}
    coor, g = (torch.from_numpy(x).cuda() for x in R.make_inputs(B, R_NET, seed=90 + B))
    saved = enc_grad.enc_forward_save(coor, params)
    grads, g_coor = enc_grad.enc_backward(params, saved, coor, g)
    pw, sv = enc_grad._params_struct(params, "params"), enc_grad._saved_struct(saved[0], B, R_NET)
    pg = enc_grad._params_struct(grads, "grads")
    nf, nb = L.gpe_map_encoder_forward_workspace(B, R_NET), L.gpe_map_encoder_backward_workspace(B, R_NET)
    wf, wb = torch.empty(nf // 4 + 64, device=dev), torch.empty(nb // 4 + 64, device=dev)
    keep = (params, coor, g, saved, grads, g_coor, wf, wb)

    def fwd():
        _lib.check(L.gpe_map_encoder_forward_save(coor.data_ptr(), ctypes.byref(pw), B, R_NET, ctypes.byref(sv), wf.data_ptr(), nf, stream()),
                   "gpe_map_encoder_forward_save")

    def bwd():
        _lib.check(L.gpe_map_encoder_backward(ctypes.byref(pw), ctypes.byref(sv), coor.data_ptr(), g.data_ptr(), B, R_NET, ctypes.byref(pg),
                                              g_coor.data_ptr(), wb.data_ptr(), nb, stream()), "gpe_map_encoder_backward")
    return fwd, bwd, keep


def chain_setup(B):
    """-> (net, the synthetic loss batch of B crops, PoseLoss): the inputs of head_grads_feat."""
    import numpy as np
    import pose_loss_ref as PR
    import torch
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, synth
    npb = synth.synth_batch(B, seed=7)
    r = np.random.Generator(np.random.Philox(key=[11, B]))
    npb["roi_mask_deform"] = (r.random(npb["roi_mask"].shape) > 0.4).astype(np.float32)
    _, gt = PR.make_inputs(B=B, P=256, seed=60)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**npb, **gt}.items()}
    return PoseNet(PoseNetConfig(), seed=0, dtype=torch.float32).cuda(), data, PoseLoss()


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
    """What the rocprofv3 run executes: four forward_save + backward pairs at B = 64 (setup's own, then three)."""
    import torch
    fwd, bwd, keep = setup(64)
    for _ in range(3):
        fwd()
        bwd()
    torch.cuda.synchronize()


def kernel_breakdown(pairs=4):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enc_backward.txt"))
    ap.add_argument("--deviations", default=None)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    a = ap.parse_args()
    if a.profile_child:
        return profile_child()
    breakdown = [] if a.no_profile else kernel_breakdown()      # first: the child runs before this process opens the device
    import torch
    ff = linear_flop_forward()
    fl, sc = ff / MATRIX_FP32_FLOPS * 1e3, scatter_bytes() / ATOMIC_BYTES_PER_S * 1e3      # ms per crop
    lines = [f"map-encoder backward (R {R_NET}, one coupling batch), milliseconds per call, median of three 1 s windows (min .. max) "
             f"({torch.cuda.get_device_name(0)}; fp32)",
             f"floors per crop: Linears {ff * 1e-9:.2f} GFLOP forward, twice that backward, at {MATRIX_FP32_FLOPS * 1e-12:.1f} TFLOP/s = {fl:.4f} / {2 * fl:.4f} ms; "
             f"d xp scatter {scatter_bytes() * 1e-6:.1f} MB at {ATOMIC_BYTES_PER_S * 1e-12:.1f} TB/s (an estimate, not measured here) = {sc:.4f} ms",
             "   B   gpe_map_encoder_forward_save (Linear floor)   gpe_map_encoder_backward (Linear floor + scatter floor)   "
             "map_encoder_backward (Python call)   head_grads_feat (Python call)"]
    f = lambda t: f"{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    for B in (4, 64):
        fwd, bwd, keep = setup(B)
        tf, tb = measure(fwd), measure(bwd)
        coor, g = keep[1], keep[2]
        del fwd, bwd, keep
        torch.cuda.empty_cache()
        net, data, pl = chain_setup(B)
        tm = measure(lambda: net.map_encoder_backward(coor, g))
        tc = measure(lambda: net.head_grads_feat(data, pl, "cuda"))
        lines.append(f"{B:4d}   {f(tf)} ({B * fl:.3f}, {tf[0] / (B * fl):.0f}x)   {f(tb)} ({2 * B * fl:.3f} + {B * sc:.3f}, {tb[0] / (2 * B * fl + B * sc):.1f}x)   "
                     f"{f(tm)}   {f(tc)}")
        del net, data, pl
        torch.cuda.empty_cache()
    lines += [""] + breakdown
    if a.deviations and os.path.exists(a.deviations):
        lines += ["", "ratios printed by tests/test_enc_backward_gpu.py (device figure / CPU float32 figure, or error / bound):"]
        with open(a.deviations) as fh:
            lines += ["  " + ln.strip().lstrip(".") for ln in fh if "largest ratio" in ln or "/ bound" in ln or "margin set" in ln]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
