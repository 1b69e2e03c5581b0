#!/usr/bin/env python3
"""Time the pose-head backward (gph_pnp_forward_save + gph_pnp_backward) on one MI355X, and write profiles/pnp_backward.txt.

Run on the GPU box:  python scripts/pnp_backward_time.py [--out profiles/pnp_backward.txt] [--deviations FILE]

Milliseconds per call at B = 4 and B = 64, every input and buffer resident on the device (the raw C entry points on preallocated
buffers: what a training step would issue).  Discipline: about two seconds of back-to-back calls first, so that the clock settles and
every code object is loaded, then three windows of at least one second each between device events; the median window is reported,
with the spread.  Next to the times, two byte floors as a fraction of the HBM bandwidth (8.0 TB/s, the specification):

  * fc1 | fc1_z dW: a 64 MB store plus B (8192 + 2048) 4 bytes read
  * fc1 | fc1_z dX: a 64 MB read (the two weight matrices once)

No threshold is asserted: these are the figures a later change has to beat.
--deviations: a text file (the `-s` output of tests/test_pnp_backward_gpu.py) whose ratio lines are appended.
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_backward_ref as R  # noqa: E402

from givepose_amd import _lib, pnp_grad  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def window(fn, seconds):
    """Calls of fn between two device events until `seconds` of host time have passed -> milliseconds per call."""
    import time
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, t0 = 0, time.perf_counter()
    a.record()
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            fn()
        n += 10
        torch.cuda.synchronize()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def measure(fn):
    window(fn, 2.0)                                  # settle
    w = sorted(window(fn, 1.0) for _ in range(3))
    return w[1], w[0], w[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_backward.txt"))
    ap.add_argument("--deviations", default=None)
    a = ap.parse_args()
    L = _lib.load()
    dev = torch.device("cuda")
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    params = {k[len(R.PREFIX):]: torch.from_numpy(v).cuda() for k, v in R.head_params().items()}
    lines = [f"pose-head backward, milliseconds per call, median of three 1 s windows (min .. max) ({torch.cuda.get_device_name(0)}; fp32; "
             "buffers resident on the device)",
             "   B   forward_save            backward                both     floor fc1 dW (share of both)   floor fc1 dX (share of both)"]
    for B in (4, 64):
        ivfc, coord, _, g_rot, g_t = (None if x is None else torch.from_numpy(x).cuda() for x in R.make_inputs(B, seed=90 + B))
        saved = pnp_grad.pnp_forward_save(ivfc, coord, params)
        grads, g_ivfc = pnp_grad.pnp_backward(params, saved, g_rot, g_t)
        pw, sv, pg = (pnp_grad._params_struct(params, 6, "params"), pnp_grad._saved_struct(saved), pnp_grad._params_struct(grads, 6, "grads"))
        nf, nb = L.gph_pnp_forward_workspace(B, 6), L.gph_pnp_backward_workspace(B, 6)
        wf, wb = torch.empty(nf // 4 + 64, device=dev), torch.empty(nb // 4 + 64, device=dev)

        def fwd():
            _lib.check(L.gph_pnp_forward_save(ivfc.data_ptr(), coord.data_ptr(), 0, ctypes.byref(pw), B, 6, ctypes.byref(sv), wf.data_ptr(), nf,
                                              stream()), "gph_pnp_forward_save")

        def bwd():
            _lib.check(L.gph_pnp_backward(ctypes.byref(pw), ctypes.byref(sv), 0, g_rot.data_ptr(), g_t.data_ptr(), B, 6, ctypes.byref(pg),
                                          g_ivfc.data_ptr(), wb.data_ptr(), nb, stream()), "gph_pnp_backward")

        def both():
            fwd()
            bwd()

        tf, tb, tt = measure(fwd), measure(bwd), measure(both)
        floor_dw = (2 * 1024 * 8192 * 4 + B * (8192 + 2048) * 4) / HBM_BYTES_PER_S * 1e3
        floor_dx = (2 * 1024 * 8192 * 4) / HBM_BYTES_PER_S * 1e3
        f = lambda t: f"{t[0]:7.3f} ({t[1]:.3f} .. {t[2]:.3f})"
        lines.append(f"{B:4d}   {f(tf)}   {f(tb)}   {tt[0]:7.3f}   {floor_dw:.4f} ms ({floor_dw / tt[0]:.3f})              "
                     f"{floor_dx:.4f} ms ({floor_dx / tt[0]:.3f})")
    if a.deviations and os.path.exists(a.deviations):
        lines += ["", "ratios printed by tests/test_pnp_backward_gpu.py (device figure / CPU float32 figure, or error / bound):"]
        with open(a.deviations) as fh:
            lines += ["  " + ln.strip().lstrip(".") for ln in fh if "largest ratio" in ln or "/ bound" in ln or "gn backward" in ln or "device gates" in ln]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
