#!/usr/bin/env python3
"""Forward latency of the AttentionPnPNet pose head (pnp_head='att') against ConvPnPNet (pnp_head='conv') on one MI355X.

Every configuration is a PoseNet with the seed-0 synthetic weights and use_graph=True: after a warm-up (eager forward, capture,
replays), forward_device is replayed back to back inside windows of at least --window seconds, timed with device events; the
median of --windows windows is reported as ms per forward (and crops/s).  Configurations: both heads at B in {1, 4, 32, 64} in fp16
and the split-operand mode, and BASELINE configs[3] (nocsmap_encoder='att') with either head at bs 32.

  python scripts/att_pnp_bench.py [--out profiles/att_pnp_head.txt]
  python scripts/att_pnp_bench.py --once      # one eager bs-32 configs[3] forward in fp16 (the run to put under rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from givepose_amd import PoseNet, PoseNetConfig, synth  # noqa: E402

MODES = {"fp16": dict(dtype=torch.float16), "split": dict(dtype=torch.float32, split_gemm=True)}


def batch(B, device):
    return {k: torch.from_numpy(v).to(device) for k, v in synth.synth_batch(B, seed=1000 + B).items()}


def time_config(net, B, window, windows):
    data = batch(B, "cuda")
    for _ in range(4):                  # eager, capture + replay, replays
        net.forward_device(data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        net.forward_device(data)
    torch.cuda.synchronize()
    n = max(10, int(window / max((time.perf_counter() - t0) / 5, 1e-6)) + 1)
    res = []
    for _ in range(windows):
        cur = torch.cuda.current_stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(cur)
        for _ in range(n):
            net.forward_device(data)
        b.record(cur)
        b.synchronize()
        res.append(a.elapsed_time(b) / n)
    res.sort()
    return res[len(res) // 2], res[0], res[-1], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window (at least)")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--batches", default="1,4,32,64")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "att_pnp_bench needs the GPU"
    if a.once:
        net = PoseNet(PoseNetConfig(pnp_head="att", nocsmap_encoder="att"), seed=0, **MODES["fp16"]).cuda()
        net.forward_device(batch(32, "cuda"))
        torch.cuda.synchronize()
        print("one eager bs-32 configs[3] forward (attention encoder + attention pose head, fp16) done")
        return
    lines = [f"# scripts/att_pnp_bench.py on {torch.cuda.get_device_name(0)}: hipGraph replay of forward_device, device events, "
             f"median (min .. max) of {a.windows} windows of >= {a.window:.1f} s; ms per forward"]
    emit = lambda s: (print(s, flush=True), lines.append(s))
    emit(f"{'config':34s} {'B':>3s} {'ms/fwd':>8s} {'min':>8s} {'max':>8s} {'crops/s':>9s} {'reps':>6s}")
    Bs = [int(b) for b in a.batches.split(",")]
    runs = [(mode, dict(pnp_head=head), f"{head} head, {mode}", Bs) for mode in MODES for head in ("conv", "att")]
    runs += [(mode, dict(pnp_head=head, nocsmap_encoder="att"), f"att enc + {head} head, {mode}", [32]) for mode in MODES for head in ("conv", "att")]
    for mode, kw, name, bs in runs:
        net = PoseNet(PoseNetConfig(**kw), seed=0, use_graph=True, **MODES[mode]).cuda()
        for B in bs:
            med, lo, hi, n = time_config(net, B, a.window, a.windows)
            emit(f"{name:34s} {B:3d} {med:8.3f} {lo:8.3f} {hi:8.3f} {B / med * 1e3:9.0f} {n:6d}")
        net._reset_plans()
        del net
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
