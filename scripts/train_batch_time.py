#!/usr/bin/env python3
"""What a training batch costs when TrainBatchBuilder makes it on the device, next to PoseNet.train_step on that batch.

    python scripts/train_batch_time.py [--batch 64] [--small] [--out FILE]

At B samples of 480 x 640 frames, one sample per frame, seeded draws, it reports
  * the device time of the two launches (gpt_crop_train, gpt_mask_deform), from the library's own per-launch events (gp_timing_*),
    and that a call makes exactly these two launches;
  * the host time of the parameter and table preparation (host_draws + host_params: the DZI boxes, the inverse maps, the tables);
  * the bytes a call uploads, against the bytes of the fp32 maps it writes (what a host loader would upload instead);
  * the wall time of a whole call from host arrays (upload included) and from frames already on the device;
  * train_step's time at the same B in the same run, for scale (--small: depths (1,1,1,1) instead of ConvNeXt-Base).
There is no threshold: the figures say whether the loader or the step bounds an iteration.  Method: a settle of the same work, then
the median of `--windows` windows of `--reps` calls; the spread is min .. max of the windows.
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
H, W = 480, 640


def median_of(fn, reps, n, sync, settle=1.0):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < settle:
        fn()
    sync()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def launches(lib, fn, calls):
    """{label: (launches, ms per launch)} of `calls` calls of fn, from the library's per-launch events."""
    import torch

    from givepose_amd import _lib
    torch.cuda.synchronize()
    _lib.check(lib.gp_timing_begin(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gp_timing_begin")
    for _ in range(calls):
        fn()
    _lib.check(lib.gp_timing_end(), "gp_timing_end")
    got = {}
    for r in range(100):
        lab = ctypes.create_string_buffer(160)
        c, n, ms, fl, by = ctypes.c_int(), ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        if lib.gp_timing_top(r, lab, 160, ctypes.byref(c), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) != 0:
            break
        got[lab.value.decode()] = (n.value, ms.value / max(n.value, 1))
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_batch_time.py needs the GPU: a time from anywhere else says nothing")
    import pose_loss_ref as PR
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, Ranger, TrainBatchBuilder, _lib, synth, train_batch as TB
    B = args.batch
    r = np.random.Generator(np.random.Philox(key=[5, 0x7B49]))
    frames = r.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    inst = np.repeat(np.repeat(r.integers(0, 4, (B, H // 8, W // 8), dtype=np.uint8), 8, 1), 8, 2)
    nocs = r.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    ivfc = r.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    y1, x1 = r.uniform(0, 300, B), r.uniform(0, 400, B)
    bbox = np.stack([y1, x1, y1 + r.uniform(40, 180, B), x1 + r.uniform(40, 240, B)], 1)
    cat = np.arange(B) % 6
    meta = [(np.array([0.01, -0.06, 0.2]), 0.91) if c == 5 else None for c in cat]
    _, gt = PR.make_inputs(B=B, P=256, seed=60)
    labels = {k: gt[k] for k in ("rotation", "translation", "real_size", "sym_info", "nocs_scale", "model_point")}
    labels["mean_size"] = synth.MEAN_SIZES[cat]
    labels["cam_K"] = np.broadcast_to(synth.REAL_INTRINSICS, (B, 3, 3)).copy()
    idx, ids = list(range(B)), [1] * B
    builder = TrainBatchBuilder(H, W, "cuda")
    sync = torch.cuda.synchronize
    say(f"device: {torch.cuda.get_device_name(0)}; B = {B}, {H} x {W} frames, one sample per frame, S = 256, R = 64, seeded draws")

    seed = [0]

    def call(fr, im, nc, iv, buffers=None):
        seed[0] += 1
        return builder(fr, im, nc, iv, idx, idx, ids, bbox, cat, meta, labels, seed=seed[0], out=buffers)
    data = call(frames, inst, nocs, ivfc)
    dev = [torch.from_numpy(a).cuda() for a in (frames, inst, nocs, ivfc)]
    lib = _lib.load()
    got = launches(lib, lambda: call(*dev, buffers=data), 10)
    for k, (n, ms) in sorted(got.items()):
        say(f"    {k}: {n} launches in 10 calls, {ms * 1e3:.1f} us each")
    mine = {k: v for k, v in got.items() if k.startswith("gpt_")}
    if sorted(mine) != ["gpt_crop_train", "gpt_mask_deform"] or any(n != 10 for n, _ in got.values()) or len(got) != _lib.GPT_TRAIN_BATCH_LAUNCHES:
        raise SystemExit("a call does not make exactly the two documented launches")
    say(f"device time of the two launches: {sum(ms for _, ms in mine.values()) * 1e3:.1f} us per batch, {sum(ms for _, ms in mine.values()) * 1e3 / B:.2f} us per sample")

    def host():
        dzi, _ = TB.host_draws(7, B, builder.mask_pro)
        builder.host_params(bbox, cat, meta, dzi)
    med, lo, hi = median_of(host, args.reps, args.windows, lambda: None)
    say(f"host preparation (draws, DZI boxes, inverse maps, tables): median {med:.3f} ms per batch ({lo:.3f} .. {hi:.3f}), {med * 1e3 / B:.1f} us per sample")
    up = sum(a.nbytes for a in (frames, inst, nocs, ivfc))
    small = B * (2 * 6 * 8 + 3 * 4 + 3 * 256 * 4 + 1) + sum(np.asarray(v, dtype=np.float32).nbytes for v in labels.values()) + B * 5 * 4
    maps = sum(data[k].numel() * 4 for k in TB.MAP_KEYS)
    say(f"uploaded per batch: {up / 1e6:.1f} MB of uint8 frames ({up / B / 1e6:.2f} MB per sample) + {small / 1e3:.1f} kB of parameters, tables and labels; "
        f"the fp32 maps a host loader uploads instead: {maps / 1e6:.1f} MB ({maps / B / 1e6:.2f} MB per sample) -- the device form moves "
        f"{up / maps:.1f} x the bytes; what it saves is host CPU time, not PCIe")
    med, lo, hi = median_of(lambda: call(frames, inst, nocs, ivfc, buffers=data), max(args.reps // 4, 2), args.windows, sync)
    say(f"whole call from pageable host arrays (upload included): median {med:.2f} ms per batch ({lo:.2f} .. {hi:.2f}), {med * 1e3 / B:.0f} us per sample")
    med, lo, hi = median_of(lambda: call(*dev, buffers=data), args.reps, args.windows, sync)
    say(f"whole call from frames on the device: median {med:.3f} ms per batch ({lo:.3f} .. {hi:.3f})")

    cfg = PoseNetConfig(convnext_depths=(1, 1, 1, 1)) if args.small else PoseNetConfig()
    net = PoseNet(cfg, dtype=torch.float32, seed=3).cuda()
    opt, pl = Ranger(net), PoseLoss()
    net.train_step(data, pl, opt, "cuda")
    sync()
    t = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        res = net.train_step(data, pl, opt, "cuda")
        sync()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    say(f"train_step on the builder's dict, {'depths (1,1,1,1)' if args.small else 'ConvNeXt-Base'}, float32, B = {B}: median {t[len(t) // 2]:.1f} ms per step "
        f"({t[0]:.1f} .. {t[-1]:.1f} over {args.steps} steps); loss terms finite: {all(bool(torch.isfinite(v).all()) for v in res['loss'].values())}")


if __name__ == "__main__":
    main()
