#!/usr/bin/env python3
"""Time the device-side weight repack (include/givepose_repack.h, PoseNet.set_repack("device")) beside the host repack it replaces.

    python scripts/repack_time.py [--out FILE]                           the repack of the ConvNeXt-Base model in the three modes, beside
                                                                         PoseNet._pack in the same process; the copy's entry classes
    python scripts/repack_time.py --train-step small|base [--out FILE]   train_step in alternating host / device rounds
    python scripts/repack_time.py --kernel-count [--out FILE]            kernels and memory copies of one params_updated() from rocprofv3

Repack times are medians of windows between device events after a settle; bytes are what the tables ask for (every source element read
once, every destination element written once).  `_pack` is timed as the next forward pays it: host clock, ending in a device
synchronise.  The entry classes are timed as tables of their own: the identity views (one contiguous run each), every other view (the plain gather),
and the folds (their launches and the copy of their results).
--kernel-count starts child processes under rocprofv3 (1 and 4 repacks after the first pack), one pair with --kernel-trace and one pair
with --memory-copy-trace, and reports the differences over 3: what one steady-state params_updated() launches and copies.
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
HBM_PEAK = 8e12      # bytes / s, the figure BASELINE.md uses
MODES = {"fp32": dict(split_gemm=False), "split": dict(split_gemm=True), "fp16": dict(split_gemm=False)}


def windows(fn, reps, n, settle=1.0):
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


def _bytes(P, entries):
    from givepose_amd import repack
    per = {repack.F32: 8, repack.F16: 6, repack.SPLIT: 8}       # 4 read + 4 / 2 / 2 x 2 written
    return sum(repack._prod(e.dims) * per[e.kind] for e in entries)


def _sub_plan(P, keep, folds=False):
    """The plan's entries for which keep(e), as a table of their own (folds=False: no fold launches, a fold result is read as it lies)."""
    from givepose_amd import repack
    Q = repack.Plan()
    Q.entries = [e for e in P.entries if keep(e)]
    if folds:
        Q.bnfolds, Q.matfolds = list(P.bnfolds), list(P.matfolds)
        Q.sources.update({n: P.sources[n] for f in P.bnfolds for n in (f.w, f.b, f.bn_w, f.bn_b, f.mean, f.var)})
        Q.sources.update({n: P.sources[n] for f in P.matfolds for n in (f.A, f.B, f.add) if n is not None and not n.startswith(repack.FOLD)})
    Q.dst.update({e.dst: P.dst[e.dst] for e in Q.entries})
    Q.scratch.update(P.scratch)
    Q.sources.update({e.src: P.sources[e.src] for e in Q.entries if not e.src.startswith(repack.FOLD)})
    Q.zero_filled = set(P.zero_filled) & set(Q.dst)
    return Q


def _identity(e):
    return [s for d, s in zip(e.dims, e.strides) if d > 1] in ([1], [])


def repack_times(args, say):
    import torch

    from givepose_amd import PoseNet, PoseNetConfig, repack
    dev = torch.device("cuda")
    cfg = PoseNetConfig()
    seeded = PoseNet(cfg, dtype=torch.float32, seed=3).cuda()
    say(f"device: {torch.cuda.get_device_name(0)}; ConvNeXt-Base configuration, {sum(p.numel() for p in seeded.parameters()) / 1e6:.1f} M parameters")
    for mode, kw in MODES.items():
        dtype = torch.float16 if mode == "fp16" else torch.float32
        net = PoseNet(cfg, dtype=dtype, seed=None, **kw).cuda()
        net.load_state_dict(seeded.state_dict())
        # the host repack, as the first forward after a step pays it
        t_host = []
        for _ in range(3):
            net._reset_plans()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            net._pack(dev)
            torch.cuda.synchronize()
            t_host.append((time.perf_counter() - t0) * 1e3)
        net._reset_plans()
        net.set_repack("device")
        net._pack(dev)
        rp = net._repacker
        P, src = rp.plan, rp.sources_of(net)
        med, lo, hi = windows(lambda: rp.run(src), 20, 7)
        nb = _bytes(P, P.entries)
        say(f"{mode}: device repack {med * 1e3:.1f} us ({lo * 1e3:.1f} .. {hi * 1e3:.1f}), {len(P.entries)} entries, {rp.launches()} launches, "
            f"{nb / 1e9:.3f} GB read + written -> {nb / med / 1e9:.2f} TB/s, {nb / (med * 1e-3) / HBM_PEAK:.2f} of the {HBM_PEAK / 1e12:g} TB/s BASELINE.md uses; "
            f"host _pack {sorted(t_host)[1]:.1f} ms ({min(t_host):.1f} .. {max(t_host):.1f}), {sorted(t_host)[1] / med:.0f} x")
        t0 = time.perf_counter()
        for _ in range(50):
            net.params_updated()
        t_call = (time.perf_counter() - t0) / 50 * 1e3
        torch.cuda.synchronize()
        say(f"    host time of one params_updated() call (state_dict walk, pointer check, the launches; no synchronise): {t_call:.2f} ms")
        is_fold = lambda e: e.src.startswith(repack.FOLD)
        for name, keep, folds in (("identity views", lambda e: _identity(e) and not is_fold(e), False),
                                  ("every other view (plain gather)", lambda e: not _identity(e) and not is_fold(e), False),
                                  (f"fold class ({rp.launches() - 1} fold launches + the copy of their results)", is_fold, True)):
            Q = _sub_plan(P, keep, folds)
            rq = repack.DeviceRepack(Q, dev)
            m, a, b = windows(lambda: rq.run(src), 20, 7)
            qb = _bytes(Q, Q.entries)
            say(f"    {name}: {len(Q.entries)} entries, {qb / 1e6:.1f} MB, {m * 1e3:.1f} us ({a * 1e3:.1f} .. {b * 1e3:.1f}) -> {qb / m / 1e9:.2f} TB/s")
            del rq
        del net, rp
        torch.cuda.empty_cache()


def train_step(args, say):
    import numpy as np
    import torch

    import pose_loss_ref as PR
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, Ranger, synth
    small = args.train_step == "small"
    B = 2 if small else 64
    cfg = PoseNetConfig(convnext_depths=(1, 1, 1, 1)) if small else PoseNetConfig()
    net = PoseNet(cfg, dtype=torch.float32, seed=3).cuda()
    npb = synth.synth_batch(B, seed=11)
    npb["roi_mask_deform"] = npb["roi_mask"]
    _, gt = PR.make_inputs(B=B, P=256, seed=60)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**npb, **gt}.items()}
    opt, pl = Ranger(net), PoseLoss()
    say(f"device: {torch.cuda.get_device_name(0)}; train_step, {'depths (1,1,1,1)' if small else 'ConvNeXt-Base'}, B = {B}, float32, size_head=None; "
        "every step ends with params_updated() and starts with the forward that needs the packed weights")
    runs = []
    for rnd in range(args.rounds):          # alternate, so that drift of the box lands on both
        for mode in ("host", "device"):
            net.set_repack(mode)
            net.train_step(data, pl, opt, "cuda")
            torch.cuda.synchronize()
            t = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                net.train_step(data, pl, opt, "cuda")
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            t.sort()
            runs.append((mode, t[len(t) // 2]))
            say(f"round {rnd + 1} set_repack({mode!r}): median {t[len(t) // 2]:.1f} ms per step ({t[0]:.1f} .. {t[-1]:.1f} over {args.steps} steps)")
    a, b = [t for n, t in runs if n == "host"], [t for n, t in runs if n == "device"]
    gain, spread = sum(a) / len(a) - sum(b) / len(b), max(a) - min(a)
    say(f"host medians {min(a):.1f} .. {max(a):.1f} ms; device medians {min(b):.1f} .. {max(b):.1f} ms; the device rounds are {gain:+.2f} ms per step "
        f"faster in the mean, against a spread of {spread:.2f} ms of the host rounds" + ("" if abs(gain) > spread else ": INSIDE the spread"))


def child(repacks, mode):
    import torch

    from givepose_amd import PoseNet, PoseNetConfig
    net = PoseNet(PoseNetConfig(convnext_depths=(1, 1, 1, 1)), dtype=torch.float16 if mode == "fp16" else torch.float32, seed=3,
                  split_gemm=mode == "split").cuda().set_repack("device")
    net._pack(torch.device("cuda"))
    torch.cuda.synchronize()
    for _ in range(repacks):
        net.params_updated()
    torch.cuda.synchronize()
    assert net.repack_count == 1 + repacks


def _trace(flag, pattern, repacks, mode):
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", flag, "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", str(repacks),
                        "--mode", mode], check=True, stdout=subprocess.DEVNULL)
        rows = []
        for f in glob.glob(os.path.join(d, "**", pattern), recursive=True):
            rows += list(csv.DictReader(open(f)))
    return rows


def kernel_count(args, say):
    from givepose_amd import _lib
    bad = []
    for mode, want in (("fp16", _lib.GPR_REPACK_LAUNCHES), ("fp32", _lib.GPR_REPACK_LAUNCHES_F32), ("split", _lib.GPR_REPACK_LAUNCHES_F32)):
        k = {n: _trace("--kernel-trace", "*kernel_trace.csv", n, mode) for n in (1, 4)}
        per = (len(k[4]) - len(k[1])) / 3
        mine = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in k[4]
                      if any(n in r.get("Kernel_Name", "") for n in ("copy_kernel", "bnfold_kernel", "matfold_kernel")))[-want:]
        say(f"{mode} (depths (1,1,1,1)): kernels per steady-state params_updated() (rocprofv3 --kernel-trace, all kernels of the process, "
            f"(4 repacks - 1 repack) / 3): {per:g}; documented constant {want}; kernels traced {len(k[1])} / {len(k[4])}")
        for a, b, n in mine:
            say(f"    {(b - a) / 1e3:8.1f} us  {n[:90]}")
        c = {n: _trace("--memory-copy-trace", "*memory_copy_trace.csv", n, mode) for n in (1, 4)}
        copies = (len(c[4]) - len(c[1])) / 3
        say(f"    memory copies per steady-state params_updated() (a separate pair of runs, --memory-copy-trace): {copies:g}; copies traced "
            f"{len(c[1])} / {len(c[4])} (the parameters' upload and the tables' one upload)")
        if per != want or copies != 0:
            bad.append(mode)
    if bad:
        raise SystemExit(f"launch or copy counts differ from the documented ones: {bad}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--train-step", choices=("small", "base"), default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kernel-count", action="store_true")
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--mode", default="fp16")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.mode)
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if args.kernel_count:
        return kernel_count(args, say)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("repack_time.py needs the GPU: a time from anywhere else says nothing")
    if args.train_step:
        return train_step(args, say)
    repack_times(args, say)


if __name__ == "__main__":
    main()
