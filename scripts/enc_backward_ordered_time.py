#!/usr/bin/env python3
"""Time the map-encoder backward with the ordered d xp (include/givepose_encgrad_ordered.h, GPE_SCATTER_ORDERED) against the atomic
mode -- this tree's default, which is the code before the mode existed -- on one MI355X, and write profiles/enc_backward_ordered.txt.

Run on the GPU box:  python scripts/enc_backward_ordered_time.py [--out profiles/enc_backward_ordered.txt] [--no-profile] [--no-train-step]

R = 64, B = 4 and 64, one coupling batch, fp32, preallocated buffers (what a training step would issue).  Discipline: about two
seconds of back-to-back calls of each mode first, then three rounds that alternate the two modes, each window at least one second
between device events; the median round is reported with min .. max.  Timed:
  * the core backward alone at the three layer resolutions (64, 32, 16), on the xp / offset / mask the encoder's forward saved for the
    batch (so the taps fall where a forward of the seeded weights puts them) and a seeded d y;
  * gpe_map_encoder_forward_save followed by the backward in either mode, as a pair.
The per-kernel split of the ordered path comes from one `rocprofv3 --kernel-trace --stats` run of its own at B = 64 (a fresh child,
started before this process touches the device).  train_step at B = 64 (float32 network, set_repack('device'), size_head=None) in
both modes: alternating rounds of 5 steps.  No threshold is asserted: the mode is opt-in and this is its first measurement.
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

import enc_backward_time as base      # noqa: E402  (window, kernel_breakdown: the same discipline and the same rocprofv3 run)

R_NET = 64
MODES = ("atomic", "ordered")


def alternate(fns, rounds=3):
    """fns {label: callable} -> {label: (median, min, max)} ms per call: a 2 s settle each, then `rounds` alternating 1 s windows."""
    for fn in fns.values():
        base.window(fn, 2.0)
    runs = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            runs[k].append(base.window(fn, 1.0))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in runs.items()}


def setup(B, first="atomic"):
    """-> (core {H: {mode: fn}}, pair {mode: fn}, workspace bytes, keep-alive).  first: the mode of the one backward that allocates."""
    import numpy as np
    import torch
    import enc_backward_ref as R
    from givepose_amd import _lib, enc_grad
    L = _lib.load()
    dev = torch.device("cuda")
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    params = {k: torch.from_numpy(v).cuda() for k, v in R.enc_params().items()}
    coor, g = (torch.from_numpy(x).cuda() for x in R.make_inputs(B, R_NET, seed=90 + B))
    saved = enc_grad.enc_forward_save(coor, params)
    grads, g_coor = enc_grad.enc_backward(params, saved, coor, g, scatter=first)
    pw, sv = enc_grad._params_struct(params, "params"), enc_grad._saved_struct(saved[0], B, R_NET)
    pg = enc_grad._params_struct(grads, "grads")
    nf = L.gpe_map_encoder_forward_workspace(B, R_NET)
    nb = {m: L.gpeo_map_encoder_backward_workspace(B, R_NET, enc_grad.SCATTER_MODES[m]) for m in MODES}
    assert nb["atomic"] == L.gpe_map_encoder_backward_workspace(B, R_NET)
    wf, wb = torch.empty(nf // 4 + 64, device=dev), torch.empty(max(nb.values()) // 4 + 64, device=dev)
    keep = [params, coor, g, saved, grads, g_coor, wf, wb]

    def pair(mode):
        def fn():
            _lib.check(L.gpe_map_encoder_forward_save(coor.data_ptr(), ctypes.byref(pw), B, R_NET, ctypes.byref(sv), wf.data_ptr(), nf, stream()),
                       "gpe_map_encoder_forward_save")
            _lib.check(L.gpeo_map_encoder_backward(ctypes.byref(pw), ctypes.byref(sv), coor.data_ptr(), g.data_ptr(), B, R_NET, ctypes.byref(pg),
                                                   g_coor.data_ptr(), wb.data_ptr(), nb[mode], stream(), enc_grad.SCATTER_MODES[mode]),
                       "gpeo_map_encoder_backward")
        return fn

    core, index_bytes = {}, {}
    r = np.random.Generator(np.random.Philox(key=[B, 0x0DE]))
    for l in range(3):
        H = R_NET >> l
        rows = B * (H // 2) ** 2
        xp, off, mask = saved[0]["xp"][l], saved[0]["offset"][l], saved[0]["mask"][l]
        dy = torch.from_numpy(r.standard_normal((rows, 256)).astype(np.float32)).cuda()
        dxp, doff, dml = torch.empty_like(xp), torch.empty_like(off), torch.empty_like(mask)
        nidx = L.gpeo_dcnv3_core_backward_workspace(B, H, H, _lib.GPE_SCATTER_ORDERED)
        ws = torch.empty(nidx // 4 + 64, device=dev)
        keep += [dy, dxp, doff, dml, ws]
        index_bytes[H] = nidx

        def one(mode, xp=xp, off=off, mask=mask, dy=dy, dxp=dxp, doff=doff, dml=dml, ws=ws, nidx=nidx, H=H):
            m = enc_grad.SCATTER_MODES[mode]
            args = (xp.data_ptr(), off.data_ptr(), mask.data_ptr(), dy.data_ptr(), B, H, H, dxp.data_ptr(), doff.data_ptr(), dml.data_ptr())
            return lambda: _lib.check(L.gpeo_dcnv3_core_backward(*args, stream(), m, ws.data_ptr() if m else None, nidx if m else 0),
                                      "gpeo_dcnv3_core_backward")
        core[H] = {m: one(m) for m in MODES}
    return core, {m: pair(m) for m in MODES}, (nb, index_bytes), keep


def profile_child():
    """What the rocprofv3 run executes: four forward_save + ordered backward pairs at B = 64 (setup's own, then three)."""
    import torch
    _, pair, _, keep = setup(64, first="ordered")
    for _ in range(3):
        pair["ordered"]()
    torch.cuda.synchronize()


def train_step_times(say, rounds=3, steps=5):
    import numpy as np
    import pose_loss_ref as PR
    import torch
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig, Ranger, synth
    B = 64
    net = PoseNet(PoseNetConfig(), dtype=torch.float32, seed=3).cuda().set_repack("device")
    npb = synth.synth_batch(B, seed=11)
    npb["roi_mask_deform"] = npb["roi_mask"]
    _, gt = PR.make_inputs(B=B, P=256, seed=60)
    data = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in {**npb, **gt}.items()}
    opt, pl = Ranger(net), PoseLoss()
    runs = {m: [] for m in MODES}
    for _ in range(rounds):
        for m in MODES:
            net.set_encoder_scatter(m)
            net.train_step(data, pl, opt, "cuda")
            torch.cuda.synchronize()
            t = []
            for _ in range(steps):
                t0 = time.perf_counter()
                net.train_step(data, pl, opt, "cuda")
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            runs[m].append(sorted(t)[len(t) // 2])
    say(f"train_step, ConvNeXt-Base, B = {B}, float32 network, set_repack('device'), size_head=None: ms per step, median of {rounds} alternating "
        f"rounds of {steps} steps (min .. max of the rounds' medians)")
    for m in MODES:
        v = runs[m]
        say(f"  set_encoder_scatter({m!r}): {sorted(v)[len(v) // 2]:8.1f} ({min(v):.1f} .. {max(v):.1f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enc_backward_ordered.txt"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    a = ap.parse_args()
    if a.profile_child:
        return profile_child()
    base.__file__ = os.path.abspath(__file__)      # the rocprofv3 run starts this script's child
    breakdown = [] if a.no_profile else base.kernel_breakdown()      # first: the child runs before this process opens the device
    import torch
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say(f"map-encoder backward, d xp by fp32 atomics against the ordered sum (R {R_NET}, one coupling batch, fp32), milliseconds per call: median of "
        f"three alternating 1 s rounds (min .. max), measured on one {torch.cuda.get_device_name(0)}")
    f = lambda t: f"{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    for B in (4, 64):
        core, pair, (nb, index_bytes), keep = setup(B)
        say(f"B = {B}: workspace of the backward {nb['atomic'] / 2 ** 20:.1f} MiB atomic, {nb['ordered'] / 2 ** 20:.1f} MiB ordered "
            f"(+{(nb['ordered'] - nb['atomic']) / 2 ** 20 / B:.3f} MiB per crop); the index of a core alone: "
            + ", ".join(f"H {H}: {v / 2 ** 20 / B:.3f} MiB per crop" for H, v in index_bytes.items()))
        total = {m: 0.0 for m in MODES}
        for H, fns in core.items():
            res = alternate(fns)
            for m in MODES:
                total[m] += res[m][0]
            say(f"  core backward H = {H:2d}: atomic {f(res['atomic'])}   ordered {f(res['ordered'])}   ordered / atomic {res['ordered'][0] / res['atomic'][0]:.2f}")
        say(f"  core backward, the three layers: atomic {total['atomic']:.3f}   ordered {total['ordered']:.3f}   (+{total['ordered'] - total['atomic']:.3f} ms)")
        res = alternate(pair)
        say(f"  forward_save + backward: atomic {f(res['atomic'])}   ordered {f(res['ordered'])}   (+{res['ordered'][0] - res['atomic'][0]:.3f} ms, "
            f"{100 * (res['ordered'][0] / res['atomic'][0] - 1):.1f} %)")
        del core, pair, keep
        torch.cuda.empty_cache()
    if not a.no_train_step:
        say("")
        train_step_times(say)
    if breakdown:
        say("")
        for ln in breakdown:
            say(ln.replace("forward_save + backward pairs", "forward_save + ORDERED backward pairs"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
