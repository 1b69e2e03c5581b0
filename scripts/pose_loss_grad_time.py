#!/usr/bin/env python3
"""Time givepose_amd.PoseLoss.value_and_grad against torch autograd over the shape of the reference's loss on the same device, and
write profiles/pose_loss_grad.txt.

Run on the GPU box:  python scripts/pose_loss_grad_time.py [--out profiles/pose_loss_grad.txt] [--deviations FILE]

  * HIP: PoseLoss().value_and_grad(pred, data) with every input already on the device: the two forward launches and one gradient
    launch, no copy to the host.  `forward only` is PoseLoss()(pred, data), for the share the gradient launch adds.
  * torch autograd: the reference's structure (losses/pose_loss.py:30-196) written with torch on the same device -- per symmetric
    crop a .cpu().numpy() round trip and a 360-candidate search in NumPy (tests/pose_loss_ref.candidates_re), float32 torch ops for
    the six terms, then `total.backward()` into the five prediction tensors, as engine/train.py does.
Microseconds per call at B = 48 and 128 (P = 1024, sym_info rows cycling as in the tests), taken with device events around a window
of calls after a warm-up of the same shape; the two versions alternate, five windows each, median and range reported.  The bytes
the gradient launch has to move (computed from the shapes) over the HBM peak of 6.3 TB/s are printed next to it: what is left is
launch latency.  No threshold is asserted.  There is no CPU path: without a device the script fails.
--deviations: a text file (the `-s` output of tests/test_pose_loss_grad_gpu.py) whose figure lines are appended.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_loss_ref as R  # noqa: E402

from givepose_amd import PoseLoss  # noqa: E402

KEYS = ("rot", "trans", "size", "nocs_coor", "ivfc_coor")
HBM_PEAK = 6.3e12


def torch_autograd(pred, data):
    """-> the five gradients of the total loss by torch autograd over the reference's loop structure."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in pred.items()}
    rot, gt = p["rot"], data["rotation"]
    B = rot.shape[0]
    sym1 = data["sym_info"][:, 0] == 1
    closest = gt.clone()
    branch = bool(sym1.sum() > 0)
    if branch:
        tab = R.sym_table()
        for b in range(B):
            if sym1[b]:
                r, g = rot[b].detach().cpu().numpy(), gt[b].cpu().numpy()
                res = R.candidates_re(r, g)
                k = int(np.argmin(res))
                if res[k] < R.re_deg(np.float64(r), np.float64(g)):
                    closest[b] = torch.from_numpy(R._times_sym_y(np.float64(g), tab[k:k + 1, 0], tab[k:k + 1, 1])[0]).to(gt)
    rs = torch.bmm(closest.transpose(1, 2), gt)
    sc = data["nocs_scale"].unsqueeze(-1)
    total = (rot - closest).abs().mean() + (p["trans"] - data["translation"] / sc).abs().mean() + (p["size"] - data["real_size"] / sc).abs().mean()
    pts = data["model_point"].permute(0, 2, 1)
    total = total + (torch.bmm(rot, pts) - torch.bmm(closest, pts)).abs().mean()
    for x, g, m in ((p["nocs_coor"], data["nocs_coord"], data["roi_mask_output"]), (p["ivfc_coor"], data["ivfc_coord"], data["roi_ivfc_mask_output"])):
        if branch:
            g = torch.bmm(rs, g.reshape(B, 3, -1)).reshape(g.shape)
        d = (x * m - g * m).abs()
        l = m * torch.where(d > 0.03, d - 0.015, d.pow(2) / 0.06)
        total = total + 0.1 * (l.sum(dim=[1, 2, 3]) / (m.sum(dim=[1, 2, 3]) + 1e-5)).mean()
    total.backward()
    return {k: p[k].grad for k in KEYS}


def window(fn, n):
    """Microseconds per call over n calls, between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_loss_grad.txt"))
    ap.add_argument("--deviations", default=None)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_loss_grad_time.py needs the GPU: nothing is measured without it")
    lines = [f"PoseLoss.value_and_grad, microseconds per call ({torch.cuda.get_device_name(0)}; P = 1024; inputs resident on the device;",
             f"device events, median [min .. max] of {a.windows} alternating windows)",
             "   B   HIP value_and_grad        HIP forward only          torch autograd (per-crop host search)   ratio   bytes of the gradient launch "
             "/ 6.3 TB/s   max |HIP - torch| / max|g|"]
    for B in (48, 128):
        pred, data = R.make_inputs(B=B, P=1024, seed=70 + B)
        tp = {k: torch.from_numpy(v).cuda() for k, v in pred.items()}
        td = {k: torch.from_numpy(v).cuda() for k, v in data.items()}
        loss = PoseLoss()
        runs = {"hip": (lambda: loss.value_and_grad(tp, td), 300), "fwd": (lambda: loss(tp, td), 300), "torch": (lambda: torch_autograd(tp, td), 3)}
        for fn, _ in runs.values():                            # warm-up of this shape
            fn()
            fn()
        t = {k: [] for k in runs}
        for _ in range(a.windows):
            for k, (fn, n) in runs.items():
                t[k].append(window(fn, n))
        got, exp = loss.value_and_grad(tp, td)[1], torch_autograd(tp, td)
        dev = max(float((got[k] - exp[k]).abs().max() / exp[k].abs().max()) for k in KEYS)
        # the gradient launch reads the two predicted and two ground-truth maps and the two masks, and writes two maps; plus the points
        nbytes = B * (64 * 64 * (3 * 4 + 2 + 3 * 2) * 4 + 1024 * 12)
        f = lambda v: f"{np.median(v):8.1f} [{min(v):7.1f} .. {max(v):7.1f}]"
        lines.append(f"{B:4d}   {f(t['hip'])}   {f(t['fwd'])}   {f(t['torch'])}   {np.median(t['torch']) / np.median(t['hip']):7.1f}   "
                     f"{nbytes / 1e6:5.1f} MB = {nbytes / HBM_PEAK * 1e6:4.1f} us   {dev:.2e}")
    if a.deviations and os.path.exists(a.deviations):
        lines += ["", "figures printed by tests/test_pose_loss_grad_gpu.py:"]
        with open(a.deviations) as f:
            lines += ["  " + ln.strip().lstrip(".") for ln in f if "|diff|" in ln or "decode backward" in ln or "head_grads" in ln]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
