#!/usr/bin/env python3
"""Time givepose_amd.PoseLoss against the shape of the reference's loop on the same device, and write profiles/pose_loss.txt.

Run on the GPU box:  python scripts/pose_loss_time.py [--out profiles/pose_loss.txt] [--deviations FILE]

  * HIP: PoseLoss()(pred, data) with every input already on the device: two launches, no copy to the host.
  * torch loop: the reference's structure (losses/pose_loss.py:30-196) written with torch on the same device -- per symmetric crop a
    .cpu().numpy() round trip and a 360-candidate search in NumPy (tests/pose_loss_ref.candidates_re), then float32 torch ops for
    the six terms and .item() of each, which is what a validation loop that logs them pays.
Microseconds per call at B = 48 and 128 (P = 1024, sym_info rows cycling as in the tests).  No threshold is asserted.
--deviations: a text file (the `-s` output of tests/test_pose_loss_gpu.py) whose lines with 'max rel' / 'vs restatement' are appended.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_loss_ref as R  # noqa: E402

from givepose_amd import PoseLoss  # noqa: E402


def torch_loop(pred, data):
    rot, gt = pred["rot"], data["rotation"]
    B = rot.shape[0]
    sym1 = data["sym_info"][:, 0] == 1
    closest = gt.clone()
    branch = bool(sym1.sum() > 0)
    if branch:
        tab = R.sym_table()
        for b in range(B):
            if sym1[b]:
                p, g = rot[b].cpu().numpy(), gt[b].cpu().numpy()
                res = R.candidates_re(p, g)
                k = int(np.argmin(res))
                if res[k] < R.re_deg(np.float64(p), np.float64(g)):
                    closest[b] = torch.from_numpy(R._times_sym_y(np.float64(g), tab[k:k + 1, 0], tab[k:k + 1, 1])[0]).to(gt)
    rs = torch.bmm(closest.transpose(1, 2), gt)
    sc = data["nocs_scale"].unsqueeze(-1)
    out = [(rot - closest).abs().mean(), (pred["trans"] - data["translation"] / sc).abs().mean(),
           (pred["size"] - data["real_size"] / sc).abs().mean()]
    pts = data["model_point"].permute(0, 2, 1)
    out.append((torch.bmm(rot, pts) - torch.bmm(closest, pts)).abs().mean())
    for p, g, m in ((pred["nocs_coor"], data["nocs_coord"], data["roi_mask_output"]), (pred["ivfc_coor"], data["ivfc_coord"], data["roi_ivfc_mask_output"])):
        if branch:
            g = torch.bmm(rs, g.reshape(B, 3, -1)).reshape(g.shape)
        d = (p * m - g * m).abs()
        l = m * torch.where(d > 0.03, d - 0.015, d * d / 0.06)
        out.append(0.1 * (l.sum(dim=[1, 2, 3]) / (m.sum(dim=[1, 2, 3]) + 1e-5)).mean())
    return [float(v.item()) for v in out]


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_loss.txt"))
    ap.add_argument("--deviations", default=None)
    a = ap.parse_args()
    lines = [f"PoseLoss, microseconds per call ({torch.cuda.get_device_name(0)}; P = 1024; inputs resident on the device)",
             "   B    HIP PoseLoss   torch loop (per-crop host search)   ratio   max rel |HIP - torch loop| over the six terms"]
    for B in (48, 128):
        pred, data = R.make_inputs(B=B, P=1024, seed=70 + B)
        tp = {k: torch.from_numpy(v).cuda() for k, v in pred.items()}
        td = {k: torch.from_numpy(v).cuda() for k, v in data.items()}
        loss = PoseLoss()
        hip = timed(lambda: loss(tp, td), 200)
        ref = timed(lambda: torch_loop(tp, td), 5)
        got = np.array([float(v) for v in loss(tp, td).values()])
        exp = np.array(torch_loop(tp, td))
        lines.append(f"{B:4d}   {hip:10.1f}      {ref:12.1f}                       {ref / hip:7.1f}   {np.max(np.abs(got - exp) / np.abs(exp)):.2e}")
    if a.deviations and os.path.exists(a.deviations):
        lines += ["", "largest deviations printed by tests/test_pose_loss_gpu.py:"]
        with open(a.deviations) as f:
            lines += ["  " + ln.strip().lstrip(".") for ln in f if "max rel" in ln or "vs restatement" in ln or "vs the reference" in ln or "forward(do_loss" in ln]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
