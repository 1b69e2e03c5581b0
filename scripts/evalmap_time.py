#!/usr/bin/env python3
"""Time the degree-cm / 3D-IoU mAP evaluation on the GPU box, on one seeded set of the size of REAL275 (2 754 frames x 3-6 detections,
givepose_amd.synth.synth_eval_results(2754, 2754)), with the coarse lists (evaluate.py:146-148) and the precise ones (:142-144):

  (a) the NumPy restatement tests/evalmap_ref.py on the host (NumPy's threads capped at 16; on the precise lists a tenth of the frames,
      scaled by ten and labelled so, when a probe says the full set would take more than a minute);
  (b) the device path givepose_amd.compute_degree_cm_mAP from host arrays to host results: H->D of the inputs, the three stages, D->H of
      the two AP arrays.  Timed with a host clock around calls that end in the D->H copy (a synchronise), after two warm-up calls; the
      median and the spread of REPS calls.

Appends the numbers, with the pair and cell counts, to profiles/evalmap.txt (or --out).  A run without a GPU fails: there is no fallback.
The reference's own loop cannot run on the GPU box; scripts/gen_golden_evalmap.py --time records it in the build container.

Run:  python scripts/evalmap_time.py [--out FILE] [--skip-precise-host]
"""
import argparse
import os
import sys
import time

for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = str(min(16, int(os.environ.get(v, "16"))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import evalmap_ref as R  # noqa: E402
from givepose_amd import compute_degree_cm_mAP, synth  # noqa: E402

LISTS = {"coarse": ([5, 10, 360], [5, 10, 1e4], [0.1, 0.25, 0.5, 0.75]),
         "precise": (list(range(0, 71, 1)), [i / 2 for i in range(51)], [i / 100 for i in range(101)])}
REPS = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evalmap.txt"))
    ap.add_argument("--frames", type=int, default=2754)
    ap.add_argument("--skip-precise-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evalmap_time.py needs a GPU: nothing is measured without one")
    names = synth.NOCS_SYNSET
    frames = synth.synth_eval_results(args.frames, 2754)
    groups = R.groups_of(frames, names)
    pairs = sum(len(g["pred"]) * len(g["gt"]) for g in groups)
    lines = [f"## timing on {torch.cuda.get_device_name(0)}: {args.frames} frames (seed 2754), {sum(len(r['pred_class_ids']) for r in frames)} predictions, "
             f"{sum(len(r['gt_class_ids']) for r in frames)} ground truths, {len(groups)} (frame, class) groups, {pairs} pairs; host threads <= 16"]
    for tag, (deg, shift, iou) in LISTS.items():
        cells = len(iou) + (len(deg) + 1) * (len(shift) + 1)
        # (b) device path
        for _ in range(2):
            got = compute_degree_cm_mAP(frames, names, None, deg, shift, iou, 0.1, True)
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = compute_degree_cm_mAP(frames, names, None, deg, shift, iou, 0.1, True)      # ends in the D->H copies of the AP arrays
            ts.append(time.perf_counter() - t)
        ts.sort()
        lines.append(f"{tag}: {cells} cells x {len(groups)} groups = {cells * len(groups)} matchings; device path (host arrays -> AP arrays, H->D and D->H "
                     f"included) median {ts[len(ts) // 2] * 1e3:.1f} ms, min {ts[0] * 1e3:.1f}, max {ts[-1] * 1e3:.1f} of {REPS} calls after 2 warm-ups")
        # (a) the restatement on the host
        sub, scale, label = frames, 1.0, "full set"
        if tag == "precise":
            if args.skip_precise_host:
                lines.append(f"{tag}: restatement on the host not measured (--skip-precise-host)")
                continue
            t = time.perf_counter()
            R.compute_degree_cm_mAP(frames[:args.frames // 10], names, deg, shift, iou, 0.1, True)
            probe = time.perf_counter() - t
            if probe * 10 > 60:
                sub, scale, label = None, 10.0, f"a tenth of the frames ({args.frames // 10}), scaled by 10"
        if sub is None:
            host = probe * scale
        else:
            t = time.perf_counter()
            ref = R.compute_degree_cm_mAP(sub, names, deg, shift, iou, 0.1, True)
            host = time.perf_counter() - t
            same = np.array_equal(ref[0], got[0], equal_nan=True) and np.array_equal(ref[1], got[1], equal_nan=True)
            lines.append(f"{tag}: device AP arrays {'equal' if same else 'DIFFER from'} the restatement's on this set (no decisiveness filter applied here)")
        lines.append(f"{tag}: restatement tests/evalmap_ref.py on the host, {label}: {host:.2f} s")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
