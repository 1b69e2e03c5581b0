"""Time the alignment stage (givepose_amd.umeyama) on the device at B = 1, 4, 64, 128 crops of the 2 500-point, 30 %-outlier
shape, next to PoseNet.forward_device for the same number of crops and next to the NumPy loop (tests/umeyama_ref.py, a restatement of
the reference's CPU loop) on the host's CPU.

    python scripts/umeyama_bench.py [--out profiles/umeyama.txt]

Device times are device events around REPS calls after WARM warm-up calls of the same shape (the median of 5 such windows); the
alignment column is the whole of pose_from_umeyama_device (three launches and its buffer allocations), `kernels` the three launches
alone on preallocated buffers.  The NumPy column is a host clock around the loop over min(B, 8) crops, scaled to B.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import umeyama_ref as R      # noqa: E402

WARM, REPS, WINDOWS = 5, 20, 5


def device_ms(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / REPS)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-forward", action="store_true")
    args = ap.parse_args()
    from givepose_amd import PoseNet, PoseNetConfig, _lib, synth
    from givepose_amd.umeyama import pose_from_umeyama_device
    dev = torch.device("cuda:0")
    L = _lib.load()
    lines = [f"# alignment stage, 2500 masked points, 30 % outliers per crop; {torch.cuda.get_device_name(0)}; ms per call, median (min .. max) of "
             f"{WINDOWS} windows of {REPS} calls",
             f"# {'B':>4} {'alignment':>24} {'kernels only':>24} {'forward_device':>24} {'NumPy loop (CPU)':>18} {'iterations run':>16}"]
    net = None if args.no_forward else PoseNet(PoseNetConfig(), dtype=torch.float16, seed=0).to(dev)
    for B in (1, 4, 64, 128):
        rng = np.random.RandomState(B)
        inputs = R.stack_crops([R.synth_crop(rng, 2500, 0.3) for _ in range(B)])
        draws = rng.randint(0, 2 ** 32, size=(B, R.MAX_ITER, R.SAMPLE), dtype=np.uint64).astype(np.uint32)
        t = [torch.from_numpy(inputs[k]).to(dev) for k in ("xyz_coor", "coor_2d", "camK", "Depth", "obj_mask")]
        d = torch.from_numpy(draws.view(np.int32)).to(dev)
        s, rot, tr, det = pose_from_umeyama_device(*t, draws=d, return_details=True)
        iters = det["iterations_run"].cpu().numpy()
        assert (det["status"].cpu().numpy() == 0).all()
        whole = device_ms(lambda: pose_from_umeyama_device(*t, draws=d))
        # the three launches alone
        e = lambda shape, dt: torch.empty(shape, device=dev, dtype=dt)
        mask = (t[4] != 0).to(torch.uint8)
        pts, idx, npt = e((B, 6, 4096), torch.float32), e((B, 4096), torch.int32), e((B,), torch.int32)
        hyp, cnt, inl = e((B, 128, 16), torch.float64), e((B, 128), torch.int32), e((B, 4096), torch.uint8)
        f64, srt, rec, f32 = e((B, 16), torch.float64), e((B, 16), torch.float64), e((B, 5), torch.int32), e((B, 13), torch.float32)
        st = torch.cuda.current_stream(dev).cuda_stream

        def kernels():
            _lib.check(L.gpa_backproject(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), mask.data_ptr(), 0, B, 64,
                                         pts.data_ptr(), idx.data_ptr(), npt.data_ptr(), 0, st))
            _lib.check(L.gpa_umeyama(pts.data_ptr(), npt.data_ptr(), d.data_ptr(), B, hyp.data_ptr(), cnt.data_ptr(), inl.data_ptr(),
                                     f64.data_ptr(), srt.data_ptr(), rec.data_ptr(), f32.data_ptr(), st))
        kern = device_ms(kernels)
        assert torch.equal(f32[:, 0], s)
        fwd = None
        if net is not None:
            static = net.static_inputs(B, dev)
            for k, v in synth.synth_batch(B, seed=1).items():
                if k in static:
                    static[k].copy_(torch.from_numpy(v))
            fwd = device_ms(lambda: net.forward_device(static, dev))
        nb = min(B, 8)
        sub = {k: v[:nb] for k, v in inputs.items()}
        t0 = time.perf_counter()
        R.pose_from_umeyama_ref(draws=draws[:nb], **sub)
        cpu = (time.perf_counter() - t0) * 1e3 * B / nb
        f = lambda m: f"{m[0]:8.3f} ({m[1]:.3f} .. {m[2]:.3f})" if m else "-"
        lines.append(f"  {B:>4} {f(whole):>24} {f(kern):>24} {f(fwd):>24} {cpu:>18.1f} {f'{iters.min()} .. {iters.max()}':>16}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
