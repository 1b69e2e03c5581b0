"""Kernel-level A/B of the two schedules of the wide 3x3 window conv (gp_gemm variant 13, 512 pixels x 128 channels): 1213 = 64-byte W
steps (4-stage ring), 1113 = the eight-phase schedule on 128-byte rows of the chunk-major weight copy (gp_gemm_desc.W_cm).  Random
operands, fused GroupNorm statistics as in the product, interleaved rounds in one process on one device; per arm the median of the
rounds with their min .. max beside it.  The heads' Cin 256 convs on 64 x 64 and 32 x 32 maps at 128 and 64 crops.
  python scripts/conv3_pp128_ab.py > profiles/conv3_pp128_ab.txt"""
import statistics, sys, torch
sys.path.insert(0, ".")
from givepose_amd import ops

g = torch.Generator(device="cuda").manual_seed(0)
ops.CO_SCHEDULED = True
OLD, NEW = 1213, 1113


def bench(fn_by_arm, reps=15, inner=6, warm=3):      # the first `warm` rounds (clock ramp, cold caches) are not counted
    times = {a: [] for a in fn_by_arm}
    for rep in range(reps):
        for a, fn in fn_by_arm.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= warm:
                times[a].append(e0.elapsed_time(e1) / inner * 1e3)
    return times


for S in (64, 32):
    for crops in (128, 64):
        Cin, N = 256, 256
        K, M = 9 * Cin, crops * S * S
        x = torch.randn(crops, S, S, Cin, device="cuda", generator=g).half()
        w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
        wcm = ops.conv3_pack_wcm(w)
        out = torch.empty(crops, S, S, N, device="cuda", dtype=torch.half)
        gn = (torch.empty(M // 64 * 32 * 2, device="cuda"), 32, S * S)
        outs = {}
        for v in (OLD, NEW):
            ops.conv2d_nhwc(x, w, 3, 3, 1, 1, out=out, variant=v, gn=gn, w_cm=wcm)
            outs[v] = (out.clone(), gn[0].clone())
        same = all(torch.equal(a, b) for a, b in zip(outs[OLD], outs[NEW]))
        t = bench({v: (lambda v=v: ops.conv2d_nhwc(x, w, 3, 3, 1, 1, out=out, variant=v, gn=gn, w_cm=wcm)) for v in (OLD, NEW)})
        fl = 2.0 * M * N * K
        cells = []
        for v in (OLD, NEW):
            med = statistics.median(t[v])
            cells.append(f"v{v} {med:7.1f} us [{min(t[v]):.1f} .. {max(t[v]):.1f}] {fl / med / 1e6:5.0f} TFLOP/s")
        ratio = statistics.median(t[OLD]) / statistics.median(t[NEW])
        below = max(t[NEW]) < min(t[OLD])
        print(f"{S}x{S} {crops:3d} crops M{M} Cin{Cin}: " + " | ".join(cells) + f" | 1213/1113 {ratio:.3f} | 1113 range wholly below {below} | bitwise equal {same}", flush=True)
        del x, w, wcm, out, outs
