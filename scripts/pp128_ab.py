"""Kernel-level A/B of the two schedules of gp_gemm's 256 x 256 ping-pong tile (variant 10): 1210 = 64-byte K steps (4-stage ring),
1110 = the eight-phase schedule on 128-byte K steps.  Random operands, interleaved rounds in one process on one device; per arm the
median of the rounds with their min .. max beside it.  The two shapes of the kernel guide first (sanity check of the port), then the
product's variant-10 shapes at 128 and 64 crops, and stage-2 fc1 (K = 512) against the weights-in-registers kernel (variant 21).
  python scripts/pp128_ab.py > profiles/pp128_ab.txt"""
import statistics, sys, torch
sys.path.insert(0, ".")
from givepose_amd import ops

g = torch.Generator(device="cuda").manual_seed(0)
ops.CO_SCHEDULED = True


def bench(fn_by_arm, reps=11, inner=6):
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
            if rep:
                times[a].append(e0.elapsed_time(e1) / inner * 1e3)
    return times


SHAPES = [("8192^3", 8192, 8192, 8192, ops.EPI_NONE, (1210, 1110)), ("4096^3", 4096, 4096, 4096, ops.EPI_NONE, (1210, 1110))]
for crops in (128, 64):
    SHAPES += [(f"s2 fc2 {crops}", 256 * crops, 512, 2048, ops.EPI_SCALE_RES, (1210, 1110)),
               (f"s3 fc1 {crops}", 64 * crops, 4096, 1024, ops.EPI_GELU, (1210, 1110)),
               (f"deconv {crops}", 64 * crops, 2304, 1024, ops.EPI_NONE, (1210, 1110)),
               (f"s2 fc1 {crops}", 256 * crops, 2048, 512, ops.EPI_GELU, (21, 1210, 1110))]

for name, M, N, K, epi, arms in SHAPES:
    x = torch.randn(M, K, device="cuda", generator=g).half()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half()
    out = torch.empty(M, N, device="cuda", dtype=torch.half)
    b = torch.zeros(N, device="cuda")
    kw = {}
    if epi == ops.EPI_SCALE_RES:
        kw = dict(gamma=torch.ones(N, device="cuda"), residual=torch.randn(M, N, device="cuda", generator=g).half())
    outs = {}
    for v in arms:
        ops.gemm(x, w, out, bias=b, epilogue=epi, variant=v, **kw)
        outs[v] = out.clone()
    same = torch.equal(outs[1210], outs[1110])
    t = bench({v: (lambda v=v: ops.gemm(x, w, out, bias=b, epilogue=epi, variant=v, **kw)) for v in arms})
    fl = 2.0 * M * N * K
    cells = []
    for v in arms:
        med = statistics.median(t[v])
        cells.append(f"v{v} {med:7.1f} us [{min(t[v]):.1f} .. {max(t[v]):.1f}] {fl / med / 1e6:5.0f} TFLOP/s")
    ratio = statistics.median(t[1210]) / statistics.median(t[1110])
    print(f"{name:12s} M{M} N{N} K{K} epi{epi}: " + " | ".join(cells) + f" | 1210/1110 {ratio:.3f} | bitwise equal {same}", flush=True)
    del x, w, out, outs
