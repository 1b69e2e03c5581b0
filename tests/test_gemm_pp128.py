"""The eight-phase schedule of gp_gemm's 256 x 256 ping-pong tile (variant 10 on 128-byte K steps; variant 1110 forces it, 1210 forces
the 64-byte schedule it stands beside).

  1  bitwise: 1110 and 1210 give the same bits for every (layout, K, epilogue), sentinels around the output included
  2  float64: the 1110 outputs meet tests/gemm_reference.py's per-element bound; nothing is written past M / N
  3  refusals: 1110 on a launch the schedule cannot run raises before the launch
  4  schedule stability: 200 back-to-back launches give the bits of the first, alone and beside a copy stream
  5  dispatch: stage-2 fc2 of an eager fp16 forward keeps its `gemm v10` label and runs the new schedule
"""
import os

import pytest
import torch

import gemm_reference as gr
from gemm_reference import EPI_GELU, EPI_LRELU, EPI_NAMES, EPI_NONE, EPI_RELU, EPI_RES_RELU, EPI_SCALE_RES, GELU_POLY2, RES_EPIS
from test_gemm_conformance import SENT, gr_error

pytestmark = pytest.mark.gpu

NEW, OLD = 1110, 1210
EPIS = (EPI_NONE, EPI_GELU, EPI_RELU, EPI_LRELU, EPI_SCALE_RES, EPI_RES_RELU)
# M, N, ldx - K, ldc, ldres
LAYOUTS = {
    "one": dict(M=256, N=256, xpad=0, ldc=256, ldres=256),            # one tile, lean epilogue
    "four": dict(M=512, N=512, xpad=0, ldc=512, ldres=512),           # four tiles through the XCD remap
    "edge": dict(M=456, N=364, xpad=0, ldc=372, ldres=364),           # edge tiles (clamped DMA rows), ldc % 8 != 0: generic epilogue
    "strided": dict(M=512, N=512, xpad=64, ldc=512, ldres=520),       # ldx = K + 64, ldres != ldc
}
KS = (256, 384, 640, 2048)      # two K-tile pairs (no steady-state iteration beyond the first), an odd number of pairs, five, 32


def _operands(lay, K):
    """As test_gemm_conformance.operands: W columns scaled by 1e-2 .. 10, mixed biases, every 17th row of X past the GELU clamp."""
    L = LAYOUTS[lay]
    M, N = L["M"], L["N"]
    g = torch.Generator().manual_seed(4000 + K + 7 * len(lay))
    x = torch.randn(M, K, generator=g)
    x[::17] *= 6.0
    colscale = 10.0 ** (torch.rand(N, generator=g) * 3.0 - 2.0)
    w = torch.randn(N, K, generator=g) * K ** -0.5 * colscale[:, None]
    b = torch.randn(N, generator=g) * torch.where(torch.arange(N) % 3 == 0, 5.0, 0.01)
    r = torch.randn(M, N, generator=g) * 2.0
    gam = (torch.rand(N, generator=g) * 1.9 + 0.1) * torch.where(torch.arange(N) % 5 == 0, -1.0, 1.0)
    return x.half().float(), w.half().float(), b, r.half().float(), gam


def _launch(o, lay, K, host, epi, variant, gn=None):
    """One launch into fresh sentinel-filled buffers; returns {name: buffer}."""
    L = LAYOUTS[lay]
    M, N = L["M"], L["N"]
    x, w, b, r, gam = host
    dev = "cuda"
    xb = torch.zeros(M, K + L["xpad"], dtype=torch.float16, device=dev)
    xb[:, :K] = x.to(dev, torch.float16)
    cb = torch.full((M + 8, L["ldc"]), SENT, dtype=torch.float16, device=dev)
    bufs = {"C": cb}
    kw = {}
    if epi in RES_EPIS:
        rb = torch.full((M, L["ldres"]), -SENT, dtype=torch.float16, device=dev)
        rb[:, :N] = r.to(dev, torch.float16)
        kw["residual"] = rb[:, :N]
    if epi == EPI_SCALE_RES:
        kw["gamma"] = gam.to(dev)
    if gn:
        cpg, hw = gn
        gb = torch.full((M // 64 * (N // cpg) * 2 + 64,), SENT, dtype=torch.float32, device=dev)
        bufs["gn"] = gb
        kw["gn"] = (gb, N // cpg, hw)
    o.gemm(xb[:, :K], w.to(dev, torch.float16), cb[:M, :N], bias=b.to(dev), epilogue=epi, variant=variant, **kw)
    return bufs


_RUNS = {}


def _runs(lay, K):
    """Per (layout, K), computed once and left unchanged: the host operands, the float64 linear part and, per epilogue, the buffers
    of a 1110 and a 1210 launch (on the CPU)."""
    key = (lay, K)
    if key not in _RUNS:
        from givepose_amd import ops as o
        gr.set_threads()
        host = _operands(lay, K)
        lin = gr.lin_plain(host[0], host[1], host[2])
        outs = {}
        for epi in EPIS:
            new, old = _launch(o, lay, K, host, epi, NEW), _launch(o, lay, K, host, epi, OLD)
            outs[epi] = ({k: v.cpu() for k, v in new.items()}, {k: v.cpu() for k, v in old.items()})
        _RUNS[key] = (host, lin, outs)
    return _RUNS[key]


CASES = [(lay, K) for lay in LAYOUTS for K in KS]


@pytest.mark.parametrize("lay,K", CASES)
def test_bitwise_against_the_64_byte_schedule(lay, K):
    _, _, outs = _runs(lay, K)
    bad = [EPI_NAMES[e] for e in EPIS if not torch.equal(outs[e][0]["C"], outs[e][1]["C"])]
    assert not bad, f"{lay} K={K}: variants 1110 and 1210 differ for {bad}"


@pytest.mark.parametrize("lay,K", CASES)
def test_against_float64(lay, K):
    L = LAYOUTS[lay]
    M, N = L["M"], L["N"]
    host, lin, outs = _runs(lay, K)
    probs = []
    worst = 0.0
    for epi in EPIS:
        ref, bound, _ = gr.epilogue(lin, epi, "f16", GELU_POLY2, r=host[3], g=host[4], lean_res=True)
        cb = outs[epi][0]["C"]
        ratio, msg = gr.check(cb[:M, :N], ref, bound, f"v{NEW} {EPI_NAMES[epi]} {lay} K={K}")
        worst = max(worst, ratio)
        if msg:
            probs.append(msg)
        if not (bool((cb[M:] == SENT).all()) and bool((cb[:M, N:] == SENT).all())):
            probs.append(f"v{NEW} {EPI_NAMES[epi]} {lay} K={K}: wrote past M or N")
    print(f"\n{lay} K={K}: max err/bound {worst:.3g}")
    assert not probs, "\n".join(probs)


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_GELU])
def test_fused_groupnorm_statistics(epi):
    """(512, 512), two images of 256 pixels, 8 channels per group: bitwise against 1210, values and statistics against float64."""
    from givepose_amd import ops as o
    lay, K, cpg, hw = "four", 640, 8, 256
    L = LAYOUTS[lay]
    M, N = L["M"], L["N"]
    host, lin, _ = _runs(lay, K)
    new, old = _launch(o, lay, K, host, epi, NEW, gn=(cpg, hw)), _launch(o, lay, K, host, epi, OLD, gn=(cpg, hw))
    for k in new:
        assert torch.equal(new[k], old[k]), f"variants 1110 and 1210 differ in {k}"
    ref, bound, pre = gr.epilogue(lin, epi, "f16", GELU_POLY2, lean_res=True)
    ratio, msg = gr.check(new["C"][:M, :N], ref, bound, f"v{NEW} {EPI_NAMES[epi]} +gn")
    assert msg is None, msg
    sref, sb = gr.gn_reference(ref, pre, M // hw, hw, N // cpg, 64)
    gb = new["gn"].cpu()
    n = sref.numel()
    ratio, msg = gr.check(gb[:n], sref, sb, f"v{NEW} {EPI_NAMES[epi]} gn_partial")
    assert msg is None, msg
    assert bool((gb[n:] == SENT).all()), "gn_partial written past the last chunk"
    assert bool((new["C"].cpu()[M:] == SENT).all())


def test_refusals():
    """Variant 1110 on a launch the schedule cannot run: GivePoseHipError, and the output keeps its sentinels."""
    from givepose_amd import ops as o
    dev = "cuda"
    g = torch.Generator().manual_seed(5)

    def refused(what, x, w, out, **kw):
        with pytest.raises(gr_error(), match="variant 1110"):
            o.gemm(x, w, out, variant=NEW, **kw)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), f"{what}: refused after writing the output"

    M, N = 256, 256
    x = torch.randn(M, 512, generator=g)
    w = torch.randn(N, 512, generator=g) * 0.05
    out16 = torch.full((M, N), SENT, dtype=torch.float16, device=dev)
    out32 = torch.full((M, N), SENT, dtype=torch.float32, device=dev)
    refused("K = 192", x[:, :192].contiguous().to(dev, torch.float16), w[:, :192].contiguous().to(dev, torch.float16), out16)
    xc = torch.randn(2, 16, 16, 128, generator=g).to(dev, torch.float16)          # 2 x 2 stride-2 conv: M = 128, K = 512
    outc = torch.full((128, N), SENT, dtype=torch.float16, device=dev)
    refused("conv", xc, w.to(dev, torch.float16), outc, conv=dict(B=2, H=16, W=16, Cin=128, KH=2, KW=2, stride=2, pad=0))
    refused("split-operand mode", x.to(dev), o.split_weights(w, dev), out32)
    refused("fp32 storage", x.to(dev), w.to(dev), out32)


@pytest.mark.parametrize("beside_copy", [False, True])
def test_schedule_stability(beside_copy):
    """200 back-to-back launches, all bitwise equal to the first (a determinism screen of the new barrier / wait structure), alone and
    while a second stream copies 512 MB."""
    from givepose_amd import ops as o
    dev = "cuda"
    g = torch.Generator().manual_seed(9)
    side = torch.cuda.Stream()
    if beside_copy:
        src = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
    for M, N, K in ((512, 512, 2048), (256, 256, 384)):
        x = torch.randn(M, K, generator=g).to(dev, torch.float16)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dev, torch.float16)
        b = torch.randn(N, generator=g).to(dev)
        first = torch.empty(M, N, dtype=torch.float16, device=dev)
        out = torch.empty_like(first)
        o.gemm(x, w, first, bias=b, variant=NEW)
        differ = torch.zeros((), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for i in range(200):
            if beside_copy and i % 25 == 0:
                with torch.cuda.stream(side):
                    dst.copy_(src, non_blocking=True)
            o.gemm(x, w, out, bias=b, variant=NEW)
            differ += (out != first).any()
        torch.cuda.synchronize()
        assert int(differ) == 0, f"({M}, {N}, {K}): {int(differ)} of 200 launches differ from the first"


def test_stage2_fc2_runs_the_new_schedule(tmp_path):
    """Eager fp16 forward at 64 crops of a net that keeps two batches in flight (the benched configuration: alone, 128 tiles of 256 x 256
    do not fill the chip and the launch goes to another tile): stage-2 fc2 keeps the label `gemm v10 M16384 N512 K2048 epi4`, and its
    launches report the entry point gp_gemm/pp128 in the per-launch timing dump (gp_gemm with GP_GEMM_PP128=0)."""
    from givepose_amd import PoseNet, PoseNetConfig, _lib
    from test_hip_posenet import _batch, _launch_labels
    dump = tmp_path / "launches.txt"
    net = PoseNet(PoseNetConfig(), dtype=torch.float16, seed=0, inflight=2).cuda()
    os.environ["GP_TIMING_DUMP"] = str(dump)
    try:
        labels = _launch_labels(net, _batch(64, 3))
    finally:
        del os.environ["GP_TIMING_DUMP"]
    lab = "gemm v10 M16384 N512 K2048 epi4"
    assert lab in labels, sorted(k for k in labels if k.startswith("gemm v10"))
    names = set()
    for line in dump.read_text().splitlines():
        f = line.split(" ", 6)
        if len(f) == 7 and f[6] == lab:
            names.add(f[2])
    off = os.environ.get("GP_GEMM_PP128", "")[:1] == "0"
    assert names == ({"gp_gemm"} if off else {"gp_gemm/pp128"}), names
