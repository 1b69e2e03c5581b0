"""The eight-phase schedule of the wide 3x3 window conv (gp_gemm variant 13 on 128-byte rows of the chunk-major weight copy,
gp_gemm_desc.W_cm; variant 1113 forces it, 1213 forces the 64-byte schedule it stands beside).

  1  bitwise: 1113 and 1213 give the same bits -- output and fused GroupNorm partials, sentinels around both included -- for the
     epilogues none / GELU / ReLU with bias, with and without statistics; the automatic variant 13 with w_cm equals both
  2  float64: the 1113 outputs (and statistics) meet tests/gemm_reference.py's per-element bound; nothing is written outside the output
  3  pack: gpw_conv3_pack_wcm is w.view(256, 9, Cin // 32, 32).permute(0, 2, 1, 3), exactly
  4  refusals: 1113 on a launch the schedule cannot run raises before the launch
  5  schedule stability: 50 back-to-back launches give the bits of the first, alone and beside a copy stream
  6  dispatch: the 64 x 64 head convs of an eager fp16 forward keep their `conv3x3 s1 v13` labels and run the new schedule

Shapes (Cout 256): the smallest at which the schedule can go wrong --
  b1w32c128  B 1, 32 x 32, Cin 128: two pixel tiles, each with one image border and one real halo; 18 K tiles (one loop body)
  b2w64c128  B 2, 64 x 64, Cin 128: interior tiles with halo on both sides, a second image base, 32 workgroups through the XCD remap
  b3w32c128  B 3, 32 x 32, Cin 128: 12 workgroups, the remainder path of the remap
  b1w32c256  B 1, 32 x 32, Cin 256: the product's 36 K tiles (two loop bodies)
"""
import os

import pytest
import torch

import gemm_reference as gr
from gemm_reference import EPI_GELU, EPI_NAMES, EPI_NONE, EPI_RELU, GELU_POLY2
from test_gemm_conformance import SENT, gr_error

pytestmark = pytest.mark.gpu

NEW, OLD, AUTO = 1113, 1213, 13
EPIS = (EPI_NONE, EPI_GELU, EPI_RELU)
N, CPG = 256, 8
SHAPES = {
    "b1w32c128": (1, 32, 128),
    "b2w64c128": (2, 64, 128),
    "b3w32c128": (3, 32, 128),
    "b1w32c256": (1, 32, 256),
}


def _operands(name):
    """As test_gemm_conformance.operands: W columns scaled by 1e-2 .. 10, mixed biases, a lattice of X pixels past the GELU clamp."""
    B, S, Cin = SHAPES[name]
    K = 9 * Cin
    g = torch.Generator().manual_seed(7000 + 31 * B + S + Cin)
    x = torch.randn(B, S, S, Cin, generator=g)
    x[:, ::2, ::3] *= 4.0
    colscale = 10.0 ** (torch.rand(N, generator=g) * 3.0 - 2.0)
    w = torch.randn(N, K, generator=g) * K ** -0.5 * colscale[:, None]
    b = torch.randn(N, generator=g) * torch.where(torch.arange(N) % 3 == 0, 5.0, 0.01)
    return x.half().float(), w.half().float(), b


def _launch(o, name, dev_ops, epi, variant, gn, w_cm=True):
    """One launch into fresh sentinel-filled buffers; returns {name: buffer}."""
    B, S, Cin = SHAPES[name]
    M = B * S * S
    xd, wd, wcm, bd = dev_ops
    cb = torch.full((M + 8, N), SENT, dtype=torch.float16, device="cuda")
    bufs = {"C": cb}
    kw = {}
    if gn:
        gb = torch.full((M // 64 * (N // CPG) * 2 + 64,), SENT, dtype=torch.float32, device="cuda")
        bufs["gn"] = gb
        kw["gn"] = (gb, N // CPG, S * S)
    o.conv2d_nhwc(xd, wd, 3, 3, 1, 1, out=cb[:M].view(B, S, S, N), bias=bd, epilogue=epi, variant=variant, w_cm=wcm if w_cm else None, **kw)
    return bufs


_RUNS = {}


def _runs(name):
    """Per shape, computed once and left unchanged: the host operands, the float64 linear part and, per (epilogue, statistics), the
    buffers of a 1113, a 1213 and an automatic launch (on the CPU)."""
    if name not in _RUNS:
        from givepose_amd import ops as o
        gr.set_threads()
        x, w, b = _operands(name)
        lin = gr.lin_conv(x, w, 3, 3, 1, 1, b)
        wd = w.to("cuda", torch.float16)
        dev_ops = (x.to("cuda", torch.float16), wd, o.conv3_pack_wcm(wd), b.to("cuda"))
        outs = {}
        for epi in EPIS:
            for gn in (False, True):
                outs[epi, gn] = tuple({k: v.cpu() for k, v in _launch(o, name, dev_ops, epi, v, gn).items()} for v in (NEW, OLD, AUTO))
        _RUNS[name] = (lin, outs)
    return _RUNS[name]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bitwise_against_the_64_byte_schedule(name):
    _, outs = _runs(name)
    bad = []
    for (epi, gn), (new, old, auto) in outs.items():
        for k in new:
            if not torch.equal(new[k], old[k]):
                bad.append(f"{EPI_NAMES[epi]}{' +gn' if gn else ''}: 1113 and 1213 differ in {k}")
            if not torch.equal(auto[k], old[k]):
                bad.append(f"{EPI_NAMES[epi]}{' +gn' if gn else ''}: variant 13 with w_cm and 1213 differ in {k}")
    assert not bad, f"{name}:\n" + "\n".join(bad)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_against_float64(name):
    B, S, Cin = SHAPES[name]
    M = B * S * S
    lin, outs = _runs(name)
    probs, worst = [], 0.0
    for (epi, gn), (new, _, _) in outs.items():
        what = f"v{NEW} {EPI_NAMES[epi]}{' +gn' if gn else ''} {name}"
        ref, bound, pre = gr.epilogue(lin, epi, "f16", GELU_POLY2, lean_res=True)
        cb = new["C"]
        ratio, msg = gr.check(cb[:M], ref, bound, what)
        worst = max(worst, ratio)
        if msg:
            probs.append(msg)
        if not bool((cb[M:] == SENT).all()):
            probs.append(f"{what}: wrote past M")
        if gn:
            sref, sb = gr.gn_reference(ref, pre, B, S * S, N // CPG, 64)
            gb, n = new["gn"], sref.numel()
            ratio, msg = gr.check(gb[:n], sref, sb, f"{what} gn_partial")
            worst = max(worst, ratio)
            if msg:
                probs.append(msg)
            if not bool((gb[n:] == SENT).all()):
                probs.append(f"{what}: gn_partial written past the last chunk")
    print(f"\n{name}: max err/bound {worst:.3g}")
    assert not probs, "\n".join(probs)


@pytest.mark.parametrize("Cin", [128, 256])
def test_pack_is_the_permutation(Cin):
    from givepose_amd import ops as o
    g = torch.Generator().manual_seed(Cin)
    w = torch.randn(N, 9 * Cin, generator=g).half()
    buf = torch.full((N * 9 * Cin + 64,), SENT, dtype=torch.float16, device="cuda")
    got = o.conv3_pack_wcm(w.cuda(), out=buf[: N * 9 * Cin].view(N, 9 * Cin))
    torch.cuda.synchronize()
    want = w.view(N, 9, Cin // 32, 32).permute(0, 2, 1, 3).reshape(N, 9 * Cin)
    assert torch.equal(got.cpu(), want)
    assert bool((buf[N * 9 * Cin:] == SENT).all()), "wrote past the copy"
    assert torch.equal(o.conv3_pack_wcm(w), want)          # the host form (PoseNet._pack('cpu'))


def test_refusals():
    """Variant 1113 on a launch the schedule cannot run: GivePoseHipError, and the output keeps its sentinels."""
    from givepose_amd import ops as o
    g = torch.Generator().manual_seed(5)

    def refused(what, B, S, Cin, match, w_cm=True, split=False):
        M, K = B * S * S, 9 * Cin
        x = torch.randn(B, S, S, Cin, generator=g)
        w = torch.randn(N, K, generator=g) * 0.05
        wd = w.to("cuda", torch.float16)
        wcm = o.conv3_pack_wcm(wd) if w_cm else None
        out = torch.full((M, N), SENT, dtype=torch.float32 if split else torch.float16, device="cuda")
        with pytest.raises(gr_error(), match=match):
            o.conv2d_nhwc(x.cuda() if split else x.to("cuda", torch.float16), o.split_weights(w, "cuda") if split else wd, 3, 3, 1, 1,
                          out=out.view(B, S, S, N), variant=NEW, w_cm=wcm)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), f"{what}: refused after writing the output"

    refused("no w_cm", 1, 32, 128, "variant 1113", w_cm=False)
    refused("16 x 16 map", 2, 16, 128, "variant 1113")
    refused("Cin 96", 1, 32, 96, "K=864 must be a multiple of 64")            # (gp_gemm's own fp16 check, before the variant is looked at)
    refused("split-operand mode", 1, 32, 128, "variant 1113", split=True)


@pytest.mark.parametrize("beside_copy", [False, True])
def test_schedule_stability(beside_copy):
    """50 back-to-back launches of the Cin 256 case, all bitwise equal to the first (a determinism screen of the barrier / wait
    structure), alone and while a second stream copies 512 MB."""
    from givepose_amd import ops as o
    name = "b1w32c256"
    B, S, Cin = SHAPES[name]
    x, w, b = _operands(name)
    xd, wd, bd = x.to("cuda", torch.float16), w.to("cuda", torch.float16), b.cuda()
    wcm = o.conv3_pack_wcm(wd)
    side = torch.cuda.Stream()
    if beside_copy:
        src = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
    first = torch.empty(B, S, S, N, dtype=torch.float16, device="cuda")
    out = torch.empty_like(first)
    o.conv2d_nhwc(xd, wd, 3, 3, 1, 1, out=first, bias=bd, variant=NEW, w_cm=wcm)
    differ = torch.zeros((), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for i in range(50):
        if beside_copy and i % 25 == 0:
            with torch.cuda.stream(side):
                dst.copy_(src, non_blocking=True)
        o.conv2d_nhwc(xd, wd, 3, 3, 1, 1, out=out, bias=bd, variant=NEW, w_cm=wcm)
        differ += (out != first).any()
    torch.cuda.synchronize()
    assert int(differ) == 0, f"{int(differ)} of 50 launches differ from the first"


# smallest crop count at which gp_gemm's automatic choice sends the 64 x 64 head convs of a one-batch-in-flight net to the wide window
# kernel: 12 crops = 192 tiles of 256 x 256, the first count that fills the chip (at 11 crops the launch goes to the 128 x 128 tile)
DISPATCH_CROPS = 12


def test_head_convs_run_the_new_schedule(tmp_path):
    """Eager fp16 forward at DISPATCH_CROPS crops: the 64 x 64 head convs keep the label `conv3x3 s1 v13 64x64 Cin256 Cout256 M49152 +gn`, and
    their launches report the entry point gp_gemm/conv3_pp128 in the per-launch timing dump (gp_gemm with GP_CONV_PP128=0)."""
    from givepose_amd import PoseNet, PoseNetConfig
    from test_hip_posenet import _batch, _launch_labels
    dump = tmp_path / "launches.txt"
    net = PoseNet(PoseNetConfig(), dtype=torch.float16, seed=0).cuda()
    os.environ["GP_TIMING_DUMP"] = str(dump)
    try:
        labels = _launch_labels(net, _batch(DISPATCH_CROPS, 3))
    finally:
        del os.environ["GP_TIMING_DUMP"]
    lab = f"conv3x3 s1 v13 64x64 Cin256 Cout256 M{DISPATCH_CROPS * 4096} +gn"
    assert labels.get(lab) == 4, sorted(k for k in labels if k.startswith("conv3x3"))
    names = set()
    for line in dump.read_text().splitlines():
        f = line.split(" ", 6)
        if len(f) == 7 and f[6] == lab:
            names.add(f[2])
    off = os.environ.get("GP_CONV_PP128", "")[:1] == "0"
    assert names == ({"gp_gemm"} if off else {"gp_gemm/conv3_pp128"}), names
