"""gp_gemm conformance: every schedule, epilogue, output form and layout the library accepts against a float64 reference with a
per-element error bound (tests/gemm_reference.py), and every combination it must refuse.

  B  the conformance table (`expected`): per combination "ok" or the fragment of the GP_REQUIRE that refuses it, written from
     include/givepose_hip.h and the checks of gp_gemm -- a change to what a variant accepts comes with a change here.  Each ok case
     checks (i) the per-element bound, (ii) sentinels past N / M and the c16 padding, (iii) every fused GroupNorm statistics chunk,
     (iv) a second launch gives the same bits.  Each refused case raises GivePoseHipError before any launch (the output stays).
  C  GELU over every finite fp16 value, per GELU form of the library.
  D  (CPU) the checker rejects the outputs of subtly wrong kernels and accepts the lean epilogue's legitimate double rounding.
  E  the kernel labels of eager forwards: every gp_gemm combination the product runs is an ok entry of the table.
"""
import re
from collections import defaultdict

import numpy as np
import pytest
import torch

import gemm_reference as gr
from gemm_reference import (EPI_GELU, EPI_LNFOLD_GELU, EPI_LRELU, EPI_NAMES, EPI_NONE, EPI_RELU, EPI_RES_RELU, EPI_SCALE_RES,
                            GELU_ERF, GELU_PK16, GELU_POLY2, RES_EPIS)

EPIS = (EPI_NONE, EPI_GELU, EPI_RELU, EPI_LRELU, EPI_SCALE_RES, EPI_RES_RELU)
TILE = (2, 3, 4, 5, 7, 8, 9, 10, 11, 12)
SENT = 1234.0

# ---------------------------------------------------------------------------------------------------------------- layouts
# plain: M, N, K, ldx (0 = K), ldc, ldres, bias.  K 64 = one 128-byte K step of fp16, 192 = three (odd).
PLAIN = {
    "full": dict(M=512, N=512, K=64, ldx=0, ldc=512, ldres=512, bias=False),        # every tile full, aligned: the lean epilogue
    "ragged": dict(M=200, N=108, K=192, ldx=0, ldc=116, ldres=112, bias=True),      # ldc % 8 != 0: generic everywhere
    "mixed": dict(M=704, N=640, K=128, ldx=0, ldc=640, ldres=640, bias=True),       # lean interior tiles, generic edge tiles
    "strided": dict(M=512, N=512, K=128, ldx=192, ldc=528, ldres=520, bias=True),   # ldx > K, ldres != ldc (both % 8 == 0)
    "sk": dict(M=64, N=256, K=2048, ldx=0, ldc=256, ldres=256, bias=True),          # split-K carrier shape (auto split 8)
    "wreg": dict(M=256, N=256, K=512, ldx=0, ldc=256, ldres=256, bias=True),        # weights-in-registers kernels (16 / 17 / 19-22)
    "wreg_ldc": dict(M=256, N=256, K=512, ldx=0, ldc=260, ldres=256, bias=True),    # ... with ldc % 8 != 0
    "gemv8": dict(M=8, N=256, K=512, ldx=0, ldc=256, ldres=256, bias=True),         # row-vector kernel (23)
    "gemv3": dict(M=3, N=136, K=1024, ldx=1088, ldc=136, ldres=136, bias=True),
    "gnp": dict(M=512, N=256, K=128, ldx=0, ldc=256, ldres=256, bias=True, hw=256),  # fused GroupNorm statistics, 2 images
    "gnp_edge": dict(M=512, N=320, K=128, ldx=0, ldc=320, ldres=320, bias=True, hw=256),  # ... with generic edge tiles in n
}
# conv: B, H, W, Cin, Cout, KH, KW, stride, pad, bias
CONV = {
    "c3s1": dict(B=2, H=16, W=16, Cin=64, Cout=128, KH=3, KW=3, s=1, p=1, bias=True),     # ResNet-34 BasicBlock conv (RES_RELU)
    "c3s2": dict(B=3, H=16, W=16, Cin=64, Cout=128, KH=3, KW=3, s=2, p=1, bias=True),
    "c2s2": dict(B=2, H=16, W=16, Cin=128, Cout=256, KH=2, KW=2, s=2, p=0, bias=True),    # ConvNeXt downsample
    "c1s2": dict(B=2, H=16, W=16, Cin=64, Cout=128, KH=1, KW=1, s=2, p=0, bias=False),    # ResNet-34 downsample
    "win16": dict(B=1, H=16, W=16, Cin=64, Cout=256, KH=3, KW=3, s=1, p=1, bias=True),    # LDS-window conv (13)
    "win32": dict(B=2, H=32, W=32, Cin=64, Cout=256, KH=3, KW=3, s=1, p=1, bias=True),
}
CONV_EPIS = {"c3s1": (EPI_RES_RELU, EPI_GELU), "c3s2": (EPI_RELU,), "c2s2": (EPI_NONE,), "c1s2": (EPI_NONE,),
             "win16": (EPI_NONE, EPI_GELU, EPI_RELU, EPI_SCALE_RES), "win32": (EPI_GELU,)}


def geom(lay):
    """(M, N, K, hw) of a layout."""
    if lay in PLAIN:
        L = PLAIN[lay]
        return L["M"], L["N"], L["K"], L.get("hw", 0)
    c = CONV[lay]
    Ho, Wo = (c["H"] + 2 * c["p"] - c["KH"]) // c["s"] + 1, (c["W"] + 2 * c["p"] - c["KW"]) // c["s"] + 1
    return c["B"] * Ho * Wo, c["Cout"], c["KH"] * c["KW"] * c["Cin"], Ho * Wo


class Case:
    """One gp_gemm launch: variant code, storage ("f16" / "f32"), output ("st" = storage type, "f32", "c16" = f32 + fp16 copy,
    "r32" = fp32 residual stream + fp16 copy, "planes" = split-operand fp16 planes), epilogue, layout, fused GroupNorm statistics
    (None or (channels per group, rows per chunk)), split-K request (None = the automatic one), split-operand mode."""

    def __init__(self, variant, st, out, epi, lay, gn=None, sk=1, split=False):
        self.variant, self.st, self.out, self.epi, self.lay, self.gn, self.sk, self.split = variant, st, out, epi, lay, gn, sk, split

    def __repr__(self):
        s = f"v{self.variant} {self.st}->{self.out} {EPI_NAMES[self.epi]} {self.lay}"
        if self.gn:
            s += f" gn{self.gn[0]}x{self.gn[1]}"
        if self.sk != 1:
            s += f" sk{self.sk}"
        return s + (" split" if self.split else "")


# ---------------------------------------------------------------------------------------------------------------- B: the table
def expected(c):
    """None = ok, else the fragment of gp_gemm's refusal.  Written from include/givepose_hip.h (gp_gemm_desc.variant and the
    fields' comments) and the GP_REQUIREs of gp_gemm, in the order gp_gemm checks them."""
    v, dbg = c.variant % 100, c.variant // 100
    M, N, K, hw = geom(c.lay)
    conv = c.lay in CONV
    f16, c16, r32 = c.st == "f16", c.out in ("c16", "r32"), c.out == "r32"
    out_f32 = c.out != "st" or c.split
    ldc = PLAIN[c.lay]["ldc"] if not conv else N
    L = PLAIN.get(c.lay, {})
    ldx = (L.get("ldx") or K) if not conv else 0
    gnr = c.gn[1] if c.gn else 0
    if c.epi == EPI_LNFOLD_GELU:
        if not f16 or out_f32 or c.sk not in (0, 1) or c.gn or conv:
            return "LNFOLD_GELU needs a plain fp16 GEMM"
        if M % 256 or N % 256 or ldc % 8:
            return "LNFOLD_GELU needs M % 256 == 0"
        if v not in (0, 8, 10, 12):
            return "LNFOLD_GELU runs on variants 8 / 10 / 12"
        return None
    if c.gn and c.sk not in (0, 1):
        return "fused GroupNorm excludes split-K"
    # variant 23 (the row-vector kernel) is decided before every other schedule
    gemv_ok = f16 and not c.split and not r32 and not c16 and not conv and not c.gn and M <= 8 and K % 512 == 0 and N % 8 == 0 \
        and ldx % 8 == 0 and c.epi <= EPI_LRELU and ldc % 2 == 0
    if v == 23:
        return None if gemv_ok else "variant 23 needs"
    if v == 0:
        return None
    splitk = c.sk is None or c.sk > 1
    if v == 18:
        splitk = False          # a split-K request is ignored
    if c.gn and gnr != 64 and v != 18:
        return "needs the small-M kernel"
    if not (2 <= v <= 13 and v != 6 or 16 <= v <= 22) or (splitk and v != 4):
        return "split-K runs on variant 4"
    if c.split and v not in (4, 7, 8, 10, 13):
        return "split-operand mode runs on variants 4 / 7 / 8 / 10 / 13"
    if r32 and v not in (7, 10):
        return "residual_f32 runs on variants 7 / 10"
    if c16 and (v in (13, 16, 17) or c.split):
        return "c16 runs on the tile kernels"
    if v == 18:
        ok = f16 and not c.split and not r32 and not c16 and N % 32 == 0 and (M % 16 == 0 or (not conv and not c.gn and M > 8)) \
            and (not out_f32 or (c.epi <= EPI_LRELU and not c.gn)) \
            and (not c.gn or (M % gnr == 0 and c.epi not in RES_EPIS)) and (not conv or CONV[c.lay]["Cin"] % 32 == 0)
        return None if ok else "variant 18 needs"
    if 16 <= v <= 22:
        wreg_ok = f16 and not conv and K == 512 and N % 256 == 0 and M % 32 == 0 and not out_f32 and not splitk and not c.gn \
            and c.epi <= EPI_LRELU
        if v == 16:
            return None if wreg_ok else "variant 16 needs"
        ok = wreg_ok and ldc % 8 == 0
        return None if ok else ("variant 17 needs" if v == 17 else "variant 19-22 needs")
    if v == 13:
        cg = CONV.get(c.lay)
        ok = f16 and cg is not None and cg["KH"] == 3 and cg["KW"] == 3 and cg["s"] == 1 and cg["p"] == 1 and N == 256 \
            and cg["Cin"] % 32 == 0 and cg["W"] in (16, 32, 64) and cg["H"] % (256 // cg["W"]) == 0 and (not out_f32 or c.split) \
            and c.epi in (EPI_NONE, EPI_GELU, EPI_RELU)
        return None if ok else "variant 13 needs"
    return None


def _cases():
    """Every case of part B, grouped by the variant name its test is parametrized with."""
    by = defaultdict(list)
    std_lays = ("full", "ragged", "mixed", "strided")
    conv_lays = ("c3s1", "c3s2", "c2s2", "c1s2")

    def common(name, v, outs16=("st", "f32", "c16"), f32=True, conv=True, gn=True, r32=True):
        for lay in std_lays:
            for epi in EPIS:
                for out in outs16:
                    by[name].append(Case(v, "f16", out, epi, lay))
                if f32:
                    by[name].append(Case(v, "f32", "st", epi, lay))
        if conv:
            for lay in conv_lays:
                for epi in CONV_EPIS[lay]:
                    by[name].append(Case(v, "f16", "st", epi, lay))
                    if f32:
                        by[name].append(Case(v, "f32", "st", epi, lay))
                by[name].append(Case(v, "f16", "st", EPI_GELU, lay, gn=(8, 64)))
            by[name].append(Case(v, "f16", "st", EPI_RELU, "c3s1", gn=(4, 64)))
        if gn:
            for epi in EPIS:
                by[name].append(Case(v, "f16", "st", epi, "gnp", gn=(8 if epi % 2 else 4, 64)))
            by[name].append(Case(v, "f16", "st", EPI_GELU, "gnp_edge", gn=(8, 64)))
            by[name].append(Case(v, "f16", "f32", EPI_RELU, "gnp", gn=(4, 64)))
            if f32:
                by[name].append(Case(v, "f32", "st", EPI_LRELU, "gnp", gn=(8, 64)))
        if r32:
            for epi in RES_EPIS:
                by[name].append(Case(v, "f16", "r32", epi, "mixed"))
                by[name].append(Case(v, "f16", "r32", epi, "strided"))

    for v in TILE:
        common(f"v{v}", v)
        by[f"v{v}"].append(Case(v, "f16", "st", EPI_NONE, "sk", sk=4))                     # split-K elsewhere than on 4: refused
        for lay in std_lays:                                                                # +500: the generic epilogue on full tiles
            for epi in EPIS:
                by[f"v{v}+500"].append(Case(500 + v, "f16", "st", epi, lay))
        by[f"v{v}+500"].append(Case(500 + v, "f16", "st", EPI_GELU, "gnp", gn=(8, 64)))
        by[f"v{v}+500"].append(Case(500 + v, "f16", "st", EPI_SCALE_RES, "c3s1"))
    common("v0", 0)
    for v in (13, 813, 913):
        for lay in ("win16", "win32"):
            for epi in EPIS:
                for out in ("st", "f32", "c16"):
                    by[f"v{v}"].append(Case(v, "f16", out, epi, lay))
            by[f"v{v}"].append(Case(v, "f16", "st", EPI_GELU, lay, gn=(8, 64)))
            by[f"v{v}"].append(Case(v, "f32", "st", EPI_NONE, lay))
        by[f"v{v}"].append(Case(v, "f16", "st", EPI_NONE, "c3s1"))                        # Cout 128: not the window kernel's
        by[f"v{v}"].append(Case(v, "f16", "r32", EPI_SCALE_RES, "win16"))
    common("v18", 18, conv=True, r32=False)
    for lay in ("c3s1", "c3s2", "win16"):
        for rows in (16, 32, 64):
            by["v18"].append(Case(18, "f16", "st", EPI_GELU, lay, gn=(8, rows)))
    by["v18"].append(Case(18, "f16", "st", EPI_NONE, "sk", sk=4))                          # ignored
    by["v18"].append(Case(18, "f16", "r32", EPI_SCALE_RES, "full"))
    by["v18"].append(Case(7, "f16", "st", EPI_GELU, "gnp", gn=(8, 32)))                    # 32-row chunks elsewhere: refused
    for v in (218, 318, 418):
        for epi in (EPI_NONE, EPI_GELU, EPI_SCALE_RES):
            by["v18"].append(Case(v, "f16", "st", epi, "mixed"))
    for lay in ("gemv8", "gemv3", "full"):
        for epi in EPIS:
            by["v23"].append(Case(23, "f16", "st", epi, lay))
        by["v23"].append(Case(23, "f16", "f32", EPI_GELU, lay))
        by["v23"].append(Case(23, "f32", "st", EPI_NONE, lay))
    for v in (16, 17, 19, 20, 21, 22):
        for lay in ("wreg", "wreg_ldc", "mixed"):
            for epi in EPIS:
                by[f"v{v}"].append(Case(v, "f16", "st", epi, lay))
        by[f"v{v}"].append(Case(v, "f16", "f32", EPI_NONE, "wreg"))
        by[f"v{v}"].append(Case(v, "f16", "c16", EPI_NONE, "wreg"))
        by[f"v{v}"].append(Case(v, "f16", "st", EPI_GELU, "gnp", gn=(8, 64)))
        by[f"v{v}"].append(Case(v, "f32", "st", EPI_NONE, "wreg"))
    for sk in (4, 7, None):                                                                 # split-K on variant 4 (reduce kernel)
        for epi in EPIS:
            for st, out in (("f16", "st"), ("f16", "f32"), ("f32", "st")):
                by["splitk"].append(Case(4, st, out, epi, "sk", sk=sk))
        by["splitk"].append(Case(4, "f16", "c16", EPI_NONE, "sk", sk=sk))                 # c16 turns split-K off (ops.gemm)
    for v in (0, 4, 7, 8, 10, 13, 3):                                                       # split-operand mode
        for lay in ("mixed", "full"):
            for epi in EPIS:
                by["split"].append(Case(v, "f16", "f32", epi, lay, split=True))
            by["split"].append(Case(v, "f16", "planes", EPI_GELU, lay, split=True))
            by["split"].append(Case(v, "f16", "planes", EPI_LRELU, lay, split=True))
        for epi in EPIS:
            by["split"].append(Case(v, "f16", "f32", epi, "gnp", gn=(8, 64), split=True))
        for lay in ("c3s1", "c3s2", "c2s2", "win16"):
            by["split"].append(Case(v, "f16", "f32", EPI_RELU if lay != "c3s1" else EPI_RES_RELU, lay, split=True))
            by["split"].append(Case(v, "f16", "f32", EPI_GELU, lay, gn=(8, 64), split=True))
        by["split"].append(Case(v, "f16", "f32", EPI_GELU, "win32", gn=(8, 64), split=True))
    for epi in EPIS:
        by["split"].append(Case(4, "f16", "f32", epi, "sk", sk=4, split=True))
    for v in (0, 8, 10, 12, 7, 4):                                                          # LayerNorm folded into the epilogue
        by["lnfold"].append(Case(v, "f16", "st", EPI_LNFOLD_GELU, "full"))
        by["lnfold"].append(Case(v, "f16", "st", EPI_LNFOLD_GELU, "mixed"))
    by["lnfold"].append(Case(8, "f16", "f32", EPI_LNFOLD_GELU, "full"))
    return by


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------- operands
def _rng(seed):
    return torch.Generator().manual_seed(seed)


def operands(lay, st, split=False, seed=0):
    """Host operands of a layout with spread magnitudes: W columns scaled by 1e-2 .. 10, biases mixed large / small, every 17th row of
    X large enough to take |v| past the GELU clamp.  Values are rounded to the storage type (fp16 storage) or kept fp32."""
    M, N, K, hw = geom(lay)
    g = _rng(1000 + seed + 7 * len(lay))
    if lay in CONV:
        c = CONV[lay]
        x = torch.randn(c["B"], c["H"], c["W"], c["Cin"], generator=g)
        x[::2, ::3] *= 4.0
    else:
        x = torch.randn(M, K, generator=g)
        x[::17] *= 6.0
    colscale = 10.0 ** (torch.rand(N, generator=g) * 3.0 - 2.0)
    w = torch.randn(N, K, generator=g) * K ** -0.5 * colscale[:, None]
    has_b = (CONV[lay] if lay in CONV else PLAIN[lay])["bias"]
    b = torch.randn(N, generator=g) * torch.where(torch.arange(N) % 3 == 0, 5.0, 0.01) if has_b else None
    r = torch.randn(M, N, generator=g) * 2.0
    gam = (torch.rand(N, generator=g) * 1.9 + 0.1) * torch.where(torch.arange(N) % 5 == 0, -1.0, 1.0)
    if st == "f16" and not split:
        x, w = x.half().float(), w.half().float()
    return x, w, b, r, gam


_LIN = {}


def lin_for(c):
    key = (c.lay, c.st, c.split)
    if key not in _LIN:
        x, w, b, r, gam = operands(c.lay, c.st, c.split)
        if c.lay in CONV:
            cg = CONV[c.lay]
            lin = gr.lin_conv(x, w, cg["KH"], cg["KW"], cg["s"], cg["p"], b, split=c.split)
        else:
            lin = gr.lin_plain(x, w, b, split=c.split)
        _LIN[key] = ((x, w, b, r, gam), lin)
    return _LIN[key]


def gelu_form(c):
    if c.st == "f32" or c.split or c.out == "r32":
        return GELU_ERF
    if c.variant % 100 in (20, 21):
        return GELU_PK16
    return GELU_POLY2          # (covers gelu_erf too, which the split-K reduce kernel runs)


# ---------------------------------------------------------------------------------------------------------------- launching
def launch(o, c, host, bufs=None):
    """Run case c once into fresh sentinel-filled buffers, collected in `bufs` ({name: buffer}) as they are made."""
    bufs = {} if bufs is None else bufs
    x, w, b, r, gam = host
    M, N, K, hw = geom(c.lay)
    dev = "cuda"
    dt = torch.float16 if c.st == "f16" else torch.float32
    conv = c.lay in CONV
    L = PLAIN.get(c.lay, {})
    ldc = L.get("ldc", N)
    ldres = L.get("ldres", N)
    if c.split:
        xd = x.to(dev)
        wd = o.split_weights(w, dev)
    else:
        if conv:
            xd = x.to(dev, dt)
        else:
            ldx = L.get("ldx") or K
            xb = torch.zeros(M, ldx, dtype=dt, device=dev)
            xb[:, :K] = x.to(dev, dt)
            xd = xb[:, :K]
        wd = w.to(dev, dt)
    out_dt = dt if c.out == "st" else torch.float32
    if c.out == "planes":
        cb = torch.full((2 * M * N + 64,), SENT, dtype=torch.float16, device=dev)
        bufs["C"] = cb
        out = cb[: 2 * M * N].view(torch.float32).view(M, N)
        ldc = N
    else:
        cb = torch.full((M + 8, ldc), SENT, dtype=out_dt, device=dev)
        bufs["C"] = cb
        out = cb[:M, :N]
    kw = {}
    if c.epi in RES_EPIS:
        rdt = torch.float32 if (c.out == "r32" or c.split) else dt
        rb = torch.full((M, ldres), -SENT, dtype=rdt, device=dev)
        rb[:, :N] = r.to(dev, rdt)
        kw["residual"] = rb[:, :N]
    if c.epi == EPI_SCALE_RES:
        kw["gamma"] = gam.to(dev)
    if c.out in ("c16", "r32"):
        c16 = torch.full((M + 8, N + 12), SENT, dtype=torch.float16, device=dev)
        bufs["c16"] = c16
        kw["out16"] = c16[:M, :N]
    if c.gn:
        cpg, rows = c.gn
        nent = M // rows * (N // cpg) * 2
        gb = torch.full((nent + 64,), SENT, dtype=torch.float32, device=dev)
        bufs["gn"] = gb
        kw["gn"] = (gb, N // cpg, hw) if rows == 64 else (gb, N // cpg, hw, rows)
    if conv:
        cg = CONV[c.lay]
        kw["conv"] = dict(B=cg["B"], H=cg["H"], W=cg["W"], Cin=cg["Cin"], KH=cg["KH"], KW=cg["KW"], stride=cg["s"], pad=cg["p"])
    o.gemm(xd, wd, out, bias=None if b is None else b.to(dev), epilogue=c.epi, variant=c.variant, splitk=c.sk,
           out_planes=c.out == "planes", **kw)
    return bufs


def _values(c, bufs, M, N):
    if c.out == "planes":
        p = bufs["C"][: 2 * M * N].double().cpu()
        return p[: M * N].view(M, N) + p[M * N:].view(M, N) * 2.0 ** -11
    return bufs["C"][:M, :N].double().cpu()


def run_case(o, c):
    """(max err / bound or None for a refusal, problems)"""
    M, N, K, hw = geom(c.lay)
    if c.epi == EPI_LNFOLD_GELU:
        return run_lnfold(o, c)
    host, lin = lin_for(c)
    exp = expected(c)
    if exp is not None:
        bufs = {}
        try:
            launch(o, c, host, bufs)
        except gr_error() as e:
            if exp not in str(e):
                return None, [f"{c}: refused with '{e}', table expects '{exp}'"]
            if "C" in bufs and not bool((bufs["C"] == SENT).all()):
                return None, [f"{c}: refused after writing the output"]
            return None, []
        torch.cuda.synchronize()
        return None, [f"{c}: ran, table expects a refusal ('{exp}')"]
    probs = []
    try:
        bufs = launch(o, c, host)
    except gr_error() as e:
        return None, [f"{c}: refused ('{e}'), table expects ok"]
    out = "f16" if (c.out == "st" and c.st == "f16") else ("planes" if c.out == "planes" else "f32")
    lean_res = out == "f16" and c.variant // 100 != 5
    r16 = c.st == "f16" and c.out != "r32" and not c.split          # the residual as the kernel reads it
    r = host[3].half().float() if r16 else host[3]
    ref, bound, pre = gr.epilogue(lin, c.epi, out, gelu_form(c), r=r, g=host[4], lean_res=lean_res)
    got = _values(c, bufs, M, N)
    ratio, msg = gr.check(got, ref, bound, str(c))
    if msg:
        probs.append(msg)
    cb = bufs["C"].cpu()
    if c.out == "planes":
        if not bool((cb[2 * M * N:] == SENT).all()):
            probs.append(f"{c}: wrote past the planes")
    else:
        if not (bool((cb[M:] == SENT).all()) and bool((cb[:M, N:] == SENT).all())):
            probs.append(f"{c}: wrote past M or N")
    if "c16" in bufs:
        c16 = bufs["c16"].cpu()
        if not torch.equal(c16[:M, :N], cb[:M, :N].half()):
            probs.append(f"{c}: c16 is not the fp32 output rounded to fp16")
        if not (bool((c16[M:] == SENT).all()) and bool((c16[:M, N:] == SENT).all())):
            probs.append(f"{c}: wrote past the c16 region")
    if c.gn:
        cpg, rows = c.gn
        sref, sb = gr.gn_reference(ref, pre, M // hw, hw, N // cpg, rows)
        gb = bufs["gn"].cpu()
        n = sref.numel()
        r2, m2 = gr.check(gb[:n], sref, sb, f"{c} gn_partial (flat index = ((image * chunks + chunk) * groups + group) * 2 + sum/sq)")
        ratio = max(ratio, r2)
        if m2:
            probs.append(m2)
        if not bool((gb[n:] == SENT).all()):
            probs.append(f"{c}: gn_partial written past the last chunk")
    again = launch(o, c, host)
    for k in bufs:
        if not torch.equal(bufs[k], again[k]):
            probs.append(f"{c}: second launch differs in {k}")
    return ratio, probs


def run_lnfold(o, c):
    """GP_EPI_LNFOLD_GELU, built as test_hip_ops.test_dwconv7_raw_stats_and_lnfold_gemm builds it: X = un-normalised rows (fp16),
    per-row (sum, sum of squares) over 128-channel slabs, W = fc.weight * ln.weight, colsum, bias = fc.weight @ ln.bias + fc.bias."""
    M, N, K, hw = geom(c.lay)
    K = 512
    g = _rng(77 + M)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).half()
    lw, lb = 1.0 + 0.3 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    w1 = torch.randn(N, K, generator=g) * K ** -0.5 * (10.0 ** (torch.rand(N, generator=g) * 2 - 1))[:, None]
    b1 = torch.randn(N, generator=g)
    wg = (w1 * lw[None, :]).half()
    cs = wg.float().sum(1)
    cb = (w1 @ lb + b1).float()
    xs = x.float().view(M, K // 128, 128)
    stats = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], 1).contiguous()        # (M, 2, nslab) fp32
    eps = 1e-6
    st64 = stats.double()
    mu = st64[:, 0].sum(-1) / K
    var = (st64[:, 1].sum(-1) / K - mu * mu).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    x64, w64 = x.double(), wg.double()
    acc, a = x64 @ w64.t(), x64.abs() @ w64.abs().t()
    v = rstd[:, None] * (acc - mu[:, None] * cs.double()[None, :]) + cb.double()[None, :]
    # the kernel: fp32 slab sums, var = E[x^2] - mu^2 in fp32 (6 roundings of E[x^2] + mu^2 relative), rsq (1 ulp), two fmas
    drel = 0.5 * 8 * gr.U32 * (st64[:, 1].sum(-1) / K + mu * mu) / (var + eps) + 4 * gr.U32
    a_v = rstd[:, None] * (a + mu.abs()[:, None] * cs.double().abs()[None, :]) + cb.double().abs()[None, :]
    e_v = gr.c_acc(K) * a_v + drel[:, None] * (v - cb.double()[None, :]).abs()
    lin = gr.Lin(v, a_v, K)
    lin.e_acc = e_v
    ref, bound, _ = gr.epilogue(lin, EPI_GELU, "f16" if c.out == "st" else "f32", GELU_POLY2)
    exp = expected(Case(c.variant, "f16", c.out, EPI_LNFOLD_GELU, "full" if M % 256 == 0 and N % 256 == 0 else c.lay))
    dev = "cuda"
    ln = (stats.to(dev), cs.to(dev), K // 128, eps)
    outs = []
    for _ in range(2):
        buf = torch.full((M + 8, N), SENT, dtype=torch.float16 if c.out == "st" else torch.float32, device=dev)
        try:
            o.gemm(x.to(dev), wg.to(dev), buf[:M], bias=cb.to(dev), epilogue=EPI_LNFOLD_GELU, ln=ln, variant=c.variant)
        except gr_error() as e:
            if exp is None or exp not in str(e):
                return None, [f"{c}: refused with '{e}', table expects {exp or 'ok'}"]
            return None, []
        if exp is not None:
            return None, [f"{c}: ran, table expects a refusal ('{exp}')"]
        outs.append(buf.cpu())
    ratio, msg = gr.check(outs[0][:M].double(), ref, bound, str(c))
    probs = [msg] if msg else []
    if not bool((outs[0][M:] == SENT).all()):
        probs.append(f"{c}: wrote past M")
    if not torch.equal(outs[0], outs[1]):
        probs.append(f"{c}: second launch differs")
    return ratio, probs


def gr_error():
    from givepose_amd._lib import GivePoseHipError
    return GivePoseHipError


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gemm_conformance(name):
    from givepose_amd import ops as o
    gr.set_threads()
    nok = nref = 0
    worst = 0.0
    probs = []
    for c in CASES[name]:
        ratio, p = run_case(o, c)
        probs += p
        if ratio is None:
            nref += 1
        else:
            nok += 1
            worst = max(worst, ratio)
    refused = [f"{c} -> '{expected(c)}'" for c in CASES[name] if expected(c) is not None]
    print(f"\n{name}: {nok} ok, {nref} refused, max err/bound {worst:.3g}")
    for line in refused:
        print("  refused:", line)
    assert not probs, "\n".join(probs[:40]) + (f"\n... {len(probs)} problems" if len(probs) > 40 else "")


# ---------------------------------------------------------------------------------------------------------------- C: GELU domain
def _finite_f16():
    bits = np.arange(65536, dtype=np.uint16)
    vals = bits.view(np.float16)
    return torch.from_numpy(vals[np.isfinite(vals)].astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["lean_f16", "generic_f16", "tile_f32", "v18", "v20", "v21", "v23"])
def test_gelu_whole_fp16_domain(form):
    """Every finite fp16 value through a GELU epilogue: one-hot X (X[m, m % K] = 1, no bias), so the accumulator is exactly one weight
    and C[m, n] = GELU(W[n, m % K]).  The accumulation is exact (one non-zero product): e_acc = 0 here."""
    from givepose_amd import ops as o
    vals = _finite_f16()
    variant, out_dt, K, N, M = {"lean_f16": (8, torch.float16, 64, 1024, 256), "generic_f16": (508, torch.float16, 64, 1024, 256),
                                "tile_f32": (8, torch.float32, 64, 1024, 256), "v18": (18, torch.float16, 64, 1024, 256),
                                "v20": (20, torch.float16, 512, 256, 512), "v21": (21, torch.float16, 512, 256, 512),
                                "v23": (23, torch.float16, 512, 8192, 8)}[form]
    krows = min(K, M)                                    # columns of W the one-hot rows reach
    slots = N * krows
    assert slots >= vals.numel()
    w = torch.zeros(N, K)
    fill = torch.cat([vals, torch.zeros(slots - vals.numel())])
    w[:, :krows] = fill.view(N, krows)
    x = torch.zeros(M, K)
    x[torch.arange(M), torch.arange(M) % K] = 1.0
    out = torch.empty(M, N, dtype=out_dt, device="cuda")
    o.gemm(x.half().cuda(), w.half().cuda(), out, epilogue=EPI_GELU, variant=variant)
    got = out.double().cpu()
    v = w.double()[:, torch.arange(M) % K].t()         # (M, N): the value each output element saw
    lin = gr.Lin(v, v.abs(), K)
    lin.e_acc = torch.zeros_like(v)
    fm = GELU_PK16 if variant in (20, 21) else GELU_POLY2
    ref, bound, _ = gr.epilogue(lin, EPI_GELU, "f16" if out_dt == torch.float16 else "f32", fm)
    err = (got - ref).abs()
    if out_dt == torch.float16:      # distance from the correctly rounded result: the activation's own error
        err = (got - ref.half().double()).abs()
    inside = v.abs() <= 4.4
    print(f"\nGELU {form} ({fm}): max |err| {float(err[inside].max()):.3g} for |v| <= 4.4, "
          f"max |err| / |v| {float((err[~inside] / v.abs()[~inside]).max()):.3g} beyond"
          f"{' (against the exact GELU rounded to fp16)' if out_dt == torch.float16 else ''}")
    ratio, msg = gr.check(got, ref, bound, f"GELU {form}")
    print(f"GELU {form}: max err/bound {ratio:.3g}")
    assert msg is None, msg


# ---------------------------------------------------------------------------------------------------------------- D: the checker
def _d_data(M=256, N=128, K=256, seed=5):
    """Host operands with the matrix's own shapes and scales (operands() of a plain layout), float64 reference."""
    g = _rng(seed)
    x = torch.randn(M, K, generator=g).half().float()
    x[::17] *= 6.0
    colscale = 10.0 ** (torch.rand(N, generator=g) * 3.0 - 2.0)
    w = (torch.randn(N, K, generator=g) * K ** -0.5 * colscale[:, None]).half().float()
    b = torch.randn(N, generator=g) * torch.where(torch.arange(N) % 3 == 0, 5.0, 0.01)
    r = (torch.randn(M, N, generator=g) * 2.0).half().float()
    gam = (torch.rand(N, generator=g) * 1.9 + 0.1) * torch.where(torch.arange(N) % 5 == 0, -1.0, 1.0)
    return x, w, b, r, gam, gr.lin_plain(x, w, b)


def _f16(t):
    return torch.from_numpy(t.numpy().astype(np.float16).astype(np.float64))


def _f32(t):
    return torch.from_numpy(t.numpy().astype(np.float32).astype(np.float64))


def _rejects(got, ref, bound):
    ratio, msg = gr.check(got, ref, bound, "perturbed")
    return msg is not None


def test_checker_rejects_bias_rounded_to_fp16():
    x, w, b, r, gam, lin = _d_data()
    ref, bound, _ = gr.epilogue(lin, EPI_NONE, "f32")
    bad = _f32(lin.v - b.double() + b.half().double())
    assert _rejects(bad, ref, bound)


def test_checker_rejects_lrelu_slope_001():
    x, w, b, r, gam, lin = _d_data()
    ref, bound, _ = gr.epilogue(lin, EPI_LRELU, "f16")
    bad = _f16(torch.where(lin.v > 0, lin.v, 0.01 * lin.v))
    assert _rejects(bad, ref, bound)


def test_checker_rejects_one_k_block_left_out_of_one_tile():
    x, w, b, r, gam, lin = _d_data()
    ref, bound, _ = gr.epilogue(lin, EPI_NONE, "f16")
    v = lin.v.clone()
    v[128:256, 0:128] -= x[128:256, 32:64].double() @ w[0:128, 32:64].double().t()
    assert _rejects(_f16(v), ref, bound)


def test_checker_rejects_residual_read_with_ldc():
    x, w, b, r, gam, lin = _d_data()
    M, N = r.shape
    ldres, ldc = N + 8, N
    rb = torch.randn(M * ldres + 64, generator=_rng(9)).half().float()
    rb.view(-1)[: M * ldres].view(M, ldres)[:, :N] = r
    right = rb[: M * ldres].view(M, ldres)[:, :N]
    wrong = torch.as_strided(rb, (M, N), (ldc, 1))
    ref, bound, _ = gr.epilogue(lin, EPI_SCALE_RES, "f16", r=right, g=gam, lean_res=True)
    bad = _f16(wrong.double() + gam.double() * lin.v)
    assert _rejects(bad, ref, bound)


def test_checker_rejects_sigmoid_gelu_fp32():
    x, w, b, r, gam, lin = _d_data()
    ref, bound, _ = gr.epilogue(lin, EPI_GELU, "f32", GELU_ERF)
    bad = _f32(lin.v * torch.sigmoid(1.702 * lin.v))
    assert _rejects(bad, ref, bound)


def test_checker_rejects_gamma_applied_twice():
    x, w, b, r, gam, lin = _d_data()
    ref, bound, _ = gr.epilogue(lin, EPI_SCALE_RES, "f16", r=r, g=gam, lean_res=True)
    g2 = gam.double() * gam.double()
    bad = _f16(r.double() + g2 * lin.v)
    assert _rejects(bad, ref, bound)


def test_checker_rejects_gn_chunk_written_into_the_next():
    x, w, b, r, gam, lin = _d_data(M=512, N=128, K=256)
    ref, bound, pre = gr.epilogue(lin, EPI_GELU, "f16", GELU_POLY2)
    hw, groups = 256, 16
    sref, sb = gr.gn_reference(ref, pre, 2, hw, groups)
    part = sref.view(2, hw // 64, groups, 2).clone()
    part[0, 2] = part[0, 1]                 # chunk 1 of image 0 written where chunk 2 belongs (and chunk 2 lost)
    assert _rejects(part.reshape(-1), sref, sb)
    assert not _rejects(sref + 0.5 * sb, sref, sb)


def test_checker_accepts_lean_double_rounding():
    """Negative control: the lean residual epilogue rounds gamma * v to fp16, adds the fp16 residual in fp16 and rounds again.
    That is legitimate and must pass: the bound is not tighter than correct code needs."""
    x, w, b, r, gam, lin = _d_data()
    v32 = lin.v.numpy().astype(np.float32)
    for epi in (EPI_SCALE_RES, EPI_RES_RELU):
        g = gam.numpy().astype(np.float32) if epi == EPI_SCALE_RES else np.ones(lin.v.shape[1], np.float32)
        h = (v32 * g[None, :]).astype(np.float16)
        o16 = (h + r.numpy().astype(np.float16)).astype(np.float16)
        if epi == EPI_RES_RELU:
            o16 = np.maximum(o16, np.float16(0))
        ref, bound, _ = gr.epilogue(lin, epi, "f16", r=r, g=gam if epi == EPI_SCALE_RES else None, lean_res=True)
        ratio, msg = gr.check(torch.from_numpy(o16.astype(np.float64)), ref, bound, "lean double rounding")
        print(f"lean double rounding {EPI_NAMES[epi]}: max err/bound {ratio:.3g}")
        assert msg is None, msg


def test_table_is_written_down():
    """The table has both outcomes for the families the issue lists (CPU: no launch)."""
    n = {k: (sum(expected(c) is None for c in v), sum(expected(c) is not None for c in v)) for k, v in CASES.items()}
    for k in ("v7", "v8", "v13", "v18", "v23", "v16", "split", "lnfold"):
        assert n[k][0] > 0 and n[k][1] > 0, (k, n[k])


# ---------------------------------------------------------------------------------------------------------------- E: dispatch closure
_GEMM = re.compile(r"^gemm v(\d+) M(\d+) N(\d+) K(\d+) epi(\d+)( splitK)?( \+gn)?( split3)?$")
_CONV = re.compile(r"^conv(\d+)x(\d+) s(\d+) v(\d+) (\d+)x(\d+) Cin(\d+) Cout(\d+) M(\d+)( \+gn(16|32)?)?( split3)?$")


def _key_of_case(c):
    v = c.variant % 100
    if v == 13 or c.variant in (813, 913):
        v = 13
    gn = "-" if not c.gn else ("gn" if c.gn[1] == 64 else f"gn{c.gn[1]}")
    sk = c.sk is None or c.sk > 1
    if c.lay in CONV:
        cg = CONV[c.lay]
        return ("conv", cg["KH"], cg["KW"], cg["s"], v, None, gn, False, c.split)
    return ("gemm", 0, 0, 0, v, c.epi, "gn" if c.gn else "-", sk and v == 4, c.split)


def ok_keys():
    keys = set()
    for cs in CASES.values():
        for c in cs:
            if c.variant % 100 != 0 and c.variant // 100 in (0, 2, 3, 4, 8, 9) and expected(c) is None and c.st == "f16":
                keys.add(_key_of_case(c))
    return keys


def _key_of_label(lab):
    m = _GEMM.match(lab)
    if m:
        return ("gemm", 0, 0, 0, int(m.group(1)), int(m.group(5)), "gn" if m.group(7) else "-", bool(m.group(6)), bool(m.group(8)))
    m = _CONV.match(lab)
    if m:
        gn = "-" if not m.group(10) else ("gn" + (m.group(11) or ""))
        return ("conv", int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), None, gn, False, bool(m.group(12)))
    return None


def test_label_parser():
    assert _key_of_label("gemm v21 M16384 N2048 K512 epi1") == ("gemm", 0, 0, 0, 21, 1, "-", False, False)
    assert _key_of_label("gemm v4 M64 N256 K8192 epi3 splitK") == ("gemm", 0, 0, 0, 4, 3, "-", True, False)
    assert _key_of_label("gemm v8 M131072 N256 K256 epi0 +gn") == ("gemm", 0, 0, 0, 8, 0, "gn", False, False)
    assert _key_of_label("conv3x3 s1 v13 64x64 Cin256 Cout256 M262144 +gn split3") == ("conv", 3, 3, 1, 13, None, "gn", False, True)
    assert _key_of_label("conv3x3 s1 v18 16x16 Cin256 Cout256 M1024 +gn32") == ("conv", 3, 3, 1, 18, None, "gn32", False, False)
    assert _key_of_label("dwconv_ln 7x7") is None


@pytest.mark.gpu
def test_dispatch_closure_of_the_product():
    from givepose_amd import PoseNet, PoseNetConfig
    from test_hip_posenet import _batch, _launch_labels
    keys = ok_keys()
    missing = []
    runs = [("fp16", PoseNetConfig(), torch.float16, False, (1, 4, 16, 64)), ("res32", PoseNetConfig(res_fp32=True), torch.float16, False, (64,)),
            ("split", PoseNetConfig(), torch.float32, True, (4, 64))]
    seen = 0
    for name, cfg, dt, split, Bs in runs:
        net = PoseNet(cfg, dtype=dt, seed=0, split_gemm=split).cuda() if split else PoseNet(cfg, dtype=dt, seed=0).cuda()
        for B in Bs:
            for lab in _launch_labels(net, _batch(B, 3)):
                k = _key_of_label(lab)
                if re.match(r"^(gemm v|conv\d)", lab) and k is None:
                    missing.append(f"{name} B={B}: unparsed label '{lab}'")
                elif k is not None:
                    seen += 1
                    if k not in keys:
                        missing.append(f"{name} B={B}: '{lab}' -> {k} is no ok entry of the table")
        del net
    print(f"\n{seen} gp_gemm labels, {len(keys)} ok table keys")
    assert seen > 0
    assert not missing, "\n".join(missing)
