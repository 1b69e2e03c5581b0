"""Float64 reference of the fused ConvNeXt block MLP (csrc/mlp.hip: gp_convnext_mlp), the per-element bound its outputs must meet,
the operand families and the case / refusal tables of tests/test_mlp_conformance_gpu.py, and a CPU emulation of the kernel's arithmetic
with the deliberately wrong variants tests/test_mlp_reference_cpu.py holds against the bound.  CPU only: nothing here touches a GPU.

    out[m][c] = res[m][c] + gamma[c] * ( sum_h GELU( sum_k x[m][k] W1[h][k] + b1[h] ) W2[c][h] + b2[c] )

The bound is put together from tests/gemm_reference.py (gr) alone -- no constant of its own:
  stage 1   l1 = gr.lin_plain(x, w1, b1);  h_ref, e_h = gr.epilogue(l1, EPI_GELU, "f16", form): the exact GELU and the bound of the fp16
            hidden value the kernel holds (fp32 accumulation over C, the GELU form's claimed error, the rounding to fp16)
  stage 2   v2 = h_ref W2^T + b2,  a2 = (|h_ref| + e_h) |W2|^T + |b2|,  e_acc = gr.c_acc(4C) a2 + e_h |W2|^T
            (fp32 accumulation over 4C of the values the kernel really holds, plus the hidden values' own error carried through W2),
            then gr.epilogue(., EPI_SCALE_RES, "f16", lean_res=True): the kernel rounds gamma * acc to fp16 and adds the fp16 residual
            with a packed fp16 add, which rounds again.
Contract: every |fc1 output| and every gamma * fc2 output stays inside the finite fp16 range.  Overflow of the fp16 hidden tensor is
outside it (the kernel holds the hidden values in fp16 registers); operands() asserts that its data respects this.
"""
import functools
import re
from collections import namedtuple

import numpy as np
import torch

import gemm_reference as gr
from gemm_reference import EPI_GELU, EPI_SCALE_RES, GELU_PK16, GELU_POLY2

SENT = 1234.0
SENT_ROWS = 256

# ---------------------------------------------------------------------------------------------------------------- launch forms
# name -> what selects it and what it launches.  env: the switch (read once per process by the library) that must be set before the
# first launch; rows: rows per workgroup (the grid is M / rows, walked through xcd_chunk); kernel: as written in gp_convnext_mlp.
Form = namedtuple("Form", "name C env s32 gelu rows kernel")
FORMS = {f.name: f for f in (
    Form("c128w4", 128, None, False, GELU_PK16, 128, "convnext_mlp_kernel<128,1,4>"),
    Form("c128w8", 128, ("GP_MLP_WAVES", "8"), False, GELU_PK16, 256, "convnext_mlp_kernel<128,1>"),
    Form("c256", 256, None, False, GELU_PK16, 256, "convnext_mlp_kernel<256,1>"),
    Form("c128g0", 128, ("GP_GELU16", "0"), False, GELU_POLY2, 256, "convnext_mlp_kernel<128,0>"),
    Form("c256g0", 256, ("GP_GELU16", "0"), False, GELU_POLY2, 256, "convnext_mlp_kernel<256,0>"),
    Form("c512", 512, None, False, GELU_PK16, 128, "convnext_mlp512_kernel"),
    Form("c128s32", 128, None, True, GELU_PK16, 128, "convnext_mlp_s32_kernel<128,4>"),
)}
PACK_KERNELS = {"mlp_pack_w2_kernel": (128, 256, 512), "mlp_pack_w2_s32_kernel": (128, 256)}
DEFAULT_FORMS = tuple(n for n, f in FORMS.items() if f.env is None)
ENV_SETTINGS = {("GP_GELU16", "0"): ("c128g0", "c256g0"), ("GP_MLP_WAVES", "8"): ("c128w8",)}
FAMILIES = ("A", "B", "C")


def dense_M(form):
    """Family A: workgroup counts below, at / above 8 and not a multiple of 8 (xcd_chunk's remainder branch): 1, 3, 9, 17 workgroups
    of 256 rows, 2, 6, 18, 34 (C = 512: 1, 5, 9, 17) of 128."""
    return (128, 640, 1152, 2176) if FORMS[form].C == 512 else (256, 768, 2304, 4352)


def cases(form, family):
    """The (family, M, selector) triples of a form."""
    C = FORMS[form].C
    if family == "A":
        return [("A", M, None) for M in dense_M(form)]
    if family == "B":
        return [("B", 128 if C == 512 else 256, s) for s in range(4)]
    if family == "C":
        return [("C", max(256, C), s) for s in range(4)]
    raise ValueError(family)


def case_name(form, case):
    fam, M, s = case
    return f"{form}-{fam}-M{M}" + ("" if s is None else f"-s{s}")


def xcd_chunk(bid, n):
    """common.hpp xcd_chunk."""
    q, r8, xcd, idx = n >> 3, n & 7, bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r8 else r8 * (q + 1) + (xcd - r8) * q) + idx


# ---------------------------------------------------------------------------------------------------------------- W2 packing
def perm16():
    """gp_convnext_mlp_pack_w2 (mlp.hip, header comment): inside every block of 32 hidden units k-slot fq*8 + nt*4 + j takes unit
    nt*16 + fq*4 + j."""
    s = np.arange(32)
    fq, nt, j = s >> 3, (s >> 2) & 1, s & 3
    return nt * 16 + fq * 4 + j


def perm32():
    """gp_convnext_mlp_pack_w2_s32 (mlp.hip, comment of convnext_mlp_s32_kernel): K slot kb*16 + hh*8 + e takes unit
    16 kb + 8 (e / 4) + 4 hh + e % 4."""
    s = np.arange(32)
    kb, hh, e = s >> 4, (s >> 3) & 1, s & 7
    return 16 * kb + 8 * (e >> 2) + 4 * hh + (e & 3)


def pack_w2(w2, perm):
    """w2 (C, 4C) -> the packed order: w2p[c, blk*32 + s] = w2[c, blk*32 + perm[s]]."""
    C, HD = w2.shape
    idx = (np.arange(HD) // 32) * 32 + perm[np.arange(HD) % 32]
    return w2[:, torch.from_numpy(idx)]


def pack_probe(C):
    """fp16 weight (as int16 bit patterns; the pack kernels only move bits) for the bit-exact check of the pack kernels: the code is
    unique per (c % 32, h % 2048) -- C * 2048 positions do not fit fp16's 2^16 codes -- and every further group of 32 rows is the
    same table rotated by 61, so no two rows and no two columns of a 32-block are equal."""
    HD = 4 * C
    c = np.arange(C)[:, None].astype(np.int64)
    h = np.arange(HD)[None, :].astype(np.int64)
    code = ((h % 2048) + 2048 * (c % 32) + 61 * (c // 32)) % 65536
    return torch.from_numpy(code.astype(np.uint16).view(np.int16).copy())


# ---------------------------------------------------------------------------------------------------------------- operands
def _rng(seed):
    return torch.Generator().manual_seed(seed)


Operands = namedtuple("Operands", "x w1 b1 w2 b2 gamma res exact")


@functools.lru_cache(maxsize=None)
def _weights(C, seed=11):
    """The operand scales of _d_data (tests/test_gemm_conformance.py): per-row scales of W1 over 10^+-1, biases mixing 5.0- and
    0.01-sized entries, gamma in +-[0.1, 2] with every 5th entry negative."""
    g = _rng(seed + C)
    HD = 4 * C
    rowscale = 10.0 ** (torch.rand(HD, generator=g) * 2.0 - 1.0)
    w1 = (torch.randn(HD, C, generator=g) * C ** -0.5 * rowscale[:, None]).half().float()
    b1 = torch.randn(HD, generator=g) * torch.where(torch.arange(HD) % 3 == 0, 5.0, 0.01)
    w2 = (torch.randn(C, HD, generator=g) * HD ** -0.5).half().float()
    b2 = torch.randn(C, generator=g) * torch.where(torch.arange(C) % 3 == 0, 5.0, 0.01)
    gamma = (torch.rand(C, generator=g) * 1.9 + 0.1) * torch.where(torch.arange(C) % 5 == 0, -1.0, 1.0)
    return w1, b1, w2, b2, gamma


def _rows(C, M, seed=23):
    g = _rng(seed + C + 7 * M)
    x = torch.randn(M, C, generator=g)
    x[::17] *= 6.0                                              # every 17th row: pre-activations far into both GELU tails
    x = x.half().float()
    res = (torch.randn(M, C, generator=g) * 2.0).half().float()
    return x, res


def onehot_w2(C, s):
    """W2[c, 4c + s] = 1: the four selectors together read every one of the 4C hidden units exactly once."""
    w2 = torch.zeros(C, 4 * C)
    w2[torch.arange(C), 4 * torch.arange(C) + s] = 1.0
    return w2


def finite_f16():
    bits = np.arange(65536, dtype=np.uint16)
    vals = bits.view(np.float16)
    return torch.from_numpy(vals[np.isfinite(vals)].astype(np.float32))


@functools.lru_cache(maxsize=None)
def operands(C, case):
    """Host operands (fp32 tensors holding the values the kernel sees: fp16-representable x, w1, w2, res; fp32 b1, b2, gamma)."""
    fam, M, s = case
    w1, b1, w2, b2, gamma = _weights(C)
    if fam == "A":
        x, res = _rows(C, M)
        return Operands(x, w1, b1, w2, b2, gamma, res, False)
    if fam == "B":
        x, res = _rows(C, M)
        return Operands(x, w1, b1, onehot_w2(C, s), b2, gamma, res, False)
    if fam == "C":
        assert M >= C
        vals = finite_f16()
        assert 4 * C * C >= vals.numel()
        g = _rng(5 + C)
        fill = torch.cat([vals, vals[torch.randint(0, vals.numel(), (4 * C * C - vals.numel(),), generator=g)]])
        w1c = fill[torch.randperm(4 * C * C, generator=g)].view(4 * C, C)
        x = torch.zeros(M, C)
        x[torch.arange(M), torch.arange(M) % C] = 1.0
        return Operands(x, w1c, torch.zeros(4 * C), onehot_w2(C, s), torch.zeros(C), torch.ones(C), torch.zeros(M, C), True)
    raise ValueError(fam)


def is_f16(t):
    return bool((t.half().float() == t).all())


# ---------------------------------------------------------------------------------------------------------------- reference, bound
@functools.lru_cache(maxsize=None)
def _stage1(C, case):
    op = operands(C, case)
    assert is_f16(op.x) and is_f16(op.w1) and is_f16(op.w2) and is_f16(op.res), "the reference must see the values the kernel sees"
    l1 = gr.lin_plain(op.x, op.w1, op.b1)
    if op.exact:                       # one-hot x, no bias: one non-zero product, the accumulation is exact
        l1.e_acc = torch.zeros_like(l1.v)
    assert float(l1.v.abs().max()) <= 65504.0, "fc1 output outside the finite fp16 range: outside the contract"
    return l1


@functools.lru_cache(maxsize=None)
def reference(C, case, gelu_form):
    """(ref, bound) of one case, float64 (M, C)."""
    gr.set_threads()
    op = operands(C, case)
    l1 = _stage1(C, case)
    h_ref, e_h, _ = gr.epilogue(l1, EPI_GELU, "f16", gelu_form)
    W2, aW2 = op.w2.double(), op.w2.double().abs()
    v2 = h_ref @ W2.t() + op.b2.double()
    a2 = (h_ref.abs() + e_h) @ aW2.t() + op.b2.double().abs()
    lin = gr.Lin(v2, a2, 4 * C)
    carried = e_h @ aW2.t()
    lin.e_acc = (torch.zeros_like(a2) if op.exact else gr.c_acc(4 * C) * a2) + carried     # family C: h * 1 + 0, exact
    assert float((op.gamma.double()[None, :] * v2).abs().max()) <= 65504.0, "gamma * fc2 output outside the finite fp16 range"
    ref, bound, _ = gr.epilogue(lin, EPI_SCALE_RES, "f16", r=op.res, g=op.gamma, lean_res=True)
    return ref, bound


def check_case(form, case, got):
    """(max err / bound, message or None) of a form's output for a case."""
    f = FORMS[form]
    ref, bound = reference(f.C, case, f.gelu)
    return gr.check(got, ref, bound, case_name(form, case))


def gelu_summary(form, case, got):
    """Family C: the two figures test_gelu_whole_fp16_domain prints -- max |err| for |v| <= 4.4 and max |err| / |v| beyond, against
    the exact GELU rounded to fp16."""
    f = FORMS[form]
    op = operands(f.C, case)
    fam, M, s = case
    hsel = 4 * torch.arange(f.C) + s
    v = op.w1.double()[hsel][:, torch.arange(M) % f.C].t()                 # (M, C): the value each output element saw
    exact = gr.gelu_exact(v)
    err = (got.detach().double().cpu() - exact.half().double()).abs()
    inside = v.abs() <= 4.4
    return float(err[inside].max()), float((err[~inside] / v.abs()[~inside]).max())


def sentinels_intact(buf, M):
    """buf: (M + SENT_ROWS, C) whose rows from M on were filled with SENT before the launch."""
    tail = buf[M:].detach().float().cpu()
    return tail.shape[0] == SENT_ROWS and bool((tail == SENT).all())


# ---------------------------------------------------------------------------------------------------------------- refusals (F)
# what: how the call departs from a valid smallest-dense-case launch; frag: what the message must contain; level: "lib" = the
# library's GP_REQUIRE (GivePoseHipError), "ops" = givepose_amd.ops's own argument check (TypeError / RuntimeError, before the library).
Refusal = namedtuple("Refusal", "name env C M what frag level")
REFUSALS = (
    Refusal("M0", None, 128, 0, None, "M=0 must be a positive multiple of 256", "lib"),
    Refusal("M100", None, 128, 100, None, "M=100 must be a positive multiple of 256", "lib"),
    Refusal("M384", None, 128, 384, None, "M=384 must be a positive multiple of 256", "lib"),
    Refusal("M192-C512", None, 512, 192, None, "M=192 must be a positive multiple of 128", "lib"),
    Refusal("C64", None, 64, 256, None, "C=64 must be 128, 256 or 512", "lib"),
    Refusal("C384", None, 384, 256, None, "C=384 must be 128, 256 or 512", "lib"),
    Refusal("fp32-raw", None, 128, 256, "fp32_raw", "fp16 storage only", "lib"),
    Refusal("offset8", None, 128, 256, "offset8", "16-byte aligned", "lib"),
    Refusal("out-is-x", None, 128, 256, "out_is_x", "x and out must not alias", "lib"),
    Refusal("s32-C256", None, 256, 256, "s32", "GP_MLP_S32 exists for C = 128", "lib"),
    Refusal("gelu16off-s32", ("GP_GELU16", "0"), 128, 256, "s32", "GP_MLP_S32 exists for C = 128 with the packed-fp16 GELU", "lib"),
    Refusal("gelu16off-C512", ("GP_GELU16", "0"), 512, 128, None, "packed-fp16 GELU only", "lib"),
    # givepose_amd.ops validates before the library sees a pointer
    Refusal("fp32-tensors", None, 128, 256, "fp32_x", "x: expected torch.float16", "ops"),
    Refusal("fp32-out", None, 128, 256, "fp32_out", "out: expected torch.float16", "ops"),
    Refusal("fp16-b1", None, 128, 256, "fp16_b1", "b1: expected torch.float32", "ops"),
    Refusal("fp16-gamma", None, 128, 256, "fp16_gamma", "gamma: expected torch.float32", "ops"),
    Refusal("strided-out", None, 128, 256, "strided_out", "out tensor has to be contiguous", "ops"),
    Refusal("strided-w1", None, 128, 256, "strided_w1", "w1 tensor has to be contiguous", "ops"),
    Refusal("w1-shape", None, 128, 256, "w1_shape", "w1: expected shape (512, 128)", "ops"),
    Refusal("b1-shape", None, 128, 256, "b1_shape", "b1: expected shape (512,)", "ops"),
    Refusal("w2p-shape", None, 128, 256, "w2p_shape", "w2p: expected shape (128, 512)", "ops"),
    Refusal("b2-shape", None, 128, 256, "b2_shape", "b2: expected shape (128,)", "ops"),
    Refusal("gamma-shape", None, 128, 256, "gamma_shape", "gamma: expected shape (128,)", "ops"),
    Refusal("res-shape", None, 128, 256, "res_shape", "residual: expected shape (256, 128)", "ops"),
    Refusal("x-3d", None, 128, 256, "x_3d", "x: expected shape (M, C)", "ops"),
    Refusal("cpu-x", None, 128, 256, "cpu_x", "x must be a CUDA tensor", "ops"),
)
REFUSAL_BY_NAME = {r.name: r for r in REFUSALS}


def expected(C, M, s32=False, env=None, what=None):
    """None when gp_convnext_mlp must run the launch, else the Refusal: the conformance table read as a function, as `expected` of
    the GEMM suite.  Every numeric case of the table must come out None here, every row of REFUSALS as itself."""
    for r in REFUSALS:
        if r.env in (None, env) and r.C == C and r.M == M and r.what == (what if what else ("s32" if s32 else None)):
            return r
    return None


# ---------------------------------------------------------------------------------------------------------------- dispatch closure
def launches_in_source(text):
    """Every kernel a hipLaunchKernelGGL line of csrc/mlp.hip launches, template arguments without blanks."""
    out = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_0-9]+)\s*(<[^>]*>)?", text):
        out.add(m.group(1) + (m.group(2) or "").replace(" ", ""))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU emulation
GELU16_C = np.array([-4.5349121094e-02, 1.7163085938e-01, -2.2192382812e-01, -1.4266967773e-02,
                     3.2568359375e-01, -2.3901367188e-01, -5.8441162109e-02, 8.1665039062e-02], np.float32).astype(np.float16)
GELU_H = (np.float32(0.5) * np.array([6.9778819482e-11, -7.3778779375e-09, 3.4381198132e-07, -9.3718131897e-06, 1.6778340171e-04,
                                      -2.1052074914e-03, 1.9270481587e-02, -1.3212860816e-01, 7.9751050727e-01], np.float32))


def _fma16(a, b, c):
    """fp16 fma: the product of two fp16 values is exact in float64, the sum is rounded once to fp16."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.float64(c)).astype(np.float16)


def gelu16_emul(v32, clamp=True):
    """common.hpp gelu16_slice, slice by slice, on fp16 values (every operation rounds once, as v_pk_*_f16 does)."""
    with np.errstate(over="ignore", invalid="ignore"):
        xh = v32.astype(np.float16)
        u = np.maximum(xh, -xh)
        if clamp:
            u = np.minimum(u, np.float16(4.0))
        u = _fma16(u, np.float16(0.5), np.float16(-1.0))
        p = _fma16(GELU16_C[7], u, GELU16_C[6])
        for k in range(5, -1, -1):
            p = _fma16(p, u, GELU16_C[k])
        xm = np.maximum(xh, np.float16(0.0))
        return (xm.astype(np.float64) + p.astype(np.float64)).astype(np.float16)


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(np.float32)


def gelu_poly2_emul(v32):
    """common.hpp gelu_poly2 in fp32, then the conversion to fp16."""
    x = v32.astype(np.float32)
    xc = np.clip(x, np.float32(-4.4), np.float32(4.4))
    t = xc * xc
    p = _fma32(np.full_like(t, GELU_H[0]), t, GELU_H[1])
    for k in range(2, 9):
        p = _fma32(p, t, GELU_H[k])
    return (x * _fma32(xc, p, np.float32(0.5))).astype(np.float16)


def gelu_sigmoid_emul(v32):
    x = v32.astype(np.float64)
    with np.errstate(over="ignore"):
        return (x / (1.0 + np.exp(-1.702 * x))).astype(np.float16)


MUTATIONS = ("pack_nt_fq", "pack_s32_for_16", "b1_prev_chunk", "skip_last_chunk", "stale_stage", "gamma_mod16", "b2_after_gamma",
             "no_xcd_remap", "no_clamp", "sigmoid", "reverse_chunks", "single_rounding")


def emulate(op, gelu_form=GELU_PK16, s32=False, mut=None, rows=256, NS=4):
    """The kernel's arithmetic on the CPU: per chunk of 32 hidden units an fp32 GEMM1 with the bias as the accumulator's initial
    value, the GELU of the form, the hidden values rounded to fp16 and laid out in the k-slot order the kernel's registers have,
    GEMM2 against the packed W2 chunk accumulated in fp32 on top of b2; then gamma * acc rounded to fp16 and an fp16 add of the
    residual.  mut: one of MUTATIONS (the last two are legitimate variants).  Returns the (M, C) fp16 output as float64."""
    assert mut is None or mut in MUTATIONS, mut
    x, w1, b1 = op.x.float(), op.w1.float(), op.b1.float()
    M, C = x.shape
    NCH = 4 * C // 32
    kperm = perm32() if s32 else perm16()                         # k-slot -> hidden unit of the chunk, as the kernel's registers hold it
    hperm = kperm
    if mut == "pack_nt_fq":                                       # the slot read as nt*16 + fq*4 + j: the host leaves W2 as it is
        hperm = np.arange(32)
    elif mut == "pack_s32_for_16":
        hperm = perm32()
    w2p = pack_w2(op.w2.float(), hperm)
    acc2 = op.b2.float()[None, :].repeat(M, 1)
    if mut == "b2_after_gamma":
        acc2 = torch.zeros(M, C)
    order = range(NCH - 1, -1, -1) if mut == "reverse_chunks" else range(NCH)
    kp = torch.from_numpy(kperm)
    for ch in order:
        if mut == "skip_last_chunk" and ch == NCH - 1:
            continue
        st = ch - NS if (mut == "stale_stage" and ch >= NS) else ch          # the ring slot never refilled
        bch = (ch - 1) % NCH if mut == "b1_prev_chunk" else ch
        acc1 = torch.addmm(b1[bch * 32:(bch + 1) * 32][None, :], x, w1[st * 32:(st + 1) * 32].t()).numpy()
        if mut == "sigmoid":
            h = gelu_sigmoid_emul(acc1)
        elif gelu_form == GELU_PK16:
            h = gelu16_emul(acc1, clamp=mut != "no_clamp")
        else:
            h = gelu_poly2_emul(acc1)
        hk = torch.from_numpy(h.astype(np.float32))[:, kp]
        acc2 = acc2 + hk @ w2p[:, st * 32:(st + 1) * 32].t()
    gamma = op.gamma.float()
    if mut == "gamma_mod16":
        gamma = gamma[torch.arange(C) % 16]
    gv = (acc2 * gamma[None, :]).numpy()
    if mut == "b2_after_gamma":
        gv = gv + op.b2.float().numpy()[None, :]
    res16 = op.res.numpy().astype(np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        if mut == "single_rounding":
            out = (gv.astype(np.float32) + res16.astype(np.float32)).astype(np.float16)
        else:
            out = (gv.astype(np.float16).astype(np.float64) + res16.astype(np.float64)).astype(np.float16)
    out = torch.from_numpy(out.astype(np.float64))
    if mut == "no_xcd_remap":                                     # workgroup b computed the rows of xcd_chunk(b), stored them at b
        n = M // rows
        src = torch.cat([torch.arange(xcd_chunk(b, n) * rows, (xcd_chunk(b, n) + 1) * rows) for b in range(n)])
        out = out[src]
    return out
