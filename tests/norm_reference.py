"""Float64 references, per-element error bounds, seeded cases and mutations of the norm family of csrc/norm.hip -- gp_dwconv_ln,
gp_dwconv7_raw_stats, gp_layernorm, gp_groupnorm_chunks / _stats / _apply / _upsample2x -- and of gp_upsample_bilinear2x (csrc/misc.hip).
No GPU here: tests/test_norm_reference_cpu.py checks this file against itself, tests/test_norm_conformance_gpu.py holds the kernels
against it.  The machinery (Op, check, check_buffer, e_out, the form of MUTATIONS) is tests/ops_reference.py's; the GELU forms and their
claimed errors are tests/gemm_reference.py's.

v is the exact value on the operands the kernel sees (fp16 operands already rounded, weights in the kernel's (tap, C) layout); every
bound is built from term counts and number formats with u = 2^-24, none is fitted to a result:

  depth-wise conv    c = sum x w + b, a = sum |x||w| + |b|, e_c = (KS^2 + 3) u a  (ops_reference._dwg_full).  The MFMA forms accumulate the
                     49 products of a channel in 32-wide K blocks padded with exact zeros, in fp32, and add the bias afterwards: the same
                     count of roundings of partial sums bounded by a.
  LayerNorm          e_stat = (C + 4) u (|mu| + sqrt(E[c^2])) for the mean and the centring, E = max_c e_c per pixel,
                     e_lin = |ln_w| / sigma (2 + |yh|) (E + e_stat) + 6 u (|ln_w yh| + |ln_b|): _dwg_full's, with 2 u more for rsqrtf (1 ulp).
  one-pass variance  dwconv7_ln_mfma_kernel ("LayerNorm statistics in ONE round", rstd = rsqrtf(fmaxf(a2 * invC - mean * mean, 0.f) + eps))
                     and dwconv7_ln_tall_kernel (the same line behind "LayerNorm statistics (one round)") form var = E[c^2] - mean^2 in fp32:
                       dvar = (C + 6) u (E[c^2] + mu^2) + 2 (|mu| + sqrt(E[c^2])) E       entering as |ln_w yh| dvar / (2 sigma^2).
                     The tall kernel's fmaf(acc, rstd, -mean * rstd) adds u |mu| / sigma, which e_stat covers.  The strip kernel, the LDS-tiled
                     kernel, dwconv3_ln_tile_kernel and the row LayerNorm kernels are two-pass (mean, then centred squares).
  activations        none / ReLU: slope 1.  LeakyReLU 0.1f: + 2 u |v|.  GELU: 1.13 e + the form's claimed error -- fp16 storage: gelu_poly1 in the
                     strip / tile kernels, which is gelu_poly2 on one lane (common.hpp: `gelu_poly2(f32x2{x, x})[0]`), so GELU_POLY1 is GELU_POLY2's
                     4.1e-5; fp32 storage: gelu_erf.
  store              ops_reference.e_out.
  raw statistics     gp_dwconv7_raw_stats: y = c with ONE fp16 rounding; stats (pixel, 2, C / 128) = (sum, sum of squares) of those ROUNDED values
                     per 128-channel slab, bound (128 + 2) u sum |y| resp. sum y^2.
  GroupNorm stats    per (b, chunk, g): (n + 2) u sum |x| resp. sum x^2, n the values of the chunk and group.
  GroupNorm apply    gn_finalize adds the fp32 partials in double: mean = S fl(1 / N), var = Q fl(1 / N) - mean^2, rstd = 1 / sqrt(var + eps) in
                     double, both rounded to fp32; sc = rstd ln_w, sh = fma(-mean, sc, ln_b), y = fma(x, sc, sh) (gn_shift / gn_norm; the fp32
                     instantiation's plain expressions round at most once more per operation).  See _gn_chain.
  upsample           align_corners = True, out = fma(hy, fma(hx, a, lx b), ly fma(hx, c, lx d)): 4 u sum |w||x| for the blend; the source
                     coordinate fl(fl((n - 1) / (2 n - 1)) * dst) is off by up to 2 u (n - 1), and 1 - l rounds once: (2 (n - 1) + 1) u times the
                     largest difference of two blended neighbours (the pair of the exact coordinate and the pair before it), per axis.
"""
import functools
import os
from collections import namedtuple

import torch
import torch.nn.functional as F

from gemm_reference import GELU_ERF, GELU_POLY2, gelu_act_err, gelu_exact
from ops_reference import F64, NAN, SENTINEL, U16, U32, Op, _d, _dw_conv, _gen, _rn, check, check_buffer, e_out, store, with_tail   # noqa: F401

ACT_NONE, ACT_GELU, ACT_RELU, ACT_LRELU = 0, 1, 2, 3
ACT_NAMES = {ACT_NONE: "none", ACT_GELU: "gelu", ACT_RELU: "relu", ACT_LRELU: "lrelu"}
GELU_POLY1 = GELU_POLY2          # gelu_poly1(x) = gelu_poly2({x, x})[0]: the same polynomial, the same claimed 4.1e-5
f16, f32 = torch.float16, torch.float32
TIGHT = 3 * 2.0 ** -11           # zero-mean fp16 cases: median over elements of bound / max(|v|, 1e-3) stays below this


def _dn(dt):
    return "f16" if dt == f16 else "f32"


def _uniform(g, n, half_width):
    return (torch.rand(n, generator=g) * 2 - 1) * half_width


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ activations
def act_value(z, act, slope=0.1):
    if act == ACT_GELU:
        return gelu_exact(z)
    if act == ACT_RELU:
        return z.clamp_min(0)
    if act == ACT_LRELU:
        return torch.where(z > 0, z, slope * z)
    return z


def act_bound(z, e, act, dt):
    """Bound in front of the store of act(z') for any z' within e of z."""
    if act == ACT_GELU:
        return 1.13 * e + gelu_act_err(z, GELU_POLY1 if dt == f16 else GELU_ERF)
    if act == ACT_LRELU:
        return e + 2 * U32 * act_value(z, act).abs()
    return e


def act_f32(z, act):
    return F.gelu(z) if act == ACT_GELU else F.relu(z) if act == ACT_RELU else F.leaky_relu(z, 0.1) if act == ACT_LRELU else z


# ------------------------------------------------------------------------------------------------ buffers with a row stride
def blank_buffer(rows, C, ldy, col0, tail, dtype=F64):
    """What a test hands the kernel: NaN where it must write, SENTINEL in every gap and in `tail` values behind the last row."""
    buf = torch.full((rows * ldy + tail,), SENTINEL, dtype=dtype)
    buf[:rows * ldy].view(rows, ldy)[:, col0:col0 + C] = NAN
    return buf


def filled_buffer(v, ldy, col0, tail):
    rows, C = v.shape
    buf = blank_buffer(rows, C, ldy, col0, tail)
    buf[:rows * ldy].view(rows, ldy)[:, col0:col0 + C] = v.double()
    return buf


def check_strided(buf, v, bound, ldy, col0, what=""):
    """check_buffer for rows of stride ldy whose data sit at columns [col0, col0 + C): every other value must still be SENTINEL."""
    rows, C = v.shape
    buf = buf.detach().cpu().reshape(-1)
    body = buf[:rows * ldy].view(rows, ldy)
    gap = torch.ones(ldy, dtype=torch.bool)
    gap[col0:col0 + C] = False
    rest = torch.cat([body[:, gap].reshape(-1), buf[rows * ldy:]]).double()
    if rest.numel() == 0 or not bool((rest == SENTINEL).all()):
        return float("inf"), f"{what}: a sentinel beside or behind the output was overwritten"
    return check(body[:, col0:col0 + C].reshape(-1), v, bound, what)


# ================================================================================================ gp_dwconv_ln
# forms (kernel instantiations up to C, which the case names)
STRIP_PPT2, STRIP_PPT8, STRIP_F32 = "strip<f16,PPT 2>", "strip<f16,PPT 8>", "strip<f32,PPT 8>"
TILED = "lds-tiled"
MFMA_11, MFMA_21, MFMA_42, MFMA_41 = "mfma<1,1>", "mfma<2,1>", "mfma<4,2>", "mfma<4,1>"
TALL_J8, TALL_J9, TALL_WIDE, QUARTER, PAIR_TH4, PAIR_TH2 = "tall<J 8>", "tall<J 9>", "tall<wide>", "tall<TH 4>", "pair<TH 4>", "pair<TH 2>"
DW3_TH4, DW3_TH2 = "dw3tile<4>", "dw3tile<2>"
REFUSED = "refused"
ONE_PASS = (MFMA_11, MFMA_21, MFMA_42, MFMA_41, TALL_J8, TALL_J9, TALL_WIDE, QUARTER, PAIR_TH4, PAIR_TH2)

# the defaults of the routing helpers of csrc/norm.hip (each reads a GP_DW* variable: with one set the routed cases are skipped)
DW_TALL_MIN_WGS, DW_PAIR_MIN_CROPS, DW3_TILE_MIN, DW_NARROW_BELOW, DW_TALL4_MIN_WGS = 130, 32, 256, 128, 52


def dw_mfma_min_wgs(C):
    return 52 if C == 512 else 33 if C == 256 else 0


def dw_tallw_min_wgs(C):
    return 384 if C == 128 else 256


def routing_env_is_default():
    return not any(k.startswith("GP_DW") for k in os.environ)


def form_taken(B, H, W, C, KS, act_code, n_pixels, dtype):
    """gp_dwconv_ln's routing (csrc/norm.hip) restated condition by condition, for out-of-place launches with every GP_DW* variable unset:
    the first block whose condition holds launches and returns.  act codes >= 100 are dbg = code - 100 with act = none."""
    h16 = dtype == f16
    esz = 2 if h16 else 4
    total = B * H * W
    dbg = act_code - 100 if act_code >= 100 else 0
    act = ACT_NONE if act_code >= 100 else act_code
    k7 = KS == 7 and act == ACT_NONE and n_pixels == total
    tall16 = W == 16 and C in (128, 256, 512)
    tallw = W > 16 and W % 16 == 0 and C in (128, 256)
    # dwconv7_ln_tall_kernel: dw_tall_min_wgs() on 16-wide maps, dw_tallw_min_wgs(C) on wider ones; 110 forces it (111: investigation builds)
    if k7 and h16 and H % 8 == 0 and (tall16 or tallw) and \
            (dbg == 10 or (dbg == 0 and B * (H // 8) * (W // 16) >= (DW_TALL_MIN_WGS if tall16 else dw_tallw_min_wgs(C)))):
        return TALL_WIDE if tallw else TALL_J8 if H <= 16 else TALL_J9
    # pair form: dw_pair_min_crops(), dw_pair_rows() = 2; 113 / 114 force TH = 4 / 2
    if k7 and h16 and W == 8 and H % 4 == 0 and C == 1024 and B % 2 == 0 and (dbg in (13, 14) or (dbg == 0 and B >= DW_PAIR_MIN_CROPS)):
        return PAIR_TH2 if dbg in (14, 0) else PAIR_TH4
    # quarter-image tiles: 52 .. dw_tall_min_wgs() (dw_tall4_enabled()); 112 forces it
    if k7 and h16 and H % 4 == 0 and tall16 and (dbg == 12 or (dbg == 0 and B * (H // 4) >= DW_TALL4_MIN_WGS and B * (H // 8) < DW_TALL_MIN_WGS)):
        return QUARTER
    # dwconv7_ln_mfma_kernel: dw_mfma_min_wgs(C); <4, 1> from 512 workgroups (dw_single_buffer() off)
    wgs = B * (H // 4) * (W // 16)
    if k7 and h16 and (dbg == 0 or dbg >= 5) and dbg < 10 and H % 4 == 0 and W % 16 == 0 and C in (128, 256, 512) and wgs >= dw_mfma_min_wgs(C):
        return MFMA_11 if C == 128 else MFMA_21 if C == 256 else MFMA_41 if wgs >= 512 else MFMA_42
    # dwconv7_ln_tiled_kernel: from 192 tiles of 8 x 8; 104 forces it; instantiated for 1 / 2 / 4 slabs in fp16, 2 / 4 / 8 / 16 in fp32
    if k7 and H % 8 == 0 and W % 8 == 0 and dbg != 7 and (B * (H // 8) * (W // 8) >= 192 or dbg == 4):
        nslab = C // (16 * (16 // esz))
        if nslab in ((1, 2, 4) if h16 else (2, 4, 8, 16)):
            return TILED
    # dwconv3_ln_tile_kernel: dw3_tile_min() tiles, dw3_tile_rows() = 2; 120 + act forces the 4-row tile, 125 + act the 2-row one
    dbg3 = 20 <= dbg < 30
    th3 = (2 if dbg >= 25 else 4) if dbg3 else 2
    act3 = (dbg - 25 if dbg >= 25 else dbg - 20) if dbg3 else act
    if KS == 3 and h16 and C == 256 and act3 == ACT_GELU and H % th3 == 0 and W % 16 == 0 and n_pixels % (th3 * W) == 0 and \
            (dbg3 or n_pixels // 64 >= DW3_TILE_MIN):
        return DW3_TH4 if th3 == 4 else DW3_TH2
    if dbg3:
        return REFUSED
    # dwconv_ln_kernel: dw_narrow_below(), dw3_narrow_always()
    CT = C // (16 // esz)
    PG = 256 // CT
    narrow = h16 and (cdiv(cdiv(n_pixels, 8), PG) < DW_NARROW_BELOW or KS == 3)
    return STRIP_PPT2 if narrow else STRIP_PPT8 if h16 else STRIP_F32


DW = namedtuple("DW", "name form dt B H W C KS act code npix eps offset large")


def _dw_cases():
    out = []

    def add(form, dt, B, H, W, C, KS, act=ACT_NONE, code=None, npix=None, eps=1e-6, offset=0.0, large=False):
        code = act if code is None else code
        total = B * H * W
        name = f"{_dn(dt)}-C{C}-B{B}-{H}x{W}-k{KS}-{ACT_NAMES[act]}" + (f"-code{code}" if code >= 100 else "") + \
            (f"-n{npix}" if npix is not None else "") + ("-eps.25" if eps != 1e-6 else "") + ("-offset" if offset else "")
        out.append(DW(name, form, dt, B, H, W, C, KS, act, code, total if npix is None else npix, eps, offset, large))

    # strip kernel, fp16, 2 pixels per thread
    add(STRIP_PPT2, f16, 2, 8, 16, 512, 7)
    add(STRIP_PPT2, f16, 2, 8, 16, 512, 7, offset=5.0)
    add(STRIP_PPT2, f16, 2, 8, 16, 512, 7, eps=0.25)
    add(STRIP_PPT2, f16, 2, 8, 8, 128, 7)                                   # W = 8: no MFMA form is eligible
    for act in (ACT_GELU, ACT_RELU, ACT_LRELU, ACT_NONE):
        add(STRIP_PPT2, f16, 2, 8, 16, 256, 3, act)
    add(STRIP_PPT2, f16, 2, 8, 16, 256, 3, ACT_GELU, npix=37)
    add(STRIP_PPT2, f16, 2, 8, 16, 256, 3, ACT_GELU, npix=19)               # one row plus 3 pixels
    add(STRIP_PPT2, f16, 2, 8, 16, 512, 7, npix=37)
    add(STRIP_PPT2, f16, 2, 8, 16, 512, 7, npix=19)
    # strip kernel, fp16, 8 pixels per thread: odd B keeps the pair form out, 132 workgroups
    add(STRIP_PPT8, f16, 33, 8, 8, 1024, 7)
    add(STRIP_PPT8, f16, 33, 8, 8, 1024, 7, npix=33 * 64 - 3)               # the last strip is partial
    # strip kernel, fp32
    for C in (64, 1024):
        add(STRIP_F32, f32, 2, 8, 8, C, 3, ACT_GELU)
        add(STRIP_F32, f32, 2, 8, 8, C, 7)
    add(STRIP_F32, f32, 2, 8, 8, 64, 3, ACT_GELU, npix=37)                  # the prefix ends inside a strip
    add(STRIP_F32, f32, 2, 8, 8, 1024, 7, npix=37)
    add(STRIP_F32, f32, 2, 8, 8, 64, 7, eps=0.25)
    # LDS-tiled kernel (act code 104): all its instantiations, 2 x 3 tiles, W % 16 != 0
    for dt, Cs in ((f16, (128, 256, 512)), (f32, (128, 256, 512, 1024))):
        for C in Cs:
            add(TILED, dt, 2, 16, 24, C, 7, code=104)
    add(TILED, f16, 2, 16, 24, 256, 7, code=104, eps=0.25)
    # dwconv7_ln_mfma_kernel: H = 12 keeps every tall form out
    add(MFMA_11, f16, 2, 12, 32, 128, 7)
    add(MFMA_11, f16, 2, 12, 32, 128, 7, offset=5.0)
    add(MFMA_21, f16, 4, 12, 48, 256, 7)
    add(MFMA_21, f16, 4, 12, 48, 256, 7, eps=0.25)
    add(MFMA_42, f16, 5, 12, 64, 512, 7)
    add(MFMA_41, f16, 43, 12, 64, 512, 7, large=True)                       # 516 workgroups: the regime exists at no smaller size
    # dwconv7_ln_tall_kernel, 16 x 8 tiles (110): H = 8 zero rows on both sides (J = 8), H = 24 an interior tile (J = 9)
    for C in (128, 256, 512):
        add(TALL_J8, f16, 2, 8, 16, C, 7, code=110)
        add(TALL_J9, f16, 2, 24, 16, C, 7, code=110)
    add(TALL_J8, f16, 2, 8, 16, 128, 7, code=110, offset=5.0)
    add(TALL_J8, f16, 2, 8, 16, 256, 7, code=110, eps=0.25)
    for C in (128, 256):                                                    # the column-halo form
        add(TALL_WIDE, f16, 2, 16, 48, C, 7, code=110)
    add(TALL_WIDE, f16, 2, 16, 48, 128, 7, code=110, offset=5.0)
    for C in (128, 256, 512):                                               # quarter-image tiles (112)
        add(QUARTER, f16, 2, 12, 16, C, 7, code=112)
    add(QUARTER, f16, 2, 12, 16, 128, 7, code=112, offset=5.0)
    add(QUARTER, f16, 2, 12, 16, 256, 7, code=112, eps=0.25)
    for code, form in ((113, PAIR_TH4), (114, PAIR_TH2)):                   # two 8-wide images per tile
        add(form, f16, 4, 12, 8, 1024, 7, code=code)
    add(PAIR_TH2, f16, 4, 12, 8, 1024, 7, code=114, offset=5.0)
    add(PAIR_TH2, f16, 4, 12, 8, 1024, 7, code=114, eps=0.25)
    # dwconv3_ln_tile_kernel (120 + GELU: 4-row tiles, 125 + GELU: 2-row tiles): whole, and a prefix of 1.5 images
    for code, form in ((121, DW3_TH4), (126, DW3_TH2)):
        add(form, f16, 3, 8, 32, 256, 3, ACT_GELU, code=code)
        add(form, f16, 3, 8, 32, 256, 3, ACT_GELU, code=code, npix=384)
    add(DW3_TH2, f16, 3, 8, 32, 256, 3, ACT_GELU, code=126, eps=0.25)
    return out


DW_CASES = _dw_cases()


@functools.lru_cache(None)
def _dw_operands(dt, B, H, W, C, KS, offset):
    g = _gen(2000 + C + 7 * KS + 13 * H + W + 101 * B + (1 if offset else 0))
    return dict(x=_rn(g, B, H, W, C).to(dt), wt=_rn(g, KS * KS, C, scale=(0.02 if offset else 1.0) / KS).to(dt), bias=_rn(g, C, scale=0.3) + offset,
                ln_w=1 + _uniform(g, C, 0.3), ln_b=_uniform(g, C, 0.3))


def dw_inputs(case):
    return _dw_operands(case.dt, case.B, case.H, case.W, case.C, case.KS, case.offset)


def _dw_conv64(x, wt, b, KS):
    """ops_reference._dw_conv (stride 1, zero padding) as KS^2 shifted multiply-adds on the channels-last tensor: the same float64 sums,
    several times faster on the large case."""
    B, H, W, C = x.shape
    R = KS // 2
    xp = F.pad(x, (0, 0, R, R, R, R))
    acc = b.expand(x.shape).clone()
    for kh in range(KS):
        for kw in range(KS):
            acc.addcmul_(xp[:, kh:kh + H, kw:kw + W, :], wt[kh * KS + kw])
    return acc


def _dw_abs_conv(I, KS):
    return _dw_conv64(_d(I["x"]).abs(), _d(I["wt"]).abs(), _d(I["bias"]).abs(), KS)


def _dw_conv_mut(I, KS, mut=None):
    x, wt, b = _d(I["x"]), _d(I["wt"]), _d(I["bias"])
    B, H, W, C = x.shape
    if mut == "taps_transposed":
        wt = wt.view(KS, KS, C).transpose(0, 1).reshape(KS * KS, C)
    if mut == "no_batch_boundary":
        return _dw_conv64(x.reshape(1, B * H, W, C), wt, b, KS).reshape(B, H, W, C)
    if mut == "pair_as_one_map":
        xp = x.view(B // 2, 2, H, W, C).permute(0, 2, 1, 3, 4).reshape(B // 2, H, 2 * W, C)
        return _dw_conv64(xp, wt, b, KS).view(B // 2, H, 2, W, C).permute(0, 2, 1, 3, 4).reshape(B, H, W, C)
    return _dw_conv(x, wt, b, KS, 1, "edge") if mut == "clamp_to_edge" else _dw_conv64(x, wt, b, KS)


def _ln(c, lw, lb, eps, mut=None, width=None):
    """(mu, sigma, yh, z) of a LayerNorm over the last axis; width: the divisor of mean and variance (the row's own length)."""
    C = c.shape[-1]
    n = C if width is None else width
    mu = c.sum(-1, keepdim=True) / n
    var = ((c - mu) ** 2).sum(-1, keepdim=True) / (n - 1 if mut == "unbiased_variance" else n)
    if mut == "eps_ignored":
        sigma = (var + 1e-6).sqrt()
    elif mut == "eps_outside_root":
        sigma = var.sqrt() + eps
    else:
        sigma = (var + eps).sqrt()
    yh = (c - mu) / sigma
    return mu, sigma, yh, lw * yh + lb


def _ln_bound(c, E, mu, sigma, yh, lw, lb, one_pass):
    C = c.shape[-1]
    m2 = (c * c).mean(-1, keepdim=True)
    e_stat = (C + 4) * U32 * (mu.abs() + m2.sqrt())
    e_lin = lw.abs() / sigma * (2 + yh.abs()) * (E + e_stat) + 6 * U32 * ((lw * yh).abs() + lb.abs())
    if one_pass:
        dvar = (C + 6) * U32 * (m2 + mu * mu) + 2 * (mu.abs() + m2.sqrt()) * E
        e_lin = e_lin + (lw * yh).abs() * dvar / (2 * sigma * sigma)
    return e_lin


def _dw_compute(case, mut=None):
    """(v, bound, pre, |mu| / std per pixel) at every pixel of the map, shape (B H W, C)."""
    I = dw_inputs(case)
    KS, C = case.KS, case.C
    lw, lb = _d(I["ln_w"]), _d(I["ln_b"])
    c = _dw_conv_mut(I, KS, mut).reshape(-1, C)
    mu, sigma, yh, z = _ln(c, lw, lb, case.eps, mut)
    act = ACT_NONE if mut == "act_dropped" else case.act
    v = act_value(z, act, 0.01 if mut == "lrelu_slope_001" else 0.1)
    if mut is not None:
        return v, None, None, None
    e_c = (KS * KS + 3) * U32 * _dw_abs_conv(I, KS).reshape(-1, C)
    E = e_c.max(1, keepdim=True).values
    pre = act_bound(z, _ln_bound(c, E, mu, sigma, yh, lw, lb, case.form is True or case.form in ONE_PASS), case.act, case.dt)
    ratio = (mu.abs() / c.std(1, unbiased=False, keepdim=True)).reshape(-1)
    return v, pre + e_out(v, pre, case.dt), pre, ratio


@functools.lru_cache(None)
def _dw_small(key):
    return _dw_compute(key)


@functools.lru_cache(1)
def _dw_large(case):
    return _dw_compute(case)


def dw_full(case):
    """Cases that differ in name, act code or prefix length only share one evaluation; of the large cases only the last one is kept."""
    return _dw_large(case) if case.large else _dw_small(case._replace(name="", code=0, npix=0, form=case.form in ONE_PASS))


def dw_ref(I, case, mut=None, stored=True):
    """(v, bound) of the case's n_pixels rows.  mut: a deliberately wrong float64 variant (its bound is None)."""
    n = case.npix
    if mut == "prefix_to_strip_boundary":       # a kernel that finishes its last 8-pixel strip: a longer flat buffer
        v = dw_full(case)[0]
        return v[:min(cdiv(n, 8) * 8, v.shape[0])], None
    if mut is not None:
        return _dw_compute(case, mut)[0][:n], None
    v, bound, pre, _ = dw_full(case)
    return v[:n], (bound if stored else pre)[:n]


def dw_mean_over_std(case):
    return float(dw_full(case)[3].median())


def dw_f32(I, case):
    C, KS = case.C, case.KS
    c = _dw_conv(I["x"].float(), I["wt"].float(), I["bias"], KS, 1).reshape(-1, C)
    return act_f32(F.layer_norm(c, (C,), I["ln_w"], I["ln_b"], case.eps), case.act)[:case.npix]


# ================================================================================================ gp_dwconv7_raw_stats
RAW = namedtuple("RAW", "name B H W C")
RAW_CASES = [RAW(f"C{C}-B2-12x32", 2, 12, 32, C) for C in (128, 512)]


def raw_inputs(case):
    return _dw_operands(f16, case.B, case.H, case.W, case.C, 7, 0.0)


def raw_y_ref(I, case, mut=None, stored=True):
    C = case.C
    c = _dw_conv_mut(I, 7, mut).reshape(-1, C)
    pre = (49 + 3) * U32 * _dw_abs_conv(I, 7).reshape(-1, C)
    return c, pre + e_out(c, pre, f16) if stored else pre


def raw_y_f32(I, case):
    return _dw_conv(I["x"].float(), I["wt"].float(), I["bias"], 7, 1).reshape(-1, case.C)


def raw_stats_of(y, mut=None):
    """(stats, bound) in the layout (pixel, 2, C / 128) from the STORED fp16 rows y (pixels, C): the kernel sums what it stores."""
    yd = _d(y).reshape(y.shape[0], -1, 128)
    s, q, a = yd.sum(-1), (yd * yd).sum(-1), yd.abs().sum(-1)
    dim = 2 if mut == "stats_layout_slab_major" else 1
    return torch.stack([s, q], dim).reshape(-1), (128 + 2) * U32 * torch.stack([a, q], 1).reshape(-1)


def raw_stats_ref(I, case, mut=None):
    y = raw_y_f32(I, case).half()
    if mut == "moments_of_unrounded_values":
        return raw_stats_of(raw_y_ref(I, case)[0])[0], None
    return raw_stats_of(y, mut)


def raw_stats_f32(I, case):
    y = raw_y_f32(I, case).half().float().reshape(-1, case.C // 128, 128)
    return torch.stack([y.sum(-1), (y * y).sum(-1)], 1).reshape(-1)


# ================================================================================================ gp_layernorm
LN = namedtuple("LN", "name dt C rows mode eps")       # mode: dense | ldy | inplace | inf32 (fp32 rows, fp16 output, rows = 100 + 0.1 randn)


def ln_pg(dt, C):
    ct = C // (8 if dt == f16 else 4)
    ctp = 1
    while ctp < ct:
        ctp *= 2
    return 256 // ctp


def ln_ldy(case):
    return case.C + (8 if case.dt == f16 else 4) if case.mode == "ldy" else case.C


def _ln_cases():
    out = []

    def add(dt, C, rows, mode="dense", eps=1e-6):
        out.append(LN(f"{_dn(dt)}-C{C}-r{rows}-{mode}" + ("-eps.25" if eps != 1e-6 else ""), dt, C, rows, mode, eps))

    for dt, Cs in ((f16, (128, 192, 1024, 2048)), (f32, (64, 192, 512, 1024))):
        for C in Cs:
            pg = ln_pg(dt, C)
            add(dt, C, 300)
            for rows in sorted({1, pg - 1, pg + 1, 300} - {0}):
                add(dt, C, rows, "ldy")
            add(dt, C, 300, "inplace")
        add(dt, Cs[0], 300, eps=0.25)
        add(dt, 192, 300, eps=0.25)
    for C in (128, 192):
        add(f16, C, 300, "inf32")
        add(f16, C, ln_pg(f16, C) + 1, "inf32")
    return out


LN_CASES = _ln_cases()


@functools.lru_cache(None)
def _ln_operands(dt, C, rows, inf32):
    g = _gen(3000 + C + rows + (7 if inf32 else 0))
    x = (100 + 0.1 * _rn(g, rows, C)) if inf32 else (_rn(g, rows, C) * 2).to(dt)
    return dict(x=x, ln_w=1 + _uniform(g, C, 0.3), ln_b=_uniform(g, C, 0.3))


def ln_inputs(case):
    return _ln_operands(case.dt, case.C, case.rows, case.mode == "inf32")


def ln_ref(I, case, mut=None, stored=True):
    x, lw, lb = _d(I["x"]), _d(I["ln_w"]), _d(I["ln_b"])
    if mut == "input_rounded_to_fp16":
        x = x.half().double()
    width = None
    if mut == "padded_width":       # the lanes of the row's group: the next power of two of C / VEC vectors
        vec = 8 if case.dt == f16 else 4
        width = vec * (1 << (case.C // vec - 1).bit_length())
    mu, sigma, yh, z = _ln(x, lw, lb, case.eps, mut, width)
    if mut is not None:
        return z, None
    pre = _ln_bound(x, torch.zeros_like(mu), mu, sigma, yh, lw, lb, False)
    return z, pre + e_out(z, pre, case.dt) if stored else pre


def ln_f32(I, case):
    return F.layer_norm(I["x"].float(), (case.C,), I["ln_w"], I["ln_b"], case.eps)


# ================================================================================================ GroupNorm
GN_G = 32
GN = namedtuple("GN", "name dt B HW C act mode eps rows bigmean large")     # mode: dense | ldy | inplace; rows: None = gp_groupnorm_stats, else the
#                                                                              caller's chunk rows (groupnorm(fused_stats=True, rows=))


def gn_pxb(B, HW):
    """Pixels per statistics chunk (csrc/norm.hip gn_pxb)."""
    return 256 if (B * HW // 256 >= 1024 or HW < 64) else 64


def gn_apply_pxb(B, HW):
    pxb = gn_pxb(B, HW)
    while pxb > 32 and B * cdiv(HW, pxb) < 2048:
        pxb //= 2
    return pxb


def gn_chunk_rows(case):
    return gn_pxb(case.B, case.HW) if case.rows is None else case.rows


def _gn_cases():
    out = []

    def add(dt, B, HW, C, act, mode="dense", eps=1e-5, rows=None, bigmean=False, large=False):
        name = f"{_dn(dt)}-C{C}-B{B}-HW{HW}-{ACT_NAMES[act]}-{mode}" + ("-eps.25" if eps != 1e-5 else "") + (f"-rows{rows}" if rows else "") + \
            ("-bigmean" if bigmean else "")
        out.append(GN(name, dt, B, HW, C, act, mode, eps, rows, bigmean, large))

    i = 0
    for dt, C in ((f16, 256), (f32, 256), (f16, 128), (f16, 64), (f32, 64)):
        for HW in (16, 35, 100, 256, 1024):
            add(dt, 3 if HW < 256 else 2, HW, C, i % 4)
            i += 1
    for dt in (f16, f32):
        for act in range(4):                      # every activation at one shape with two chunks and a tail
            add(dt, 2, 100, 256, act, "ldy")
        add(dt, 2, 100, 256, ACT_GELU, "inplace")
        add(dt, 2, 100, 256, ACT_GELU, eps=0.25)
        add(dt, 2, 256, 256, ACT_GELU, bigmean=True)
    add(f16, 3, 35, 64, ACT_RELU, "ldy")
    add(f16, 2, 35, 128, ACT_LRELU, eps=0.25)
    for rows in (64, 32, 16):                     # statistics the caller supplies in `rows`-row chunks
        add(f16, 2, 256, 256, ACT_GELU, rows=rows)
    add(f32, 2, 256, 256, ACT_RELU, rows=32)
    # the product's regimes: apply granularity 64 (statistics chunks of 64) and 128 (chunks of 256)
    add(f16, 32, 4096, 64, ACT_GELU, large=True)
    add(f16, 64, 4096, 64, ACT_GELU, large=True)
    return out


GN_CASES = _gn_cases()
# (gn_pxb, gn_apply_pxb) of the large cases.  Granularity 256 (C 64, B 128, HW 4096: 33.5 M values) has no case: its float64 reference, the
# float32 evaluation and the comparison take 3.5 s and 3 GB on the CPU alone, more than a test of this suite may
GN_LARGE_REGIMES = {"f16-C64-B32-HW4096-gelu-dense": (64, 64), "f16-C64-B64-HW4096-gelu-dense": (256, 128)}


@functools.lru_cache(None)
def _gn_operands(dt, B, HW, C, bigmean):
    g = _gen(4000 + C + HW + 3 * B + (1 if bigmean else 0))
    x = _rn(g, B, HW, C) * 1.5 + 0.3
    if bigmean:
        cpg = C // GN_G
        x[:, :, 3 * cpg:4 * cpg] = 20 + _rn(g, B, HW, cpg)              # group 3: |mean| = 20 std
    return dict(x=x.to(dt), gn_w=1 + _uniform(g, C, 0.3), gn_b=_uniform(g, C, 0.3))


def gn_inputs(case):
    return _gn_operands(case.dt, case.B, case.HW, case.C, case.bigmean)


def _group_matrix(C, G, mut=None):
    g = torch.arange(C) % G if mut == "group_is_channel_mod_G" else torch.arange(C) // (C // G)
    return g, F.one_hot(g, G).double()


def gn_stats_ref(I, case, mut=None):
    """(partials, bound) in the layout ((b chunks + chunk) G + g) 2 + {0, 1}: (sum, sum of squares), n = the chunk's pixels x C / G values each."""
    x = _d(I["x"])
    B, HW, C = x.shape
    pxb = gn_chunk_rows(case)
    _, M = _group_matrix(C, GN_G)
    out, bnd = [], []
    for p0 in range(0, HW, pxb):
        xs = x[:, p0:p0 + pxb]
        n = xs.shape[1] * (C // GN_G)
        s, q, a = xs.sum(1) @ M, (xs * xs).sum(1) @ M, xs.abs().sum(1) @ M
        out.append(torch.stack([s, q], -1))
        bnd.append((n + 2) * U32 * torch.stack([a, q], -1))
    dim = 2 if mut == "stats_layout_group_major" else 1
    return torch.stack(out, dim).reshape(-1), torch.stack(bnd, 1).reshape(-1)


def gn_stats_f32(I, case):
    x = I["x"].float()
    B, HW, C = x.shape
    pxb = gn_chunk_rows(case)
    out = []
    for p0 in range(0, HW, pxb):
        xs = x[:, p0:p0 + pxb].reshape(B, -1, GN_G, C // GN_G)
        out.append(torch.stack([xs.sum((1, 3)), (xs * xs).sum((1, 3))], -1))
    return torch.stack(out, 1).reshape(-1)


def gn_supplied_partials(I, case):
    """What a producing kernel leaves for groupnorm(fused_stats=True, rows=case.rows): the float64 chunk sums rounded to fp32."""
    return gn_stats_ref(I, case)[0].float()


def _gn_chain(x, gw, gb, eps, act, dt, chunk, mut=None):
    """GroupNorm + activation of x (B, HW, C) in float64 with statistics chunks of `chunk` pixels: (v, pre).
    S, Q: the image's sums per group, known to within sb, qb (the chunk bounds added up; gn_finalize adds the partials in double).
      mean = S fl(1 / N) -> fp32             d_mean = sb / N + 2 u |mean|
      var  = Q fl(1 / N) - mean^2 (double)   d_var  = qb / N + u Q / N + 2 |mean| (sb / N + u |mean|)
      rstd = 1 / sqrt(var + eps) -> fp32     relative d_var / (2 (var + eps)) + u;  sc = rstd w: + u
      y = fma(x, sc, fma(-mean, sc, b))      (|x sc| + |mean sc|) (r_sc + 2 u) + d_mean |sc| + 2 u (|sh| + |y|)
    (the last line also covers the fp32 instantiation's unfused `b - mean * sc` and `x * sc + sh`: one more rounding of each product)."""
    B, HW, C = x.shape
    cpg = C // GN_G
    gidx, M = _group_matrix(C, GN_G, mut)
    if mut == "statistics_of_own_chunk":
        return torch.cat([_gn_chain(x[:, p0:p0 + chunk], gw, gb, eps, act, dt, chunk)[0] for p0 in range(0, HW, chunk)], 1), None
    N = (cdiv(HW, chunk) * chunk if mut == "count_rounded_up_to_chunk" else HW) * cpg
    S, Q, A = x.sum(1) @ M, (x * x).sum(1) @ M, x.abs().sum(1) @ M
    mean = S / N
    var = (Q / N - mean * mean).clamp_min(0)
    if mut is None:         # exact: the centred form (the line above loses digits at |mean| = 20 std even in float64)
        var = (((x - mean[:, gidx][:, None, :]) ** 2).sum(1) @ M) / N
    if mut == "unbiased_variance":
        var = var * N / (N - 1)
    rstd = 1 / (var + (1e-5 if mut == "eps_ignored" else eps)).sqrt()
    sc = rstd[:, gidx] * gw
    mean_c = mean[:, gidx]
    sh = gb - mean_c * sc
    y = x * sc[:, None, :] + sh[:, None, :]
    if mut == "activation_of_the_neighbour":
        act = (act + 1) % 4
    v = act_value(y, act)
    if mut is not None:
        return v, None
    n = min(chunk, HW) * cpg
    sb, qb = (n + 2) * U32 * A, (n + 2) * U32 * Q
    d_mean_d = sb / N + U32 * mean.abs()
    d_mean = d_mean_d + U32 * mean.abs()
    d_var = qb / N + U32 * Q / N + 2 * mean.abs() * d_mean_d
    r_sc = (d_var / (2 * (var + eps)) + 2 * U32)[:, gidx]
    e = ((x * sc[:, None, :]).abs() + (mean_c * sc).abs()[:, None, :]) * (r_sc + 2 * U32)[:, None, :] + (d_mean[:, gidx] * sc.abs())[:, None, :] + \
        2 * U32 * (sh.abs()[:, None, :] + y.abs())
    return v, act_bound(y, e, act, dt)      # gn_apply_kernel's GELU: gelu_poly2 in fp16 storage, apply_act's gelu_erf in fp32


@functools.lru_cache(1)
def _gn_last(case):
    I = gn_inputs(case)
    v, pre = _gn_chain(_d(I["x"]), _d(I["gn_w"]), _d(I["gn_b"]), case.eps, case.act, case.dt, gn_chunk_rows(case))
    return v.reshape(-1, case.C), pre.reshape(-1, case.C)


def gn_ref(I, case, mut=None, stored=True):
    """(v, bound) as rows (B HW, C).  (The last evaluation is kept: the bound behind the store and the one in front of it are asked for in turn.)"""
    if mut is not None:
        return _gn_chain(_d(I["x"]), _d(I["gn_w"]), _d(I["gn_b"]), case.eps, case.act, case.dt, gn_chunk_rows(case), mut)[0].reshape(-1, case.C), None
    v, pre = _gn_last(case)
    return v, pre + e_out(v, pre, case.dt) if stored else pre


def gn_f32(I, case):
    x = I["x"].float()
    y = F.group_norm(x.permute(0, 2, 1), GN_G, I["gn_w"], I["gn_b"], case.eps).permute(0, 2, 1)
    return act_f32(y, case.act).reshape(-1, case.C)


def gn_layout(case):
    """(ldy, col0) of the output rows: ldy = 2 C puts the data in the right half, behind a sentinel-filled left half."""
    return (2 * case.C, case.C) if case.mode == "ldy" else (case.C, 0)


# ================================================================================================ bilinear x2 (align_corners = True)
def _axis(n, mut=None, other=None):
    """(i0, i1, l) per output index of an axis of n source pixels: src = dst (n - 1) / (2 n - 1), exact."""
    o = torch.arange(2 * n)
    if mut == "align_corners_false":
        s = ((o.double() + 0.5) / 2 - 0.5).clamp_min(0)
        i0 = s.floor().long()
        return i0, (i0 + 1).clamp_max(n - 1), s - i0
    if mut == "ratios_swapped":
        s = (o.double() * (other - 1) / (2 * other - 1)).clamp_max(n - 1)
        i0 = s.floor().long()
        return i0, (i0 + 1).clamp_max(n - 1), s - i0
    num, den = o * (n - 1), 2 * n - 1
    i0 = num // den
    return i0, (i0 + 1).clamp_max(n - 1), (num % den).double() / den


def blend2x(x, mut=None):
    """x (B, H, W, C) float64 -> (v, a, dx, dy): the blend, the blend of |x|, and the largest difference of the two neighbours the
    horizontal resp. vertical weight blends."""
    B, H, W, C = x.shape
    y0, y1, ly = _axis(H, mut, W)
    x0, x1, lx = _axis(W, mut, H)
    ly, lx = ly.view(1, -1, 1, 1), lx.view(1, 1, -1, 1)
    r0, r1 = x[:, y0], x[:, y1]
    v00, v01, v10, v11 = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    h0, h1 = (1 - lx) * v00 + lx * v01, (1 - lx) * v10 + lx * v11
    v = (1 - ly) * h0 + ly * h1
    a = (1 - ly) * ((1 - lx) * v00.abs() + lx * v01.abs()) + ly * ((1 - lx) * v10.abs() + lx * v11.abs())
    # a source coordinate that is an integer exactly (the last row / column) may come out one ulp below it: the kernel then blends the
    # PREVIOUS pair with a weight within the same 2 u (n - 1) of (0, 1), so the pair before (i0 - 1, i0) counts as well
    xm, ym = (x0 - 1).clamp_min(0), (y0 - 1).clamp_min(0)
    rm = x[:, ym]
    hm = (1 - lx) * rm[:, :, x0] + lx * rm[:, :, x1]
    dx = torch.stack([(v01 - v00).abs(), (v11 - v10).abs(), (v00 - r0[:, :, xm]).abs(), (v10 - r1[:, :, xm]).abs()]).max(0).values
    return v, a, dx, torch.maximum((h1 - h0).abs(), (h0 - hm).abs())


def blend_arith_bound(a, dx, dy, H, W):
    return 4 * U32 * a + (2 * (W - 1) + 1) * U32 * dx + (2 * (H - 1) + 1) * U32 * dy


UP = namedtuple("UP", "name dt B H W C")
UP_CASES = [UP(f"{_dn(dt)}-B{B}-{H}x{W}-C{C}", dt, B, H, W, C) for (B, H, W, C) in [(2, 3, 7, 64), (1, 8, 5, 256), (1, 4, 3, 96)] for dt in (f16, f32)]      # C 96: C / VEC is no power of two, the flat kernel


@functools.lru_cache(None)
def _up_operands(dt, B, H, W, C):
    return dict(x=(_rn(_gen(5000 + H + C), B, H, W, C) * 1.5 + 0.3).to(dt))


def up_inputs(case):
    return _up_operands(case.dt, case.B, case.H, case.W, case.C)


def up_ref(I, case, mut=None, stored=True):
    v, a, dx, dy = blend2x(_d(I["x"]), mut)
    v = v.reshape(-1, case.C)
    if mut is not None:
        return v, None
    pre = blend_arith_bound(a, dx, dy, case.H, case.W).reshape(-1, case.C)
    return v, pre + e_out(v, pre, case.dt) if stored else pre


def up_f32(I, case):
    x = I["x"].float().permute(0, 3, 1, 2)
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1).reshape(-1, case.C)


# ================================================================================================ gp_groupnorm_upsample2x
# CPT = 4 / 2 / 1 are C = 512 / 256 / <= 128.  C = 512 needs (8 / 2 + 2) x 10 x 512 x 2 = 61 440 B of LDS, which IS 60 KB: the launcher's
# `lds <= 60 * 1024` admits it.
GU = namedtuple("GU", "name B H W C act eps")
GU_CASES = [GU(f"B{B}-{H}x{W}-C{C}-{ACT_NAMES[act]}" + ("-eps.25" if eps != 1e-5 else ""), B, H, W, C, act, eps)
            for (B, H, W) in [(3, 8, 24), (1, 5, 7)] for (C, act, eps) in [(512, ACT_GELU, 1e-5), (256, ACT_GELU, 1e-5), (128, ACT_RELU, 1e-5), (64, ACT_GELU, 0.25)]]


def gu_gn_case(case):
    """The gp_groupnorm_apply case behind it (statistics from gp_groupnorm_stats)."""
    return GN("gu-" + case.name, f16, case.B, case.H * case.W, case.C, case.act, "dense", case.eps, None, False, False)


def gu_inputs(case):
    return gn_inputs(gu_gn_case(case))


def gu_ref(I, case, mut=None, stored=True):
    """The reference of apply rounded to fp16, then the blend.  A kernel's fp16 intermediate is within apply's bound of apply's exact value, so
    within that bound plus the reference's own rounding of the rounded reference: both enter through the blend's weights."""
    g = gu_gn_case(case)
    B, H, W, C = case.B, case.H, case.W, case.C
    mid_v, mid_b = gn_ref(I, g)
    mid16 = store(mid_v, f16).view(B, H, W, C)
    v, a, dx, dy = blend2x(mid16, mut)
    v = v.reshape(-1, C)
    if mut is not None:
        return v, None
    mid_e = (mid_b + U16 * mid_v.abs() + 2.0 ** -25).view(B, H, W, C)
    pre = blend2x(mid_e)[0].reshape(-1, C) + blend_arith_bound(a, dx, dy, H, W).reshape(-1, C)
    return v, pre + e_out(v, pre, f16) if stored else pre


def gu_mid_rounding(I, case):
    """The share of gu_ref's bound in front of the store that is the fp16 ROUNDING of the intermediate tensor (its e_out and the
    reference's own rounding), carried through the blend: a correct evaluation may use all of it, as it may use all of a store's e_out."""
    g = gu_gn_case(case)
    mid_v, mid_b = gn_ref(I, g)
    mid_pre = gn_ref(I, g, stored=False)[1]
    r = (mid_b - mid_pre + U16 * mid_v.abs() + 2.0 ** -25).view(case.B, case.H, case.W, case.C)
    return blend2x(r)[0].reshape(-1, case.C)


def gu_f32(I, case):
    g = gu_gn_case(case)
    mid = gn_f32(I, g).half().float().view(case.B, case.H, case.W, case.C).permute(0, 3, 1, 2)
    return F.interpolate(mid, scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1).reshape(-1, case.C)


# ================================================================================================ registry
def _dtype_of(case):
    return getattr(case, "dt", f16)


OPS = {o.name: o for o in [
    Op("gp_dwconv_ln", DW_CASES, dw_inputs, dw_ref, dw_f32, functools.partial(dw_ref, stored=False)),
    Op("gp_dwconv7_raw_stats y", RAW_CASES, raw_inputs, raw_y_ref, raw_y_f32, functools.partial(raw_y_ref, stored=False)),
    Op("gp_dwconv7_raw_stats stats", RAW_CASES, raw_inputs, raw_stats_ref, raw_stats_f32),
    Op("gp_layernorm", LN_CASES, ln_inputs, ln_ref, ln_f32, functools.partial(ln_ref, stored=False)),
    Op("gp_groupnorm_stats", [c for c in GN_CASES if c.mode == "dense"], gn_inputs, gn_stats_ref, gn_stats_f32),
    Op("gp_groupnorm_apply", GN_CASES, gn_inputs, gn_ref, gn_f32, functools.partial(gn_ref, stored=False)),
    Op("gp_groupnorm_upsample2x", GU_CASES, gu_inputs, gu_ref, gu_f32, functools.partial(gu_ref, stored=False)),
    Op("gp_upsample_bilinear2x", UP_CASES, up_inputs, up_ref, up_f32, functools.partial(up_ref, stored=False)),
]}
ROUNDING_IN_PRE = {"gp_groupnorm_upsample2x": gu_mid_rounding}
FP32_OUTPUT = ("gp_dwconv7_raw_stats stats", "gp_groupnorm_stats")      # fp32 sums whatever the storage type of x


def out_dtype(name, case):
    return f32 if name in FP32_OUTPUT else _dtype_of(case)


def is_large(case):
    return bool(getattr(case, "large", False))


def _zero_mean_f16(c):
    return c.dt == f16 and not c.offset


def _multi_chunk(c):
    return c.rows is None and cdiv(c.HW, gn_pxb(c.B, c.HW)) > 1


# (operation, mutation, which cases must expose it).  Every filter excludes the large cases (their float32 self-check runs, no mutation).
#   unbiased_variance   changes yh by 1 / (2 C) relative: 3.9e-3 at C 128, 9.8e-4 at C 512 -- against a bound of about one fp16 half ulp, 4.9e-4
#                       relative -- so it must show from C 128 to C 512 on zero-mean fp16 cases; at C 1024 it is 4.9e-4, the size of the bound
#                       itself, and the filter stops at 512 (the bound is NOT widened).  fp32 storage: exposed at every C.  GELU / ReLU outputs
#                       near zero shrink the change with the value, so the fp16 filter keeps the cases without an activation.
#   eps_*               only eps = 0.25 tells a wrong eps apart: var ~ 1, so sigma moves by about 10 %.
#   clamp_to_edge, taps_transposed, no_batch_boundary, pair_as_one_map: wrong pixels under the filter, errors of the order of the values.
#   prefix_to_strip_boundary: rows behind the prefix overwrite the sentinel row; needs n_pixels % 8 != 0.
#   moments_of_unrounded_values: 128 rounding errors of up to 2^-11 |y| add up to ~ 11 x 2^-12 rms(y) at random signs, against (130 u) sum |y|
#                       = 7.7e-6 x 128 mean |y|: above the bound in some slab of some pixel for certain over 768 pixels.
#   padded_width        C = 192 only (the zero-padded lane group of layernorm_padded_kernel): divisor 256.
#   input_rounded_to_fp16: rows 100 + 0.1 randn lose all but 3 bits of their spread.
#   statistics_of_own_chunk, count_rounded_up_to_chunk: need more than one chunk resp. HW % chunk != 0.
MUTATIONS = [
    ("gp_dwconv_ln", "clamp_to_edge", lambda c: not c.large),
    ("gp_dwconv_ln", "taps_transposed", lambda c: not c.large),
    ("gp_dwconv_ln", "no_batch_boundary", lambda c: not c.large and c.npix >= c.H * c.W),
    ("gp_dwconv_ln", "pair_as_one_map", lambda c: c.form in (PAIR_TH4, PAIR_TH2)),
    ("gp_dwconv_ln", "unbiased_variance", lambda c: not c.large and ((_zero_mean_f16(c) and c.C <= 512 and c.act == ACT_NONE and c.eps == 1e-6) or c.dt == f32)),
    ("gp_dwconv_ln", "eps_ignored", lambda c: c.eps == 0.25),
    ("gp_dwconv_ln", "eps_outside_root", lambda c: c.eps == 0.25),
    ("gp_dwconv_ln", "lrelu_slope_001", lambda c: c.act == ACT_LRELU),
    ("gp_dwconv_ln", "act_dropped", lambda c: c.act != ACT_NONE),
    ("gp_dwconv_ln", "prefix_to_strip_boundary", lambda c: c.npix % 8 != 0),
    ("gp_dwconv7_raw_stats y", "clamp_to_edge", lambda c: True),
    ("gp_dwconv7_raw_stats y", "taps_transposed", lambda c: True),
    ("gp_dwconv7_raw_stats stats", "stats_layout_slab_major", lambda c: c.C > 128),
    ("gp_dwconv7_raw_stats stats", "moments_of_unrounded_values", lambda c: True),
    ("gp_layernorm", "unbiased_variance", lambda c: (c.dt == f32 or c.C <= 512) and c.mode != "inf32" and c.rows >= 8 and c.eps == 1e-6),
    ("gp_layernorm", "eps_ignored", lambda c: c.eps == 0.25),
    ("gp_layernorm", "eps_outside_root", lambda c: c.eps == 0.25),
    ("gp_layernorm", "padded_width", lambda c: c.C == 192),
    ("gp_layernorm", "ldy_ignored", lambda c: c.mode == "ldy" and c.rows > 1),
    ("gp_layernorm", "input_rounded_to_fp16", lambda c: c.mode == "inf32"),
    ("gp_groupnorm_stats", "stats_layout_group_major", lambda c: not c.large and cdiv(c.HW, gn_chunk_rows(c)) > 1),
    ("gp_groupnorm_apply", "statistics_of_own_chunk", lambda c: not c.large and (c.rows is not None or _multi_chunk(c))),
    ("gp_groupnorm_apply", "group_is_channel_mod_G", lambda c: not c.large),
    ("gp_groupnorm_apply", "count_rounded_up_to_chunk", lambda c: c.HW in (100, 35) and c.rows is None),
    ("gp_groupnorm_apply", "unbiased_variance", lambda c: not c.large and c.HW * c.C // GN_G <= 512 and (c.dt == f32 or c.act in (ACT_NONE, ACT_LRELU))),
    ("gp_groupnorm_apply", "eps_ignored", lambda c: c.eps == 0.25),
    ("gp_groupnorm_apply", "activation_of_the_neighbour", lambda c: not c.large),
    ("gp_groupnorm_apply", "ldy_ignored", lambda c: c.mode == "ldy"),
    ("gp_groupnorm_upsample2x", "align_corners_false", lambda c: True),
    ("gp_groupnorm_upsample2x", "ratios_swapped", lambda c: c.H != c.W),
    ("gp_upsample_bilinear2x", "align_corners_false", lambda c: True),
    ("gp_upsample_bilinear2x", "ratios_swapped", lambda c: c.H != c.W),
]


def mutant_buffer(name, case, mut):
    """The flat buffer a kernel with this defect would leave, together with (v, bound, ldy, col0) of the correct one."""
    op = OPS[name]
    I = op.inputs(case)
    v, bound = op.ref(I, case)
    if v.dim() == 1:
        v, bound = v.view(1, -1), bound.view(1, -1)
    rows, C = v.shape
    ldy, col0 = (ln_ldy(case), 0) if name == "gp_layernorm" else gn_layout(case) if name == "gp_groupnorm_apply" else (C, 0)
    if mut == "ldy_ignored":
        buf = blank_buffer(rows, C, ldy, col0, C)
        buf[col0:col0 + rows * C] = v.reshape(-1)
        return buf, v, bound, ldy, col0
    wrong = op.ref(I, case, mut=mut)[0]
    if wrong.numel() > v.numel():
        return wrong.reshape(-1), v, bound, ldy, col0
    return filled_buffer(wrong.reshape(rows, C), ldy, col0, C), v, bound, ldy, col0
