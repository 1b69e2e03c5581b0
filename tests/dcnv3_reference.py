"""Float64 reference, per-element error bound, input sets and cases of the DCNv3 forward: gp_dcnv3_forward (csrc/dcnv3.hip: dcnv3_wave8_kernel,
dcnv3_wave_kernel<.,.,3,PATCH>, dcnv3_wave_kernel<.,.,3>, the run-time-K dcnv3_wave_kernel, dcnv3_generic_kernel) and gp_dcnv3_forward_any
(csrc/dcnv3_any.hip).  No GPU here: tests/test_dcnv3_reference_cpu.py checks this file against itself, the oracles and the goldens;
tests/test_dcnv3_conformance_gpu.py holds the kernels against it.  check / check_buffer / with_tail / store / e_out / SENTINEL / Op are
those of tests/ops_reference.py.

The operation (a restatement of dcnv3_im2col_cuda.cuh:216-282 from its definition).  Output row r = (b Ho + ho) Wo + wo, group g, tap
slot q = 0 .. P - 1 in the order kernel_w OUTER, kernel_h inner (i along w, j along h; remove_center drops the centre tap AND its slot):

    off_w, off_h = offset[r off_ld + (g P + q) 2 + {0, 1}]          m = mask[r mask_ld + g P + q]   (or softmax over the group's P logits)
    p0_w_ = (halfk_w - pad_w + wo stride_w) - halfk_w os            halfk = (dil (k - 1)) >> 1
    loc_w = p0_w_ + (i dil_w + off_w) os                            (the same along h)
    the tap counts when loc_h > -1, loc_w > -1, loc_h < H, loc_w < W;  its value is the bilinear sample at (loc_h, loc_w), a corner outside
    the map contributing zero:  t = w1 v1 + w2 v2 + w3 v3 + w4 v4,  w = (hh hw, hh lw, lh hw, lh lw),  lh = loc_h - floor loc_h, hh = 1 - lh
    out[r, g, :] = sum_q t_q m_q

ref(inputs, case) -> (v, bound), float64.  v is the exact value on the operands the kernel sees (fp16 tensors already rounded).  The
sampling LOCATION is evaluated in the kernel's opmath (float32 for half / float, float64 for double) by the kernel's expression above; the
reference CUDA forms it in float too, and a float64 location differs from it by ~ulp(loc) ~ 200 u of a weight, which is no kernel error.
So that the float32 location is unambiguous under FMA contraction (fma(x, os, p0_) against a rounded product), inputs are restricted:
continuous offsets only with os == 1 (the product is exact either way); for os != 1 the offsets lie on a dyadic grid and os is one of
0.5, 2, 1.5, so every intermediate is exact (the builders assert float32 location == float64 location on those sets).  Everything behind
the location is float64.

Bound = c u a + e_soft + e_out, a = sum_q |m_q| sum_corners |w| |v| (the same sum on absolute values), u = 2^-24 (2^-53 for double):

  c = P + 10      per tap, on magnitudes bounded by that tap's share of a: 3 roundings of a corner weight (lh or hh, lw or hw -- each one
                  subtraction -- and their product), 1 for the corner products (in parallel), 3 for the corner sums, 1 for the product
                  with the mask weight = 8 (the FMA forms round less often); the accumulation over the taps rounds P partial sums, each
                  bounded by a; + 2 for the (1 + u)^n growth of the first-order terms, as in ops_reference.  (The one weight whose
                  RELATIVE error is unbounded -- hh = 1 - fl(1 + loc) for loc in (-0.5, 0) -- belongs to the corners of row / column -1,
                  which are outside the map and count zero.)
  e_soft          logits only: m_q carries the relative error eps_q = (|d_q| + E) u + sum_j p_j (|d_j| + E) u + (P - 1) u + 2 u, d = l - max:
                  the rounding of d changes exp(d) by |d| u; E u = the device expf; the numerator's error, then the same on the
                  probability-weighted terms of the denominator; P - 1 additions of positive terms (sequential in the generic kernel; the
                  16-lane butterfly rounds at most min(4, P - 1) times); the division (1 / s and a product in the generic kernel: 2).
                  E = 4: expf assumed accurate to 2 ulp = 4 u.  ROCm documents its device expf at 1 ulp; that table is not shipped
                  with the toolkit, so the assumption is twice the figure and not read from a file.  e_soft = sum_q eps_q a_q.
  e_out           ops_reference.e_out (u64 |v| for double).
  a == 0          (every tap of the pixel and group outside the map, or only zero operands): bound 0, the output must be exactly 0.

f32(inputs, case): the same operation in the opmath type with the kernel's association ((w1 v1 + w2 v2 + w3 v3 + w4 v4) m, accumulated tap
by tap); it must stay within HALF of the bound in front of the store on every case (tests/test_dcnv3_reference_cpu.py).

ref(..., mut=...): deliberately wrong float64 variants (MUTATIONS); the checker must reject each.
poison_sets(inputs, case): for a case with one non-finite input pixel ((v, bound) are computed with that pixel at zero), which outputs
touch the pixel through a corner INSIDE the map (`hard`: with non-zero weight and mask -- the output is non-finite; `soft`: at zero weight,
where the reference CUDA multiplies and gp_dcnv3_forward_any selects -- either).  Every other output reaches the pixel at most as the
clamped address of an out-of-range tap and must be finite and within its bound.
"""
import functools
import zlib
from collections import namedtuple

import torch

import ops_reference as R
from ops_reference import SENTINEL, Op, check, check_buffer, store, with_tail  # noqa: F401  (re-exported for the two test files)

F16, F32, F64 = torch.float16, torch.float32, torch.float64
U32, U64 = 2.0 ** -24, 2.0 ** -53
EXPF_U = 4.0                 # device expf: 2 ulp assumed = 4 u (see the module docstring)
NAN, INF = float("nan"), float("inf")

Case = namedtuple("Case", "name entry dt om_dt N H W G D kh kw sh sw ph pw dh dw os rc ld logits iset poison")


def mk(name, dt, N, H, W, G=4, D=64, K=3, s=1, p=1, d=1, os=1.0, rc=0, om=F32, ld=None, logits=False, iset="c3", entry="fwd", k=None, ss=None,
       pp=None, dd=None, poison=None):
    """ld: None = dense offset (rows, 2 G P) and mask (rows, G P) buffers; a number = ONE buffer of rows x ld, offsets in columns [0, 2 G P),
    mask in [2 G P, 3 G P), SENTINEL in the rest (off_ld = mask_ld = ld, the mask pointer 2 G P values behind the offset pointer)."""
    kh, kw = k or (K, K)
    sh, sw = ss or (s, s)
    ph, pw = pp or (p, p)
    dh, dw = dd or (d, d)
    if entry == "any":
        om = dt
    return Case(name, entry, dt, om, N, H, W, G, D, kh, kw, sh, sw, ph, pw, dh, dw, float(os), rc, ld, logits, iset, poison)


def out_hw(c):
    return (c.H + 2 * c.ph - (c.dh * (c.kh - 1) + 1)) // c.sh + 1, (c.W + 2 * c.pw - (c.dw * (c.kw - 1) + 1)) // c.sw + 1


def n_taps(c):
    return c.kh * c.kw - c.rc


def n_rows(c):
    Ho, Wo = out_hw(c)
    return c.N * Ho * Wo


def lds(c, mut=None):
    """(off_ld, mask_ld, values between the offset and the mask pointer or None for separate buffers)."""
    GP = c.G * n_taps(c)
    if c.ld is None or mut == "ld_dense":
        return 2 * GP, GP, (None if c.ld is None else 2 * GP)
    return c.ld, c.ld, 2 * GP


def opmath(c):
    return F64 if c.dt == F64 else F32


def tap_positions(c, mut=None):
    """(i, j, slot) of every tap in accumulation order: i along w (outer), j along h (inner)."""
    out = []
    if mut == "h_outer":
        order = [(i, j) for j in range(c.kh) for i in range(c.kw)]
    else:
        order = [(i, j) for i in range(c.kw) for j in range(c.kh)]
    for i, j in order:
        if c.rc and i == c.kw // 2 and j == c.kh // 2:
            continue
        out.append((i, j, (order.index((i, j)) if mut == "rc_slot" else len(out))))
    return out


# ------------------------------------------------------------------------------------------------ routing (csrc/dcnv3.hip launch())
def form_taken(c, env=None):
    env = env or {}
    if c.entry == "any":
        return f"dcnv3_any_fwd_kernel<{_tn(c.dt)}>"
    Ho, Wo = out_hw(c)
    T, OT = _tn(c.dt), _tn(c.om_dt)
    square3 = c.G == 4 and c.D == 64 and c.kh == 3 and not c.rc
    patch = square3 and Ho % 4 == 0 and Wo % 4 == 0
    if c.dt == F16 and patch and env.get("GP_DCN_WAVE8") != "0":
        return f"dcnv3_wave8_kernel<{OT},{'LB' if env.get('GP_DCN_LDSBC') == '1' else 'DPP'}>"
    if patch:
        return f"dcnv3_wave_kernel<{T},{OT},3,PATCH>"
    if square3:
        return f"dcnv3_wave_kernel<{T},{OT},3>"
    if c.G == 4 and c.D == 64 and c.kh * c.kh - c.rc <= 16:
        return f"dcnv3_wave_kernel<{T},{OT}>"
    return f"dcnv3_generic_kernel<{T},{OT}>"


def _tn(dt):
    return {F16: "half", F32: "float", F64: "double"}[dt]


def grid_x(c):
    """Workgroups along x of the patch forms / the wave-per-pixel forms (xcd_chunk's n)."""
    Ho, Wo = out_hw(c)
    return c.N * (Ho // 4) * (Wo // 4) if "PATCH" in form_taken(c) or "wave8" in form_taken(c) else -(-n_rows(c) // 4)


# ------------------------------------------------------------------------------------------------ cases
def _patch_cases(dt):
    t = "h" if dt == F16 else "f"
    A, B, C, Dd = dict(N=3, H=8, W=16, s=2), dict(N=13, H=8, W=8, s=2), dict(N=2, H=4, W=8, s=1), dict(N=2, H=16, W=8, s=2)
    one16 = dict(om=F16) if dt == F16 else {}          # fp32 storage: fp16 rows on ONE case (A-c12)
    return [
        mk(f"{t}-A-c3-logits-ld108", dt, **A, ld=108, logits=True),
        mk(f"{t}-A-c3-weights-ld128", dt, **A, ld=128),
        mk(f"{t}-A-c12-logits-om16", dt, **A, om=F16, logits=True, iset="c12"),
        mk(f"{t}-A-edges-weights-ld108", dt, **A, ld=108, iset="edges"),
        mk(f"{t}-A-edges-logits-ld128-os0.5", dt, **A, ld=128, logits=True, iset="edges", os=0.5),
        mk(f"{t}-A-edges-weights-os2", dt, **A, iset="edges", os=2.0, **(one16 or dict(ld=108))),
        mk(f"{t}-B-c3-logits-ld108", dt, **B, ld=108, logits=True),
        mk(f"{t}-B-edges-weights-ld128", dt, **B, ld=128, iset="edges"),
        mk(f"{t}-C-c3-logits-ld108", dt, **C, ld=108, logits=True),
        mk(f"{t}-C-edges-weights", dt, **C, iset="edges", **one16),
        mk(f"{t}-D-c3-weights-ld108", dt, **Dd, ld=108),
        mk(f"{t}-D-edges-logits-ld128", dt, **Dd, ld=128, logits=True, iset="edges"),
        mk(f"{t}-dil2-pad2-edges-weights-ld108", dt, N=2, H=8, W=16, s=2, p=2, d=2, ld=108, iset="edges"),
        mk(f"{t}-dil2-pad2-dyadic-logits-os2", dt, N=2, H=8, W=16, s=2, p=2, d=2, ld=128, logits=True, iset="dyadic", os=2.0),
        mk(f"{t}-pad0-edges-weights", dt, N=2, H=9, W=17, s=2, p=0, iset="edges", **one16),
        mk(f"{t}-pad2-edges-logits-ld108-os0.5", dt, N=2, H=6, W=14, s=2, p=2, ld=108, logits=True, iset="edges", os=0.5),
    ]


def _wave3_cases(dt):
    t = "h" if dt == F16 else "f"
    A, B = dict(N=3, H=10, W=14, s=2), dict(N=1, H=6, W=10, s=1)          # 5 x 7 outputs: 105 rows, the last workgroup partial; 60 rows
    return [
        mk(f"{t}-w3-A-c3-logits-ld108", dt, **A, ld=108, logits=True),
        mk(f"{t}-w3-A-edges-weights-om16", dt, **A, om=F16, iset="edges"),
        mk(f"{t}-w3-B-c12-weights-ld128", dt, **B, ld=128, iset="c12"),
        mk(f"{t}-w3-B-edges-logits-os2", dt, **B, ld=108, logits=True, iset="edges", os=2.0),
    ]


def _rtk_cases(dt):
    t = "h" if dt == F16 else "f"
    rc, k4, k2, k1 = dict(N=2, H=6, W=10, K=3, rc=1), dict(N=1, H=10, W=14, K=4, s=2, p=1), dict(N=1, H=6, W=8, K=2, p=0), dict(N=2, H=5, W=7, K=1, p=0)
    return [
        mk(f"{t}-rc-c3-logits-om16-ld100", dt, **rc, om=F16, ld=100, logits=True),          # P 8; fp16 rows with a gap behind them
        mk(f"{t}-rc-edges-weights-os2", dt, **rc, iset="edges", os=2.0),
        mk(f"{t}-K4-c3-logits-ld192", dt, **k4, ld=192, logits=True),                        # P 16, 35 rows
        mk(f"{t}-K4-edges-weights-om16", dt, **k4, om=F16, iset="edges"),
        mk(f"{t}-K2-c3-logits", dt, **k2, logits=True),                                      # P 4, 35 rows
        mk(f"{t}-K2-edges-weights-ld50-om16", dt, **k2, om=F16, ld=50, iset="edges"),
        mk(f"{t}-K1-c3-logits-ld16", dt, **k1, ld=16, logits=True),                          # P 1, 70 rows
        mk(f"{t}-K1-edges-weights", dt, **k1, iset="edges"),
    ]


def _generic_cases():
    g1, g2, g3, g4 = dict(N=1, H=5, W=7, G=3, D=8, K=5, p=2), dict(N=1, H=5, W=7, G=1, D=4, K=3), dict(N=1, H=10, W=14, G=4, D=32, K=3, s=2), \
        dict(N=1, H=5, W=7, G=8, D=64, K=3)
    return [
        mk("f-gen-G3D8K5-dyadic-os1.5", F32, **g1, iset="dyadic", os=1.5),
        mk("f-gen-G3D8K5-c3", F32, **g1),
        mk("h-gen-G3D8K5-edges-om16", F16, **g1, om=F16, iset="edges"),
        mk("f-gen-G1D4K3-edges", F32, **g2, iset="edges"),
        mk("h-gen-G1D4K3-c3-logits", F16, **g2, logits=True),
        mk("h-gen-G4D32K3s2-c3-logits-ld108", F16, **g3, ld=108, logits=True),
        mk("f-gen-G4D32K3s2-edges-logits-om16", F32, **g3, om=F16, logits=True, iset="edges"),
        mk("f-gen-G8D64K3-c12", F32, **g4, iset="c12"),
        mk("h-gen-G8D64K3-edges-ld220", F16, **g4, ld=220, iset="edges"),
    ]


def _any_cases():
    out = []
    big = dict(N=1, H=6, W=7, G=1, D=71, k=(9, 8), pp=(4, 4))                           # 72 taps (two owner chunks), D > 64: 6 x 8 outputs
    k35 = dict(N=2, H=5, W=7, G=2, k=(3, 5), pp=(1, 2))                                 # 15 taps, 5 x 7 outputs
    rcg = dict(N=2, H=6, W=11, G=2, D=30, K=3, rc=1, ss=(1, 2), pp=(1, 0), dd=(1, 2))   # per-axis stride / pad / dil: 6 x 4 outputs
    for dt in (F64, F32, F16):
        t = _tn(dt)[0]
        out += [
            mk(f"any-{t}-9x8-D71-c3", dt, **big, entry="any"),
            mk(f"any-{t}-9x8-D71-dyadic-os1.5", dt, **big, entry="any", iset="dyadic", os=1.5),
            mk(f"any-{t}-3x5-D1-edges", dt, **k35, D=1, entry="any", iset="edges"),
            mk(f"any-{t}-3x5-D30-c12", dt, **k35, D=30, entry="any", iset="c12"),
            mk(f"any-{t}-rc-axes-edges-os0.5", dt, **rcg, entry="any", iset="edges", os=0.5),
            mk(f"any-{t}-rc-axes-c3", dt, **rcg, entry="any"),
        ]
    out += [mk("any-f-3x5-D30-edges-inf", F32, **k35, D=30, entry="any", iset="edges", poison=INF),
            mk("any-h-3x5-D30-edges-nan", F16, **k35, D=30, entry="any", iset="edges", poison=NAN)]
    return out


PATCH_CASES = _patch_cases(F16) + _patch_cases(F32)
FWD_CASES = PATCH_CASES + _wave3_cases(F16) + _wave3_cases(F32) + _rtk_cases(F16) + _rtk_cases(F32) + _generic_cases()
ANY_CASES = _any_cases()
CASES = FWD_CASES + ANY_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# every kernel form a default build can launch for these entry points, and the per-call arms of the fp16 patch cases
WAVE8_ARMS = [("GP_DCN_WAVE8", "0"), ("GP_DCN_LDSBC", "1")]
FORMS = ([f"dcnv3_wave8_kernel<{ot},{a}>" for ot in ("float", "half") for a in ("DPP", "LB")] +
         [f"dcnv3_wave_kernel<{t},{ot},3,PATCH>" for t in ("half", "float") for ot in ("float", "half")] +
         [f"dcnv3_wave_kernel<{t},{ot},3>" for t in ("half", "float") for ot in ("float", "half")] +
         [f"dcnv3_wave_kernel<{t},{ot}>" for t in ("half", "float") for ot in ("float", "half")] +
         [f"dcnv3_generic_kernel<{t},{ot}>" for t in ("half", "float") for ot in ("float", "half")] +
         [f"dcnv3_any_fwd_kernel<{t}>" for t in ("double", "float", "half")])


def forms_reached():
    """form -> the names of the cases (and arms) that reach it."""
    out = {}
    for c in CASES:
        out.setdefault(form_taken(c), []).append(c.name)
        if "wave8" in form_taken(c):
            for k, v in WAVE8_ARMS:
                out.setdefault(form_taken(c, {k: v}), []).append(f"{c.name} [{k}={v}]")
    return out


# ------------------------------------------------------------------------------------------------ inputs
def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)


def _exact(t, dt, what):
    assert bool((store(t, dt) == t.double()).all()), f"{what}: not representable in {dt}"
    return t.to(dt)


def _p0(c, ct, mut=None):
    """(p0_h_, p0_w_, image index) of every output row, in the opmath type ct."""
    Ho, Wo = out_hw(c)
    r = torch.arange(c.N * Ho * Wo)
    if mut == "wo_ho_swapped":
        ho, wo = r % Ho, (r // Ho) % Wo
    else:
        wo, ho = r % Wo, (r // Wo) % Ho
    b = r // (Ho * Wo)
    hh_, hw_ = (c.dh * (c.kh - 1)) >> 1, (c.dw * (c.kw - 1)) >> 1
    os = torch.tensor(c.os, dtype=ct)
    sub_h, sub_w = torch.tensor(float(hh_), dtype=ct) * os, torch.tensor(float(hw_), dtype=ct) * os
    if mut == "p0_no_halfk_os":
        sub_h = sub_w = torch.zeros((), dtype=ct)
    if mut == "p0_halfk_unscaled":
        sub_h, sub_w = torch.tensor(float(hh_), dtype=ct), torch.tensor(float(hw_), dtype=ct)
    p0h = (hh_ - c.ph + ho * c.sh).to(ct) - sub_h
    p0w = (hw_ - c.pw + wo * c.sw).to(ct) - sub_w
    if mut == "patch_image_square" and Ho % 4 == 0 and Wo % 4 == 0:
        ppr, ppi = Wo // 4, (Wo // 4) * (Ho // 4)
        pid = b * ppi + (ho // 4) * ppr + wo // 4
        b = (pid // (ppr * ppr)).clamp_max(c.N - 1)
    return p0h, p0w, b


def _edge_table(S):
    S = float(S)
    return [0.0, 1.0, S - 2.0, S - 1.0, -1.0, S, -0.5, -0.25, S - 0.5, S - 0.75, 0.5, S - 1.5, 1.25, -40.0, S + 40.0, S - 1.25]


def _edge_targets(c):
    """(th, tw) of shape (rows, G, P): every pair of the two tables once per 240 taps; every 5th row's last group entirely outside."""
    R_, G, P = n_rows(c), c.G, n_taps(c)
    n = torch.arange(R_ * G * P)
    th = torch.tensor(_edge_table(c.H), dtype=F64)[n % 16].view(R_, G, P)
    tw = torch.tensor(_edge_table(c.W)[:15], dtype=F64)[n % 15].view(R_, G, P)
    far = torch.tensor([-40.0, c.H + 40.0, -1.0, float(c.H)], dtype=F64)[torch.arange(P) % 4]
    th[2::5, G - 1, :] = far
    return th, tw


@functools.lru_cache(None)
def inputs(c):
    """x (N, H, W, G D) in the storage type; off / mask: flat buffers in the offset / mask type (views of `om` where the case has one)."""
    g = _gen(c)
    R_, G, P = n_rows(c), c.G, n_taps(c)
    GP = G * P
    x = torch.randn(c.N, c.H, c.W, G * c.D, generator=g, dtype=F64).to(c.dt)
    taps = tap_positions(c)
    ti = torch.tensor([t[0] for t in taps], dtype=F64)
    tj = torch.tensor([t[1] for t in taps], dtype=F64)
    if c.iset in ("c3", "c12"):
        assert c.os == 1.0, "continuous offsets only with offset_scale 1"
        amp = 3.0 if c.iset == "c3" else 12.0
        off = ((torch.rand(R_, G, P, 2, generator=g, dtype=F64) * 2 - 1) * amp).to(c.om_dt)
    elif c.iset == "dyadic":
        assert c.os in (0.5, 1.0, 1.5, 2.0)
        off = _exact(torch.randint(-16, 17, (R_, G, P, 2), generator=g).double() / 4, c.om_dt, "dyadic offsets")
    else:
        assert c.iset == "edges" and c.os in (0.5, 1.0, 2.0)
        p0h, p0w, _ = _p0(c, F64)
        th, tw = _edge_targets(c)
        off_w = (tw - p0w.view(-1, 1, 1)) / c.os - ti * c.dw
        off_h = (th - p0h.view(-1, 1, 1)) / c.os - tj * c.dh
        off = _exact(torch.stack([off_w, off_h], -1), c.om_dt, "edge offsets")
    lg = torch.randn(R_, G, P, generator=g, dtype=F64) * 2
    if c.logits:
        rows = torch.arange(R_)
        dom = rows % 4 == 0                                                # one dominant logit of +60
        for gi in range(G):
            lg[rows[dom], gi, (rows[dom] + gi) % P] = 60.0
        lg[rows % 4 == 1] = 1.5                                            # all equal
        spread = torch.linspace(-15.0, 15.0, P, dtype=F64) if P > 1 else torch.zeros(1, dtype=F64)
        lg[rows % 4 == 2] = spread[torch.randperm(P, generator=g)]         # a spread of 30
        m = lg.to(c.om_dt)
    else:
        m = torch.softmax(lg, -1).to(c.om_dt)
    assert bool((store(off.double(), c.om_dt) == off.double()).all()) and bool((store(x.double(), c.dt) == x.double()).all())
    I = dict(x=x, om=None, poison=None)
    if c.ld is None:
        I["off"], I["mask"] = off.reshape(-1).clone(), m.reshape(-1).clone()
    else:
        assert c.ld >= 3 * GP
        om = torch.full((R_, c.ld), SENTINEL, dtype=c.om_dt)
        om[:, :2 * GP] = off.reshape(R_, 2 * GP)
        om[:, 2 * GP:3 * GP] = m.reshape(R_, GP)
        I["om"] = om.reshape(-1)
        I["off"], I["mask"] = I["om"], I["om"][2 * GP:]
    if c.poison is not None:
        I["poison"] = (0, 0, 0)                                            # (image, y, x): where a clamped / out-of-range fetch lands
        I["x"] = x.clone()
        I["x"][0, 0, 0, :] = c.poison
    if c.iset in ("edges", "dyadic"):                                      # the location is exact: float32 == float64
        l32, l64 = locations(c, I, F32), locations(c, I, F64)
        assert all(bool((a.double() == b).all()) for a, b in zip(l32[:2], l64[:2])), c.name
    return I


# ------------------------------------------------------------------------------------------------ the operation
def _read_slots(c, I, mut=None):
    """(off_w, off_h, mask) of shape (rows, G, P) as the kernel addresses them, float64."""
    R_, G, P = n_rows(c), c.G, n_taps(c)
    off_ld, mask_ld, _ = lds(c, mut)
    slot = torch.tensor([t[2] for t in tap_positions(c, mut)])
    r, g = torch.arange(R_).view(-1, 1, 1), torch.arange(G).view(1, -1, 1)
    oi = (r * off_ld + (g * P + slot) * 2).clamp_max(I["off"].numel() - 2)
    mi = (r * mask_ld + g * P + slot).clamp_max(I["mask"].numel() - 1)
    o, m = I["off"].double(), I["mask"].double()
    ow, oh = o[oi], o[oi + 1]
    if mut == "offset_hw":
        ow, oh = oh, ow
    return ow, oh, m[mi]


def locations(c, I, ct, mut=None):
    """(loc_h, loc_w, image index) in the type ct by the kernel's expression: p0_ + ((i dil) + off) os, every operation rounded to ct."""
    p0h, p0w, b = _p0(c, ct, mut)
    ow, oh, _ = _read_slots(c, I, mut)
    taps = tap_positions(c, mut)
    dh, dw = (1, 1) if mut == "no_dilation" else (c.dh, c.dw)
    ti = torch.tensor([t[0] * dw for t in taps], dtype=ct)
    tj = torch.tensor([t[1] * dh for t in taps], dtype=ct)
    os = torch.tensor(c.os, dtype=ct)
    loc_w = p0w.view(-1, 1, 1) + (ti + ow.to(ct)) * os
    loc_h = p0h.view(-1, 1, 1) + (tj + oh.to(ct)) * os
    return loc_h, loc_w, b


def _mask_weights(c, I, ct, mut=None):
    """(m, eps): the mask weights (rows, G, P) in ct and their relative error bound in units of u (zero for weights handed over)."""
    _, _, l = _read_slots(c, I, mut)
    l = l.to(ct)
    if not c.logits:
        return l, torch.zeros_like(l, dtype=F64)
    P = l.shape[-1]
    d = l - l.max(-1, keepdim=True).values
    e = torch.exp(d)
    s = e.sum(-1, keepdim=True)
    if mut == "softmax_16":
        s = s + (16 - P) * torch.exp(-l.max(-1, keepdim=True).values)
    m = e / s
    own = d.double().abs() + EXPF_U
    eps = own + (m.double() * own).sum(-1, keepdim=True) + (P - 1) + 2
    if mut == "mask_fp16":
        m = m.to(F16).to(ct)
    return m, eps


def _evaluate(c, I, ct, mut=None):
    """_evaluate_on on one thread: some thousand operations on tensors of a few thousand values, which a thread pool only slows down."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _evaluate_on(c, I, ct, mut)
    finally:
        torch.set_num_threads(n)


def _evaluate_on(c, I, ct, mut=None):
    """The operation in the type ct on the location of the case's opmath -> dict(v, a, es) of shape (rows, G D) (a, es: float64 sums for the
    bound) and, for a poisoned case, hard / soft (rows, G)."""
    R_, G, D, P, H, W = n_rows(c), c.G, c.D, n_taps(c), c.H, c.W
    loc_h, loc_w, b = locations(c, I, opmath(c), mut)
    loc_h, loc_w = loc_h.to(ct), loc_w.to(ct)
    m, eps = _mask_weights(c, I, ct, mut)
    if mut == "mask_fp16" and not c.logits:
        m = m.to(F16).to(ct)
    x = I["x"].to(ct)
    pz = I["poison"]
    if pz is not None:
        x = x.clone()
        x[pz[0], pz[1], pz[2], :] = 0
    x = x.reshape(c.N, H * W, G, D)
    Hc, Wc = (W, H) if mut == "hw_swapped_validity" else (H, W)
    inr = (loc_h > -1) & (loc_w > -1) & (loc_h < H) & (loc_w < W)
    fh, fw = torch.floor(loc_h), torch.floor(loc_w)
    lh, lw = loc_h - fh, loc_w - fw
    hh, hw = 1 - lh, 1 - lw
    y0, x0 = fh.long(), fw.long()
    bidx = b.view(-1, 1).expand(R_, G)
    gidx = torch.arange(G).view(1, -1).expand(R_, G)
    v = torch.zeros(R_, G, D, dtype=ct)
    a = torch.zeros(R_, G, D, dtype=F64)
    es = torch.zeros(R_, G, D, dtype=F64)
    hard = torch.zeros(R_, G, dtype=torch.bool)
    soft = torch.zeros(R_, G, dtype=torch.bool)
    for q in range(P):
        t = torch.zeros(R_, G, D, dtype=ct)
        at = torch.zeros(R_, G, D, dtype=F64)
        for yy, xx, wt in ((y0, x0, hh * hw), (y0, x0 + 1, hh * lw), (y0 + 1, x0, lh * hw), (y0 + 1, x0 + 1, lh * lw)):
            yy, xx, wt = yy[..., q], xx[..., q], wt[..., q]
            if mut == "lt_last":
                ok = (yy >= 0) & (yy < Hc - 1) & (xx >= 0) & (xx < Wc - 1)
            else:
                ok = (yy >= 0) & (yy <= Hc - 1) & (xx >= 0) & (xx <= Wc - 1)
            ok = inr[..., q] & (ok if mut != "replicate" else torch.ones_like(ok))
            lin = yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)
            val = x[bidx, lin, gidx]
            wq = torch.where(ok, wt, torch.zeros_like(wt)).unsqueeze(-1)
            prod = wq * val
            if mut == "products_fp16":
                prod = prod.to(F16).to(ct)
            t = t + prod
            at = at + wq.double().abs() * val.double().abs()
            if pz is not None:
                touch = ok & (bidx == pz[0]) & (lin == pz[1] * W + pz[2])
                live = (wt != 0) & (m[..., q] != 0)
                hard |= touch & live
                soft |= touch & ~live
        mq = m[..., q].unsqueeze(-1)
        v = v + t * mq
        aq = at * mq.double().abs()
        a = a + aq
        es = es + aq * eps[..., q].unsqueeze(-1)
    return dict(v=v.reshape(R_, G * D), a=a.reshape(R_, G * D), es=es.reshape(R_, G * D), hard=hard, soft=soft & ~hard)


def _e_out(v, pre, dt):
    return U64 * v.abs() if dt == F64 else R.e_out(v, pre, dt)


@functools.lru_cache(None)
def _true(c):
    return _evaluate(c, inputs(c), F64)


def ref(I, c, mut=None, stored=True):
    """(v, bound), float64, shape (rows, G D).  stored=False: the bound in front of the store.  The true reference of a case's own inputs
    is computed once and shared (callers leave it unchanged)."""
    e = _true(c) if mut is None and c.name in BY_NAME and I is inputs(c) else _evaluate(c, I, F64, mut)
    u = U64 if c.dt == F64 else U32
    pre = (n_taps(c) + 10) * u * e["a"] + u * e["es"]
    bound = pre + _e_out(e["v"], pre, c.dt) if stored else pre
    return e["v"], torch.where(e["a"] == 0, torch.zeros_like(bound), bound)


def f32(I, c):
    """The kernel's association in the opmath type, in front of the store."""
    return _evaluate(c, I, opmath(c)).get("v")


def poison_sets(I, c):
    """(hard, soft) expanded to (rows, G D): see the module docstring."""
    e = _true(c)
    ex = lambda t: t.unsqueeze(-1).expand(-1, -1, c.D).reshape(n_rows(c), c.G * c.D)
    return ex(e["hard"]), ex(e["soft"])


OP = Op("gp_dcnv3_forward", CASES, inputs, ref, f32, functools.partial(ref, stored=False))


# ------------------------------------------------------------------------------------------------ what the input sets reach
def classify(c, I):
    """Counts of the taps of a case per class (the issue's list): a integer position in both axes (inside the map); b_m1 / b_last / b_size a
    location exactly -1 / H-1 or W-1 / H or W; c_lo / c_hi strictly inside (-1, 0) / (H-1, H) (or W); d one axis inside, the other outside;
    e beyond +-40; f half-pixel positions in both axes (inside); g (pixel, group) pairs with every tap outside."""
    lh, lw, _ = locations(c, I, opmath(c))
    lh, lw = lh.double(), lw.double()
    H, W = c.H, c.W
    inh, inw = (lh >= 0) & (lh <= H - 1), (lw >= 0) & (lw <= W - 1)
    outh, outw = (lh <= -1) | (lh >= H), (lw <= -1) | (lw >= W)
    isint = lambda t: t == torch.floor(t)
    ishalf = lambda t: t - torch.floor(t) == 0.5
    n = lambda t: int(t.sum())
    inr = (lh > -1) & (lw > -1) & (lh < H) & (lw < W)
    return dict(a=n(inh & inw & isint(lh) & isint(lw)), b_m1=n((lh == -1) | (lw == -1)), b_last=n((lh == H - 1) | (lw == W - 1)), b_size=n((lh == H) | (lw == W)),
                c_lo=n(((lh > -1) & (lh < 0) & ~outw) | ((lw > -1) & (lw < 0) & ~outh)),
                c_hi=n(((lh > H - 1) & (lh < H) & ~outw) | ((lw > W - 1) & (lw < W) & ~outh)),
                d=n((inh & outw) | (inw & outh)), e=n((lh.abs() >= 40) | (lw.abs() >= 40)), f=n(inh & inw & ishalf(lh) & ishalf(lw)),
                g=n((~inr).all(-1)))


def outside_fraction(c, I):
    """Share of the (pixel, group) samples with at least one bilinear corner of a tap outside the map."""
    lh, lw, _ = locations(c, I, opmath(c))
    fh, fw = torch.floor(lh.double()), torch.floor(lw.double())
    out = (fh < 0) | (fh + 1 > c.H - 1) | (fw < 0) | (fw + 1 > c.W - 1)
    return float(out.any(-1).double().mean())


# ------------------------------------------------------------------------------------------------ mutations
def _nonsquare_out(c):
    Ho, Wo = out_hw(c)
    return Ho != Wo


# (mutation, the cases that can expose it): the checker must reject it on at least one of them (tests/test_dcnv3_reference_cpu.py prints which)
MUTATIONS = [
    ("h_outer", lambda c: c.kh * c.kw > 1),
    ("offset_hw", lambda c: True),
    ("hw_swapped_validity", lambda c: c.H != c.W),
    ("lt_last", lambda c: True),
    ("replicate", lambda c: True),
    ("p0_no_halfk_os", lambda c: c.kh > 2 or c.kw > 2),
    ("p0_halfk_unscaled", lambda c: c.os != 1.0 and (c.kh > 2 or c.kw > 2)),
    ("no_dilation", lambda c: c.dh > 1 or c.dw > 1),
    ("softmax_16", lambda c: c.logits and n_taps(c) < 16),
    ("rc_slot", lambda c: c.rc == 1),
    ("ld_dense", lambda c: c.ld is not None),
    ("wo_ho_swapped", _nonsquare_out),
    ("patch_image_square", lambda c: c in PATCH_CASES and _nonsquare_out(c) and c.N > 1),
    ("mask_fp16", lambda c: c.dt == F16 and (c.logits or c.om_dt == F32)),
    ("products_fp16", lambda c: c.dt == F32),
]
