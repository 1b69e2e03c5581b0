"""Float64 reference, per-element error bounds, cases and mutations of the DCNv3 BACKWARD: gp_dcnv3_backward (csrc/dcnv3_any.hip:
dcnv3_any_bwd_kernel<double | float | half>, behind givepose_amd.dcnv3_backward and DCNv3Function.backward) and the encoder's
gpe_dcnv3_core_backward (csrc/encgrad.hip: core_backward_kernel, the same operation at G 4, D 64, K 3, stride 2, pad 1, os 1, float32).
No GPU here: tests/test_dcnv3_backward_reference_cpu.py checks this file against itself, the goldens, the C oracle and autograd;
tests/test_dcnv3_backward_conformance_gpu.py and tests/test_enc_backward_gpu.py hold the kernels against it.  Case, mk, the input sets,
locations, classify, check / check_buffer and SENTINEL are those of tests/dcnv3_reference.py, which this file imports and leaves alone.

The operation (a restatement of dcnv3_im2col_cuda.cuh:386-487 from its definition; rows, groups, tap slots, the location and the validity
test are the forward's -- see the dcnv3_reference docstring).  With g = grad_output[r, g, :] (D channels), m the mask weight of the tap,
(h, w) its location, h_low = floor h, lh = h - h_low, hh = 1 - lh (the same along w), corner k = 1 .. 4 at (h_low, w_low), (h_low, w_low + 1),
(h_low + 1, w_low), (h_low + 1, w_low + 1) with weight W_k = (hh hw, hh lw, lh hw, lh lw) and value v_k (zero and skipped for a corner outside
the map), for every tap with h > -1, w > -1, h < H, w < W:

    grad_input[b, corner k, g, c] += W_k g_c m                                         (scattered: one term per (row, tap, corner))
    grad_mask[r, g, q]      = sum_c g_c (W_1 v_1c + W_2 v_2c + W_3 v_3c + W_4 v_4c)
    grad_offset[r, g, q, 0] = sum_c os gwc_c g_c m,   gwc_c = -hh v_1c + hh v_2c - lh v_3c + lh v_4c       (the w slot)
    grad_offset[r, g, q, 1] = sum_c os ghc_c g_c m,   ghc_c = -hw v_1c - lw v_2c + hw v_3c + lw v_4c       (the h slot)

At an integer location floor puts the whole weight on corner 1 and the derivative is the one towards corner 2 / 3 (the right-hand one).  A
tap outside the map leaves its grad_offset / grad_mask slots at zero and scatters nothing.

ref(I, c) -> {"grad_input": (v, bound) of shape (N, H, W, G D), "grad_offset": (rows, G, P, 2), "grad_mask": (rows, G, P)}, float64.  v is
exact on the operands the kernel sees; the LOCATION is evaluated in the kernel's opmath by dcnv3_reference.locations (the same restriction
of the inputs: continuous offsets only with os 1, otherwise the exact "edges" / "dyadic" sets), everything behind it in float64.

Bound = c u a + t + e_out per element; a = the same sum on absolute values, u = 2^-24 (2^-53 for double), counted from the kernel:

  grad_input    c = n + 6, n = the number of (row, tap, corner) terms that reach the element (from the reference).  One term carries 5
                roundings: 3 in the corner weight (lh or hh, lw or hw -- one subtraction each: h - h_low is exact for h >= 0 and 1 - lh
                rounds once; for h in (-1, 0) h + 1 rounds once and 1 - lh is exact -- and their product), 1 in tg = g_c m, 1 in W_k tg.
                The atomics add the n terms in an unspecified order: whatever the order, n - 1 additions (the first one, onto the zero
                of the memset, is exact), each of a partial sum bounded by a.  5 + (n - 1) + 2, the 2 for the (1 + u)^k growth of the
                first-order terms as in ops_reference.  a = sum over the terms of |W_k| |g_c| |m|.
  grad_mask     c = s + 10.  Per channel 8 roundings on magnitudes bounded by |g_c| sum_k |W_k| |v_kc|: 3 in a corner weight, 1 in W_k v_k,
                3 additions, 1 product with g_c (the FMA forms round less often).  The channel sum is a chain of ceil(D / 64) additions
                per lane (lane l holds channels l, l + 64, ...) and a 6-level butterfly; lanes without a channel add exact zeros.  An
                element of the sum passes at most ceil(D / 64) + 6 additions, and no summation order of D terms has more than D - 1:
                s = min(D - 1, ceil(D / 64) + 6) roundings of partial sums bounded by a.  + 2 for growth.
  grad_offset   c = s + 10.  Per channel: gwc_c has 5 roundings on |hh| (|v_1| + |v_2|) + |lh| (|v_3| + |v_4|) -- 1 in the factor lh or hh
                (the other of the pair is exact, see above), 1 in its product with v_k, at most 3 in the accumulation -- and the three
                products os gwc, g_c m and their product 3 more: 8, the channel sum s as above, + 2.  a takes the absolute values INSIDE
                gwc / ghc, where the four corner terms cancel, and carries |os|: a = |os| |m| sum_c |g_c| sum_k |factor_k| |v_kc|.
                (The one factor whose RELATIVE error is unbounded -- hh = 1 - fl(1 + h) for h in (-0.5, 0) -- multiplies only the
                corners of row / column -1, which are outside the map and skipped, as in the forward.)
  t             underflow: 2^-126 (2^-1022 for double) per operation counted in c, where a > 0 -- a product below the smallest normal
                number loses at most that much whether the hardware rounds it to a subnormal or flushes it.
  e_out         0 at the C ABI, whose three results are the opmath accumulators themselves (float for half / float operands).  For
                float16 operands givepose_amd.dcnv3_backward rounds the three results once to half: stored=torch.float16 adds
                ops_reference.e_out (2^-11 (|v| + the bound so far) + 2^-25).
  a == 0        bound 0 and the value must be an exact zero: every grad_offset / grad_mask slot of a tap outside the map, every
                grad_input element that no valid corner reaches (or reaches only with zero operands), and the unconsumed tail of an
                offset / mask buffer longer than the kernel consumes (buffers()).

f32(I, c): the kernel's association in the opmath type -- per lane the chain over its channels, then the butterfly; the scatter in one
fixed order of the terms.  It must stay within HALF of the bound in front of the store on every case and tensor
(tests/test_dcnv3_backward_reference_cpu.py); no count had to be raised to meet it.

ref(..., mut=...): deliberately wrong float64 variants (MUTATIONS); the checker must reject each on at least one case.

dlogits_ref(m, gm, e_gm, P): the encoder's softmax backward dmask_logits_q = m_q (gm_q - sum_j m_j gm_j) in float64 on the saved mask m, and
its bound from grad_mask's bound e pushed through the expression.  The kernel forms dot = fma(m_j, gm_j, dot) over the P taps, then
m_q (gm_q - dot):  err(dot) <= sum_j |m_j| e_j + P u S, S = sum_j |m_j| |gm_j| (P roundings of partial sums bounded by S);
err(gm_q - dot) <= e_q + err(dot) + u (|gm_q| + S); the product with m_q rounds once more on |m_q| (|gm_q| + S).  With 2 for growth:
bound_q = |m_q| (e_q + sum_j |m_j| e_j) + (P + 4) u |m_q| (|gm_q| + S) + 2^-126.
"""
import functools
import zlib

import torch

import dcnv3_reference as D
import ops_reference as R
from dcnv3_reference import F16, F32, F64, SENTINEL, U32, U64, mk, n_rows, n_taps, opmath  # noqa: F401

TENSORS = ("grad_input", "grad_offset", "grad_mask")
TINY = {F32: 2.0 ** -126, F64: 2.0 ** -1022}


# ------------------------------------------------------------------------------------------------ cases
def _new_cases():
    pn = dict(N=3, H=5, W=8, G=4, K=3, s=2, p=1)                      # the PoseNet geometry on a non-square map with an odd side: 3 x 4 outputs
    out = []
    for dt in (F64, F32, F16):
        t = D._tn(dt)[0]
        out += [mk(f"bwd-{t}-pn-D64-edges-full", dt, **pn, D=64, entry="any", iset="edges"),
                mk(f"bwd-{t}-pn-D16-c3-full", dt, **pn, D=16, entry="any"),
                mk(f"bwd-{t}-D128-c3", dt, N=1, H=4, W=6, G=2, D=128, K=3, entry="any"),                     # the channel loop runs twice, all lanes live
                mk(f"bwd-{t}-partial-G3D8-edges-os2", dt, N=1, H=3, W=5, G=3, D=8, K=3, entry="any", iset="edges", os=2.0)]   # 45 waves: 11 workgroups + 1
    return out


CASES = [c for c in D.ANY_CASES if c.poison is None] + _new_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def full_buffers(c):
    """The offset / mask buffers are as long as the FULL-resolution map (N H W rows), of which the kernel consumes the first rows."""
    return c.name.endswith("-full")


def buf_rows(c):
    return c.N * c.H * c.W if full_buffers(c) else n_rows(c)


def n_sum(c):
    return min(c.D - 1, -(-c.D // 64) + 6)


# ------------------------------------------------------------------------------------------------ inputs
def grad_output(c):
    """Seeded normal in the case's type; every 7th output row all zeros; at (row 1, the last group) a single non-zero channel; where
    D > 1, channel 0 of group 0 zero in every row, so that every case has grad_input elements that only zero terms reach."""
    g = torch.Generator().manual_seed(zlib.crc32((c.name + "/grad_output").encode()) & 0x7FFFFFFF)
    go = torch.randn(n_rows(c), c.G, c.D, generator=g, dtype=F64)
    go[::7] = 0
    if c.D > 1:
        go[:, 0, 0] = 0
    one = go[1, c.G - 1, c.D // 2].clone()
    go[1, c.G - 1] = 0
    go[1, c.G - 1, c.D // 2] = one
    return go.to(c.dt).reshape(n_rows(c), c.G * c.D)


@functools.lru_cache(None)
def inputs(c):
    """x (N, H, W, G D); off / mask: the flat buffers of buf_rows(c) rows (SENTINEL behind the consumed rows); gout (rows, G D).  All in c.dt."""
    assert c.entry == "any" and c.ld is None and not c.logits and c.poison is None
    I = D.inputs(c)
    extra = (buf_rows(c) - n_rows(c)) * c.G * n_taps(c)
    tail = lambda k: torch.full((k,), SENTINEL, dtype=c.dt)
    return dict(x=I["x"], off=torch.cat([I["off"], tail(2 * extra)]), mask=torch.cat([I["mask"], tail(extra)]), gout=grad_output(c))


# ------------------------------------------------------------------------------------------------ the operation
LOCATION_MUTATIONS = ("h_outer", "rc_slot", "wo_ho_swapped", "no_dilation")


def _wave_reduce(t):
    """Sum over the last axis as the wave does it: lane l chains channels l, l + 64, ..., then v += v[lane ^ o] for o = 32 .. 1."""
    n = t.shape[-1]
    pad = -n % 64
    if pad:
        t = torch.cat([t, torch.zeros(*t.shape[:-1], pad, dtype=t.dtype)], -1)
    t = t.reshape(*t.shape[:-1], -1, 64)
    v = torch.zeros(*t.shape[:-2], 64, dtype=t.dtype)
    for k in range(t.shape[-2]):
        v = v + t[..., k, :]
    lane = torch.arange(64)
    o = 32
    while o:
        v = v + v[..., lane ^ o]
        o >>= 1
    return v[..., 0]


def _evaluate(c, I, ct, mut=None, emulate=False):
    n = torch.get_num_threads()
    torch.set_num_threads(1)           # small tensors, and index_add_ in one fixed order
    try:
        return _evaluate_on(c, I, ct, mut, emulate)
    finally:
        torch.set_num_threads(n)


def _evaluate_on(c, I, ct, mut, emulate):
    """The backward in the type ct on the location of the case's opmath -> dict of the three gradients (ct), their a (float64) and the
    number of terms n that reach every grad_input element."""
    R_, G, Dc, P, H, W, N = n_rows(c), c.G, c.D, n_taps(c), c.H, c.W, c.N
    lmut = mut if mut in LOCATION_MUTATIONS else None
    Ir = dict(off=I["off"], mask=I["mask"])
    loc_h, loc_w, b = D.locations(c, Ir, opmath(c), lmut)
    loc_h, loc_w = loc_h.to(ct), loc_w.to(ct)
    m = D._read_slots(c, Ir, lmut)[2].to(ct)
    g = I["gout"].to(ct).reshape(R_, G, Dc)
    if mut == "d64_dropped":
        g = g.clone()
        g[..., 64:] = 0
    x = I["x"].to(ct).reshape(N * H * W, G, Dc)
    os = torch.tensor(1.0 if mut == "no_os" else c.os, dtype=ct)
    Hv, Wv = (W, H) if mut == "hw_swapped_validity" else (H, W)
    lo = (lambda t: t >= -1) if mut == "ge_m1" else (lambda t: t > -1)
    hi = (lambda t, S: t <= S) if mut == "le_H" else (lambda t, S: t < S)
    inr = lo(loc_h) & lo(loc_w) & hi(loc_h, Hv) & hi(loc_w, Wv)
    fh, fw = torch.floor(loc_h), torch.floor(loc_w)
    lh, lw = loc_h - fh, loc_w - fw
    hh, hw = 1 - lh, 1 - lw
    y0, x0 = fh.long(), fw.long()
    y1, x1 = y0 + 1, x0 + 1
    top, bot, lef, rig = y0 >= 0, y1 <= H - 1, x0 >= 0, x1 <= W - 1            # the kernel's o1 .. o4
    gidx = torch.arange(G).view(1, -1).expand(R_, G)
    base = (b * (H * W)).view(-1, 1)
    gi = torch.zeros(N * H * W * G, Dc, dtype=ct)
    a_gi = torch.zeros(N * H * W * G, Dc, dtype=F64)
    n_gi = torch.zeros(N * H * W * G, dtype=F64)
    gm, gw, gh = (torch.zeros(R_, G, P, dtype=ct) for _ in range(3))
    a_gm, a_gw, a_gh = (torch.zeros(R_, G, P, dtype=F64) for _ in range(3))
    red = _wave_reduce if emulate else (lambda t: t.sum(-1))
    sgn_w2 = -1.0 if mut == "gwc_sign" else 1.0
    sgn_h3 = -1.0 if mut == "ghc_sign" else 1.0
    for q in range(P):
        s = lambda t: t[..., q]
        valid, mq = s(inr), s(m).unsqueeze(-1)
        tg = g * mq
        corners = ((s(y0), s(x0), s(hh) * s(hw), s(top) & s(lef), -s(hh), -s(hw)),
                   (s(y0), s(x1), s(hh) * s(lw), s(top) & s(rig), sgn_w2 * s(hh), -s(lw)),
                   (s(y1), s(x0), s(lh) * s(hw), s(bot) & s(lef), -s(lh), sgn_h3 * s(hw)),
                   (s(y1), s(x1), s(lh) * s(lw), s(bot) & s(rig), s(lh), s(lw)))
        S, gwc, ghc = (torch.zeros(R_, G, Dc, dtype=ct) for _ in range(3))
        Sa, gwa, gha = (torch.zeros(R_, G, Dc, dtype=F64) for _ in range(3))
        for yy, xx, wt, flag, cw, ch in corners:
            if mut == "clamped_scatter":
                yy, xx, flag = yy.clamp(0, H - 1), xx.clamp(0, W - 1), torch.ones_like(flag)
            if mut == "all_a1":
                yy, xx = s(y0).clamp(0, H - 1), s(x0).clamp(0, W - 1)
            ok = valid & flag
            lin = base + yy * W + xx
            if mut is None:
                assert bool(((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W))[ok].all())
            lin = lin.clamp(0, N * H * W - 1)                    # (a mutant's row H is row 0 of the next image)
            z = lambda t: torch.where(ok, t, torch.zeros_like(t)).unsqueeze(-1)
            val = x[lin, gidx] * ok.unsqueeze(-1).to(ct)
            wq, cw, ch = z(wt), z(cw), z(ch)
            S = S + wq * val
            gwc = gwc + cw * val
            ghc = ghc + ch * val
            va = val.double().abs()
            Sa += wq.double().abs() * va
            gwa += cw.double().abs() * va
            gha += ch.double().abs() * va
            term = wq * (g if mut == "gin_no_m" else tg)
            idx = (lin * G + gidx).reshape(-1)
            gi.index_add_(0, idx, term.reshape(-1, Dc))
            a_gi.index_add_(0, idx, (wq.double().abs() * (g if mut == "gin_no_m" else tg).double().abs()).reshape(-1, Dc))
            n_gi.index_add_(0, idx, ok.reshape(-1).double())
        gm[..., q] = red(g * S) * (s(m) if mut == "gmask_times_m" else 1)
        gw[..., q] = red(os * gwc * tg)
        gh[..., q] = red(os * ghc * tg)
        ga = g.double().abs()
        oa = abs(float(os)) * s(m).double().abs()
        a_gm[..., q] = (ga * Sa).sum(-1)
        a_gw[..., q] = oa * (ga * gwa).sum(-1)
        a_gh[..., q] = oa * (ga * gha).sum(-1)
    go = torch.stack([gh, gw] if mut == "goff_swapped" else [gw, gh], -1)
    return dict(grad_input=gi.reshape(N, H, W, G * Dc), grad_offset=go, grad_mask=gm, a_grad_input=a_gi.reshape(N, H, W, G * Dc),
                a_grad_offset=torch.stack([a_gw, a_gh], -1), a_grad_mask=a_gm, n=n_gi.view(N, H, W, G, 1).expand(N, H, W, G, Dc).reshape(N, H, W, G * Dc))


@functools.lru_cache(None)
def _true(c):
    return _evaluate(c, inputs(c), F64)


def ref(I, c, mut=None, stored=None):
    """{tensor: (v, bound)}, float64.  stored=None: the C ABI (opmath results); stored=torch.float16: behind the rounding to half of
    givepose_amd.dcnv3_backward.  The true reference of a case's own inputs is computed once and shared (callers leave it unchanged)."""
    e = _true(c) if mut is None and BY_NAME.get(c.name) is c and I is inputs(c) else _evaluate(c, I, F64, mut)
    u = U64 if c.dt == F64 else U32
    counts = dict(grad_input=e["n"] + 6, grad_offset=n_sum(c) + 10, grad_mask=n_sum(c) + 10)
    out = {}
    for k in TENSORS:
        v, a = e[k], e["a_" + k]
        pre = counts[k] * (u * a + TINY[opmath(c)])
        bound = pre + R.e_out(v, pre, stored) if stored is not None else pre
        out[k] = (v, torch.where(a == 0, torch.zeros_like(bound), bound))
    return out


def f32(I, c):
    """The kernel's association in the opmath type: {tensor: value}."""
    e = _evaluate(c, I, opmath(c), emulate=True)
    return {k: e[k] for k in TENSORS}


def buffers(c, res, mut=None):
    """{tensor: (v, bound)} as flat buffers of the size the entry is handed: grad_offset / grad_mask are as long as the offset / mask
    buffers, the unconsumed tail exactly zero."""
    extra = (buf_rows(c) - n_rows(c)) * c.G * n_taps(c)
    out = {}
    for k, mult in (("grad_input", 0), ("grad_offset", 2), ("grad_mask", 1)):
        v, bound = (t.reshape(-1) for t in res[k])
        fill = 1.0 if mut == "tail_not_zero" else 0.0
        out[k] = (torch.cat([v, torch.full((mult * extra,), fill, dtype=F64)]), torch.cat([bound, torch.zeros(mult * extra, dtype=F64)]))
    return out


def dlogits_ref(m, gm, e_gm, P):
    """(v, bound) of m_q (gm_q - sum_j m_j gm_j) over groups of P taps (the last axis), float64: see the module docstring."""
    m, gm, e_gm = m.double(), gm.double(), e_gm.double()
    dot = (m * gm).sum(-1, keepdim=True)
    S = (m.abs() * gm.abs()).sum(-1, keepdim=True)
    v = m * (gm - dot)
    bound = m.abs() * (e_gm + (m.abs() * e_gm).sum(-1, keepdim=True)) + (P + 4) * U32 * m.abs() * (gm.abs() + S) + TINY[F32]
    return v, bound


# ------------------------------------------------------------------------------------------------ mutations
# (mutation, the cases that can expose it): the checker must reject it on at least one of them
MUTATIONS = [
    ("goff_swapped", lambda c: True),
    ("no_os", lambda c: c.os != 1.0),
    ("gwc_sign", lambda c: True),
    ("ghc_sign", lambda c: True),
    ("gmask_times_m", lambda c: True),
    ("gin_no_m", lambda c: True),
    ("clamped_scatter", lambda c: True),
    ("ge_m1", lambda c: c.iset == "edges"),
    ("le_H", lambda c: c.iset == "edges"),
    ("hw_swapped_validity", lambda c: c.H != c.W),
    ("h_outer", lambda c: c.kh * c.kw > 1),
    ("rc_slot", lambda c: c.rc == 1),
    ("wo_ho_swapped", D._nonsquare_out),
    ("no_dilation", lambda c: c.dh > 1 or c.dw > 1),
    ("d64_dropped", lambda c: c.D > 64),
    ("all_a1", lambda c: True),
    ("tail_not_zero", full_buffers),
]
