"""Numpy float32 restatement of the ORDERED d xp of the encoder's DCNv3 core (include/givepose_encgrad_ordered.h, GPE_SCATTER_ORDERED),
and the inputs of the tests that hold the kernels against it (tests/test_enc_ordered_cpu.py, tests/test_enc_ordered_gpu.py).

The contract, restated: d xp at destination (b, h, w, g, lane) is the sum of the terms c = fmul(w_k, fmul(dy[(row 4 + g) 64 + lane],
mask[(row 4 + g) 9 + q])) over every source (row, g, tap q, corner k = 1..4) whose corner is the pixel (b, h, w) and lies in the image,
with w_1 = fmul(hh, hw), w_2 = fmul(hh, lw), w_3 = fmul(lh, hw), w_4 = fmul(lh, lw); the terms are added in ascending order of the source
id s = (row 9 + q) 4 + (k - 1), starting from +0, every product and every sum rounded to float32 on its own (numpy's float32 operators do
exactly that: no fused multiply-add).  A destination nothing reaches is +0.

The locations are tests/enc_backward_ref.core_locations on float32 tensors -- (2 wo - 1) + (i + offset), tap q = 3 i + j -- and the cell,
the validity test and lh, lw, hh = 1 - lh, hw = 1 - lw are formed from them as tap_of (csrc/encgrad.hip) forms them, in float32.
"""
import numpy as np
import torch

import enc_backward_ref as R

F = np.float32


def ordered_dxp(offset, mask, dy, N, H, W):
    """offset (rows,72), mask (rows,36) probabilities, dy (rows,256), float32 -> (dxp (N,H,W,256) float32, the per-destination list
    lengths (N,H,W,4) int64)."""
    rows = R.core_rows(N, H, W)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    offset, mask, dy = (np.ascontiguousarray(a, F) for a in (offset, mask, dy))
    assert offset.shape == (rows, 72) and mask.shape == (rows, 36) and dy.shape == (rows, 256)
    lw, lh = (t.numpy() for t in R.core_locations(torch.from_numpy(offset), N, H, W))      # (rows,4,9) float32
    assert lw.dtype == F and lh.dtype == F
    valid = (lh > F(-1)) & (lw > F(-1)) & (lh < F(H)) & (lw < F(W))
    h0 = np.where(valid, np.floor(lh), 0).astype(np.int64)
    w0 = np.where(valid, np.floor(lw), 0).astype(np.int64)
    flh, flw = lh - h0.astype(F), lw - w0.astype(F)
    fhh, fhw = F(1) - flh, F(1) - flw
    assert all(a.dtype == F for a in (flh, flw, fhh, fhw))
    row = np.broadcast_to(np.arange(rows)[:, None, None], (rows, 4, 9))
    g = np.broadcast_to(np.arange(4)[None, :, None], (rows, 4, 9))
    q = np.broadcast_to(np.arange(9)[None, None, :], (rows, 4, 9))
    b = row // (Ho * Wo)
    dest, sid, wt = [], [], []
    for k, (hy, wx, wk) in enumerate(((h0, w0, fhh * fhw), (h0, w0 + 1, fhh * flw), (h0 + 1, w0, flh * fhw), (h0 + 1, w0 + 1, flh * flw))):
        ok = valid & (hy >= 0) & (hy <= H - 1) & (wx >= 0) & (wx <= W - 1)
        dest.append((((b * H + hy) * W + wx) * 4 + g)[ok])
        sid.append(((row * 9 + q) * 4 + k)[ok])
        wt.append(wk[ok])
    dest, sid, wt = np.concatenate(dest), np.concatenate(sid), np.concatenate(wt)
    assert wt.dtype == F
    ndest = N * H * W * 4
    lengths = np.bincount(dest, minlength=ndest)
    order = np.lexsort((sid, dest))      # by destination, then ascending source id
    dest, sid, wt = dest[order], sid[order], wt[order]
    first = np.concatenate(([0], np.cumsum(lengths)))[dest]
    place = np.arange(dest.size) - first      # position inside its destination's list
    srow, sq = sid // 36, sid // 4 % 9
    sg = dest % 4
    acc = np.zeros((ndest, 64), F)            # +0
    dyg = dy.reshape(rows, 4, 64)
    for p in range(int(lengths.max()) if dest.size else 0):
        sel = np.nonzero(place == p)[0]       # at most one term per destination
        tg = dyg[srow[sel], sg[sel]] * mask[srow[sel], sg[sel] * 9 + sq[sel]][:, None]
        c = wt[sel][:, None] * tg
        assert tg.dtype == F and c.dtype == F
        acc[dest[sel]] = acc[dest[sel]] + c
    return acc.reshape(N, H, W, 256), lengths.reshape(N, H, W, 4)


# ------------------------------------------------------------------------------------------------ the cases
PILE_TARGET = (3.25, 2.5)      # (w, h): every tap of the pile-up case samples here


def _rng(seed):
    return np.random.Generator(np.random.Philox(key=[seed, 0x0D3]))


def random_case(N, H, W, seed, scale=2.0, grid=None):
    """xp, offset, mask logits, dy: normal offsets of `scale` pixels (rounded to multiples of `grid` if given, which makes the float32
    locations exact)."""
    r = _rng(seed)
    rows = R.core_rows(N, H, W)
    xp = r.standard_normal((N, H, W, 256)).astype(F)
    off = (r.standard_normal((rows, 72)) * scale).astype(F)
    if grid is not None:
        off = (np.round(off / grid) * grid).astype(F)
    return xp, off, r.standard_normal((rows, 36)).astype(F), r.standard_normal((rows, 256)).astype(F)


def pile_up_case(N=1, H=16, W=16, seed=7):
    """Every tap's offset is target - ((2 wo - 1) + i, (2 ho - 1) + j): exact in float32, so all rows x 9 taps of a group land in the
    one cell around PILE_TARGET and each of its four pixels receives rows x 9 terms per group; every other pixel receives none."""
    xp, off, logits, dy = random_case(N, H, W, seed)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rows = N * Ho * Wo
    r = np.arange(rows)
    wo, ho = r % Wo, r // Wo % Ho
    qq = np.arange(9)
    off = np.empty((rows, 4, 9, 2), np.float64)
    off[..., 0] = PILE_TARGET[0] - ((2 * wo - 1)[:, None, None] + (qq // 3)[None, None, :])
    off[..., 1] = PILE_TARGET[1] - ((2 * ho - 1)[:, None, None] + (qq % 3)[None, None, :])
    assert np.array_equal(off.astype(F).astype(np.float64), off)
    return xp, off.astype(F).reshape(rows, 72), logits, dy


THRESHOLD_COUNTS = (64, 65, 63, 1)      # per group: the longest list one wavefront holds, the shortest that it walks, and two below


def threshold_case(N=1, H=8, W=8, seed=9):
    """The pile-up case with only the first THRESHOLD_COUNTS[g] taps of group g (in id order) on the target; every other tap is far
    outside the image.  The four pixels of the target cell then hold lists of exactly 64, 65, 63 and 1 ids: either side of the
    length at which the gather changes from one id per lane to repeated selection."""
    xp, off, logits, dy = pile_up_case(N, H, W, seed)
    rows = off.shape[0]
    assert rows * 9 >= max(THRESHOLD_COUNTS)
    off = off.reshape(rows, 4, 9, 2).copy()
    tap = np.arange(rows * 9).reshape(rows, 9)      # (row 9 + q): the id order inside a group
    for g, n in enumerate(THRESHOLD_COUNTS):
        off[:, g][tap >= n] = F(-1000.0)
    return xp, off.reshape(rows, 72), logits, dy


def softmax_mask(logits):
    """(rows,36) float32 logits -> probabilities per group of 9, float32 (the CPU tests' stand-in for the mask the device saves)."""
    return torch.softmax(torch.from_numpy(logits).reshape(-1, 4, 9), -1).reshape(-1, 36).numpy()
