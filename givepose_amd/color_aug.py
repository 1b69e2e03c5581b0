"""The colour augmentation on the device: uint8 frames -> augmented uint8 frames, before TrainBatchBuilder crops them.

Host side of `gpca_luma_partials` and `gpca_apply` (include/givepose_coloraug.h, which states the arithmetic).  The reference's loader
augments the whole RGB frame with probability color_aug_prob = 0.8 before any crop (datasets/load_data_nocs.py:231-237, 559-574); its
default color_aug_type 'new' is

    Sequential([Sometimes(0.3, pillike.EnhanceSharpness(factor=(0, 2))), Sometimes(0.5, pillike.EnhanceContrast(factor=(0.5, 1.5))),
                Sometimes(0.5, pillike.EnhanceBrightness(factor=(0.5, 1.5))), Sometimes(0.3, pillike.EnhanceColor(factor=(0, 3)))],
               random_order=True)

and imgaug's pillike operations wrap PIL.ImageEnhance, whose integer and float32 arithmetic the kernels restate byte for byte
(tests/color_aug_ref.py is the numpy form, tests/golden/color_aug_pil.npz Pillow's own output).

What is drawn is the reference's DISTRIBUTION, not imgaug's stream: imgaug is not installed where this library is tested and its
generator is not restated.  Per frame `color_aug_draws` draws whether to augment at all (u < prob), a uniform random order of the four
operations, each operation on with its own probability, and a factor uniform in its range, from numpy's Philox keyed by the seed (as
train_batch.host_draws draws the DZI boxes).  A caller who needs other draws passes an explicit plan.

Only 'new' is built.  The other color_aug_type values of the reference use imgaug or cv2 operations that this library does not
restate, and are refused by name.
"""
import numpy as np
import torch

from . import _lib

OPS = {"none": 0, "sharpness": 1, "contrast": 2, "brightness": 3, "color": 4}
DRAW_TAG = 0x6361          # Philox key [seed, DRAW_TAG]: the draws of a seeded call
# the children of 'new' in the order the reference lists them: (operation, probability, factor range)
NEW_CHILDREN = (("sharpness", 0.3, (0.0, 2.0)), ("contrast", 0.5, (0.5, 1.5)), ("brightness", 0.5, (0.5, 1.5)), ("color", 0.3, (0.0, 3.0)))
AUG_REFUSED = {"aae": "imgaug operations (CoarseDropout, GaussianBlur, Add, Invert, Multiply, LinearContrast)",
               "cosy+aae": "imgaug operations (CoarseDropout, GaussianBlur, Add, Invert, Multiply, AdditiveGaussianNoise, LinearContrast) next to "
                           "the pillike ones",
               "new1": "imgaug operations (MultiplyHueAndSaturation, a cv2 colour-space round trip) next to the pillike ones",
               "code": "imgaug operations (whatever expression color_aug_code holds, evaluated)",
               "code_albu": "cv2 operations (an albumentations pipeline, which the reference's own loader never constructs)"}


def _check_aug_type(aug_type):
    aug_type = str(aug_type).lower()
    if aug_type in AUG_REFUSED:
        raise ValueError(f"color_aug_type {aug_type!r} is not supported: it uses {AUG_REFUSED[aug_type]} that this library does not restate")
    if aug_type != "new":
        raise ValueError(f"color_aug_type {aug_type!r}: only 'new' is built")
    return aug_type


def color_aug_draws(seed, F, aug_type="new", prob=0.8, enable=None):
    """The plan of a seeded call: {"ops": (F,4) int32 codes of OPS, "factors": (F,4) float32}.

    From np.random.Generator(np.random.Philox(key=[seed, DRAW_TAG])), in this order: F uniforms (augment the frame where u < prob),
    (F,4) uniforms whose ascending order is the frame's order of the four operations, (F,4) uniforms (operation c of NEW_CHILDREN is on
    where u < its probability), (F,4) uniforms (its factor lo + (hi - lo) u, rounded to float32).  Operations that are off are "none";
    the others stand compacted to the left in the frame's order.  enable: (F,) bool, False switches a frame's augmentation off (the
    reference's COLOR_AUG_SYN_ONLY is such a choice); the draws of the other frames do not depend on it.

    This is the distribution of the reference's augmenter, NOT imgaug's stream: imgaug's generator is not restated (module docstring)."""
    _check_aug_type(aug_type)
    seed, F = int(seed), int(F)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed: {seed} is not in [0, 2^64)")
    if F < 0 or not 0.0 <= prob <= 1.0:
        raise ValueError(f"color_aug_draws: F = {F} must be >= 0 and prob = {prob} in [0, 1]")
    g = np.random.Generator(np.random.Philox(key=[seed, DRAW_TAG]))
    aug = g.random(F) < prob
    order = np.argsort(g.random((F, 4)), axis=1, kind="stable")            # order[f, j]: the child that runs j-th
    on = g.random((F, 4)) < np.array([c[1] for c in NEW_CHILDREN])
    lo, hi = (np.array([c[2][i] for c in NEW_CHILDREN]) for i in (0, 1))
    fac = (lo + (hi - lo) * g.random((F, 4))).astype(np.float32)
    if enable is not None:
        enable = np.asarray(enable)
        if enable.shape != (F,) or enable.dtype != np.bool_:
            raise ValueError(f"enable must be ({F},) bool, not {enable.shape} {enable.dtype}")
        aug = aug & enable
    codes = np.array([OPS[c[0]] for c in NEW_CHILDREN], dtype=np.int32)
    live = np.take_along_axis(on, order, 1) & aug[:, None]
    ops = np.where(live, codes[order], 0).astype(np.int32)
    factors = np.where(live, np.take_along_axis(fac, order, 1), np.float32(1)).astype(np.float32)
    left = np.argsort(~live, axis=1, kind="stable")                       # live entries first, in their order
    return {"ops": np.take_along_axis(ops, left, 1), "factors": np.take_along_axis(factors, left, 1)}


def stage_tables(ops, factors):
    """The device's stage tables of a plan (include/givepose_coloraug.h): (n_stages, F, 4) int32 rows {op, factor bits, src, dst}, one
    table per position of the plan that some frame uses, and the number of operations of the busiest frame.  A frame's i-th operation
    reads `frames` (i = 0) or the buffer the one before wrote, and writes `out` (its last) or tmp0 / tmp1 in turn; a frame without
    operations is copied by a "none" row of the first table."""
    F, S = ops.shape
    live = ops != 0
    i = np.cumsum(live, axis=1) - 1
    k = live.sum(1)
    src = np.where(i == 0, _lib.GPCA_BUF_FRAMES, _lib.GPCA_BUF_TMP0 + (i - 1) % 2)
    dst = np.where(i == k[:, None] - 1, _lib.GPCA_BUF_OUT, _lib.GPCA_BUF_TMP0 + i % 2)
    rows = np.stack([np.where(live, ops, _lib.GPCA_OP_SKIP), np.ascontiguousarray(factors, dtype=np.float32).view(np.int32), src, dst], -1)
    rows = np.ascontiguousarray(rows.transpose(1, 0, 2)[live.any(0)], dtype=np.int32)
    copy = np.array([_lib.GPCA_OP_NONE, np.float32(1).view(np.int32), _lib.GPCA_BUF_FRAMES, _lib.GPCA_BUF_OUT], dtype=np.int32)
    if len(rows) == 0:
        rows = np.broadcast_to(copy, (1, F, 4)).copy()
    else:
        rows[0, k == 0] = copy
    return rows, int(k.max())


class ColorAugmenter:
    """Device-side form of the reference's colour augmentation of a frame (color_aug_type 'new').

        aug = ColorAugmenter(480, 640, device)
        frames = aug(frames, seed=step)                       # (F,480,640,3) uint8 -> the same, augmented
        data = builder(frames, ...)                           # TrainBatchBuilder

    The launch count does not depend on F: per position of the plan that some frame uses, one apply launch and, where a frame's
    operation there is a Contrast, one reduction launch before it."""

    def __init__(self, im_H, im_W, device, aug_type="new", prob=0.8):
        self.aug_type = _check_aug_type(aug_type)
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f"prob {prob} must lie in [0, 1]")
        if im_H < 3 or im_W < 3 or 3 * im_H * im_W >= 1 << 30:
            raise ValueError(f"ColorAugmenter: im_H {im_H} and im_W {im_W} must be at least 3 and 3 H W below 2^30")
        self.H, self.W, self.prob = int(im_H), int(im_W), float(prob)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ColorAugmenter runs on a HIP device only (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._tmp = [None, None]          # the ping-pong buffers, (capacity,H,W,3) uint8 each, made when a plan first needs them
        self._partials = None             # (capacity, GPCA_PARTIALS) sums of L
        self.launches = 0                 # of the last call

    def _plan(self, plan, F):
        if not isinstance(plan, dict) or set(plan) != {"ops", "factors"}:
            raise ValueError("plan must be {'ops': (F,S) int32, 'factors': (F,S) float32}")
        ops, factors = np.asarray(plan["ops"]), np.asarray(plan["factors"])
        if ops.ndim != 2 or ops.shape[0] != F or ops.shape[1] < 1 or ops.dtype.kind not in "iu":
            raise ValueError(f"plan['ops'] must be an integer ({F},S) array with S >= 1, not {ops.shape} {ops.dtype}")
        if factors.shape != ops.shape or factors.dtype.kind != "f":
            raise ValueError(f"plan['factors'] must be a float {ops.shape} array, not {factors.shape} {factors.dtype}")
        if ops.min() < 0 or ops.max() > max(OPS.values()):
            raise ValueError(f"plan['ops'] must hold the codes 0..{max(OPS.values())} of OPS")        # the kernels trust the table
        with np.errstate(over="ignore"):
            factors = factors.astype(np.float32)
        if not np.isfinite(factors).all():
            raise ValueError("plan['factors'] must be finite (in float32)")
        return ops.astype(np.int32), factors

    def _buffer(self, slot, F):
        t = self._tmp[slot]
        if t is None or t.shape[0] < F:
            self._tmp[slot] = None        # let the smaller one go first
            t = self._tmp[slot] = torch.empty((F, self.H, self.W, 3), device=self.device, dtype=torch.uint8)
        return t

    def __call__(self, frames, plan=None, seed=None, enable=None, out=None):
        """frames (F,H,W,3) uint8, on the device (or host: copied); never written.  Exactly one of
            plan = {"ops": (F,S) codes of OPS, any sequence, repeats included, "factors": (F,S) finite floats}
            seed = an int in [0, 2^64): the plan is color_aug_draws(seed, F, aug_type, prob, enable).
        enable (F,) bool switches frames off in either form.  Writes into `out` (caller-owned, (F,H,W,3) uint8 on the device, not
        overlapping `frames`) or a fresh tensor, and returns it."""
        dev, H, W = self.device, self.H, self.W
        if (plan is None) == (seed is None):
            raise ValueError("ColorAugmenter: exactly one of plan and seed must be given")
        frames = torch.as_tensor(frames)
        if frames.dtype != torch.uint8:
            raise ValueError(f"frames must be uint8, not {frames.dtype}")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (H, W, 3) or not 1 <= frames.shape[0] <= _lib.GPCA_MAX_FRAMES:
            raise ValueError(f"frames {tuple(frames.shape)} does not match (F,{H},{W},3) with 1 <= F <= {_lib.GPCA_MAX_FRAMES}")
        frames = frames.to(dev).contiguous()
        F = frames.shape[0]
        if seed is not None:
            plan = color_aug_draws(seed, F, self.aug_type, self.prob, enable)
            ops, factors = plan["ops"], plan["factors"]
        else:
            ops, factors = self._plan(plan, F)
            if enable is not None:
                enable = np.asarray(enable)
                if enable.shape != (F,) or enable.dtype != np.bool_:
                    raise ValueError(f"enable must be ({F},) bool, not {enable.shape} {enable.dtype}")
                ops = np.where(enable[:, None], ops, 0).astype(np.int32)
        if out is None:
            out = torch.empty_like(frames)
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(frames.shape) or out.dtype != torch.uint8 or \
                not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous uint8 {tuple(frames.shape)} tensor on {dev}")
        nbytes = frames.numel()
        if out.data_ptr() < frames.data_ptr() + nbytes and frames.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError("out must not alias frames")
        tables, kmax = stage_tables(ops, factors)
        tmp = [self._buffer(s, F).data_ptr() if kmax >= 2 + s else None for s in (0, 1)]
        contrast = (tables[:, :, 0] == _lib.GPCA_OP_CONTRAST).any(1)
        if contrast.any() and (self._partials is None or self._partials.shape[0] < F):
            self._partials = torch.empty((F, _lib.GPCA_PARTIALS), device=dev, dtype=torch.int64)
        partials = self._partials.data_ptr() if contrast.any() else None
        table = torch.from_numpy(tables).pin_memory().to(dev, non_blocking=True)
        L = _lib.load()
        stream = torch.cuda.current_stream(dev).cuda_stream
        self.launches = 0
        for st in range(len(tables)):
            tp = table.data_ptr() + st * F * 16
            if contrast[st]:
                _lib.check(L.gpca_luma_partials(frames.data_ptr(), tmp[0], tmp[1], tp, partials, F, H, W, stream), "gpca_luma_partials")
                self.launches += 1
            _lib.check(L.gpca_apply(frames.data_ptr(), tmp[0], tmp[1], out.data_ptr(), tp, partials, F, H, W, stream), "gpca_apply")
            self.launches += 1
        return out
