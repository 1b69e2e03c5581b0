"""Restatement of the "bf16" precision of the coordinate-head backward family (include/givepose_xyzgrad_bf16.h, gpxm_*): the head of
tests/xyz_backward_ref.py with a rounding hook `q` at the operands of the 21 contractions of its 3x3 layers.

The sites, as the device stages them (7 layers: the stride-2 transposed conv and six stride-1 convs):
    forward   Y  = conv(q(X), q(W))                     7 contractions, 14 hook calls
    dX        dX = gather(q(dY), q(W))                  7 contractions
    dW        dW = sum_b q(dY)_b cols(q(X))_b^T         7 contractions; with dX 21 hook calls a pass: dY is rounded once for both
The conv input and the weight are rounded as whole tensors before the conv: rounding commutes with the gather of a window, and a padded
0 stays 0.  Everything else -- GroupNorm + GELU and their backward, the bilinear x2, the 1x1 output conv with its dX, dW and db -- reads
unrounded values, as on the device.

With q the identity the functions below call xyz_backward_ref's own operators on their own arguments, and give its bits
(tests/test_xyz_bf16_cpu.py).  round_bf16 is tests/bb_bf16_ref.py's: round-to-nearest-even on the fp32 bit pattern by integer arithmetic.
"""
import contextlib
import functools

import torch

import xyz_backward_ref as R
from bb_bf16_ref import identity, round_bf16

OPERATORS = ("conv3x3_forward", "conv3x3_backward", "deconv_forward", "deconv_backward")


def conv3x3_forward(X, W, q=identity):
    return _PLAIN["conv3x3_forward"](q(X), q(W))


def conv3x3_backward(dY, X, W, q=identity):
    return _PLAIN["conv3x3_backward"](q(dY), q(X), q(W))


def deconv_forward(X, W, q=identity):
    return _PLAIN["deconv_forward"](q(X), q(W))


def deconv_backward(dY, X, W, q=identity):
    return _PLAIN["deconv_backward"](q(dY), q(X), q(W))


# xyz_backward_ref's operators as they are at import: the hooked forms call these, whatever the module's names point to meanwhile
_PLAIN = {k: getattr(R, k) for k in OPERATORS}


@contextlib.contextmanager
def hooked(q):
    """xyz_backward_ref.head_forward / head_backward find their 3x3 operators through the module: run them on the hooked ones."""
    mine = {"conv3x3_forward": conv3x3_forward, "conv3x3_backward": conv3x3_backward, "deconv_forward": deconv_forward,
            "deconv_backward": deconv_backward}
    for k in OPERATORS:
        setattr(R, k, functools.partial(mine[k], q=q))
    try:
        yield
    finally:
        for k in OPERATORS:
            setattr(R, k, _PLAIN[k])


def head_run(params, feat, g_coor, dtype=torch.float32, q=round_bf16):
    """xyz_backward_ref.head_run with the hook at the 3x3 layers' operands -> {"saved": flat dict, "grads": {name: numpy} + "feat"}."""
    with hooked(q):
        return R.head_run(params, feat, g_coor, dtype)


def flat(run):
    """The 31 saved tensors and the 24 gradients of a head_run in one dict."""
    return {**run["saved"], **run["grads"]}


@functools.lru_cache(maxsize=None)
def case_reference_bf16(case):
    """The CPU float32 restatement with the bf16 hook of one of xyz_backward_ref.CASES, flat.  Computed once and shared; callers must not
    modify it."""
    params, feat, g, _, _ = R.case_reference(case)
    return flat(head_run(params, feat, g))
