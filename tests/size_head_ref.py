"""Restatement of the size head as the training loop runs it (SizeHead, network/pose_head.py:17-42, under network.train()) for the tests of
the gps_* family (include/givepose_sizegrad.h): nn.BatchNorm1d in train mode, F.conv1d and autograd, in float64 or float32 on the CPU.
The given mask stands in the place of F.dropout.  Also the numpy restatement of the seeded mask rule of the header, and the seeded
inputs of every test case.

Inputs.  feat holds fp16-representable values, so that one reference serves the NCHW float32, NHWC float32 and NHWC float16 entry
points; where two elements of a map tie for its maximum the first of them is moved up one fp16 step (`untie`), so that no case of
`make_case` has a tie and the choice of index is not what is measured.  Two weight scales: "sqrt" (conv weights of std 1 / sqrt(fan-in),
gamma and beta perturbed) and "init" (the reference's initialisation: conv weights of std 0.001 with zero bias, gamma 1, beta 0), where
the batch variance is of the order of eps.

The seeds of CASES were searched on the CPU (scripts/gen_golden_size_head.py --search) for inputs whose float64 reference has no y
within 1e-4 max|y| of zero: a relu gate that flips between precisions is then not what is measured.  `gate_margin` is asserted by the
tests on the CPU and on the GPU.
"""
import functools
import os
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P_DROP, BN_EPS, BN_MOMENTUM = 0.2, 1e-5, 0.1
DROP_THRESHOLD = 858993459          # floor(0.2 * 2^32)
PARAM_KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "bn1.weight", "bn1.bias")
GATE_MARGIN = 1e-4
M32 = 0xFFFFFFFF

# (B, C, HW, F), scale -> seed
CASES = {
    ((2, 64, 4, 16), "sqrt"): 1, ((2, 64, 4, 16), "init"): 1,
    ((3, 64, 64, 16), "sqrt"): 1, ((3, 64, 64, 16), "init"): 1,
    ((5, 256, 64, 32), "sqrt"): 1, ((5, 256, 64, 32), "init"): 1,
    ((65, 512, 64, 128), "sqrt"): 269, ((65, 512, 64, 128), "init"): 45,
    ((64, 1024, 64, 128), "sqrt"): 384, ((64, 1024, 64, 128), "init"): 164,
}
GOLDEN_CASES = {"b5": (5, 256, 64, 32), "b2": (2, 64, 4, 16)}
GOLDEN_SEEDS = {"b5": 1, "b2": 1}
SHAPES = [(2, 64, 4, 16), (3, 64, 64, 16), (5, 256, 64, 32), (65, 512, 64, 128), (64, 1024, 64, 128)]
SCALES = ("sqrt", "init")


# ------------------------------------------------------------------------------------------------ the seeded mask rule
def keep_mask(seed, B, F):
    """The rule of include/givepose_sizegrad.h in numpy: unit idx = b F + f is kept iff the murmur3 finaliser of
    seed_lo ^ (idx * 0x9E3779B9) ^ rotl32(seed_hi, 16) is >= floor(0.2 * 2^32).  -> (B,F) uint8."""
    seed = int(seed)
    assert 0 <= seed < 1 << 64
    lo, hi = seed & M32, seed >> 32
    rot = ((hi << 16) | (hi >> 16)) & M32
    idx = np.arange(B * F, dtype=np.uint64)
    x = ((idx * np.uint64(0x9E3779B9)) & np.uint64(M32)) ^ np.uint64(lo) ^ np.uint64(rot)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return (x >= np.uint64(DROP_THRESHOLD)).astype(np.uint8).reshape(B, F)


# ------------------------------------------------------------------------------------------------ inputs
def rng(seed):
    return np.random.Generator(np.random.Philox(key=[seed, 0x517E]))


def untie(feat):
    """feat (B,C,HW) of fp16-representable float32: where the maximum of a map is attained twice, its first occurrence moves up one
    fp16 step.  -> the number of maps changed."""
    mx = feat.max(axis=-1, keepdims=True)
    tied = (feat == mx).sum(axis=-1) > 1
    first = feat.argmax(axis=-1)
    b, c = np.nonzero(tied)
    up = np.nextafter(feat[b, c, first[b, c]].astype(np.float16), np.float16(np.inf)).astype(np.float32)
    feat[b, c, first[b, c]] = up
    return int(tied.sum())


def make_case(B, C, HW, F, scale, seed):
    """The seeded inputs of one case: feat (B,C,HW), the six parameters in the reference's shapes, keep (B,F) uint8, g_out (B,3)."""
    r = rng(seed)
    n = lambda *s: r.standard_normal(s).astype(np.float32)
    feat = n(B, C, HW).astype(np.float16).astype(np.float32)
    untie(feat)
    if scale == "sqrt":
        p = {"conv1.weight": n(F, C, 1) / np.float32(np.sqrt(C)), "conv1.bias": 0.1 * n(F), "conv2.weight": n(3, F, 1) / np.float32(np.sqrt(F)),
             "conv2.bias": 0.1 * n(3), "bn1.weight": 1 + 0.2 * n(F), "bn1.bias": 0.3 * n(F)}
    else:
        assert scale == "init"
        p = {"conv1.weight": np.float32(0.001) * n(F, C, 1), "conv1.bias": np.zeros(F, np.float32), "conv2.weight": np.float32(0.001) * n(3, F, 1),
             "conv2.bias": np.zeros(3, np.float32), "bn1.weight": np.ones(F, np.float32), "bn1.bias": np.zeros(F, np.float32)}
    keep = (r.random((B, F)) >= P_DROP).astype(np.uint8)
    return {"feat": feat, "params": {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}, "keep": keep, "g_out": n(B, 3)}


def case_crc(case):
    crc = 0
    for a in [case["feat"], case["keep"], case["g_out"]] + [case["params"][k] for k in PARAM_KEYS]:
        crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    return crc


def case(shape, scale):
    return make_case(*shape, scale, CASES[(tuple(shape), scale)])


def golden_case(name):
    return make_case(*GOLDEN_CASES[name], "sqrt", GOLDEN_SEEDS[name])


# ------------------------------------------------------------------------------------------------ the function
def reference(case, dtype, calls=1):
    """The train-mode head and its gradients by autograd in `dtype` on the CPU.  -> dict of tensors: out, pooled, arg, y, mean,
    var_unbiased, the six parameter gradients under their names, feat (d feat, (B,C,HW)), dh, and running_mean / running_var /
    num_batches_tracked after `calls` forward calls from a fresh BatchNorm1d (0 / 1 / 0)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    feat = T(case["feat"]).requires_grad_()
    P = {k: T(v).requires_grad_() for k, v in case["params"].items()}
    keep, g_out = T(case["keep"]), T(case["g_out"])
    F = keep.shape[1]
    bn = nn.BatchNorm1d(F, eps=BN_EPS, momentum=BN_MOMENTUM).to(dtype).train()
    with torch.no_grad():
        bn.weight.copy_(P["bn1.weight"]), bn.bias.copy_(P["bn1.bias"])
    for _ in range(calls):
        for t in [feat, bn.weight, bn.bias, *P.values()]:
            t.grad = None
        pooled, arg = feat.max(dim=-1, keepdim=True)
        h = Fn.conv1d(pooled, P["conv1.weight"], P["conv1.bias"])
        h.retain_grad()
        y = bn(h)
        d = Fn.relu(y) * keep[:, :, None] / (1 - P_DROP)
        out = Fn.conv1d(d, P["conv2.weight"], P["conv2.bias"]).squeeze(2)
        out.backward(g_out)
    hh = h.detach().squeeze(2)
    res = {"out": out.detach(), "pooled": pooled.detach().squeeze(2), "arg": arg.squeeze(2), "y": y.detach().squeeze(2), "mean": hh.mean(0),
           "var_unbiased": hh.var(0, unbiased=True), "feat": feat.grad, "dh": h.grad.squeeze(2),
           "running_mean": bn.running_mean.detach().clone(), "running_var": bn.running_var.detach().clone(),
           "num_batches_tracked": bn.num_batches_tracked.clone()}
    for k in PARAM_KEYS:
        res[k] = (bn.weight.grad if k == "bn1.weight" else bn.bias.grad if k == "bn1.bias" else P[k].grad).detach()
    return res


@functools.lru_cache(maxsize=None)
def cached_reference(shape, scale):
    """(case, float64 reference, float32 reference) of a case of CASES; computed once and shared: treat as read-only."""
    c = case(shape, scale)
    return c, reference(c, torch.float64), reference(c, torch.float32)


def gate_margin(ref64):
    """min|y| / max|y| of the float64 reference: the tests want it above GATE_MARGIN."""
    y = ref64["y"].abs()
    return float(y.min() / y.max())


def has_ties(feat):
    mx = feat.max(axis=-1, keepdims=True)
    return bool(((feat == mx).sum(axis=-1) > 1).any())
