"""Clip + Ranger restated in plain torch ops from the formulas of include/givepose_optim.h, generic in dtype and device: in float64 the
reference of tests/test_optim_cpu.py and tests/test_optim_gpu.py, in float32 on the CPU their yardstick, in float32 on the GPU the timing
baseline of scripts/optim_step_time.py.  Also the seeded cases the tests and scripts/gen_golden_ranger.py share.

Per step, over the tensors that have a gradient (a tensor without one is skipped and its step count stays):
    norm = sqrt(sum over tensors of sum g^2),   coef = min(1, max_norm / (norm + 1e-6))       (1 without clipping)
    g' = coef g, minus its mean over all dims but the first where the tensor is centralised (ndim > 1, or > 3 with gc_conv_only)
    v = beta2 v + (1 - beta2) g' g';   m = beta1 m + (1 - beta1) g'
    t = the tensor's step;  N_max = 2 / (1 - beta2) - 1;  N = N_max - 2 t beta2^t / (1 - beta2^t)
    rectified (N > threshold):  G = m / (sqrt(v) + eps),  size = sqrt((1 - beta2^t) (N - 4) / (N_max - 4) (N - 2) / N N_max / (N_max - 2)) / (1 - beta1^t)
    else:                       G = m,                     size = 1 / (1 - beta1^t)
    G += weight_decay p (and m = G on an unrectified step, as ranger2020.py:225-228 adds the decay to exp_avg in place);   p -= size lr G;   every k-th step of the tensor:  slow += alpha (p - slow),  p = slow
"""
import math
import zlib

import numpy as np
import torch

STATE_KEYS = ("p", "exp_avg", "exp_avg_sq", "slow_buffer")


class RangerRef:
    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0, use_gc=True,
                 gc_conv_only=False):
        """params: {name: tensor}; the tensors are cloned, their dtype and device are the arithmetic's."""
        self.p = {n: t.clone() for n, t in params.items()}
        self.lr, self.alpha, self.k, self.threshold, self.betas, self.eps, self.wd = lr, alpha, k, N_sma_threshhold, betas, eps, weight_decay
        self.use_gc, self.gc_conv_only = use_gc, gc_conv_only
        self.state = {}
        self.norm = self.coef = None

    def centralised(self, t):
        return self.use_gc and t.dim() > (3 if self.gc_conv_only else 1)

    def step(self, grads, clip_norm=None, lr=None):
        """grads: {name: tensor} for the tensors that take part.  Sets self.norm and self.coef (tensors; coef is None without clipping)."""
        lr = self.lr if lr is None else lr
        b1, b2 = self.betas
        # the 2-norm of all gradients as the 2-norm of the tensors' 2-norms (the same number; this grouping is clip_grad_norm_'s)
        self.norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads.values()]))
        self.coef = None if clip_norm is None else torch.clamp(clip_norm / (self.norm + 1e-6), max=1.0)
        for n, g in grads.items():
            p = self.p[n]
            st = self.state.setdefault(n, {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p), "slow_buffer": p.clone()})
            g = g if self.coef is None else g * self.coef
            if self.centralised(g):
                g = g - g.mean(dim=tuple(range(1, g.dim())), keepdim=True)
            st["step"] += 1
            t = st["step"]
            st["exp_avg_sq"] = b2 * st["exp_avg_sq"] + (1 - b2) * g * g
            st["exp_avg"] = b1 * st["exp_avg"] + (1 - b1) * g
            b2t = b2 ** t
            n_max = 2 / (1 - b2) - 1
            n_sma = n_max - 2 * t * b2t / (1 - b2t)
            if n_sma > self.threshold:
                size = math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - b1 ** t)
                G = st["exp_avg"] / (st["exp_avg_sq"].sqrt() + self.eps)
            else:
                size = 1.0 / (1 - b1 ** t)
                G = st["exp_avg"]
            if self.wd != 0:
                G = G + self.wd * p
                if not n_sma > self.threshold:       # the reference's G is exp_avg itself here and the decay is added in place: it stays in m
                    st["exp_avg"] = G
            p = p - (size * lr) * G
            if t % self.k == 0:
                st["slow_buffer"] = st["slow_buffer"] + self.alpha * (p - st["slow_buffer"])
                p = st["slow_buffer"].clone()
            self.p[n] = p

    def tensors(self, name):
        """{state key: tensor} of `name` (exp_avg, exp_avg_sq and slow_buffer are None before its first step)."""
        st = self.state.get(name, {})
        return {"p": self.p[name], **{k: st.get(k) for k in STATE_KEYS[1:]}}


# ------------------------------------------------------------------------------------------------ the seeded cases
STEPS = 13
CLIP = 5.0
SHAPES = {
    "w51": (5, 1),            # row length 1: centralised to an exact 0
    "b7": (7,), "b1": (1,),   # 1-D: not centralised
    "conv": (6, 3, 3, 3),
    "dw": (64, 1, 7, 7),      # depth-wise weight: rows of 49
    "odd": (3, 1031),         # odd row length across 16-byte boundaries
    "long": (2, 4099),        # a row longer than a chunk: two segments
    "rows": (130, 3, 4, 4),   # more rows than a workgroup has waves
    "skip": (4, 6),           # no gradient on steps 3 and 9
}
SKIP_STEPS = {"skip": (3, 9)}
VARIANTS = {
    "gc": {},
    "nogc": {"use_gc": False},
    "convonly": {"gc_conv_only": True},
    "wd": {"weight_decay": 0.01, "betas": (0.9, 0.99), "k": 5, "alpha": 0.6, "eps": 1e-6},
}
RUNS = {"seeded": 1e-3, "zero": 0.1}         # run -> lr: seeded parameters, or parameters 0 (p is then the accumulated update itself)
GOLDEN = [("gc", "seeded"), ("gc", "zero"), ("nogc", "seeded"), ("convonly", "seeded"), ("wd", "seeded")]
SAMPLES = 8                                  # elements per tensor the golden files keep (next to each tensor's sum and sum of |.|)


def _rng(*key):
    return np.random.Generator(np.random.Philox(key=[0x52A6, sum(k << (16 * i) for i, k in enumerate(key))]))


def case_params(run):
    """{name: float32 array}: seeded normals of scale 0.5 ("seeded") or zeros ("zero")."""
    if run == "zero":
        return {n: np.zeros(s, np.float32) for n, s in SHAPES.items()}
    r = _rng(1)
    return {n: (0.5 * r.standard_normal(s)).astype(np.float32) for n, s in SHAPES.items()}


def grad_scale(step):
    """Odd steps: scale 1, total norm near 145, far above CLIP; even steps: scale 0.01, norm near 1.5, coefficient exactly 1."""
    return 1.0 if step % 2 else 0.01


def case_grads(step):
    """{name: float32 array} of step 1 .. STEPS; a tensor is absent on its SKIP_STEPS."""
    r = _rng(2, step)
    out = {}
    for n, s in SHAPES.items():
        g = (grad_scale(step) * r.standard_normal(s)).astype(np.float32)       # drawn for every tensor, so that a skip shifts no stream
        if step not in SKIP_STEPS.get(n, ()):
            out[n] = g
    return out


def sample_index():
    """{name: SAMPLES flat indices}: the first and the last element and seeded ones in between (all elements of a smaller tensor)."""
    r = _rng(3)
    out = {}
    for n, s in SHAPES.items():
        size = int(np.prod(s))
        if size <= SAMPLES:
            out[n] = np.arange(size)
        else:
            out[n] = np.sort(np.concatenate([[0, size - 1], 1 + r.choice(size - 2, SAMPLES - 2, replace=False)]))
    return out


def input_crc(run):
    c = 0
    for arrs in [case_params(run)] + [case_grads(s) for s in range(1, STEPS + 1)]:
        for n in sorted(arrs):
            c = zlib.crc32(arrs[n].tobytes(), c)
    return c


def run_case(variant, run, dtype, device="cpu", steps=STEPS, on_step=None):
    """The case with RangerRef in `dtype`; on_step(step, ref) is called after every step.  -> the RangerRef."""
    T = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)
    ref = RangerRef({n: T(a) for n, a in case_params(run).items()}, lr=RUNS[run], **VARIANTS[variant])
    for step in range(1, steps + 1):
        ref.step({n: T(g) for n, g in case_grads(step).items()}, clip_norm=CLIP)
        if on_step:
            on_step(step, ref)
    return ref


def summarise(tensors_of):
    """tensors_of(name) -> {state key: tensor}.  -> {key: (samples concatenated over the tensors, per-tensor sums, per-tensor sums of |.|)} in float64."""
    idx = sample_index()
    out = {}
    for key in STATE_KEYS:
        samples, sums, sabs = [], [], []
        for n in SHAPES:
            t = tensors_of(n)[key].detach().double().cpu().reshape(-1).numpy()
            samples.append(t[idx[n]])
            sums.append(t.sum())
            sabs.append(np.abs(t).sum())
        out[key] = (np.concatenate(samples), np.array(sums), np.array(sabs))
    return out
