"""Adam / AdamW restated in numpy float32 from the contract of include/givepose_adam.h: every product, sum, quotient and square root is one
numpy float32 operation, so one correctly rounded fp32 result, in the header's order (torch.optim.adam._single_tensor_adam's,
non-capturable path).  The clip coefficient is an INPUT: tests/test_adam_gpu.py feeds it the device's own scalars[1] and asks for equal
bits; tests/test_adam_cpu.py feeds it float32 clip_grad_norm_'s and holds the restatement against torch in float64.

Also the cases both tests share: those of tests/ranger_ref.py (imported, unmodified) plus two flat tensors of exactly GPO_CHUNK and
GPO_CHUNK + 1 elements, and the four variants the tests run.
"""
import numpy as np
import torch

import ranger_ref as R

F = np.float32
CHUNK = 4096                                  # GPO_CHUNK (tests/test_adam_cpu.py checks it against the header)
EXTRA_SHAPES = {"chunk": (CHUNK,), "chunk1": (CHUNK + 1,)}
SHAPES = {**R.SHAPES, **EXTRA_SHAPES}
STEPS, CLIP, RUNS, SKIP_STEPS = R.STEPS, R.CLIP, R.RUNS, R.SKIP_STEPS
STATE_KEYS = ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")
# name -> (class name, keyword arguments): Adam wd 0, AdamW wd 1e-2 (its default), Adam wd 1e-2 (L2 on the gradient), AdamW with amsgrad
VARIANTS = {
    "adam": ("Adam", {}),
    "adamw": ("AdamW", {}),
    "adam_wd": ("Adam", {"weight_decay": 1e-2}),
    "adamw_ams": ("AdamW", {"amsgrad": True}),
}


def rule(got, ref64, ref32, what, allow=8.0, quiet=False):
    """DESIGN.md 1e's rule, per key: max|got - ref64| / max|ref64| <= allow x max(the same figure of ref32, 2^-24); where the float64
    reference is all zeros, got must be all zeros.  -> the largest ratio."""
    worst = 0.0
    for k, want in ref64.items():
        want, g, c = (np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, np.float64) for x in (want, got[k], ref32[k]))
        assert g.shape == want.shape == c.shape, (what, k, g.shape, want.shape)
        scale = np.max(np.abs(want))
        if scale == 0:
            assert not g.any(), (what, k, "the reference is an exact 0")
            continue
        dev, cpu = np.max(np.abs(g - want)) / scale, max(np.max(np.abs(c - want)) / scale, 2.0 ** -24)
        if not quiet:
            print(f"{what} {k}: got {dev:.2e}, float32 {cpu:.2e}, ratio {dev / cpu:.2f}")
        assert dev <= allow * cpu, (what, k, dev, cpu)
        worst = max(worst, dev / cpu)
    return worst


def _rng(*key):
    return np.random.Generator(np.random.Philox(key=[0xADA3, sum(k << (16 * i) for i, k in enumerate(key))]))


def case_params(run):
    """R.case_params(run) and the two chunk-sized tensors, drawn like them."""
    out = dict(R.case_params(run))
    r = _rng(1)
    for n, s in EXTRA_SHAPES.items():
        out[n] = np.zeros(s, np.float32) if run == "zero" else (0.5 * r.standard_normal(s)).astype(np.float32)
    return out


def case_grads(step):
    """R.case_grads(step) and the two chunk-sized tensors at a tenth of its scale, which keeps the norm's two regimes (far above CLIP on
    the odd steps, below it on the even ones)."""
    out = dict(R.case_grads(step))
    r = _rng(2, step)
    for n, s in EXTRA_SHAPES.items():
        out[n] = (0.1 * R.grad_scale(step) * r.standard_normal(s)).astype(np.float32)
    return out


def step_scalars(step, lr, beta1, beta2, weight_decay):
    """torch's Python-float expressions (torch/optim/adam.py, _single_tensor_adam): step_size, bias_correction2_sqrt, 1 - lr * wd."""
    step = float(step)                       # _get_value(step_t) is a float
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return lr / bias_correction1, bias_correction2 ** 0.5, 1 - lr * weight_decay


class AdamRef:
    """params: {name: float32 array} (copied).  decoupled: AdamW.  The defaults are torch.optim.Adam's; AdamW's weight_decay is 1e-2."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, decoupled=False):
        self.p = {n: np.array(a, np.float32) for n, a in params.items()}
        self.lr, self.betas, self.eps, self.wd, self.amsgrad, self.decoupled = lr, betas, eps, weight_decay, amsgrad, decoupled
        self.state = {}

    def step(self, grads, coef, lr=None):
        """grads: {name: float32 array} of the tensors that take part; coef: the clip coefficient, a float32 (1 without clipping)."""
        lr = self.lr if lr is None else lr
        b1, b2 = self.betas
        coef, beta2, omb1, omb2, eps, wd = F(coef), F(b2), F(1.0 - b1), F(1.0 - b2), F(self.eps), F(self.wd)
        for n, g in grads.items():
            assert g.dtype == np.float32
            p = self.p[n]
            st = self.state.setdefault(n, {"step": 0, "exp_avg": np.zeros_like(p), "exp_avg_sq": np.zeros_like(p), "max_exp_avg_sq": np.zeros_like(p)})
            st["step"] += 1
            size, bc2, decay = (F(x) for x in step_scalars(st["step"], lr, b1, b2, self.wd))
            m, v = st["exp_avg"], st["exp_avg_sq"]
            g = coef * g
            if wd != 0 and not self.decoupled:
                g = g + wd * p
            if wd != 0 and self.decoupled:
                p = p * decay
            m = m + omb1 * (g - m)
            v = v * beta2 + (omb2 * g) * g
            u = v
            if self.amsgrad:
                u = st["max_exp_avg_sq"] = np.maximum(st["max_exp_avg_sq"], v)
            den = np.sqrt(u) / bc2 + eps
            p = p - size * (m / den)
            assert all(a.dtype == np.float32 for a in (p, m, v, u, den))
            self.p[n], st["exp_avg"], st["exp_avg_sq"] = p, m, v

    def tensors(self, name):
        """{state key: array} of `name`: zeros before its first step, max_exp_avg_sq only under amsgrad."""
        st = self.state.get(name)
        zero = np.zeros_like(self.p[name])
        keys = STATE_KEYS[1:] if self.amsgrad else STATE_KEYS[1:3]
        return {"p": self.p[name], **{k: st[k] if st else zero for k in keys}}


def make_ref(variant, params, lr):
    cls, kw = VARIANTS[variant]
    kw = {"weight_decay": 1e-2 if cls == "AdamW" else 0.0, **kw}
    return AdamRef(params, lr=lr, decoupled=cls == "AdamW", **kw)


def make_torch(variant, params, lr, dtype):
    """torch's own optimiser (foreach=False) over {name: array} in `dtype` on the CPU.  -> (optimizer, {name: Parameter})."""
    cls, kw = VARIANTS[variant]
    ps = {n: torch.nn.Parameter(torch.from_numpy(np.array(a)).to(dtype)) for n, a in params.items()}
    return getattr(torch.optim, cls)(list(ps.values()), lr=lr, foreach=False, **kw), ps


def torch_step(opt, ps, grads, clip=CLIP):
    """The reference's loop on torch: .grad, clip_grad_norm_, step.  A tensor absent from grads has no .grad.  -> the norm (tensor)."""
    for n, p in ps.items():
        p.grad = torch.from_numpy(grads[n]).to(p.dtype).clone() if n in grads else None
    norm = torch.nn.utils.clip_grad_norm_([p for p in ps.values() if p.grad is not None], clip) if clip is not None else None
    opt.step()
    return norm


def torch_tensors(opt, ps, name, amsgrad):
    """{state key: array} of `name` in the optimiser's dtype, zeros before its first step."""
    p = ps[name]
    st = opt.state.get(p, {})
    keys = STATE_KEYS[1:] if amsgrad else STATE_KEYS[1:3]
    return {"p": p.detach().numpy().copy(), **{k: st[k].numpy().copy() if k in st else np.zeros(p.shape, p.detach().numpy().dtype) for k in keys}}
