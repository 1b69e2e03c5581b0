"""The accumulated gradient of the reference's loop (engine/train.py:117-131) restated in plain torch ops from the formulas of
include/givepose_accum.h, generic in dtype: in float64 the reference of tests/test_grad_accum_cpu.py and tests/test_grad_accum_gpu.py,
in float32 on the CPU their yardstick.

The loop, with A = FLAGS.accumulate and global_step counting micro-steps from 0:
    loss = loss / A;  loss.backward()                      acc += g / A        (a parameter's first gradient since zero_grad: acc = g / A;
                                                                                a parameter the loss does not reach keeps its acc)
    clip_grad_norm_(parameters, clip)                      norm = sqrt(sum over the parameters that HAVE a .grad of sum acc^2)
                                                           acc *= min(1, clip / (norm + 1e-6))            in place, on every micro-step
    if global_step % A == 0:  optimizer.step();  optimizer.zero_grad()          (.grad = None: no parameter has an acc)
With several ranks the gradient of a micro-step is the mean of the ranks' gradients (DDP).
"""
import torch

from ranger_ref import RangerRef


class AccumRef:
    def __init__(self):
        self.acc = {}                       # {name: accumulated gradient} of the live parameters
        self.norm = self.coef = None

    def add(self, grads, scale=1.0, clip_norm=None, world_grads=None):
        """grads: {name: tensor}; world_grads: the ranks' dicts instead (grads is then ignored): their mean is added.
        Sets self.norm and self.coef (tensors; coef is None without clipping)."""
        if world_grads is not None:
            grads = {n: sum(w[n] for w in world_grads) / len(world_grads) for n in world_grads[0]}
        for n, g in grads.items():
            self.acc[n] = scale * g if n not in self.acc else self.acc[n] + scale * g
        # the grouping of clip_grad_norm_: the 2-norm of the tensors' 2-norms
        self.norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(a) for a in self.acc.values()]))
        self.coef = None if clip_norm is None else torch.clamp(clip_norm / (self.norm + 1e-6), max=1.0)
        if self.coef is not None:
            for n in self.acc:
                self.acc[n] = self.acc[n] * self.coef

    def zero(self):
        self.acc = {}


def loop_ref(params, grads_per_micro_step, accumulate, clip, lr, dtype, optimizer=None, on_micro_step=None):
    """The loop over grads_per_micro_step: a list whose entry i is {name: array or tensor} (one rank) or a list of such dicts (the
    ranks' gradients of micro-step i).  params: {name: array or tensor}.  optimizer(params) -> an object with .p and
    .step(grads, lr=) (default: RangerRef with the project's defaults).  on_micro_step(i, acc, opt, stepped) is called after every
    micro-step, before the accumulator is zeroed.  -> (the optimiser, the AccumRef)."""
    T = lambda a: torch.as_tensor(a).to(dtype)
    opt = (optimizer or (lambda p: RangerRef(p, lr=lr)))({n: T(a) for n, a in params.items()})
    acc = AccumRef()
    for i, g in enumerate(grads_per_micro_step):
        if isinstance(g, dict):
            acc.add({n: T(a) for n, a in g.items()}, 1.0 / accumulate, clip)
        else:
            acc.add(None, 1.0 / accumulate, clip, world_grads=[{n: T(a) for n, a in w.items()} for w in g])
        stepped = i % accumulate == 0
        if stepped:
            opt.step(dict(acc.acc), lr=lr)
        if on_micro_step:
            on_micro_step(i, acc, opt, stepped)
        if stepped:
            acc.zero()
    return opt, acc
