"""The optimiser family (include/givepose_optim.h, gpo_*): what the reference's training loop does after backward()
(engine/train.py:117-129) -- clip_grad_norm_(parameters, max_norm), a step of Ranger (tools/torch_utils/solver/ranger2020.py: RAdam +
Lookahead + gradient centralisation, built by tools/training_utils.py:build_optimizer) and the flat_and_anneal schedule
(tools/torch_utils/solver/lr_scheduler.py:177-263).

The step runs on the device in this library's HIP kernels, in _lib.GPO_STEP_LAUNCHES launches whatever the number of tensors; there is
no CPU path.  The host computes the per-tensor step scalars (N_sma, step_size) in Python floats exactly as ranger2020.py:192-214 does and
writes them, with the pointers, into a host table that the entry point sends to the device with one asynchronous copy.  Nothing comes back
to the host.

Gradients arrive as `param_grads`, {state_dict name: fp32 device tensor in the parameter's shape}: what PoseNet.head_grads_backbone
returns.  A parameter registered under two names (ConvModule's .gn / .norm) is one parameter and is updated once.

`Adam` and `AdamW` (include/givepose_adam.h, gpad_*) are the loop's other two FLAGS.optimizer_type choices (engine/train.py:66-72):
torch.optim.Adam / AdamW with the same interface as `Ranger`, in _lib.GPAD_STEP_LAUNCHES launches, their state dicts in torch's layout;
`build_optimizer` restates the loop's choice between the three.

`flat_and_anneal_lr` is host arithmetic: the factor on the base rate at iteration `it`.

`GradAccumulator` (include/givepose_accum.h, gpc_*) is the loop's `.grad` when FLAGS.accumulate > 1 or more than one rank trains: one flat
buffer in the layout of the optimiser's state, into which every micro-step's gradients are added and clipped in place in
_lib.GPC_ACCUM_LAUNCHES launches, and which one all_reduce exchanges between ranks.  `rank_accum_selfcheck` is the rank worker of its
multi-process tests.
"""
import ctypes
import math
from bisect import bisect_right

import numpy as np
import torch

from . import _lib
from .pnp_grad import _default_alloc, _stream

# gpo_tensor as a numpy record (checked against ctypes.sizeof(_lib.OptTensor) at the first table)
_TENSOR = np.dtype([("p", "u8"), ("g", "u8"), ("m", "u8"), ("v", "u8"), ("slow", "u8"), ("n", "i8"), ("rows", "i4"), ("row_len", "i4"),
                    ("flags", "i4"), ("step_lr", "f4")])
_STATE_KEYS = ("exp_avg", "exp_avg_sq", "slow_buffer")
# gpad_tensor (include/givepose_adam.h), checked against ctypes.sizeof(_lib.AdamTensor) in the same way
_ADAM_TENSOR = np.dtype([("p", "u8"), ("g", "u8"), ("m", "u8"), ("v", "u8"), ("vmax", "u8"), ("n", "i8"), ("step_size", "f4"), ("bc2_sqrt", "f4"),
                         ("decay", "f4"), ("pad", "i4")])
_ADAM_STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _describe(t):
    if not torch.is_tensor(t):
        return type(t).__name__
    return f"{tuple(t.shape)} {t.dtype} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}"


def _check_grad(name, g, dev, shape=None):
    if (not torch.is_tensor(g) or g.device != dev or g.dtype != torch.float32 or not g.is_contiguous()
            or (shape is not None and tuple(g.shape) != tuple(shape))):
        want = f" {tuple(shape)}" if shape is not None else ""
        raise ValueError(f"param_grads[{name!r}]: {_describe(g)}, expected contiguous float32{want} on {dev}")
    return g


def _table_ptr(tab):
    assert tab.dtype == _TENSOR and tab.flags.c_contiguous and _TENSOR.itemsize == ctypes.sizeof(_lib.OptTensor)
    return tab.ctypes.data_as(ctypes.POINTER(_lib.OptTensor))


def _adam_table_ptr(tab):
    assert tab.dtype == _ADAM_TENSOR and tab.flags.c_contiguous and _ADAM_TENSOR.itemsize == ctypes.sizeof(_lib.AdamTensor)
    return tab.ctypes.data_as(ctypes.POINTER(_lib.AdamTensor))


def _gc_rows(shape, use_gc, gc_conv_only):
    """(rows, row_len) of gradient centralisation for a tensor of `shape`, (0, 0) if it is not centralised: a row is one index of dim 0."""
    if not use_gc or len(shape) <= (3 if gc_conv_only else 1):
        return 0, 0
    n = 1
    for d in shape[1:]:
        n *= int(d)
    return int(shape[0]), n


def radam_step_size(step, beta1, beta2, n_sma_threshold):
    """-> (rectified, step_size) of RAdam at `step`, in Python floats as ranger2020.py:192-214 computes them."""
    beta2_t = beta2 ** step
    n_sma_max = 2 / (1 - beta2) - 1
    n_sma = n_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma > n_sma_threshold:
        return True, math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma * n_sma_max / (n_sma_max - 2)) / (1 - beta1 ** step)
    return False, 1.0 / (1 - beta1 ** step)


def _workspace(owner, nbytes):
    """owner._ws grown to nbytes through owner._alloc("workspace", .): the workspace of the optimisers and of the accumulator."""
    if owner._ws is None or owner._ws.numel() * 4 < nbytes:
        owner._ws = owner._alloc("workspace", (max(int(nbytes) // 4, 64),))
        assert owner._ws.data_ptr() % 256 == 0, "workspace buffers must be 256-byte aligned"
    return owner._ws


def _launch(entry, device, workspace, scalars, ptr, n, query_args, args):
    """One call of the entry point `entry` over the table (ptr, n): `entry`_workspace(ptr, n, *query_args) sizes the workspace, a table it
    refuses is an error under its name, workspace(nbytes) supplies the buffer and the launch runs under `device`.  scalars: the two
    device scalars, or a function that allocates them once the workspace exists.  -> scalars"""
    L = _lib.load()
    nbytes = getattr(L, entry + "_workspace")(ptr, n, *query_args)
    if nbytes <= 0:
        _lib.check(-1, entry + "_workspace")
    ws = workspace(nbytes)
    if callable(scalars):
        scalars = scalars()
    with torch.cuda.device(device):
        _lib.check(getattr(L, entry)(ptr, n, *args, scalars.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream(device)), entry)
    return scalars


class _FlatOptimizer:
    """What the optimisers of this module share: the distinct parameters of a model in model.parameters() order with every name they are
    registered under, flat fp32 state buffers in which every tensor starts at a multiple of 64 elements, the loading of a state dict,
    the check of a step's gradients and the step's skeleton.  A subclass supplies _who, _entry (its entry point, whose size query is
    `_entry`_workspace), _query_takes_hyper, _ptr (the table's pointer cast), _state_keys, and the methods _take_group, _step_scalars
    and _fill, with _check_group and _before_step where it has something to check or to prepare."""

    _require_device = True       # the table and the state-dict layout need no device: tests/test_optim_cpu.py builds them on the host
    _who = "optimizer"

    def _discover(self, model, alloc):
        """Sets model, params, param_names, _index, device, steps, _offsets and _alloc."""
        who = self._who
        self.model = model
        self.params, self.param_names, self._index = [], [], {}
        by_ptr = {}
        for name, p in model.named_parameters(remove_duplicate=False):
            if (self._require_device and p.device.type != "cuda") or p.dtype != torch.float32 or not p.is_contiguous() or p.numel() < 1:
                raise ValueError(f"{who}: parameter {name}: {_describe(p)}, expected a non-empty contiguous float32 tensor on a HIP device "
                                 "(move the model to the device first)")
            i = by_ptr.get(p.data_ptr())
            if i is None:
                i = by_ptr[p.data_ptr()] = len(self.params)
                self.params.append(p)
                self.param_names.append(name)
            elif tuple(self.params[i].shape) != tuple(p.shape):
                raise ValueError(f"{who}: {name} and {self.param_names[i]} share storage but not a shape")
            self._index[name] = i
        if not self.params:
            raise ValueError(f"{who}: the model has no parameters")
        if [id(p) for p in model.parameters()] != [id(p) for p in self.params]:
            raise ValueError(f"{who}: distinct Parameter objects of the model share storage")
        self.device = self.params[0].device
        if any(p.device != self.device for p in self.params):
            raise ValueError(f"{who}: the parameters lie on more than one device")
        self.steps = [0] * len(self.params)
        sizes = np.array([p.numel() for p in self.params], np.int64)
        self._offsets = np.concatenate([[0], np.cumsum((sizes + 63) // 64 * 64)])
        self._alloc = alloc or _default_alloc(self.device)
        self._ws = None
        return sizes

    def _view(self, key, i):
        o = int(self._offsets[i])
        return self._flat[key][o:o + self.params[i].numel()].view(self.params[i].shape)

    def _collect(self, param_grads):
        """{parameter index: gradient} of the names in param_grads, aliases merged."""
        grads = {}
        for name, g in param_grads.items():
            i = self._index.get(name)
            if i is None:
                raise ValueError(f"param_grads[{name!r}]: the model has no parameter of that name")
            _check_grad(name, g, self.device, self.params[i].shape)
            seen = grads.get(i)
            if seen is not None and seen[1].data_ptr() != g.data_ptr() and not torch.equal(seen[1], g):
                raise ValueError(f"param_grads[{name!r}] and param_grads[{seen[0]!r}] name one parameter but carry different gradients")
            if seen is None:
                grads[i] = (name, g)
        return grads

    def _make_state(self, sizes, dtype, fields):
        """The flat state buffers (_state_keys, the table's `fields`), the scalars and the table columns that no step changes."""
        total = int(self._offsets[-1])
        self._flat = {key: self._alloc(key, (total,)).zero_() for key in self._state_keys}
        self.scalars = self._alloc("scalars", (2,)).zero_()
        st = np.zeros(len(self.params), dtype)
        st["p"] = [p.data_ptr() for p in self.params]
        for key, field in zip(self._state_keys, fields):
            st[field] = self._flat[key].data_ptr() + 4 * self._offsets[:-1]
        st["n"] = sizes
        self._static = st
        self._scalar_cache = {}

    # ------------------------------------------------------------------ state
    def _check_group(self, g, who):
        pass

    def load_state_dict(self, sd):
        who = f"{self._who}.load_state_dict"
        groups = sd["param_groups"]
        if len(groups) != 1 or list(groups[0]["params"]) != list(range(len(self.params))):
            raise ValueError(f"{who}: one parameter group over {len(self.params)} parameters is expected")
        g = groups[0]
        if "param_names" in g and list(g["param_names"]) != self.param_names:
            bad = [(a, b) for a, b in zip(g["param_names"], self.param_names) if a != b][:3]
            raise ValueError(f"{who}: the parameter names differ, first {bad}")
        self._check_group(g, who)
        for i, s in sd["state"].items():
            if not 0 <= int(i) < len(self.params):
                raise ValueError(f"{who}: state index {i} out of range")
            for key in self._state_keys:
                if key not in s or tuple(s[key].shape) != tuple(self.params[int(i)].shape):
                    raise ValueError(f"{who}: state[{i}][{key}] {tuple(s[key].shape) if key in s else 'is missing'}, expected {tuple(self.params[int(i)].shape)}")
        self._take_group(g)
        self._scalar_cache = {}
        for key in self._state_keys:
            self._flat[key].zero_()
        self.steps = [0] * len(self.params)
        for i, s in sd["state"].items():
            self.steps[int(i)] = int(float(s["step"]))          # a number, or torch's 0-d tensor (torch >= 1.12)
            for key in self._state_keys:
                self._view(key, int(i)).copy_(s[key])

    # ------------------------------------------------------------------ the step
    def _scalars_of(self, step, lr):
        key = (step, lr)
        hit = self._scalar_cache.get(key)
        if hit is None:
            if len(self._scalar_cache) > 64:
                self._scalar_cache.clear()
            hit = self._scalar_cache[key] = self._step_scalars(step, lr)
        return hit

    def _before_step(self, active):
        pass

    @torch.no_grad()
    def step(self, param_grads, clip_norm=None, lr=None):
        """One step over the parameters that have an entry in param_grads; a parameter without one is skipped and its step count does
        not advance (p.grad is None in the reference and in torch).  clip_norm: clip_grad_norm_'s max_norm over these gradients, applied
        inside the update (the gradients themselves are not scaled).  lr: this call's learning rate (default: the optimiser's).  The
        step counts advance after the launch, so a refused step leaves them alone."""
        lr = self.lr if lr is None else float(lr)
        if clip_norm is not None and not float(clip_norm) > 0:
            raise ValueError(f"{self._who}.step: clip_norm {clip_norm} must be positive (or None)")
        grads = self._collect(param_grads)
        if not grads:
            return
        active = sorted(grads)
        self._before_step(active)
        tab = self._static[active]
        tab["p"] = [self.params[i].data_ptr() for i in active]
        tab["g"] = [grads[i][1].data_ptr() for i in active]
        hyper = self._fill(tab, [self._scalars_of(self.steps[i] + 1, lr) for i in active], float(clip_norm) if clip_norm is not None else 0.0)
        h = ctypes.byref(hyper)
        _launch(self._entry, self.device, lambda nbytes: _workspace(self, nbytes), self.scalars, self._ptr(tab), len(active),
                (h,) if self._query_takes_hyper else (), (h,))
        for i in active:
            self.steps[i] += 1
        if hasattr(self.model, "params_updated"):
            self.model.params_updated()


class Ranger(_FlatOptimizer):
    """Ranger over the distinct parameters of `model`, stepped on the device by gpo_ranger_step.

    model: a module on a HIP device whose parameters are fp32 and contiguous.  The optimiser owns three flat fp32 device buffers
    (exp_avg, exp_avg_sq, slow_buffer; every tensor starts at a multiple of 64 elements) and updates the parameters in place through
    their pointers; a step ends with model.params_updated() if the model has one.
    alloc(name, shape): optional hook that supplies the state buffers, the two device scalars and the workspace (default torch.empty).
    `scalars` holds the gradients' total 2-norm and the clip coefficient of the last step, on the device."""

    _who, _entry, _query_takes_hyper = "Ranger", "gpo_ranger_step", False
    _ptr = staticmethod(_table_ptr)
    _state_keys = _STATE_KEYS

    def __init__(self, model, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0, use_gc=True,
                 gc_conv_only=False, gc_loc=True, alloc=None):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if not 1 <= k:
            raise ValueError(f"Invalid lookahead steps: {k}")
        if not lr > 0:
            raise ValueError(f"Invalid Learning Rate: {lr}")
        if not eps > 0:
            raise ValueError(f"Invalid eps: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid betas: {betas}")
        if not gc_loc:
            raise NotImplementedError("Ranger: gc_loc=False -- centralising the generalised gradient (after the division by sqrt(v)) is not "
                                      "built; only gc_loc=True, centralising the gradient itself, is")
        self.lr, self.alpha, self.k, self.N_sma_threshhold = float(lr), float(alpha), int(k), N_sma_threshhold
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.use_gc, self.gc_conv_only, self.gc_loc = bool(use_gc), bool(gc_conv_only), True
        self._make_state(self._discover(model, alloc), _TENSOR, ("m", "v", "slow"))
        rows = [_gc_rows(p.shape, self.use_gc, self.gc_conv_only) for p in self.params]
        self._static["rows"], self._static["row_len"] = [r[0] for r in rows], [r[1] for r in rows]

    # ------------------------------------------------------------------ state
    def state_dict(self):
        """torch.optim.Optimizer's layout: state[i] for every parameter that has been stepped, i the index in model.parameters() order;
        param_groups[0]["param_names"] names each index (the first of a shared parameter's names)."""
        state = {i: {"step": s, **{key: self._view(key, i).clone() for key in _STATE_KEYS}} for i, s in enumerate(self.steps) if s > 0}
        group = {"lr": self.lr, "alpha": self.alpha, "k": self.k, "step_counter": 0, "betas": self.betas, "N_sma_threshhold": self.N_sma_threshhold,
                 "eps": self.eps, "weight_decay": self.weight_decay, "params": list(range(len(self.params))), "param_names": list(self.param_names)}
        return {"state": state, "param_groups": [group]}

    def _take_group(self, g):
        self.lr, self.alpha, self.k = float(g["lr"]), float(g["alpha"]), int(g["k"])
        self.betas, self.eps, self.weight_decay = (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"]), float(g["weight_decay"])
        self.N_sma_threshhold = g["N_sma_threshhold"]

    # ------------------------------------------------------------------ the step
    def _step_scalars(self, step, lr):
        rect, size = radam_step_size(step, self.betas[0], self.betas[1], self.N_sma_threshhold)
        return (_lib.GPO_FLAG_RECTIFIED if rect else 0) | (_lib.GPO_FLAG_LOOKAHEAD if step % self.k == 0 else 0), size * lr

    def _before_step(self, active):
        first = [i for i in active if self.steps[i] == 0]
        if first:        # the reference creates a parameter's state at its first step: slow_buffer starts as a copy of the parameter
            dst, src = [self._view("slow_buffer", i) for i in first], [self.params[i].detach() for i in first]
            if hasattr(torch, "_foreach_copy_"):
                torch._foreach_copy_(dst, src)
            else:
                for d, s in zip(dst, src):
                    d.copy_(s)

    def _fill(self, tab, sc, max_norm):
        tab["flags"], tab["step_lr"] = [s[0] for s in sc], [s[1] for s in sc]
        return _lib.OptHyper(self.betas[0], self.betas[1], self.eps, self.alpha, self.weight_decay, max_norm)


def adam_step_scalars(step, lr, beta1, beta2, weight_decay):
    """-> (step_size, bias_correction2_sqrt, 1 - lr * weight_decay) of Adam / AdamW at `step`, in Python floats as
    torch.optim.adam._single_tensor_adam computes them; the device takes each rounded to fp32."""
    return lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5, 1 - lr * weight_decay


class Adam(_FlatOptimizer):
    """torch.optim.Adam over the distinct parameters of `model`, stepped on the device by gpad_adam_step (include/givepose_adam.h): the
    `else` branch of the reference's FLAGS.optimizer_type (engine/train.py:66-72).  The arguments and defaults are torch's.

    model: a module on a HIP device whose parameters are fp32 and contiguous.  The optimiser owns the flat fp32 device buffers exp_avg
    and exp_avg_sq (and max_exp_avg_sq under amsgrad; every tensor starts at a multiple of 64 elements) and updates the parameters in
    place through their pointers; a step ends with model.params_updated() if the model has one.
    alloc(name, shape): optional hook that supplies the state buffers, the two device scalars and the workspace (default torch.empty).
    `scalars` holds the gradients' total 2-norm and the clip coefficient of the last step, on the device.
    maximize, capturable, differentiable and fused are torch's keywords for paths that are not built: they must be false or None;
    foreach is accepted and has no meaning here (one launch serves all tensors)."""

    _who, _entry, _query_takes_hyper = "Adam", "gpad_adam_step", True
    _ptr = staticmethod(_adam_table_ptr)
    _decoupled = False
    _default_weight_decay = 0

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=None, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, alloc=None):
        who = self._who
        weight_decay = self._default_weight_decay if weight_decay is None else weight_decay
        if torch.is_tensor(lr) or torch.is_tensor(betas[0]) or torch.is_tensor(betas[1]):
            raise NotImplementedError(f"{who}: a tensor lr or beta is not built; pass Python floats")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        for key, value in (("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable), ("fused", fused)):
            if value:
                raise NotImplementedError(f"{who}: {key}={value!r} is not built; only the plain step is (leave {key} at its default)")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.amsgrad = float(weight_decay), bool(amsgrad)
        self._state_keys = _ADAM_STATE_KEYS if self.amsgrad else _ADAM_STATE_KEYS[:2]
        self._make_state(self._discover(model, alloc), _ADAM_TENSOR, ("m", "v", "vmax"))

    # ------------------------------------------------------------------ state
    def _group(self):
        return {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": self.amsgrad,
                "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                "decoupled_weight_decay": self._decoupled}

    def state_dict(self):
        """The layout of torch.optim.Adam / AdamW (what the reference's last_optimizer.pth holds, engine/train.py:74-77, 159), so that a
        dict saved here loads into torch's class and one saved by torch's loads here: state[i] = {"step": 0-d float32 tensor, "exp_avg",
        "exp_avg_sq"[, "max_exp_avg_sq"]} for every parameter that has been stepped, i the index in model.parameters() order; one
        param group with torch's keys, and "param_names" naming each index (the first of a shared parameter's names)."""
        state = {i: {"step": torch.tensor(float(s), dtype=torch.float32), **{key: self._view(key, i).clone() for key in self._state_keys}}
                 for i, s in enumerate(self.steps) if s > 0}
        return {"state": state, "param_groups": [{**self._group(), "params": list(range(len(self.params))), "param_names": list(self.param_names)}]}

    def _check_group(self, g, who):
        for key in ("maximize", "capturable", "differentiable", "fused"):
            if g.get(key):
                raise NotImplementedError(f"{who}: the saved group has {key}={g[key]!r}, which is not built")
        if bool(g.get("amsgrad", False)) != self.amsgrad:
            raise ValueError(f"{who}: the saved group has amsgrad={g.get('amsgrad', False)}, this optimiser was built with amsgrad={self.amsgrad}")
        if "decoupled_weight_decay" in g and bool(g["decoupled_weight_decay"]) != self._decoupled:
            raise ValueError(f"{who}: the saved group has decoupled_weight_decay={g['decoupled_weight_decay']} "
                             f"({'AdamW' if g['decoupled_weight_decay'] else 'Adam'}), this optimiser is {self._who}")

    def _take_group(self, g):
        self.lr, self.betas = float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1]))
        self.eps, self.weight_decay = float(g["eps"]), float(g["weight_decay"])

    # ------------------------------------------------------------------ the step
    def _step_scalars(self, step, lr):
        return adam_step_scalars(step, lr, self.betas[0], self.betas[1], self.weight_decay)

    def _fill(self, tab, sc, max_norm):
        tab["step_size"], tab["bc2_sqrt"], tab["decay"] = [s[0] for s in sc], [s[1] for s in sc], [s[2] for s in sc]
        return _lib.AdamHyper(self.betas[0], self.betas[1], self.eps, self.weight_decay, max_norm,
                              _lib.GPAD_MODE_ADAMW if self._decoupled else _lib.GPAD_MODE_ADAM, int(self.amsgrad))


class AdamW(Adam):
    """torch.optim.AdamW (decoupled weight decay, default 1e-2): the 'AdamW' branch of the reference's FLAGS.optimizer_type.  See Adam."""

    _who = "AdamW"
    _decoupled = True
    _default_weight_decay = 1e-2


def build_optimizer(model, optimizer_type, lr):
    """The reference's choice of optimiser (engine/train.py:66-72, FLAGS.optimizer_type, FLAGS.lr): 'Ranger' -> Ranger(model, lr=lr),
    'AdamW' -> AdamW(model, lr=lr), anything else -> Adam(model) at torch's default rate, as the reference builds it."""
    if optimizer_type == "Ranger":
        return Ranger(model, lr=lr)
    if optimizer_type == "AdamW":
        return AdamW(model, lr=lr)
    return Adam(model)


@torch.no_grad()
def clip_grad_norm_(param_grads, max_norm, alloc=None):
    """torch.nn.utils.clip_grad_norm_(., max_norm, norm_type=2) over the gradients of param_grads ({name: tensor}; one tensor under two
    names counts once): scales them in place by min(1, max_norm / (norm + 1e-6)) on the device (gpo_clip_grad_norm) and returns the total
    norm as a 0-d device tensor.  Nothing is copied to the host."""
    if not float(max_norm) > 0:
        raise ValueError(f"clip_grad_norm_: max_norm {max_norm} must be positive")
    seen, dev = {}, None
    for name, g in param_grads.items():
        if not torch.is_tensor(g) or g.device.type != "cuda":
            raise ValueError(f"param_grads[{name!r}]: {_describe(g)}, expected contiguous float32 on a HIP device")
        dev = dev or g.device
        _check_grad(name, g, dev)
        if g.numel():
            seen.setdefault(g.data_ptr(), g)
    if not seen:
        raise ValueError("clip_grad_norm_: no gradients")
    tab = np.zeros(len(seen), _TENSOR)
    tab["g"], tab["n"] = list(seen), [g.numel() for g in seen.values()]
    alloc = alloc or _default_alloc(dev)
    scalars = _launch("gpo_clip_grad_norm", dev, lambda nbytes: alloc("workspace", (max(int(nbytes) // 4, 64),)), lambda: alloc("scalars", (2,)),
                      _table_ptr(tab), len(tab), (), (float(max_norm),))
    return scalars[0]


class GradAccumulator:
    """The accumulated gradient of the reference's loop (engine/train.py:117-131 with FLAGS.accumulate, and DDP's gradient average) as one
    flat fp32 device buffer in the layout of `optimizer`'s state buffers, filled by gpc_grad_accumulate (include/givepose_accum.h).

    optimizer: a Ranger, Adam or AdamW; the accumulator takes its parameters, names, aliases and offsets.  It owns
      flat     the accumulated gradients, every tensor at a multiple of 64 elements; the padding is zeroed once and never written;
      stage    a second buffer of the same size for the exchange between ranks, allocated at the first add() with a group;
      scalars  the 2-norm of the accumulated gradients (before the clip) and the clip coefficient of the last add(), on the device.
    alloc(name, shape): optional hook that supplies "flat", "stage", "scalars" and "workspace" (default torch.empty)."""

    def __init__(self, optimizer, alloc=None):
        if not isinstance(optimizer, (Ranger, Adam)):        # AdamW is an Adam
            raise ValueError(f"GradAccumulator: a givepose_amd.optim.Ranger is expected, got {type(optimizer).__name__}")
        self.optimizer, self.device = optimizer, optimizer.device
        self._offsets = optimizer._offsets
        self._alloc = alloc or _default_alloc(self.device)
        total = int(self._offsets[-1])
        self.flat = self._alloc("flat", (total,)).zero_()
        self.stage = None
        self.scalars = self._alloc("scalars", (2,)).zero_()
        self._ws = None
        self._live = set()
        self._staged = frozenset()
        st = np.zeros(len(optimizer.params), _TENSOR)
        st["p"] = self.flat.data_ptr() + 4 * self._offsets[:-1]
        st["n"] = [p.numel() for p in optimizer.params]
        self._static = st

    def _view(self, i, buf=None):
        o, p = int(self._offsets[i]), self.optimizer.params[i]
        return (self.flat if buf is None else buf)[o:o + p.numel()].view(p.shape)

    @property
    def live(self):
        """The names (aliases included) of the parameters that have an accumulated gradient since the last zero()."""
        return [name for name, i in self.optimizer._index.items() if i in self._live]

    @property
    def grads(self):
        """{name: view into flat} of the live parameters under every one of their names: what Ranger.step takes."""
        return {name: self._view(i) for name, i in self.optimizer._index.items() if i in self._live}

    def zero(self):
        """optimizer.zero_grad(): no parameter has an accumulated gradient.  Nothing is written: the next add() overwrites."""
        self._live = set()

    def _table(self, param_grads):
        """-> (parameter indices, gpo_tensor table) of one add(): the parameters of param_grads and the live ones, in index order."""
        grads = self.optimizer._collect(param_grads)
        entries = sorted(set(grads) | self._live)
        tab = self._static[entries]
        tab["g"] = [grads[i][1].data_ptr() if i in grads else 0 for i in entries]
        tab["flags"] = [_lib.GPC_FLAG_OVERWRITE if i not in self._live else 0 for i in entries]
        return entries, tab, grads

    def _launch(self, tab, scale, max_norm):
        _launch("gpc_grad_accumulate", self.device, lambda nbytes: _workspace(self, nbytes), self.scalars, _table_ptr(tab), len(tab), (),
                (scale, max_norm))

    def _world(self, group):
        import torch.distributed as dist
        return dist.get_world_size(group)

    def _all_reduce(self, group):
        """The one collective of an add(): the whole of `stage`, summed in place, on the current stream."""
        import torch.distributed as dist
        dist.all_reduce(self.stage, op=dist.ReduceOp.SUM, group=group)

    @torch.no_grad()
    def add(self, param_grads, scale=1.0, clip_norm=None, group=None):
        """One micro-step: acc += scale * g for every entry of param_grads ({name: fp32 device tensor}, checked as Ranger.step checks
        them), then clip_grad_norm_(., clip_norm) in place over ALL live parameters -- also those that are live but absent from
        param_grads, which are counted in the norm and scaled (None: no clipping; scalars still receives the norm).  A parameter added
        for the first time since zero() is overwritten.  A refused call changes nothing.  The entries are taken in parameter order.
        group: a torch.distributed process group of `world` ranks: the gradients are first written to `stage` scaled by scale / world,
        `stage` is summed over the ranks by ONE all_reduce on the current stream, and the sum is then added exactly as the gradients of
        a one-rank call are, with the same per-tensor chunking, so the norm has the bits of the one-rank path on equal data.  Every rank
        must pass the same set of names on the same micro-step: that cannot be checked locally and is not checked."""
        scale = float(scale)
        if not math.isfinite(scale):
            raise ValueError(f"GradAccumulator.add: scale {scale} must be finite")
        if clip_norm is not None and not float(clip_norm) > 0:
            raise ValueError(f"GradAccumulator.add: clip_norm {clip_norm} must be positive (or None)")
        max_norm = float(clip_norm) if clip_norm is not None else 0.0
        entries, tab, grads = self._table(param_grads)
        if not entries:
            return
        if group is None:
            self._launch(tab, scale, max_norm)
        else:
            world = self._world(group)
            if self.stage is None:
                self.stage = self._alloc("stage", (int(self._offsets[-1]),)).zero_()
            given = frozenset(grads)
            if not self._staged <= given:        # slices no longer rewritten would be summed again and again: keep them 0
                self.stage.zero_()
            self._staged = given
            has = [k for k, i in enumerate(entries) if i in grads]
            if has:
                first = tab[has]
                first["p"] = self.stage.data_ptr() + 4 * self._offsets[[entries[k] for k in has]]
                first["flags"] = _lib.GPC_FLAG_OVERWRITE
                self._launch(first, scale / world, 0.0)
            self._all_reduce(group)
            tab["g"] = [self.stage.data_ptr() + 4 * int(self._offsets[i]) if i in grads else 0 for i in entries]
            self._launch(tab, 1.0, max_norm)
        self._live.update(grads)


def rank_accum_selfcheck(rank, world, port, queue, backend, params, grads_per_micro_step, accumulate, clip_norm, lr, device_index=0):
    """Entry point of ONE rank process of the accumulation self-check (tests/test_grad_accum_gpu.py starts `world` of them from a fork
    server that never touched the GPU): a module whose parameters are the float32 arrays `params` ({name: array}), a Ranger and a
    GradAccumulator over it, and the reference's loop over grads_per_micro_step (a list of {name: array}, this rank's gradients): every
    micro-step i adds with scale 1 / accumulate, clip_norm and the process group, and steps and zeroes when i % accumulate == 0.
    Puts (rank, "ok", {name: parameter}, {name: exp_avg}, (norm, coef) of the last add) on the queue as numpy arrays, or
    (rank, "error: ...", None, None, None).  backend "gloo" lets the ranks share one GPU; "nccl" = RCCL, one rank per GPU, or world == 1
    on a one-rank communicator; None: no process group at all (the one-rank path)."""
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(device_index if backend == "nccl" else rank))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # as runner.rank_selfcheck: this RCCL needs dmabuf IPC
    try:
        import torch.distributed as dist
        from . import dist as gd
        group = None
        if backend is not None:
            gd.init_from_env(backend=backend, force=world == 1)
            group = dist.group.WORLD
        torch.cuda.set_device(device_index)
        dev = torch.device("cuda", device_index)
        net = torch.nn.Module()
        for name, a in params.items():
            net.register_parameter(name, torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev), requires_grad=False))
        opt = Ranger(net, lr=lr)
        acc = GradAccumulator(opt)
        for i, grads in enumerate(grads_per_micro_step):
            g = {name: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for name, a in grads.items()}
            acc.add(g, scale=1.0 / accumulate, clip_norm=clip_norm, group=group)
            if i % accumulate == 0:
                opt.step(acc.grads, clip_norm=None, lr=lr)
                acc.zero()
        torch.cuda.synchronize(dev)
        out_p = {name: p.detach().cpu().numpy() for name, p in net.named_parameters()}
        out_m = {name: opt._view("exp_avg", opt._index[name]).cpu().numpy() for name in out_p}
        queue.put((rank, "ok", out_p, out_m, acc.scalars.cpu().numpy()))
        if group is not None:
            dist.barrier(device_ids=[device_index]) if backend == "nccl" else dist.barrier()
            dist.destroy_process_group()
    except Exception as e:   # the parent must never wait for a dead rank
        import traceback
        queue.put((rank, "error: " + repr(e) + "\n" + traceback.format_exc(), None, None, None))


def flat_and_anneal_lr(it, total_iters, warmup_iters=0, warmup_factor=0.1, warmup_method="linear", anneal_point=0.72, anneal_method="cosine",
                       target_lr_factor=0, poly_power=1.0, step_gamma=0.1, steps=(2 / 3.0, 8 / 9.0)):
    """The factor on the base learning rate at iteration `it` of the flat_and_anneal schedule
    (tools/torch_utils/solver/lr_scheduler.py:177-263, the lambda its LambdaLR wraps): warm-up, flat, then the anneal."""
    if warmup_method not in ("constant", "linear"):
        raise ValueError(f"Only 'constant' or 'linear' warmup_method accepted, got {warmup_method}")
    if anneal_method not in ("cosine", "linear", "poly", "exp", "step", "none"):
        raise ValueError(f"Only 'cosine', 'linear', 'poly', 'exp', 'step' or 'none' anneal_method accepted, got {anneal_method}")
    if anneal_method == "step":
        if any(s < warmup_iters / total_iters or s > 1 for s in steps):
            raise ValueError(f"error in steps: {steps}. warmup_iters: {warmup_iters} total_iters: {total_iters}. "
                             f"steps should be in ({warmup_iters / total_iters},1)")
        if list(steps) != sorted(steps):
            raise ValueError(f"steps {steps} is not in ascending order.")
        anneal_start = steps[0] * total_iters        # anneal_point is ignored
    else:
        if anneal_point > 1 or anneal_point < 0:
            raise ValueError(f"anneal_point should be in [0,1], got {anneal_point}")
        anneal_start = anneal_point * total_iters
    x = it
    if x < warmup_iters:
        if warmup_method == "linear":
            a = float(x) / warmup_iters
            return warmup_factor * (1 - a) + a
        return warmup_factor
    if x >= anneal_start:
        if anneal_method == "step":
            return step_gamma ** bisect_right([s * total_iters for s in steps], float(x))
        if anneal_method == "cosine":
            return target_lr_factor + 0.5 * (1 - target_lr_factor) * (1 + math.cos(math.pi * ((float(x) - anneal_start) / (total_iters - anneal_start))))
        if anneal_method == "linear":
            return target_lr_factor + (1 - target_lr_factor) * (total_iters - float(x)) / (total_iters - anneal_start)
        if anneal_method == "poly":
            return target_lr_factor + (1 - target_lr_factor) * ((total_iters - float(x)) / (total_iters - anneal_start)) ** poly_power
        if anneal_method == "exp":
            return max(target_lr_factor, 5e-3) ** ((float(x) - anneal_start) / (total_iters - anneal_start))
        return 1
    return 1
