"""PoseNet on hand-written HIP kernels -- drop-in for the reference ``network.PoseNet.PoseNet``.

Same public surface as the reference (network/PoseNet.py:134-231):
  * ``PoseNet(cfg)``; ``forward(data, device, do_loss=False, pred_scale=None) -> dict`` with keys
    ``rot`` (CPU fp32, as the reference returns it), ``trans``, ``size``, ``mask``, ``nocs_coor``,
    ``ivfc_coor``;
  * ``state_dict()`` / ``load_state_dict()`` use the reference's tensor names and shapes
    (tests/golden/state_dict_manifest.json), including ConvModule's duplicated ``.norm``/``.gn`` keys and the
    unused ``DCNv3_C.bn`` tensors, so ``evaluation/evaluate.py:51-56`` works unchanged.
The arithmetic runs entirely in libgivepose_hip.so (givepose_amd/csrc); there is no PyTorch/CPU fallback.
Everything is channels-last on the device; the whole launch sequence of one forward is optionally captured
in a hipGraph and replayed (``use_graph=True``).
"""
import ctypes
import functools
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops, synth
from ._lib import (ACT_GELU, ACT_RELU, EPI_GELU, EPI_LNFOLD_GELU, EPI_LRELU, EPI_NONE, EPI_SCALE_RES)
from .config import FLAT_OPS, ROT_TYPES, PoseNetConfig, validate

CONV3_WCM_LAYERS = (6, 7, 9, 10)      # the xyz heads' 3x3 convs on 32 x 32 and 64 x 64 maps (repack.CONV3_WCM_LAYERS)
OM_LD = 128     # row length of the DCNv3 offset | mask projection output (108 used columns)


def enc0_xyz_pack(sd, prefix="nocs_encoder.features.0.", dtype=torch.float32):
    """Reference-layout state dict -> (M (256, 16), b (256,)) fp32 of gp_dcnv3_xyz_project: the first DCNv3_C layer of the MAPEncoder
    as a gather of 16 numbers per output pixel and one matrix.  conv1x1, input_proj, the bilinear samples, the
    mask-weighted tap sum and output_proj are linear in the sampled value and a corner outside the map contributes zero, so with
    S_g = the gather of [x, y, z] and T_g = the same gather of a constant 1 for group g,
        out = sum_g M_g . [S_g; T_g] + out_b,   M_g = out_w[:, 64g:64g+64] @ [fold_w[64g:64g+64] | fold_b[64g:64g+64]]
    (fold_w = input_proj.weight @ conv.weight, fold_b = input_proj.weight @ conv.bias + input_proj.bias).  The products are formed in
    float64 from the unrounded tensors and rounded to `dtype` once (float64: the unrounded matrix, for tests)."""
    f64 = lambda k: sd[prefix + k].detach().to(device="cpu", dtype=torch.float64)
    cw, cb = f64("conv.weight").reshape(256, -1), f64("conv.bias")
    iw, ib = f64("dcnv3.input_proj.weight"), f64("dcnv3.input_proj.bias")
    ow, ob = f64("dcnv3.output_proj.weight"), f64("dcnv3.output_proj.bias")
    fold = torch.cat([iw @ cw, (iw @ cb + ib)[:, None]], 1)                                   # (256, 4): [fold_w | fold_b]
    m = torch.cat([ow[:, 64 * g:64 * g + 64] @ fold[64 * g:64 * g + 64] for g in range(4)], 1)    # (256, 16), column 4 g + c
    return m.to(dtype).contiguous(), ob.to(dtype).contiguous()


class _Node(nn.Module):
    """Container mirroring one level of the reference module tree (names only)."""


def _register(root, name, tensor, is_param):
    parts = name.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, _Node())
        mod = mod._modules[p]
    if is_param:
        mod.register_parameter(parts[-1], tensor)
    else:
        mod.register_buffer(parts[-1], tensor)


# TopDownXyzHead: GroupNorm apply + GELU fused into the bilinear x2 that follows (gp_groupnorm_upsample2x; fp16 storage only).
# GP_FUSE_GN_UPSAMPLE=0 runs the two passes (scripts/gn_upsample_ab.py measures both; the results are bitwise the same).
FUSE_GN_UPSAMPLE = os.environ.get("GP_FUSE_GN_UPSAMPLE", "1") != "0"

_BUFFER_SUFFIXES = ("running_mean", "running_var", "num_batches_tracked")


def _size_head_keyword(impl):
    """Decorator of `head_grads_feat` and `head_grads_backbone`: the method also accepts the keyword-only option size_head= (None, the
    default: the decorated method itself runs, as it always did; {"seed": s} or {"keep": mask}: checked, then `impl`, the method's
    private form, runs with it).  The option is taken here and not in the `def` line because the chain's five methods -- head_grads,
    head_grads_pnp, head_grads_xyz, head_grads_feat, head_grads_backbone -- keep one parameter list (data, pose_loss, device, gout,
    groups), and the first three, which stop before `feat`, have no use for it: inspect.signature() shows that shared list, the docstrings
    name the option."""
    def deco(fn):
        @functools.wraps(fn)
        def method(self, *args, size_head=None, **kwargs):
            if size_head is None:
                return fn(self, *args, **kwargs)
            self._size_head_mask(size_head, fn.__name__)
            return getattr(self, impl)(*args, **kwargs, size_head=size_head)
        return method
    return deco


def _accumulator_keywords(impl):
    """Decorator of `train_step`: the method also accepts the keyword-only options accumulator=, accumulate=, micro_step= and group=.
    accumulator=None (the default): the decorated method itself runs, as it always did, and the other three must keep their defaults;
    a GradAccumulator: `impl`, the accumulating form, runs with the same arguments.  The options are taken here and not in the `def`
    line for the reason `_size_head_keyword` gives: inspect.signature() keeps showing the parameter list that callers and tests know,
    which ends with size_head; the docstring names the options."""
    def deco(fn):
        @functools.wraps(fn)
        def method(self, *args, accumulator=None, accumulate=1, micro_step=0, group=None, **kwargs):
            if accumulator is None:
                if group is not None or accumulate != 1 or micro_step != 0:
                    raise ValueError(f"{fn.__name__}: group, accumulate and micro_step need accumulator=GradAccumulator(optimizer)")
                return fn(self, *args, **kwargs)
            return getattr(self, impl)(*args, **kwargs, accumulator=accumulator, accumulate=accumulate, micro_step=micro_step, group=group)
        return method
    return deco


class PoseNet(nn.Module):
    def __init__(self, cfg: PoseNetConfig = PoseNetConfig(), dtype=torch.float16, use_graph=False, seed=None, inflight=1,
                 split_gemm=False, dcn_couple=None):
        """dtype: storage type of activations / weights (float16 = throughput mode, float32 = parity mode).
        split_gemm (float32 only): the dense contractions run on the fp16 matrix pipe with split operands (hi + 2^-11 lo'
        planes, three MFMAs per product, fp32 accumulate: gp_gemm_desc.split_shift) instead of the fp32 MFMA; everything
        else is the float32 mode.  Error against the reference at the level of the fp32 mode (tests/precision_split.py).
        dcn_couple (grouped launches): a forward over B = G * dcn_couple crops is G independent batches of dcn_couple crops in
        ONE launch sequence -- every kernel sees G times the rows, the weights pass through the chip once for all of them --
        while the one thing that ties the crops of a batch together, the DCNv3 stride-2 offset / mask prefix (crop b reads
        the rows of crop b // 4 OF ITS BATCH), stays per group.  The results are those of G separate
        forwards up to the summation order (tile choice, split-K factor and GroupNorm chunking follow the row count): numerically
        equivalent, NOT bitwise -- tests/test_grouped_launch.py bounds the difference over all crops and checks every group against
        the oracle of its batch; bench.py reports the measured difference (overlap_check.grouped_vs_separate_batches)."""
        super().__init__()
        self.dcn_couple = None if not dcn_couple else int(dcn_couple)
        if split_gemm and dtype != torch.float32:
            raise ValueError("split_gemm is a float32-storage mode")
        self.split_gemm = bool(split_gemm)
        # the reference asserts backbone == 'convnext' (network/PoseNet.py:142); 'resnet34' (network/resnet.py:167-176,
        # defined but never wired there) is this build's throughput variant with feature_channel 512
        if cfg.main_backbone not in ("convnext", "resnet34"):
            raise NotImplementedError(f"unknown backbone {cfg.main_backbone}")
        validate(cfg)        # the pose-head flags (flat_op, mask_attention_type, r_type, ...): each works or refuses
        if cfg.res_fp32 and (dtype != torch.float16 or cfg.defer_ln or cfg.main_backbone != "convnext"):
            raise ValueError("res_fp32 is an option of the float16 ConvNeXt path (without defer_ln)")
        self.cfg = cfg
        self.compute_dtype = dtype
        self.use_graph = use_graph
        self.ROT_TYPE, self.TRANS_TYPE, self.Z_TYPE = cfg.r_type, "centroid_z", "REL"
        self.out_res = cfg.out_res
        aliases = {}
        for name, shape in synth.param_manifest(cfg).items():
            is_buf = name.endswith(_BUFFER_SUFFIXES)
            key = name.replace(".gn.", ".norm.")
            if key in aliases and key != name:       # ConvModule: .gn is the same Parameter as .norm
                t = aliases[key]
            else:
                if seed is None:
                    val = torch.zeros(shape, dtype=torch.int64 if name.endswith("num_batches_tracked") else torch.float32)
                else:
                    val = torch.from_numpy(synth.synth_tensor(name, shape, seed))
                t = val if is_buf else nn.Parameter(val, requires_grad=False)
                aliases[key] = t
            _register(self, name, t, not is_buf)
        self._packed = None       # device-side packed weights
        self._pnp_f32 = None      # device-side fp32 copies of the pnp_net parameters in the reference's layout (pnp_backward)
        self._xyz_f32 = {}        # head -> the same for a coordinate head (xyz_head_backward)
        self._enc_f32 = {}        # module -> the same for nocs_encoder / feat_reducer (map_encoder_backward, feat_reducer_backward)
        self.inflight = int(inflight)   # batches the caller keeps in flight (forward_device slots)
        if self.inflight > 1 and os.environ.get("GP_PACKED_FP32") == "1":
            # the A/B build with packed fp32 VALU ops: v_pk_fma_f32 results of one kernel's waves come out wrong beside another
            # kernel's MFMA stream on the same SIMD -- only strictly serial launches are safe with it
            raise RuntimeError("GP_PACKED_FP32=1 builds must not keep batches in flight (inflight > 1)")
        self._plans = OrderedDict()   # (B, slot, ragged) -> buffers / graph, least recently used first
        self.max_plans = int(os.environ.get("GP_MAX_PLANS", "12"))   # per model: a caller with B in 1 .. 48 would otherwise keep 48 buffer sets + graphs
        self._streams = {}        # slot -> dedicated stream of the hipGraph path
        self.eval()

    # ------------------------------------------------------------------ weights
    def _reset_plans(self):
        """Drop the packed weights and every plan (buffers + hipGraph).  Work of any slot stream may still be in flight on
        buffers that are about to return to the allocator, and a graph exec holds raw pointers into them: synchronise the
        device first, destroy the graph execs, then let the tensors go."""
        if getattr(self, "_plans", None):
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            lib = _lib.load()
            for plan in self._plans.values():
                if plan.get("graph") is not None:
                    lib.gp_graph_destroy(plan["graph"])
                    plan["graph"] = None
        self._packed = None
        self._repacker = None
        self._pnp_f32 = None
        self._xyz_f32 = {}
        self._enc_f32 = {}
        self._plans = OrderedDict()

    def params_updated(self):
        """Call after the parameters were changed through their storage (a kernel that writes through raw pointers, such as
        givepose_amd.optim.Ranger.step, changes neither data_ptr nor the version counter the caches are keyed on): drops the packed
        weights of the forward (`_packed`) and the fp32 copies of the backward (`_pnp_f32`, `_xyz_f32`, `_enc_f32`), so that the next
        forward repacks from the state_dict and the next backward reads the parameters again.
        The plans go too (`_reset_plans`): a plan is not only activation buffers -- its captured hipGraph holds raw pointers to the
        packed weight tensors that are dropped here, and its buffers hold weight-derived rows (the position embeddings of the 'att'
        heads, a_pos / p_pos, are copied from `_packed` when the plan is built).  The next forward rebuilds its plan, as after
        load_state_dict.
        Under set_repack("device") with packed weights present, none of that is dropped but the backward's caches: the current stream is made
        to wait for every slot stream (a forward issued with wait=False may still read the weights), then the packed tensors are rewritten
        in place from the parameters by gpr_repack on the current stream (givepose_amd/repack.py: no host copy, no device synchronise).
        Every packed tensor keeps its address, so the plans and their captured graphs stay valid, and forward_device makes its slot stream
        wait for the current one, which orders the next forward behind the repack."""
        if self._repack_mode == "device" and self._packed is not None and self._repacker is not None:
            cur = torch.cuda.current_stream(self._repacker.device)
            for s in self._streams.values():
                cur.wait_stream(s)
            self._repacker.run(self._repacker.sources_of(self))
            self.repack_count += 1
            self._pnp_f32 = None
            self._xyz_f32 = {}
            self._enc_f32 = {}
            return
        self._reset_plans()

    # how `_packed` is made and refreshed: "host" (`_pack`: host folds and roundings, plans rebuilt after every change) or "device"
    _repack_mode = "host"
    _repacker = None          # repack.DeviceRepack of the current `_packed` ("device" mode)
    repack_count = 0          # device repacks run so far (the first pack included)

    def set_repack(self, mode):
        """"host" (the default): `_pack` builds the packed weights on the host and `params_updated()` drops them with every plan.
        "device": the packed weights are built and refreshed on the device by the gpr_ family; the configuration is checked here
        (NotImplementedError names what the device repack does not serve: the resnet34 backbone, the 'att' encoder and head, use_dcn='',
        defer_ln=True).  Switching drops the packed weights and the plans, as load_state_dict does."""
        if mode not in ("host", "device"):
            raise ValueError(f"set_repack: {mode!r}, expected 'host' or 'device'")
        if mode == "device":
            from . import repack
            repack.plan(self.cfg, self.compute_dtype, self.split_gemm)
        if mode != self._repack_mode:
            self._reset_plans()
            self._repack_mode = mode
        return self

    # the precision of the backbone's recompute and backward (`backbone_backward`, and with it `head_grads_backbone` and `train_step`)
    _backward_precision = "fp32"
    # the same for the two coordinate heads (`xyz_head_backward`, and with it `head_grads_xyz`, `head_grads_feat`, ... and `train_step`)
    _xyz_backward_precision = "fp32"

    # how the map encoder's backward sums d xp of its DCNv3 cores (`map_encoder_backward`, and with it `head_grads_feat`,
    # `head_grads_backbone`, `train_step` and the accumulated `train_step`)
    _encoder_scatter = "atomic"

    @property
    def encoder_scatter(self):
        """"atomic" (the default) or "ordered": see `set_encoder_scatter`."""
        return self._encoder_scatter

    def set_encoder_scatter(self, mode):
        """"atomic" (the default): d xp of the encoder's three DCNv3 cores is scattered with fp32 atomic adds; `map_encoder_backward`
        and everything that runs through it repeat to rounding between two calls.
        "ordered": the same terms are added per element in ascending order of their source id, without a floating-point atomic
        (include/givepose_encgrad_ordered.h): all 48 encoder gradients and d coor, and what is chained below them, are equal bits
        between two calls.  Slower, and a larger workspace; the forward and the inference path are untouched.
        Anything else raises ValueError.  Returns self."""
        from . import enc_grad
        enc_grad.scatter_mode(mode)
        self._encoder_scatter = mode
        return self

    @property
    def backward_precision(self):
        """"fp32" (the default) or "bf16": see `set_backward_precision`."""
        return self._backward_precision

    @property
    def xyz_backward_precision(self):
        """"fp32" (the default) or "bf16": the `xyz_heads` argument of the last `set_backward_precision`."""
        return self._xyz_backward_precision

    def set_backward_precision(self, mode, xyz_heads="fp32"):
        """"fp32" (the default): the backbone's recompute and backward are the fp32 chains of the gpb_ family.
        "bf16": the six dense contractions of every ConvNeXt block multiply bf16-rounded operands and add in fp32, as
        torch.autocast(bfloat16) does elsewhere (givepose_amd.bb_grad, precision="bf16"; include/givepose_bbgrad_bf16.h); no loss scaling
        is needed.  Everything else in the chain -- the heads, the encoder, the loss, the optimiser, the forward -- is unchanged, and
        switching back to "fp32" gives the bits of before.  Nothing is cached per mode: the switch costs nothing.
        xyz_heads, "fp32" (the default) or "bf16", is the same switch for the two coordinate heads (`xyz_head_backward` of
        xyz_nocs_head and xyz_deform_head): with "bf16" the 21 contractions of a head's 3x3 layers, in its recompute and in its backward,
        take bf16-rounded operands (givepose_amd.xyz_grad, precision="bf16"; include/givepose_xyzgrad_bf16.h), the rest of the head stays
        fp32.  Every call sets both: set_backward_precision("bf16") alone leaves the heads at their fp32 bits, and
        set_backward_precision("fp32") is everything as before."""
        if mode not in ("fp32", "bf16"):
            raise ValueError(f"set_backward_precision: {mode!r}, expected 'fp32' or 'bf16'")
        if xyz_heads not in ("fp32", "bf16"):
            raise ValueError(f"set_backward_precision: xyz_heads {xyz_heads!r}, expected 'fp32' or 'bf16'")
        self._backward_precision = mode
        self._xyz_backward_precision = xyz_heads
        return self

    def _pack_device(self, device):
        """`_pack` under set_repack("device"): allocates the packed tensors (the keys, shapes and dtypes of `_pack`) and fills them on the
        device.  The parameters must be contiguous float32 on `device` (ValueError names the first that is not)."""
        from . import repack
        rp = repack.DeviceRepack(repack.plan(self.cfg, self.compute_dtype, self.split_gemm), device)
        rp.run(rp.sources_of(self))
        self.repack_count += 1
        self._repacker, self._packed = rp, rp.packed
        return self._packed

    def __del__(self):
        try:
            self._reset_plans()
        except Exception:
            pass

    def load_state_dict(self, state_dict, strict=True):
        r = super().load_state_dict(state_dict, strict=strict)
        self._reset_plans()
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._reset_plans()
        return r

    @torch.no_grad()
    def _pack(self, device):
        """Reference-layout fp32 state dict -> kernel-layout device tensors (done once).  Every fold (eval BatchNorm into
        a conv, conv1x1 into input_proj, LayerNorm affine into fc1) and every rounding to the storage type happens on the
        HOST; the device only ever runs this library's kernels (the one device-side step is gp_convnext_mlp_pack_w2).
        Under set_repack("device") the same tensors are made on the device instead (`_pack_device`)."""
        if self._repack_mode == "device":
            return self._pack_device(device)
        sd = {k: v.detach().to(device="cpu", dtype=torch.float32) if v.is_floating_point() else v.detach().cpu()
              for k, v in self.state_dict().items()}
        T = self.compute_dtype
        f32 = lambda t: t.contiguous().float().to(device)
        lowp = lambda t: t.contiguous().to(T).to(device)
        # operands of gp_gemm: storage type, or hi / lo' fp16 planes in the split-operand mode
        gw = (lambda t: ops.split_weights(t.reshape(t.shape[0], -1), device)) if self.split_gemm else lowp
        W = {}
        cfg = self.cfg
        g = lambda k: sd["backbone." + k]
        if cfg.main_backbone == "resnet34":
            def fold(conv, bn):      # eval BatchNorm folded into the conv: w' = w * s[co], b' = beta - mean * s
                sc = g(bn + ".weight") / torch.sqrt(g(bn + ".running_var") + 1e-5)
                return g(conv + ".weight") * sc[:, None, None, None], g(bn + ".bias") - g(bn + ".running_mean") * sc
            w, b = fold("conv1", "bn1")
            W["rs.stem_w"], W["rs.stem_b"] = f32(w.reshape(64, 147).t()), f32(b)
            for li, (planes, blocks, stride) in enumerate(synth.RESNET34_LAYERS, 1):
                for bi in range(blocks):
                    p, q = f"layer{li}.{bi}", f"rs{li}.{bi}."
                    for c in ("1", "2"):
                        w, b = fold(p + ".conv" + c, p + ".bn" + c)
                        W[q + "w" + c], W[q + "b" + c] = gw(w.permute(0, 2, 3, 1).reshape(planes, -1)), f32(b)
                    if ("backbone." + p + ".downsample.0.weight") in sd:
                        w, b = fold(p + ".downsample.0", p + ".downsample.1")
                        W[q + "wd"], W[q + "bd"] = gw(w.reshape(planes, -1)), f32(b)
        for s, (d, n) in enumerate(zip(cfg.convnext_dims, cfg.convnext_depths) if cfg.main_backbone == "convnext" else ()):
            if s == 0:
                W["stem.w"], W["stem.b"] = f32(g("stem_0.weight").reshape(-1, 48).t()), f32(g("stem_0.bias"))
                W["stem.ln_w"], W["stem.ln_b"] = f32(g("stem_1.weight")), f32(g("stem_1.bias"))
            if s > 0:
                p = f"stages_{s}.downsample."
                W[f"ds{s}.ln_w"], W[f"ds{s}.ln_b"] = f32(g(p + "0.weight")), f32(g(p + "0.bias"))
                W[f"ds{s}.w"] = gw(g(p + "1.weight").permute(0, 2, 3, 1).reshape(d, -1))
                W[f"ds{s}.b"] = f32(g(p + "1.bias"))
            for b in range(n):
                p, q = f"stages_{s}.blocks.{b}.", f"s{s}b{b}."
                W[q + "dw_w"] = lowp(g(p + "conv_dw.weight").reshape(d, 49).t())
                W[q + "dw_b"] = f32(g(p + "conv_dw.bias"))
                W[q + "ln_w"], W[q + "ln_b"] = f32(g(p + "norm.weight")), f32(g(p + "norm.bias"))
                W[q + "fc1_w"], W[q + "fc1_b"] = gw(g(p + "mlp.fc1.weight")), f32(g(p + "mlp.fc1.bias"))
                W[q + "fc2_w"], W[q + "fc2_b"] = gw(g(p + "mlp.fc2.weight")), f32(g(p + "mlp.fc2.bias"))
                W[q + "gamma"] = f32(g(p + "gamma"))
                fuse512 = d == 512 and (cfg.fuse_mlp512 or os.environ.get("GP_FUSE_MLP512") == "1")      # (env: A/B switch)
                if T == torch.float16 and (d in (128, 256) or fuse512) and cfg.fuse_mlp:   # fused fc1->GELU->fc2 (csrc/mlp.hip)
                    W[q + "fc2_wp"] = ops.convnext_mlp_pack_w2(W[q + "fc2_w"])
                if T == torch.float16 and d == 512 and cfg.defer_ln:   # LayerNorm folded into fc1's epilogue
                    w1, lw, lb = g(p + "mlp.fc1.weight"), g(p + "norm.weight"), g(p + "norm.bias")
                    wg = (w1 * lw[None, :]).to(T)
                    W[q + "fc1_wg"] = lowp(wg)
                    W[q + "fc1_cs"] = f32(wg.float().sum(1))                          # column sums of the ROUNDED weights
                    W[q + "fc1_cb"] = f32(w1 @ lb + g(p + "mlp.fc1.bias"))
        for head in ("xyz_nocs_head", "xyz_deform_head"):
            h = lambda k: sd[f"{head}.{k}"]
            W[head + ".deconv_w"] = gw(h("features.0.weight").permute(2, 3, 1, 0).reshape(9 * 256, -1))
            W[head + ".gn0_w"], W[head + ".gn0_b"] = f32(h("features.1.weight")), f32(h("features.1.bias"))
            for i in (3, 4, 6, 7, 9, 10):
                W[f"{head}.c{i}_w"] = gw(h(f"features.{i}.conv.weight").permute(0, 2, 3, 1).reshape(256, -1))
                if T == torch.float16 and i in CONV3_WCM_LAYERS:     # chunk-major copy for the eight-phase window conv (gp_gemm_desc.W_cm), made once
                    W[f"{head}.c{i}_wcm"] = ops.conv3_pack_wcm(W[f"{head}.c{i}_w"])
                W[f"{head}.c{i}_gw"], W[f"{head}.c{i}_gb"] = f32(h(f"features.{i}.norm.weight")), f32(h(f"features.{i}.norm.bias"))
            W[head + ".out_w"], W[head + ".out_b"] = f32(h("out_layer.weight").reshape(3, 256)), f32(h("out_layer.bias"))
        # SizeHead: fold eval BatchNorm1d into conv1 (pose_head.py:34-35)
        sc = sd["size_head.bn1.weight"] / torch.sqrt(sd["size_head.bn1.running_var"] + 1e-5)
        W["size.w1"] = f32(sd["size_head.conv1.weight"].squeeze(-1) * sc[:, None])
        W["size.b1"] = f32((sd["size_head.conv1.bias"] - sd["size_head.bn1.running_mean"]) * sc + sd["size_head.bn1.bias"])
        W["size.w2"], W["size.b2"] = f32(sd["size_head.conv2.weight"].squeeze(-1)), f32(sd["size_head.conv2.bias"])
        if cfg.nocsmap_encoder == "att":      # MAPTransformerEncoer (network/attention_pnp_net.py:126-157)
            a = lambda k: sd["nocs_encoder." + k]
            W["att.pe_w"] = gw(a("patch_embed.proj.weight").permute(0, 2, 3, 1).reshape(256, -1))   # K = (ky,kx,c)
            W["att.pe_b"] = f32(a("patch_embed.proj.bias"))
            W["att.pos"] = f32(a("pos_embed").reshape(64, 256))                                      # tiled per batch in _plan
            W["att.ones"] = torch.ones(256, dtype=torch.float32, device=device)
            W["att.norm_w"], W["att.norm_b"] = f32(a("norm.weight")), f32(a("norm.bias"))
            for i in range(3):
                q = f"att{i}."
                for n in ("norm1", "norm2"):
                    W[q + n + "_w"], W[q + n + "_b"] = f32(a(f"block.{i}.{n}.weight")), f32(a(f"block.{i}.{n}.bias"))
                W[q + "qkv_w"] = gw(a(f"block.{i}.attn.qkv.weight"))
                W[q + "proj_w"], W[q + "proj_b"] = gw(a(f"block.{i}.attn.proj.weight")), f32(a(f"block.{i}.attn.proj.bias"))
                W[q + "fc1_w"], W[q + "fc1_b"] = gw(a(f"block.{i}.mlp.fc1.weight")), f32(a(f"block.{i}.mlp.fc1.bias"))
                W[q + "fc2_w"], W[q + "fc2_b"] = gw(a(f"block.{i}.mlp.fc2.weight")), f32(a(f"block.{i}.mlp.fc2.bias"))
        for li, i in enumerate((0, 3, 6) if cfg.nocsmap_encoder == "conv" else ()):
            p, q = f"nocs_encoder.features.{i}.", f"enc{li}."
            if cfg.use_dcn == "dcnv3":
                cw = sd[p + "conv.weight"].reshape(256, -1)
                W[q + "conv_w"] = f32(cw) if li == 0 else gw(cw)
                W[q + "conv_b"] = f32(sd[p + "conv.bias"])
                d = p + "dcnv3."
                W[q + "dw_w"] = lowp(sd[d + "dw_conv.0.weight"].reshape(256, 9).t())
                W[q + "dw_b"] = f32(sd[d + "dw_conv.0.bias"])
                W[q + "ln_w"], W[q + "ln_b"] = f32(sd[d + "dw_conv.1.1.weight"]), f32(sd[d + "dw_conv.1.1.bias"])
                # offset (72) | mask (36) projections as one GEMM, padded with zero rows to 128 columns: N % 32 == 0 lets the few-crop case run on the
                # small-M kernel (a 108-wide output took a 128 x 128 tile: 12-14 us per launch at one crop); the consumers read columns 0..107 of rows of 128
                omw = torch.cat([sd[d + "offset.weight"], sd[d + "mask.weight"]], 0)
                omb = torch.cat([sd[d + "offset.bias"], sd[d + "mask.bias"]], 0)
                W[q + "om_w"] = gw(torch.cat([omw, omw.new_zeros(OM_LD - omw.shape[0], omw.shape[1])], 0))
                W[q + "om_b"] = f32(torch.cat([omb, omb.new_zeros(OM_LD - omb.shape[0])], 0))
                W[q + "in_w"], W[q + "in_b"] = gw(sd[d + "input_proj.weight"]), f32(sd[d + "input_proj.bias"])
                # input_proj(conv1x1(x)) is one linear map: fold the two (fp32 product, then storage rounding) so the
                # full-resolution 256-channel `conv` output is only materialised for the prefix the dw_conv branch reads
                wf = sd[d + "input_proj.weight"] @ cw
                W[q + "fold_w"] = f32(wf) if li == 0 else gw(wf)
                W[q + "fold_b"] = f32(sd[d + "input_proj.weight"] @ sd[p + "conv.bias"] + sd[d + "input_proj.bias"])
                W[q + "out_w"], W[q + "out_b"] = gw(sd[d + "output_proj.weight"]), f32(sd[d + "output_proj.bias"])
                if li == 0 and T == torch.float16 and not self.split_gemm:     # layer 0 as one gather + one 256 x 16 matrix (gp_dcnv3_xyz_project)
                    W[q + "xyz_m"], W[q + "xyz_b"] = (f32(t) for t in enc0_xyz_pack(sd, p))
            else:
                cw = sd[p + "weight"]
                W[q + "conv_w"] = f32(cw.reshape(256, -1).t()) if li == 0 else gw(cw.permute(0, 2, 3, 1).reshape(256, -1))
            W[q + "gn_w"], W[q + "gn_b"] = f32(sd[f"nocs_encoder.features.{i + 1}.weight"]), f32(sd[f"nocs_encoder.features.{i + 1}.bias"])
        W["red.w"], W["red.b"] = gw(sd["feat_reducer.weight"].reshape(256, -1)), f32(sd["feat_reducer.bias"])
        if cfg.pnp_head == "att":      # AttentionPnPNet (network/attention_pnp_net.py:36-124): the MAPTransformerEncoer layout at 192 channels
            a = lambda k: sd["pnp_net." + k]
            W["apn.pe_w"] = gw(a("patch_embed.proj.weight").permute(0, 2, 3, 1).reshape(192, -1))   # K = (ky,kx,c): gp_patchify_pnp's rows
            W["apn.pe_b"] = f32(a("patch_embed.proj.bias"))
            W["apn.pos"] = f32(a("pos_embed").reshape(64, 192))                                      # tiled per batch in _plan
            W["apn.ones"] = torch.ones(192, dtype=torch.float32, device=device)
            W["apn.norm_w"], W["apn.norm_b"] = f32(a("norm.weight")), f32(a("norm.bias"))
            for i in range(3):
                q = f"apn{i}."
                for n in ("norm1", "norm2"):
                    W[q + n + "_w"], W[q + n + "_b"] = f32(a(f"block.{i}.{n}.weight")), f32(a(f"block.{i}.{n}.bias"))
                W[q + "qkv_w"] = gw(a(f"block.{i}.attn.qkv.weight"))
                W[q + "proj_w"], W[q + "proj_b"] = gw(a(f"block.{i}.attn.proj.weight")), f32(a(f"block.{i}.attn.proj.bias"))
                W[q + "fc1_w"], W[q + "fc1_b"] = gw(a(f"block.{i}.mlp.fc1.weight")), f32(a(f"block.{i}.mlp.fc1.bias"))
                W[q + "fc2_w"], W[q + "fc2_b"] = gw(a(f"block.{i}.mlp.fc2.weight")), f32(a(f"block.{i}.mlp.fc2.bias"))
        else:
            W["pnp.c0_w"] = f32(sd["pnp_net.features.0.weight"].reshape(128, -1).t())
            for li, i in enumerate((0, 3, 6)):
                if li > 0:
                    W[f"pnp.c{li}_w"] = gw(sd[f"pnp_net.features.{i}.weight"].permute(0, 2, 3, 1).reshape(128, -1))
                W[f"pnp.g{li}_w"], W[f"pnp.g{li}_b"] = f32(sd[f"pnp_net.features.{i + 1}.weight"]), f32(sd[f"pnp_net.features.{i + 1}.bias"])
        # fc1 || fc1_z as one GEMM; flat_op 'flatten': columns permuted from the reference's NCHW flatten (c*64+hw,
        # conv_pnp_net.py:170-172) to the channels-last flatten (hw*128+c) used on the device.  The pooled modes' columns
        # [mean c0..127 | max | min] are already in the order gp_pool_mmm writes.  The attention head's flatten(1) of its
        # (B, 64, 192) tokens (token*192+c) IS the device's row order: no permutation
        if cfg.flat_op == "flatten" and cfg.pnp_head == "conv":
            perm = lambda w: w.reshape(-1, 128, 64).permute(0, 2, 1).reshape(-1, 8192)
        else:
            perm = lambda w: w
        W["pnp.fc1_w"] = gw(torch.cat([perm(sd["pnp_net.fc1.weight"]), perm(sd["pnp_net.fc1_z.weight"])], 0))
        W["pnp.fc1_b"] = f32(torch.cat([sd["pnp_net.fc1.bias"], sd["pnp_net.fc1_z.bias"]], 0))
        W["pnp.fc2_w"], W["pnp.fc2_b"] = gw(sd["pnp_net.fc2.weight"]), f32(sd["pnp_net.fc2.bias"])
        W["pnp.fc2z_w"], W["pnp.fc2z_b"] = gw(sd["pnp_net.fc2_z.weight"]), f32(sd["pnp_net.fc2_z.bias"])
        for n in ("fc_r", "fc_t", "fc_z"):
            W[n + ".w"], W[n + ".b"] = f32(sd[f"pnp_net.{n}.weight"]), f32(sd[f"pnp_net.{n}.bias"])
        self._packed = W
        return W

    # ------------------------------------------------------------------ buffers
    # total crop counts a multi-frame (ragged) forward is padded to: a few graph shapes instead of one per total
    RAGGED_BUCKETS = (8, 16, 24, 32, 48, 64, 96, 128)

    @classmethod
    def ragged_bucket(cls, n):
        for b in cls.RAGGED_BUCKETS:
            if n <= b:
                return b
        return (n + 63) // 64 * 64

    def _evict_plans(self, keep):
        """Least-recently-used plans beyond max_plans go: the device is synchronised first (a slot's stream may still run the graph
        whose exec holds raw pointers into the buffers), the graph exec destroyed, then the tensors released."""
        while len(self._plans) > max(self.max_plans, 1):
            key = next(k for k in self._plans if k != keep)
            torch.cuda.synchronize()
            plan = self._plans.pop(key)
            if plan.get("graph") is not None:
                _lib.load().gp_graph_destroy(plan["graph"])
                plan["graph"] = None

    def _plan(self, B, device, slot=0, ragged=False):
        key = (B, slot, bool(ragged))
        plan = self._plans.get(key)
        if plan is not None:
            self._plans.move_to_end(key)
            return plan
        T, cfg = self.compute_dtype, self.cfg
        R, S = cfg.out_res, cfg.img_size
        e = lambda *shape, dtype=T: torch.empty(*shape, dtype=dtype, device=device)
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=device)
        buf = {}
        # static inputs
        buf["roi_img"], buf["roi_mask"] = f(B, 3, S, S), f(B, 1, S, S)
        buf["roi_coord_2d"], buf["cam_K"], buf["roi_wh"] = f(B, 2, R, R), f(B, 3, 3), f(B, 2)
        buf["bbox_center"], buf["resize_ratio"], buf["mean_size"] = f(B, 2), f(B), f(B, 3)
        # trunk
        dims = cfg.convnext_dims if cfg.main_backbone == "convnext" else ()
        H = S // 4
        if cfg.main_backbone == "resnet34":
            buf["rs_stem"] = e(B, S // 2, S // 2, 64)
            for li, (planes, _, _) in enumerate(synth.RESNET34_LAYERS, 1):
                h = S // (2 << li)          # 64, 32, 16, 8
                for n in ("a", "b", "c"):    # block input/output ping-pong + conv1 output
                    buf[f"rs{li}{n}"] = e(B, h, h, planes)
        for s, d in enumerate(dims):
            h = H >> s
            if cfg.res_fp32 and T == torch.float16 and d == 512:     # fp32 residual stream (+ the fp16 copy the branch reads)
                buf[f"x{s}"], buf[f"x{s}h"] = f(B, h, h, d), e(B, h, h, d)
            else:
                buf[f"x{s}"] = e(B, h, h, d)
            buf[f"t{s}"] = e(B, h, h, d)
            buf[f"h{s}"] = e(B * h * h, 4 * d)
            if d == 512:
                buf["ln_stats"] = f(B * h * h, 2, d // 128)
            if s > 0:
                buf[f"dsn{s}"] = e(B, h * 2, h * 2, dims[s - 1])
        # heads
        # deconv-as-GEMM output: fp16 in the fp16 mode (round 5: the GEMM's lean epilogue, half the bytes for col2im), fp32 otherwise
        buf["cols"] = e(B * 64, 9 * 256) if (T == torch.float16 and cfg.deconv_cols_f16 and os.environ.get("GP_DECONV_COLS_F32") != "1") else f(B * 64, 9 * 256)   # (env: A/B switch)
        for r in (16, 32, 64):
            buf[f"ya{r}"], buf[f"yb{r}"] = e(B, r, r, 256), e(B, r, r, 256)
        chunks = max(ops.groupnorm_chunks(B, r * r) for r in (8, 16, 32, 64))
        # fused statistics come in 16- / 32- / 64-row chunks (gp_gemm_gn_rows: the library's choice per launch): sized for the finest one at the
        # largest map, whatever the cost model picks (the small-M kernel would otherwise write past the buffer without any error); _gnarg checks
        buf["gn_partial"], buf["size_scratch"] = f(B * max(chunks, R * R // 16) * 32 * 2), f(B * (cfg.feat_ts + (512 if cfg.main_backbone == "resnet34" else cfg.convnext_dims[-1])))
        buf["nocs_nchw"], buf["nocs_nhwc4"] = f(B, 3, R, R), f(B * R * R, 4)
        buf["ivfc_nchw"], buf["ivfc_nhwc4"] = f(B, 3, R, R), f(B * R * R, 4)
        buf["mask_out"], buf["size"] = f(B, 1, R, R), f(B, 3)
        # GP_ENC0_XYZ=0 (A/B switch, read here): encoder layer 0 on the three launches of the 256-channel layers instead of gp_dcnv3_xyz_project
        enc0_xyz = "enc0.xyz_m" in self._packed and os.environ.get("GP_ENC0_XYZ") != "0"
        for li, r in enumerate((64, 32, 16)):
            buf[f"e_in{li}"], buf[f"e_x1{li}"] = e(B, r, r, 256), e(B * r * r // 4, 256)
            buf[f"e_om{li}"] = f(B * r * r // 4, OM_LD)
            buf[f"e_o{li}"] = e(B, r // 2, r // 2, 256)
            if li > 0 or not enc0_xyz:      # (the folded layer 0 has neither the projected full-resolution map nor the gathered one)
                buf[f"e_proj{li}"], buf[f"e_g{li}"] = e(B, r, r, 256), e(B, r // 2, r // 2, 256)
        if cfg.nocsmap_encoder == "att":
            buf["a_patch"], buf["a_x"], buf["a_h"] = e(B * 64, 192), e(B * 64, 256), e(B * 64, 256)
            buf["a_qkv"], buf["a_att"], buf["a_mlp"] = e(B * 64, 768), e(B * 64, 256), e(B * 64, 1024)
            buf["a_pos"] = self._packed["att.pos"].to(T).repeat(B, 1).contiguous()      # pos_embed per token row
        buf["feat_cat"] = e(B, 8, 8, 512)
        if cfg.pnp_head == "att":     # AttentionPnPNet: 64 tokens x 192 per crop; p_flat (B*64, 192) viewed as (B, 12288) is fc1's input
            buf["p_patch"], buf["p_x"], buf["p_h"] = e(B * 64, 320), e(B * 64, 192), e(B * 64, 192)
            buf["p_qkv"], buf["p_att"], buf["p_mlp"], buf["p_flat"] = e(B * 64, 576), e(B * 64, 192), e(B * 64, 768), e(B * 64, 192)
            buf["p_pos"] = self._packed["apn.pos"].to(T).repeat(B, 1).contiguous()      # pos_embed per token row
        else:
            buf["p0"], buf["p1"], buf["p2"] = e(B, 32, 32, 128), e(B, 16, 16, 128), e(B, 8, 8, 128)
        buf["fc1"] = e(B, 2048)
        buf["hh"], buf["hz"] = f(B, 256), f(B, 256)
        if FLAT_OPS[cfg.flat_op]:     # flat_op avg / avg-max / avg-max-min: the pooled fc1 input (storage type; fp32 in split mode: gp_gemm splits X)
            buf["pooled"] = e(B, 128 * FLAT_OPS[cfg.flat_op])
        buf["pred_rot"], buf["pred_t"], buf["rot_allo"], buf["rot_ego"], buf["trans"] = f(B, cfg.rot_dim), f(B, 3), f(B, 9), f(B, 9), f(B, 3)
        buf["rot6d"] = buf["pred_rot"] if cfg.rot_dim == 6 else None
        plan = {"buf": buf, "graph": None, "warm": False, "ragged": bool(ragged), "enc0_xyz": enc0_xyz}
        if ragged:
            # crop -> first crop of its batch (gp_dwconv_ln_groups); rewritten before every launch, the pointer is what the graph holds.
            # Padding crops (beyond the real ones) are batches of their own and keep benign inputs: zero image, identity camera.
            buf["grp"] = torch.arange(B, dtype=torch.int32, device=device)
            buf["grp_host"] = torch.arange(B, dtype=torch.int32).pin_memory()
            for k in ("roi_img", "roi_mask", "roi_coord_2d", "bbox_center", "mean_size"):
                buf[k].zero_()
            buf["roi_wh"].fill_(1.0)
            buf["resize_ratio"].fill_(1.0)
            buf["cam_K"].copy_(torch.eye(3, device=device).expand(B, 3, 3))
        self._plans[key] = plan
        self._evict_plans(key)
        return plan

    # ------------------------------------------------------------------ launch sequence
    def _gn(self, x, w, b, act, buf, G=32, out=None, ldy=None, fused=False, out_planes=False, rows=64):
        """GroupNorm(32)+act in place (or into a concat target); fused: the producing GEMM already wrote the statistics.
        out_planes (split-operand mode): `out` (another buffer of x's shape) receives the result as the fp16 planes the next
        conv reads."""
        B = x.shape[0]
        C = x.shape[-1]
        xv = x.view(B, -1, C)
        ops.groupnorm(xv, w, b, xv if out is None else out, G, act, buf["gn_partial"], ldy=ldy, fused_stats=fused, out_planes=out_planes, rows=rows)

    def _gnrows(self, M, N, K, hw):
        """Rows per statistics chunk of a fused-GroupNorm launch: the library's choice in plain fp16 mode (16 / 32 where the small-M kernel takes the launch:
        the detections of one frame), 64 -- the tile kernels' -- otherwise."""
        if self.split_gemm or self.compute_dtype != torch.float16 or os.environ.get("GP_GN_ROWS64") == "1":
            return 64
        return ops.gemm_gn_rows(M, N, K, hw)

    @staticmethod
    def _gnarg(buf, hw, rows=64):
        B = buf["mask_out"].shape[0]
        if B * (hw // rows) * 32 * 2 > buf["gn_partial"].numel():
            raise RuntimeError(f"fused GroupNorm statistics: {hw // rows} chunks of {rows} rows per image do not fit the plan's gn_partial buffer")
        return (buf["gn_partial"], 32, hw, rows)

    def _xyz_head(self, W, head, feat2d, B, buf, out_nchw, out_nhwc4):
        """network/xyz_head.py:349-366; feat2d (B*64, Cin) channels-last rows.
        Split-operand mode: whatever feeds a 3x3 conv (GroupNorm apply, bilinear upsample) writes the conv's fp16 operand planes
        directly (out of place, into the level's other ping-pong buffer) instead of fp32 + a split pass."""
        pl = self.split_gemm
        ops.gemm(feat2d, W[head + ".deconv_w"], buf["cols"], prefetch=W[f"{head}.c3_w"])
        y = ops.deconv_col2im(buf["cols"], buf["ya16"], B, 8, 8, 256)
        if pl:
            self._gn(y, W[head + ".gn0_w"], W[head + ".gn0_b"], ACT_GELU, buf, out=buf["yb16"].view(B, -1, 256), out_planes=True)
            y = buf["yb16"]
        else:
            self._gn(y, W[head + ".gn0_w"], W[head + ".gn0_b"], ACT_GELU, buf)
        cur, r = y, 16
        rows = {rr: self._gnrows(B * rr * rr, 256, 2304, rr * rr) for rr in (16, 32, 64)}
        fuse_up = FUSE_GN_UPSAMPLE and not pl and y.dtype == torch.float16
        for i in (3, 4, 6, 7, 9, 10):
            if i in (6, 9):
                r *= 2
                if fuse_up:   # GroupNorm apply + GELU of conv i-2 and the bilinear x2 in one pass (cur holds the raw conv output)
                    cur = ops.groupnorm_upsample2x(cur, W[f"{head}.c{i - 2}_gw"], W[f"{head}.c{i - 2}_gb"], buf[f"ya{r}"], 32, ACT_GELU,
                                                   buf["gn_partial"], rows=rows[r // 2])
                else:
                    cur = ops.upsample_bilinear2x(cur, buf[f"ya{r}"], out_planes=pl)
            dst = buf[f"yb{r}"] if cur is buf[f"ya{r}"] else buf[f"ya{r}"]
            nxt = {3: 4, 4: 6, 6: 7, 7: 9, 9: 10}.get(i)
            # (the launches that take the eight-phase window conv read the chunk-major copy: that is what the launch before them prefetches)
            wide = lambda rr: rr >= 32 and B * rr * rr % 512 == 0 and B * rr * rr > 16384
            nr = r * 2 if nxt in (6, 9) else r
            nxt_w = (W.get(f"{head}.c{nxt}_wcm") if wide(nr) else None) if nxt else None
            ops.conv2d_nhwc(cur, W[f"{head}.c{i}_w"], 3, 3, 1, 1, out=dst, gn=self._gnarg(buf, r * r, rows[r]),
                            prefetch=(nxt_w if nxt_w is not None else W[f"{head}.c{nxt}_w"]) if nxt else None, x_planes=pl,
                            w_cm=W.get(f"{head}.c{i}_wcm"))
            if i == 10:   # last ConvModule: GN + GELU + the 1x1 out layer in one pass, the 64x64x256 tensor is never written
                ops.groupnorm_apply_xyz(dst.view(B, r * r, 256), W[f"{head}.c{i}_gw"], W[f"{head}.c{i}_gb"], W[head + ".out_w"],
                                        W[head + ".out_b"], out_nchw, out_nhwc4, 32, ACT_GELU, buf["gn_partial"], rows=rows[r],
                                        packed16=self.cfg.gnxyz16 and dst.dtype == torch.float16 and os.environ.get("GP_GNXYZ16") != "0")
            elif fuse_up and i in (4, 7):
                pass          # applied by the upsample that follows
            elif pl and i not in (4, 7):   # the next consumer is a conv: planes into the buffer that conv's input just vacated
                self._gn(dst, W[f"{head}.c{i}_gw"], W[f"{head}.c{i}_gb"], ACT_GELU, buf, fused=True, out=cur.view(B, -1, 256), out_planes=True, rows=rows[r])
                dst = cur
            else:
                self._gn(dst, W[f"{head}.c{i}_gw"], W[f"{head}.c{i}_gb"], ACT_GELU, buf, fused=True, rows=rows[r])
            cur = dst

    def _resnet34(self, W, buf):
        """network/resnet.py:137-147 (ResNet.forward up to layer4), BasicBlock :38-52; eval BatchNorm folded into the
        convs, ReLU / residual+ReLU fused into the implicit-GEMM epilogues.  Returns (B,8,8,512)."""
        from ._lib import EPI_RELU, EPI_RES_RELU
        s = ops.resnet_stem(buf["roi_img"], W["rs.stem_w"], W["rs.stem_b"], buf["rs_stem"])
        x = ops.maxpool3x3s2(s, buf["rs1a"])
        for li, (planes, blocks, stride) in enumerate(synth.RESNET34_LAYERS, 1):
            for bi in range(blocks):
                q = f"rs{li}.{bi}."
                st = stride if bi == 0 else 1
                out = buf[f"rs{li}b"] if x is buf[f"rs{li}a"] or li > 1 and bi == 0 else buf[f"rs{li}a"]
                h = ops.conv2d_nhwc(x, W[q + "w1"], 3, 3, st, 1, out=buf[f"rs{li}c"], bias=W[q + "b1"], epilogue=EPI_RELU)
                if (q + "wd") in W:
                    res = ops.conv2d_nhwc(x, W[q + "wd"], 1, 1, st, 0, out=buf[f"rs{li}a"], bias=W[q + "bd"])
                    out = buf[f"rs{li}b"]
                else:
                    res = x
                x = ops.conv2d_nhwc(h, W[q + "w2"], 3, 3, 1, 1, out=out, bias=W[q + "b2"], epilogue=EPI_RES_RELU, residual=res)
        return x

    def _launch_all(self, B, plan):
        prev = ops.CO_SCHEDULED
        ops.CO_SCHEDULED = self.inflight > 1      # tile choice only; the launch sequence is the same in both modes
        try:
            self._launch_seq(B, plan)
        finally:
            ops.CO_SCHEDULED = prev

    def _launch_seq(self, B, plan):
        W, buf, cfg = self._packed, plan["buf"], self.cfg
        dims, depths = cfg.convnext_dims, cfg.convnext_depths
        ops.mask_resize_nearest(buf["roi_mask"], buf["mask_out"])
        if cfg.main_backbone == "resnet34":
            feat = self._resnet34(W, buf)
            dims, depths = (512,), ()
        else:
            # ---- ConvNeXt trunk (network/backbone.py:36-46)
            x = ops.convnext_stem(buf["roi_img"], W["stem.w"], W["stem.b"], W["stem.ln_w"], W["stem.ln_b"], buf["x0"])
        for s, (d, n) in enumerate(zip(dims, depths)):
            if s > 0:
                t = ops.layernorm(x, W[f"ds{s}.ln_w"], W[f"ds{s}.ln_b"], buf[f"dsn{s}"], out_planes=self.split_gemm)
                x = ops.conv2d_nhwc(t, W[f"ds{s}.w"], 2, 2, 2, 0, out=buf[f"x{s}"], bias=W[f"ds{s}.b"], x_planes=self.split_gemm,
                                    out16=buf.get(f"x{s}h"))
            x2d = x.view(-1, d)
            xh = buf.get(f"x{s}h")          # fp32 residual stream (cfg.res_fp32): x is fp32, the branch reads this fp16 copy
            xin = x if xh is None else xh
            for b in range(n):
                q = f"s{s}b{b}."
                if (q + "fc1_wg") in W and x2d.shape[0] % 256 == 0 and x.shape[1] % 4 == 0 and x.shape[2] % 16 == 0:
                    t = ops.dwconv7_raw_stats(x, W[q + "dw_w"], W[q + "dw_b"], buf[f"t{s}"], buf["ln_stats"])
                    ops.gemm(t.view(-1, d), W[q + "fc1_wg"], buf[f"h{s}"], bias=W[q + "fc1_cb"], epilogue=EPI_LNFOLD_GELU,
                             ln=(buf["ln_stats"], W[q + "fc1_cs"], d // 128, 1e-6))
                    ops.gemm(buf[f"h{s}"], W[q + "fc2_w"], x2d, bias=W[q + "fc2_b"], epilogue=EPI_SCALE_RES,
                             gamma=W[q + "gamma"], residual=x2d)
                    continue
                t = ops.dwconv_ln(xin, W[q + "dw_w"], W[q + "dw_b"], W[q + "ln_w"], W[q + "ln_b"], buf[f"t{s}"], 7, out_planes=self.split_gemm)
                if (q + "fc2_wp") in W and x2d.shape[0] % 256 == 0 and B >= cfg.fuse_mlp_min_batch and (d != 512 or x2d.shape[0] >= 32768):
                    ops.convnext_mlp(t.view(-1, d), W[q + "fc1_w"], W[q + "fc1_b"], W[q + "fc2_wp"], W[q + "fc2_b"],
                                     W[q + "gamma"], x2d, x2d)
                    continue
                # every GEMM-class launch may pull the weights of a later one towards the caches while it runs
                # (gp_gemm_desc.prefetch: a hint; the 128x128-tile GEMMs run 10-25 % longer on weights that come from HBM)
                # (split-operand mode: fc1 writes the hidden tensor as the fp16 planes fc2 reads -- no fp32 round trip, no split pass)
                pl = self.split_gemm
                ops.gemm(t.view(-1, d), W[q + "fc1_w"], buf[f"h{s}"], bias=W[q + "fc1_b"], epilogue=EPI_GELU, prefetch=W[q + "fc2_w"],
                         x_planes=pl, out_planes=pl)
                ops.gemm(buf[f"h{s}"], W[q + "fc2_w"], x2d, bias=W[q + "fc2_b"], epilogue=EPI_SCALE_RES,
                         gamma=W[q + "gamma"], residual=x2d, x_planes=pl, out16=None if xh is None else xh.view(-1, d),
                         prefetch=W.get(f"ds{s + 1}.w") if b == n - 1 else None)
        if cfg.main_backbone == "convnext":
            feat = x                                # (B,8,8,1024)
        fc = dims[-1]
        feat2d = feat.view(B * 64, fc)
        ops.size_head(feat.view(B, 64, fc), W["size.w1"], W["size.b1"], W["size.w2"], W["size.b2"], buf["mean_size"], buf["size"], buf["size_scratch"])
        self._xyz_head(W, "xyz_nocs_head", feat2d, B, buf, buf["nocs_nchw"], buf["nocs_nhwc4"])
        self._seq_encoder(B, plan)
        cat2d = buf["feat_cat"].view(B * 64, 512)
        ops.gemm(feat2d, W["red.w"], cat2d, bias=W["red.b"], ldc=512)
        self._xyz_head(W, "xyz_deform_head", cat2d, B, buf, buf["ivfc_nchw"], buf["ivfc_nhwc4"])
        self._seq_pnp(B, plan)

    def _seq_encoder(self, B, plan, only_layer=None, weights_of=None):
        """nocs_nhwc4 -> right half of feat_cat.  MAPEncoder (network/conv_pnp_net.py:303-332) or MAPTransformerEncoer.
        only_layer (tests): run DCNv3_C layer `only_layer` alone on buf["e_o{only_layer-1}"] (with the weights of layer
        `weights_of`, default its own) and stop before its GroupNorm."""
        W, buf, cfg = self._packed, plan["buf"], self.cfg
        cat2d = buf["feat_cat"].view(B * 64, 512)
        prev = None
        if cfg.nocsmap_encoder == "att":
            # ---- MAPTransformerEncoer (network/attention_pnp_net.py:143-157): 64 tokens x 256, 3 pre-norm ViT blocks
            x = buf["a_x"]
            ops.patchify_xyz(buf["nocs_nhwc4"], buf["a_patch"], B, cfg.out_res, 8)
            ops.gemm(buf["a_patch"], W["att.pe_w"], x, bias=W["att.pe_b"], epilogue=EPI_SCALE_RES, gamma=W["att.ones"],
                     residual=buf["a_pos"])                                   # proj(x) + bias + pos_embed
            for i in range(3):
                q = f"att{i}."
                h = ops.layernorm(x, W[q + "norm1_w"], W[q + "norm1_b"], buf["a_h"], eps=1e-5)
                ops.gemm(h, W[q + "qkv_w"], buf["a_qkv"])
                ops.attention64(buf["a_qkv"], buf["a_att"], B, 8)
                ops.gemm(buf["a_att"], W[q + "proj_w"], x, bias=W[q + "proj_b"], epilogue=EPI_SCALE_RES, gamma=W["att.ones"], residual=x)
                h = ops.layernorm(x, W[q + "norm2_w"], W[q + "norm2_b"], buf["a_h"], eps=1e-5)
                ops.gemm(h, W[q + "fc1_w"], buf["a_mlp"], bias=W[q + "fc1_b"], epilogue=EPI_GELU)
                ops.gemm(buf["a_mlp"], W[q + "fc2_w"], x, bias=W[q + "fc2_b"], epilogue=EPI_SCALE_RES, gamma=W["att.ones"], residual=x)
            ops.layernorm(x, W["att.norm_w"], W["att.norm_b"], cat2d[:, 256:], eps=1e-5, ldy=512)   # -> right half of feat_cat
        for li, r in enumerate((64, 32, 16) if cfg.nocsmap_encoder == "conv" else ()):
            q = f"enc{li}."
            ro = r // 2
            if only_layer is not None:
                if li != only_layer:
                    continue
                prev = buf[f"e_o{li - 1}"]
                if weights_of is not None:
                    q = f"enc{weights_of}."
            if cfg.use_dcn == "dcnv3":
                xin = buf[f"e_in{li}"]
                # layer 0 in fp16 mode: only the offset / mask branch below, then ONE launch from the 3-channel map to e_o0 (gp_dcnv3_xyz_project)
                xyz0 = li == 0 and plan.get("enc0_xyz") and only_layer is None
                # otherwise the full-resolution projection of every crop: one launch over all groups
                if xyz0:
                    # the reference's im2col_step rule (dcnv3_cuda.cu:46-49) is about ONE batch: checked here, per coupling group, as its gather would
                    nb = B if (plan.get("ragged") or not (self.dcn_couple and B > self.dcn_couple)) else self.dcn_couple
                    if nb % min(nb, 256):
                        raise RuntimeError(f"gp_dcnv3_forward: batch({nb}) must divide im2col_step({min(nb, 256)})")
                elif li == 0:
                    ops.pointwise_k3(buf["nocs_nhwc4"], W[q + "fold_w"], W[q + "fold_b"], buf[f"e_proj{li}"].view(-1, 256))
                else:
                    ops.gemm(prev.view(-1, 256), W[q + "fold_w"], buf[f"e_proj{li}"].view(-1, 256), bias=W[q + "fold_b"])
                if plan.get("ragged"):
                    # several batches of ANY sizes (the detections of several frames) in one launch each: output row j of the quarter-size
                    # offset / mask grid IS global output pixel j whatever the batch structure -- only the dw3x3 branch has to know that
                    # the rows of a batch are the flat prefix of THAT batch's full-resolution pixels (device table buf["grp"]); the
                    # conv1x1 in front of it runs over every crop's rows (the prefixes lie somewhere in them)
                    if li == 0:
                        ops.pointwise_k3(buf["nocs_nhwc4"], W[q + "conv_w"], W[q + "conv_b"], xin.view(-1, 256))
                    else:
                        ops.gemm(prev.view(-1, 256), W[q + "conv_w"], xin.view(-1, 256), bias=W[q + "conv_b"])
                    ops.dwconv_ln_groups(xin, W[q + "dw_w"], W[q + "dw_b"], W[q + "ln_w"], W[q + "ln_b"], buf[f"e_x1{li}"], 3, buf["grp"], act=ACT_GELU)
                    ops.gemm(buf[f"e_x1{li}"], W[q + "om_w"], buf[f"e_om{li}"], bias=W[q + "om_b"])
                    if not xyz0:
                        ops.dcnv3_forward_into(buf[f"e_proj{li}"], buf[f"e_om{li}"], buf[f"e_om{li}"][:, 72:], buf[f"e_g{li}"], 3, 2, 1, 1, 4, 64, 1.0,
                                               off_ld=OM_LD, mask_ld=OM_LD, mask_is_logits=True)
                # the offset / mask branch and the gather see ONE batch's flat prefix at a time (grouped launches: a group =
                # one batch of dcn_couple crops; otherwise the whole forward is the one group)
                Bg = self.dcn_couple if (self.dcn_couple and B > self.dcn_couple) else B
                if plan.get("ragged"):
                    Bg = B + 1          # (no per-batch launches: range() below is empty)
                if B % Bg and not plan.get("ragged"):
                    raise ValueError(f"batch {B} is not a multiple of dcn_couple = {Bg}")
                for g0 in range(0, B if not plan.get("ragged") else 0, Bg):
                    gs = slice(g0, g0 + Bg)
                    nq = Bg * ro * ro      # rows of the full-resolution offset/mask grid the gather consumes
                    # + one image row of halo for the 3x3 depth-wise conv; rounded up to 16 rows so that the few-crop case (88 / 296 rows at one crop) takes the
                    # small-M GEMM kernel (M % 16 == 0) instead of a 128 x 128 tile (the extra rows are rows of the same map, computed and not read)
                    npre = min(Bg * r * r, (nq + r + 8 + 15) // 16 * 16)
                    xin_g = xin[gs]
                    if li == 0:
                        ops.pointwise_k3(buf["nocs_nhwc4"][g0 * r * r:][:npre], W[q + "conv_w"], W[q + "conv_b"], xin_g.view(-1, 256)[:npre])
                    else:
                        ops.gemm(prev[gs].view(-1, 256)[:npre], W[q + "conv_w"], xin_g.view(-1, 256)[:npre], bias=W[q + "conv_b"])
                    x1_g = buf[f"e_x1{li}"][g0 * r * r // 4:(g0 + Bg) * r * r // 4]
                    om_g = buf[f"e_om{li}"][g0 * r * r // 4:(g0 + Bg) * r * r // 4]
                    ops.dwconv_ln(xin_g, W[q + "dw_w"], W[q + "dw_b"], W[q + "ln_w"], W[q + "ln_b"], x1_g, 3, act=ACT_GELU, n_pixels=nq)
                    ops.gemm(x1_g, W[q + "om_w"], om_g, bias=W[q + "om_b"])
                    if not xyz0:
                        ops.dcnv3_forward_into(buf[f"e_proj{li}"][gs], om_g, om_g[:, 72:], buf[f"e_g{li}"][gs], 3, 2, 1, 1, 4, 64, 1.0,
                                               off_ld=OM_LD, mask_ld=OM_LD, mask_is_logits=True)
                y = buf[f"e_o{li}"]
                if xyz0:     # the rows of e_om0 of all groups are contiguous, output row j is global output pixel j: one launch for every crop
                    ops.dcnv3_xyz_project(buf["nocs_nhwc4"], buf["e_om0"], W[q + "xyz_m"], W[q + "xyz_b"], y.view(-1, 256),
                                          gn=self._gnarg(buf, ro * ro, 32))
                    self._gn(y, W[q + "gn_w"], W[q + "gn_b"], ACT_RELU, buf, fused=True, rows=32)
                    prev = y
                    continue
                ops.gemm(buf[f"e_g{li}"].view(-1, 256), W[q + "out_w"], y.view(-1, 256), bias=W[q + "out_b"],
                         gn=self._gnarg(buf, ro * ro))
                fused = True
                if only_layer is not None:
                    return
            else:
                y = buf[f"e_o{li}"]
                fused = li > 0
                if li == 0:
                    ops.xyz_conv3x3_s2(buf["nocs_nhwc4"], W[q + "conv_w"], y, B, r)
                else:
                    ops.conv2d_nhwc(prev, W[q + "conv_w"], 3, 3, 2, 1, out=y, gn=self._gnarg(buf, ro * ro))
            if li < 2:
                self._gn(y, W[q + "gn_w"], W[q + "gn_b"], ACT_RELU, buf, fused=fused)
                prev = y
            else:   # last layer normalises straight into the right half of feat_cat (PoseNet.py:193)
                self._gn(y, W[q + "gn_w"], W[q + "gn_b"], ACT_RELU, buf, out=cat2d[:, 256:], ldy=512, fused=fused)

    def _seq_pnp(self, B, plan):
        """ivfc_nhwc4 + roi_coord_2d (+ mask_out) -> pred_rot / pred_t / rot / trans: ConvPnPNet (network/conv_pnp_net.py:137-201)
        + pose decode."""
        W, buf, cfg = self._packed, plan["buf"], self.cfg
        R = cfg.out_res
        k = FLAT_OPS[cfg.flat_op]
        if cfg.pnp_head == "att":
            self._seq_att_pnp(B, plan)
            return
        if cfg.mask_attention_type == "mul":     # coor_feat * mask_attention (conv_pnp_net.py:146-154), applied while the conv stages its input
            p = ops.pnp_conv1_masked(buf["ivfc_nhwc4"], buf["roi_coord_2d"], buf["mask_out"], W["pnp.c0_w"], buf["p0"], B, R)
        else:
            p = ops.pnp_conv1(buf["ivfc_nhwc4"], buf["roi_coord_2d"], W["pnp.c0_w"], buf["p0"], B, R)
        self._gn(p, W["pnp.g0_w"], W["pnp.g0_b"], ACT_RELU, buf)
        for li in (1, 2):
            hw = nxt_hw = (32 >> li) ** 2
            rows = self._gnrows(B * hw, 128, 9 * 128, hw)
            nxt = ops.conv2d_nhwc(p, W[f"pnp.c{li}_w"], 3, 3, 2, 1, out=buf[f"p{li}"], gn=self._gnarg(buf, hw, rows),
                                  prefetch=W["pnp.c2_w"] if li == 1 else W["pnp.fc1_w"])     # (fc1: the first 4 of its 33 MB; all of it pooled)
            self._gn(nxt, W[f"pnp.g{li}_w"], W[f"pnp.g{li}_b"], ACT_RELU, buf, fused=True, rows=rows)
            p = nxt
        if k:    # flat_op avg / avg-max / avg-max-min: [mean | max | min] over the 64 pixels, fc1 at K = 128 k
            x = ops.pool_mmm(p.view(B, 64, 128), buf["pooled"], k)
        else:
            x = p.view(B, 8192)
        ops.gemm(x, W["pnp.fc1_w"], buf["fc1"], bias=W["pnp.fc1_b"], epilogue=EPI_LRELU, prefetch=W["pnp.fc2_w"])
        ops.gemm(buf["fc1"], W["pnp.fc2_w"], buf["hh"], bias=W["pnp.fc2_b"], epilogue=EPI_LRELU, M=B, K=1024, ldx=2048, prefetch=W["pnp.fc2z_w"])
        ops.gemm(buf["fc1"][:, 1024:], W["pnp.fc2z_w"], buf["hz"], bias=W["pnp.fc2z_b"], epilogue=EPI_LRELU, M=B, K=1024, ldx=2048)
        rot_dim, kind, is_allo = ROT_TYPES[cfg.r_type]
        ops.pose_tail_rt(buf["hh"], buf["hz"], 256, W, buf["cam_K"], buf["bbox_center"], buf["resize_ratio"], buf["roi_wh"],
                         cfg.dataset == "wild6d", cfg.t_type == "site", rot_dim, kind, is_allo, buf, B)

    def _seq_att_pnp(self, B, plan):
        """AttentionPnPNet.forward (network/attention_pnp_net.py:79-124) on cat(ivfc, roi_coord_2d) (PoseNet.py:196-197): patch embed +
        pos_embed, 3 pre-norm ViT blocks (192 = 8 heads x 24), LayerNorm, flatten(1), the exact-GELU fc tail, then the pose decode."""
        W, buf, cfg = self._packed, plan["buf"], self.cfg
        x = buf["p_x"]
        ops.patchify_pnp(buf["ivfc_nhwc4"], buf["roi_coord_2d"], buf["p_patch"], B, cfg.out_res, 8)
        ops.gemm(buf["p_patch"], W["apn.pe_w"], x, bias=W["apn.pe_b"], epilogue=EPI_SCALE_RES, gamma=W["apn.ones"],
                 residual=buf["p_pos"])                                   # proj(x) + bias + pos_embed
        for i in range(3):
            q = f"apn{i}."
            h = ops.layernorm(x, W[q + "norm1_w"], W[q + "norm1_b"], buf["p_h"], eps=1e-5)
            ops.gemm(h, W[q + "qkv_w"], buf["p_qkv"])
            ops.attention64_hd(buf["p_qkv"], buf["p_att"], B, 8, 24)
            ops.gemm(buf["p_att"], W[q + "proj_w"], x, bias=W[q + "proj_b"], epilogue=EPI_SCALE_RES, gamma=W["apn.ones"], residual=x)
            h = ops.layernorm(x, W[q + "norm2_w"], W[q + "norm2_b"], buf["p_h"], eps=1e-5)
            ops.gemm(h, W[q + "fc1_w"], buf["p_mlp"], bias=W[q + "fc1_b"], epilogue=EPI_GELU)
            ops.gemm(buf["p_mlp"], W[q + "fc2_w"], x, bias=W[q + "fc2_b"], epilogue=EPI_SCALE_RES, gamma=W["apn.ones"], residual=x,
                     prefetch=W["pnp.fc1_w"] if i == 2 else None)
        ops.layernorm(x, W["apn.norm_w"], W["apn.norm_b"], buf["p_flat"], eps=1e-5)
        ops.gemm(buf["p_flat"].view(B, 64 * 192), W["pnp.fc1_w"], buf["fc1"], bias=W["pnp.fc1_b"], epilogue=EPI_GELU, prefetch=W["pnp.fc2_w"])
        ops.gemm(buf["fc1"], W["pnp.fc2_w"], buf["hh"], bias=W["pnp.fc2_b"], epilogue=EPI_GELU, M=B, K=1024, ldx=2048, prefetch=W["pnp.fc2z_w"])
        ops.gemm(buf["fc1"][:, 1024:], W["pnp.fc2z_w"], buf["hz"], bias=W["pnp.fc2z_b"], epilogue=EPI_GELU, M=B, K=1024, ldx=2048)
        rot_dim, kind, is_allo = ROT_TYPES[cfg.r_type]
        ops.pose_tail_rt(buf["hh"], buf["hz"], 256, W, buf["cam_K"], buf["bbox_center"], buf["resize_ratio"], buf["roi_wh"],
                         cfg.dataset == "wild6d", cfg.t_type == "site", rot_dim, kind, is_allo, buf, B)

    # ------------------------------------------------------------------ public API
    _INPUT_KEYS = ("roi_img", "roi_mask", "roi_coord_2d", "cam_K", "roi_wh", "bbox_center", "resize_ratio", "mean_size")

    def stream(self, slot=0):
        """The stream slot `slot`'s hipGraph is launched on (None before its first use / without use_graph)."""
        return self._streams.get(slot)

    def ensure_stream(self, slot=0, device="cuda"):
        """As stream(), creating it if need be (callers that queue work in front of the slot's next forward)."""
        if slot not in self._streams:
            self._streams[slot] = torch.cuda.Stream(device=torch.device(device))
        return self._streams[slot]

    @torch.no_grad()
    def forward_device(self, data, device="cuda", slot=0, wait=True, groups=None):
        """Runs the path and returns views of the static output buffers, all on the device (no D->H sync).

        groups: a list of batch sizes summing to the crop count -- the crops are the concatenated inputs of len(groups) separate
        ``forward`` calls of the reference (the detections of several frames, evaluation/evaluate.py:89-114) and every batch keeps its own
        DCNv3 prefix coupling, in ONE launch sequence whose length does not depend on the number of batches.  The
        total is padded to a bucket size (RAGGED_BUCKETS) with one-crop batches so that a few hipGraphs serve every frame set.

        slot / wait: independent batches in flight.  Every slot owns its buffers, hipGraph and stream (the packed
        weights are shared); with ``wait=False`` the calling stream is not made to wait for the result, so forwards
        of different slots overlap on the device -- the launches that cannot fill 256 CUs on their own (the 8x8 / 16x16
        stages, the small heads, kernel tails) run beside another batch's.  The caller then orders its reads after
        ``net.stream(slot)`` (or a device synchronise)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("givepose_amd.PoseNet runs on the HIP device only (no CPU path)")
        if slot >= max(self.inflight, 1):
            raise ValueError(f"slot {slot} needs PoseNet(..., inflight>={slot + 1})")
        _lib.load()
        if self._packed is None:
            self._pack(device)
        B = data["roi_img"].shape[0]
        n_real = B
        if groups is not None:
            groups = [int(g) for g in groups]
            if not groups or min(groups) < 1 or sum(groups) != B:
                raise ValueError(f"groups {groups} must be positive batch sizes summing to the {B} crops")
            if self.cfg.nocsmap_encoder != "conv" or self.cfg.use_dcn != "dcnv3":
                groups = None           # nothing couples the crops of a batch: the plain forward IS the multi-frame forward
            else:
                B = self.ragged_bucket(n_real)
        cur = torch.cuda.current_stream()
        if self.use_graph:
            # hipGraph capture is not permitted on the legacy default stream: the graph path owns a stream (per slot)
            if slot not in self._streams:
                self._streams[slot] = torch.cuda.Stream(device=device)
            run_stream = self._streams[slot]
            run_stream.wait_stream(cur)
        else:
            run_stream = cur
        with torch.cuda.stream(run_stream):
            plan = self._plan(B, device, slot, ragged=groups is not None)   # a new plan's buffers belong to the stream that will use them
            buf = plan["buf"]
            for k in self._INPUT_KEYS:
                src = data[k]
                if src.data_ptr() != buf[k].data_ptr():
                    buf[k][:n_real].copy_(src.reshape((n_real,) + tuple(buf[k].shape[1:])), non_blocking=True)
                    if src.is_cuda and run_stream is not cur:
                        src.record_stream(run_stream)   # the caller may free `src` while this copy is still queued
            if groups is not None:
                gh = buf["grp_host"]
                if plan.get("grp_event") is not None:
                    plan["grp_event"].synchronize()     # the previous launch's table copy has left the pinned buffer
                i = 0
                for g in groups:
                    gh[i:i + g] = i
                    i += g
                gh[n_real:] = torch.arange(n_real, B, dtype=torch.int32)
                buf["grp"].copy_(gh, non_blocking=True)
                plan["grp_event"] = torch.cuda.Event()
                plan["grp_event"].record(run_stream)
            if self.use_graph and plan["warm"]:
                lib = _lib.load()
                sp = ctypes.c_void_p(run_stream.cuda_stream)
                if plan["graph"] is None:
                    _lib.check(lib.gp_graph_begin(sp), "gp_graph_begin")
                    _lib._capturing += 1
                    try:
                        self._launch_all(B, plan)
                    finally:
                        _lib._capturing -= 1
                        ge = ctypes.c_void_p()
                        rc = lib.gp_graph_end(sp, ctypes.byref(ge))
                    _lib.check(rc, "gp_graph_end")
                    plan["graph"] = ge
                _lib.check(lib.gp_graph_launch(plan["graph"], sp), "gp_graph_launch")
            else:
                self._launch_all(B, plan)
                plan["warm"] = True
        if run_stream is not cur and wait:
            cur.wait_stream(run_stream)
        n = n_real
        feat = buf.get(f"x{len(self.cfg.convnext_dims) - 1}")
        return {"rot": buf["rot_ego"].view(B, 3, 3)[:n], "trans": buf["trans"][:n], "size": buf["size"][:n], "mask": buf["mask_out"][:n],
                "nocs_coor": buf["nocs_nchw"][:n], "ivfc_coor": buf["ivfc_nchw"][:n], "rot6d": None if buf["rot6d"] is None else buf["rot6d"][:n],
                "pred_rot": buf["pred_rot"][:n], "pred_t": buf["pred_t"][:n],
                "rot_allo": buf["rot_allo"].view(B, 3, 3)[:n], "feat": None if feat is None else feat[:n],
                "feat_cat": buf["feat_cat"][:n]}

    # ---- sub-sequences of the path, eager, for the per-module golden vectors (tests/test_hip_modules.py); every one
    #      runs exactly the launches forward_device runs for that module, on the same plan buffers
    def _module_plan(self, B, device):
        device = torch.device(device)
        _lib.load()
        if self._packed is None:
            self._pack(device)
        return self._plan(B, device, 0)

    @torch.no_grad()
    def run_xyz_head(self, head, feat_nchw, device="cuda"):
        """TopDownXyzHead.forward (network/xyz_head.py:349-366): (B,Cin,8,8) -> (B,3,64,64) fp32; head in
        {"xyz_nocs_head", "xyz_deform_head"}."""
        B, C = feat_nchw.shape[:2]
        plan = self._module_plan(B, device)
        buf = plan["buf"]
        x = feat_nchw.to(device).permute(0, 2, 3, 1).reshape(B * 64, C).to(self.compute_dtype).contiguous()
        key = "nocs" if head == "xyz_nocs_head" else "ivfc"
        self._xyz_head(self._packed, head, x, B, buf, buf[key + "_nchw"], buf[key + "_nhwc4"])
        return buf[key + "_nchw"].clone()

    @torch.no_grad()
    def run_map_encoder(self, coor_nchw, device="cuda"):
        """MAPEncoder.forward (network/conv_pnp_net.py:303-332) / MAPTransformerEncoer: (B,3,64,64) -> (B,256,8,8) fp32."""
        B = coor_nchw.shape[0]
        plan = self._module_plan(B, device)
        buf = plan["buf"]
        buf["nocs_nhwc4"].zero_()
        buf["nocs_nhwc4"][:, :3] = coor_nchw.to(device).float().permute(0, 2, 3, 1).reshape(-1, 3)
        self._seq_encoder(B, plan)
        return buf["feat_cat"].view(B, 8, 8, 512)[..., 256:].permute(0, 3, 1, 2).float().contiguous()

    @torch.no_grad()
    def run_dcnv3_c(self, layer, x_nchw, device="cuda", weights_of=None):
        """DCNv3_C.forward (network/dcnv3.py:32-38 -> ops_dcnv3/modules/dcnv3.py:318-356) at the geometry of MAPEncoder
        layer `layer` in {1, 2} (r = 32 / 16) with the weights of layer `weights_of` (default `layer`):
        (B,256,r,r) -> (B,256,r/2,r/2) fp32, before the layer's GroupNorm."""
        assert self.cfg.use_dcn == "dcnv3" and layer in (1, 2) and weights_of in (None, 1, 2)
        B = x_nchw.shape[0]
        plan = self._module_plan(B, device)
        buf = plan["buf"]
        buf[f"e_o{layer - 1}"].copy_(x_nchw.to(device).permute(0, 2, 3, 1).to(self.compute_dtype))
        self._seq_encoder(B, plan, only_layer=layer, weights_of=weights_of)
        return buf[f"e_o{layer}"].permute(0, 3, 1, 2).float().contiguous()

    @torch.no_grad()
    def run_pnp(self, x_nchw, data, device="cuda", mask=None):
        """ConvPnPNet.forward (network/conv_pnp_net.py:137-201) -- AttentionPnPNet.forward (network/attention_pnp_net.py:119-124) with
        pnp_head='att' -- on x = cat(coor, roi_coord_2d) (B,5,64,64): returns
        (pred_rot (B,rot_dim), t (B,3)); `data` supplies the camera scalars the fused pose tail also reads.  mask (B,1,64,64):
        the mask_attention input, required when mask_attention_type='mul'."""
        B = x_nchw.shape[0]
        if self.cfg.mask_attention_type == "mul" and mask is None:
            raise ValueError("run_pnp: mask_attention_type='mul' needs the (B,1,64,64) mask")
        plan = self._module_plan(B, device)
        buf = plan["buf"]
        if mask is not None:
            buf["mask_out"].copy_(mask.reshape(buf["mask_out"].shape))
        for k in ("cam_K", "roi_wh", "bbox_center", "resize_ratio"):
            buf[k].copy_(data[k].reshape(buf[k].shape))
        buf["ivfc_nhwc4"].zero_()
        buf["ivfc_nhwc4"][:, :3] = x_nchw[:, :3].to(device).float().permute(0, 2, 3, 1).reshape(-1, 3)
        buf["roi_coord_2d"].copy_(x_nchw[:, 3:5])
        self._seq_pnp(B, plan)
        return buf["pred_rot"].clone(), buf["pred_t"].clone()

    def static_inputs(self, B, device="cuda", slot=0, ragged=False):
        """The plan's device-resident input buffers (fill these to skip the per-call H->D copies).  ragged: the buffers of the
        multi-frame plan that serves B crops (its first B rows; forward_device(..., groups=...) finds them in place)."""
        if self._packed is None:
            self._pack(torch.device(device))
        if ragged and self.cfg.nocsmap_encoder == "conv" and self.cfg.use_dcn == "dcnv3":
            buf = self._plan(self.ragged_bucket(B), torch.device(device), slot, ragged=True)["buf"]
            return {k: buf[k][:B] for k in self._INPUT_KEYS}
        return {k: self._plan(B, torch.device(device), slot)["buf"][k] for k in self._INPUT_KEYS}

    @torch.no_grad()
    def forward(self, data, device="cuda", do_loss=False, pred_scale=None, groups=None):
        """Reference signature (network/PoseNet.py:173).  groups (extension): see forward_device.

        do_loss=True is the reference's validation / train-time forward, values only (no gradient): the network reads
        ``data['roi_mask_deform']`` in the place of ``roi_mask`` and the pose is decoded by pose_from_predictions_train
        (gpl_pose_decode_train, a plain launch after the forward's graph), which keeps ``rot`` on the device.  The result feeds
        givepose_amd.PoseLoss."""
        if do_loss:
            return self._forward_do_loss(data, device, groups)[0]
        out = self.forward_device(data, device, groups=groups)
        # the reference returns rot as a CPU tensor (pose_from_pred_centroid_z.py:157) and fresh tensors
        return {"rot": out["rot"].cpu(), "trans": out["trans"].clone(), "size": out["size"].clone(),
                "mask": out["mask"].clone(), "nocs_coor": out["nocs_coor"].clone(), "ivfc_coor": out["ivfc_coor"].clone()}

    def _forward_do_loss(self, data, device, groups):
        """-> (the dict of forward(do_loss=True), the raw head outputs the pose was decoded from: pred_rot, pred_t, rot_allo, and
        feat_cat (B,512,8,8) fp32 NCHW, the input of xyz_deform_head: cat(conv_feat256, nocs_feat), network/PoseNet.py:192-193)."""
        from . import loss
        cfg = self.cfg
        out = self.forward_device({**data, "roi_mask": data["roi_mask_deform"]}, device, groups=groups)
        raw = {k: out[k].clone() for k in ("pred_rot", "pred_t", "rot_allo")}
        raw["feat_cat"] = out["feat_cat"].permute(0, 3, 1, 2).float().contiguous()
        raw["feat"] = out["feat"]      # NHWC (B,8,8,Cfeat), the backbone's output, in the forward's dtype
        rot, trans = loss.pose_decode_train(raw["pred_t"], raw["rot_allo"], data["cam_K"], data["bbox_center"], data["resize_ratio"],
                                            data["roi_wh"], t_site=cfg.t_type == "site", is_allo=ROT_TYPES[cfg.r_type][2], eps=1e-4)
        return {"rot": rot, "trans": trans, "size": out["size"].clone(), "mask": out["mask"].clone(),
                "nocs_coor": out["nocs_coor"].clone(), "ivfc_coor": out["ivfc_coor"].clone()}, raw

    @torch.no_grad()
    def head_grads(self, data, pose_loss, device="cuda", gout=None, groups=None):
        """The loss half of a training step: forward(do_loss=True), `pose_loss` (a givepose_amd.PoseLoss; `data` also holds the
        ground truth it reads), the loss gradient and the backward of the train-time pose decode, everything on the device.
        -> {"loss": the six terms, "output": the dict of forward(do_loss=True), "grads": {"rot6d", "pred_t", "size", "nocs_coor",
        "ivfc_coor"}}: the gradient of sum_k gout[k] * term_k (gout None: the total loss) at the tensors the heads emit -- the
        ConvPnPNet rotation vector, pred_t, the size head's output (pred_size = head + norm_mean_size, so d head = d size) and
        the two coordinate maps.  The backward pass stops at these tensors; `head_grads_pnp` carries it on through the pose head
        (ConvPnPNet), `head_grads_xyz` from there through xyz_deform_head and `head_grads_feat` through MAPEncoder, xyz_nocs_head
        and feat_reducer to the backbone's output and `head_grads_backbone` through the backbone to the image.  The size head is
        evaluated in eval mode here; `head_grads_feat` and what follows it take size_head= for the train-mode head and its backward.

        For an r_type whose raw vector is not decoded by rot6d_to_mat_batch (kind != 0 in config.ROT_TYPES: the fixed-axis 6d
        forms, quaternion, Euler) grads["rot6d"] is the gradient of the (B,3,3) allocentric rotation matrix `rot_allo` instead."""
        return self._head_grads(data, pose_loss, device, gout, groups)[0]

    def _head_grads(self, data, pose_loss, device, gout, groups, size_head=None):
        """-> (what head_grads returns, the forward's raw tensors of _forward_do_loss).  size_head ({"seed": s} or {"keep": mask}, from
        `head_grads_feat`): the size head runs in TRAIN mode on the forward's feat before the loss (`_size_head_train`), output["size"] and
        the Size term are taken at that prediction, raw gains "size_saved" and the result "size_head": {"outputs": {"size_raw", "keep"},
        "stats": {"mean", "var_unbiased"}}."""
        from . import loss
        cfg = self.cfg
        out, raw = self._forward_do_loss(data, device, groups)
        if size_head is not None:
            raw["size_saved"] = self._size_head_train(raw["feat"], data["mean_size"], size_head, device)
            out["size"] = raw["size_saved"]["size"]
        terms, g = pose_loss.value_and_grad(out, data, gout=gout)
        kind, is_allo = ROT_TYPES[cfg.r_type][1], ROT_TYPES[cfg.r_type][2]
        d = loss.pose_decode_train_backward(g["rot"], g["trans"], raw["pred_t"], raw["rot_allo"], data["cam_K"], data["bbox_center"],
                                            data["resize_ratio"], data["roi_wh"], rot6d=raw["pred_rot"] if kind == 0 else None,
                                            t_site=cfg.t_type == "site", is_allo=is_allo, eps=1e-4)
        res = {"loss": terms, "output": out,
               "grads": {"rot6d": d["rot6d"] if kind == 0 else d["rot_allo"], "pred_t": d["pred_t"], "size": g["size"],
                         "nocs_coor": g["nocs_coor"], "ivfc_coor": g["ivfc_coor"]}}
        if size_head is not None:
            sv = raw["size_saved"]
            res["size_head"] = {"outputs": {"size_raw": sv["out"], "keep": sv["keep"]}, "stats": {"mean": sv["mean"], "var_unbiased": sv["var_unbiased"]}}
        return res, raw

    # ------------------------------------------------------------------ the size head in train mode
    @staticmethod
    def _size_head_mask(size_head, who):
        """{"seed": s} or {"keep": mask} -> (keep, seed), one of them None."""
        if not isinstance(size_head, dict) or set(size_head) - {"seed", "keep"}:
            raise ValueError(f"{who}: size_head must be None, {{'seed': int}} or {{'keep': (B,F) uint8 mask}}, got {size_head!r}")
        keep, seed = size_head.get("keep"), size_head.get("seed")
        if (keep is None) == (seed is None):
            raise ValueError(f"{who}: exactly one of keep and seed must be given")
        return keep, seed

    def _size_head_train(self, feat_nhwc, mean_size, size_head, device):
        """The train-mode size head on the forward's own feat (NHWC, the forward's dtype, read in place) -> what size_forward_save saves,
        with "size" = out + mean_size / |mean_size| (network/PoseNet.py:199-202)."""
        from . import size_grad
        keep, seed = self._size_head_mask(size_head, "size_head")
        if feat_nhwc is None:
            raise NotImplementedError(f"size_head: main_backbone={self.cfg.main_backbone!r} -- the forward returns the backbone's output for "
                                      "the ConvNeXt backbone only")
        dev = torch.device(device)
        P = self._module_params_f32("size_head", size_grad.PARAM_KEYS, dev)
        return size_grad.size_forward_save(feat_nhwc, P, keep=keep, seed=seed, nhwc=True, mean_size=torch.as_tensor(mean_size).to(dev))

    @torch.no_grad()
    def size_head_backward(self, feat, g_size, keep=None, seed=None, device="cuda", return_saved=False):
        """Backward of the size head as the training loop runs it (SizeHead, network/pose_head.py:17-42, under network.train()): the head
        is recomputed in fp32 from feat (B,C,H,W) in TRAIN mode -- max over the map (of equal maxima the lowest index takes the gradient),
        conv1, BatchNorm1d on the statistics of these B crops (B >= 2), relu, Dropout(0.2), conv2 --, saving what the backward needs
        (gps_size_forward_save), then differentiated at that point from g_size (B,3) (gps_size_backward; pred_size = head +
        norm_mean_size, so d head = d size).
        The dropout mask is an input, exactly one of: keep, a (B,F) uint8 tensor (non-zero = kept), or seed, an int in [0, 2^64) for
        the counter-based rule of include/givepose_sizegrad.h (torch's generator cannot be matched).
        -> {"param_grads": {state_dict name: fp32 gradient in that parameter's own shape} for the six size_head.* parameters,
            "feat": (B,C,H,W), the gradient of the input feature (one non-zero per crop and channel),
            "outputs": {"size_raw": (B,3) the head's output, "keep": (B,F) the mask that was used},
            "stats": {"mean": (F,), "var_unbiased": (F,)}, what bn1.running_mean / running_var take (size_grad.bn_running_update)};
        return_saved adds "saved" (givepose_amd.size_grad.saved_shapes).
        No atomic: two calls give equal bits.  The weights are read at every call, as in `xyz_head_backward`."""
        from . import size_grad
        if (keep is None) == (seed is None):
            raise ValueError("size_head_backward: exactly one of keep and seed must be given")
        dev = torch.device(device)
        _lib.load()
        P = self._module_params_f32("size_head", size_grad.PARAM_KEYS, dev)
        feat = torch.as_tensor(feat).to(dev).to(torch.float32).contiguous()
        saved = size_grad.size_forward_save(feat, P, keep=keep, seed=seed)
        grads, g_feat = size_grad.size_backward(P, saved, torch.as_tensor(g_size).to(dev), feat.shape)
        res = {"param_grads": {"size_head." + k: v for k, v in grads.items()}, "feat": g_feat,
               "outputs": {"size_raw": saved["out"], "keep": saved["keep"]},
               "stats": {"mean": saved["mean"], "var_unbiased": saved["var_unbiased"]}}
        if return_saved:
            res["saved"] = saved
        return res

    # ------------------------------------------------------------------ backward through the pose head
    def _pnp_backward_supported(self, need_rot6d=False):
        """ConvPnPNet with flat_op 'flatten' and mask_attention_type 'none' | 'mul' is what gph_pnp_backward differentiates."""
        cfg = self.cfg
        if cfg.pnp_head != "conv":
            raise NotImplementedError(f"pnp_backward: pnp_head={cfg.pnp_head!r} -- only the ConvPnPNet head (pnp_head='conv') has a backward")
        if cfg.flat_op != "flatten":
            raise NotImplementedError(f"pnp_backward: flat_op={cfg.flat_op!r} -- only flat_op='flatten' has a backward (the pooled modes do not)")
        if cfg.mask_attention_type not in ("none", "mul"):
            raise NotImplementedError(f"pnp_backward: mask_attention_type={cfg.mask_attention_type!r} -- only 'none' and 'mul' have a backward")
        if need_rot6d and ROT_TYPES[cfg.r_type][1] != 0:
            raise NotImplementedError(f"head_grads_pnp: r_type={cfg.r_type!r} -- its raw vector is not decoded by rot6d_to_mat_batch, so head_grads "
                                      "has the gradient of rot_allo, not of pred_rot, and there is nothing to feed the pose head's backward")

    def _pnp_params_f32(self, device):
        """The pnp_net parameters as fp32 device tensors in the reference's own layout, from the state_dict (never from the packed
        fp16 / split-plane copies of the forward path).  The copies are kept until a parameter changes: the key holds every
        parameter's storage and version counter, so an in-place update (an optimiser step) or a replaced tensor is seen at the
        next call, whatever the module's dtype and device."""
        from . import pnp_grad
        device = torch.device(device)
        sd = self.state_dict()
        src = [sd["pnp_net." + k] for k in pnp_grad.PARAM_KEYS]
        key = (device, tuple((t.data_ptr(), t._version) for t in src))
        if self._pnp_f32 is None or self._pnp_f32[0] != key:
            self._pnp_f32 = (key, {k: t.detach().to(device=device, dtype=torch.float32).contiguous() for k, t in zip(pnp_grad.PARAM_KEYS, src)})
        return self._pnp_f32[1]

    @torch.no_grad()
    def pnp_backward(self, ivfc_coor, roi_coord_2d, g_pred_rot, g_pred_t, mask=None, device="cuda", return_saved=False):
        """Backward of the pose head (ConvPnPNet, network/conv_pnp_net.py:137-201) in fp32 on the device: the head is recomputed in
        fp32 from ivfc_coor (B,3,64,64) and roi_coord_2d (B,2,64,64) -- and mask (B,1,64,64), required with mask_attention_type='mul' and
        ignored with 'none' -- saving what the backward needs (gph_pnp_forward_save), then differentiated at that point from
        g_pred_rot (B,rot_dim) and g_pred_t (B,3) (gph_pnp_backward).
        -> {"param_grads": {state_dict name: fp32 gradient in that parameter's own shape and layout} for the 23 pnp_net.* tensors,
            "ivfc_coor": (B,3,64,64), the head's part of d ivfc_coor, "outputs": {"pred_rot", "pred_t"} of the fp32 recompute};
        return_saved adds "saved", the saved activations (givepose_amd.pnp_grad.saved_shapes).
        The weights are read at every call: a parameter updated in place between two calls is differentiated at its new value."""
        from . import pnp_grad
        self._pnp_backward_supported()
        cfg = self.cfg
        if cfg.mask_attention_type == "mul" and mask is None:
            raise ValueError("pnp_backward: mask_attention_type='mul' needs the (B,1,64,64) mask")
        dev = torch.device(device)
        _lib.load()
        m = None if cfg.mask_attention_type == "none" else torch.as_tensor(mask).to(dev)
        P = self._pnp_params_f32(dev)
        rot_dim = ROT_TYPES[cfg.r_type][0]
        saved = pnp_grad.pnp_forward_save(torch.as_tensor(ivfc_coor).to(dev), torch.as_tensor(roi_coord_2d).to(dev), P, mask=m, rot_dim=rot_dim)
        grads, g_ivfc = pnp_grad.pnp_backward(P, saved, torch.as_tensor(g_pred_rot).to(dev), torch.as_tensor(g_pred_t).to(dev), mask=m)
        res = {"param_grads": {"pnp_net." + k: v for k, v in grads.items()}, "ivfc_coor": g_ivfc,
               "outputs": {"pred_rot": saved["pred_rot"], "pred_t": saved["pred_t"]}}
        if return_saved:
            res["saved"] = saved
        return res

    @torch.no_grad()
    def head_grads_pnp(self, data, pose_loss, device="cuda", gout=None, groups=None):
        """`head_grads` carried on through the pose head: the same result, where grads["ivfc_coor"] is now the total -- the direct part
        of the sp2d_coor term plus what comes back through pnp_net from d pred_rot and d pred_t (the reference does not detach the map,
        network/PoseNet.py:195-197), added in that order --, grads["ivfc_coor_direct"] keeps the direct part, and "param_grads" holds
        the gradient of every pnp_net.* parameter (`pnp_backward` on the forward's own ivfc_coor, roi_coord_2d and mask)."""
        return self._head_grads_pnp(data, pose_loss, device, gout, groups)[0]

    def _head_grads_pnp(self, data, pose_loss, device, gout, groups, size_head=None):
        self._pnp_backward_supported(need_rot6d=True)
        res, raw = self._head_grads(data, pose_loss, device, gout, groups, size_head)
        g, out = res["grads"], res["output"]
        back = self.pnp_backward(out["ivfc_coor"], data["roi_coord_2d"], g["rot6d"], g["pred_t"], mask=out["mask"], device=device)
        g["ivfc_coor_direct"] = g["ivfc_coor"]
        g["ivfc_coor"] = g["ivfc_coor"] + back["ivfc_coor"]
        res["param_grads"] = back["param_grads"]
        return res, raw

    # ------------------------------------------------------------------ backward through a coordinate head
    _XYZ_HEADS = ("xyz_nocs_head", "xyz_deform_head")

    def _xyz_params_f32(self, head, device):
        """The parameters of one coordinate head as fp32 device tensors in the reference's own layout, from the state_dict, kept
        until a parameter changes (keyed on storage and version counter, as _pnp_params_f32)."""
        from . import xyz_grad
        device = torch.device(device)
        sd = self.state_dict()
        src = [sd[f"{head}.{k}"] for k in xyz_grad.PARAM_KEYS]
        key = (device, tuple((t.data_ptr(), t._version) for t in src))
        hit = self._xyz_f32.get(head)
        if hit is None or hit[0] != key:
            hit = (key, {k: t.detach().to(device=device, dtype=torch.float32).contiguous() for k, t in zip(xyz_grad.PARAM_KEYS, src)})
            self._xyz_f32[head] = hit
        return hit[1]

    @torch.no_grad()
    def xyz_head_backward(self, head, feat, g_coor, device="cuda", return_saved=False):
        """Backward of a coordinate head (TopDownXyzHead, network/xyz_head.py:195-366; head in {"xyz_nocs_head", "xyz_deform_head"}) in
        fp32 on the device: the head is recomputed in fp32 from feat (B,Cin,8,8) -- Cin 1024 for xyz_nocs_head (the backbone feature),
        512 for xyz_deform_head (feat_cat) --, saving what the backward needs (gpx_xyz_forward_save), then differentiated at that point
        from g_coor (B,3,64,64) (gpx_xyz_backward).
        -> {"param_grads": {state_dict name: fp32 gradient in that parameter's own shape and layout} for all 35 names of the head -- a
            features.N.gn.* entry IS the tensor object of its features.N.norm.* entry, as in the reference, where the two names are one
            Parameter with one .grad; there are 23 distinct tensors --,
            "feat": (B,Cin,8,8), the gradient of the input feature, "outputs": {"coor": (B,3,64,64)} of the fp32 recompute};
        return_saved adds "saved", the saved activations (givepose_amd.xyz_grad.saved_shapes).
        The weights are read at every call: a parameter updated in place between two calls is differentiated at its new value.
        Under set_backward_precision(..., xyz_heads="bf16") (`xyz_backward_precision`) the 3x3 layers' contractions of both passes take
        bf16-rounded operands (fp32 sums); parameters, saved tensors and results stay fp32."""
        from . import xyz_grad
        precision = self._xyz_backward_precision
        if head not in self._XYZ_HEADS:
            raise ValueError(f"xyz_head_backward: head {head!r}, expected one of {self._XYZ_HEADS}")
        dev = torch.device(device)
        _lib.load()
        P = self._xyz_params_f32(head, dev)
        Cin = P["features.0.weight"].shape[0]
        feat = torch.as_tensor(feat).to(dev)
        if feat.dim() != 4 or feat.shape[1] != Cin or feat.shape[2] != feat.shape[3]:
            raise ValueError(f"xyz_head_backward: feat {tuple(feat.shape)}, expected (B,{Cin},H0,H0)")
        feat = feat.to(torch.float32).contiguous()
        saved = xyz_grad.xyz_forward_save(feat, P, precision=precision)
        grads, g_feat = xyz_grad.xyz_backward(P, saved, feat, torch.as_tensor(g_coor).to(dev), precision=precision)
        pg = {f"{head}.{k}": v for k, v in grads.items()}
        for alias, k in xyz_grad.ALIASES.items():
            pg[f"{head}.{alias}"] = grads[k]
        res = {"param_grads": pg, "feat": g_feat, "outputs": {"coor": saved["coor"]}}
        if return_saved:
            res["saved"] = saved
        return res

    @torch.no_grad()
    def head_grads_xyz(self, data, pose_loss, device="cuda", gout=None, groups=None):
        """`head_grads_pnp` carried on through xyz_deform_head: the same result, where "param_grads" also holds the gradient of every
        xyz_deform_head.* parameter and grads gains "feat_cat" (B,512,8,8), the gradient of the head's input, and its halves (views of
        its channels) "conv_feat256" = 0..255 and "nocs_feat" = 256..511 (network/PoseNet.py:192-193).  The upstream gradient is the
        total grads["ivfc_coor"]; the input is the forward's own feat_cat in fp32 (`xyz_head_backward` on it).  The chain stops at
        feat_cat here: nocs_feat feeds back into nocs_coor through MAPEncoder, which `head_grads_feat` carries on."""
        return self._head_grads_xyz(data, pose_loss, device, gout, groups)[0]

    def _head_grads_xyz(self, data, pose_loss, device, gout, groups, size_head=None):
        res, raw = self._head_grads_pnp(data, pose_loss, device, gout, groups, size_head)
        back = self.xyz_head_backward("xyz_deform_head", raw["feat_cat"], res["grads"]["ivfc_coor"], device=device)
        res["param_grads"].update(back["param_grads"])
        g = res["grads"]
        g["feat_cat"] = back["feat"]
        g["conv_feat256"], g["nocs_feat"] = back["feat"][:, :256], back["feat"][:, 256:]
        return res, raw

    # ------------------------------------------------------------------ backward through the map encoder and to the backbone feature
    def _enc_backward_supported(self, who):
        """MAPEncoder with DCNv3 layers is what gpe_map_encoder_backward differentiates."""
        cfg = self.cfg
        if cfg.nocsmap_encoder != "conv":
            raise NotImplementedError(f"{who}: nocsmap_encoder={cfg.nocsmap_encoder!r} -- only the convolutional MAPEncoder "
                                      "(nocsmap_encoder='conv') has a backward, the transformer encoder ('att') does not")
        if cfg.use_dcn != "dcnv3":
            raise NotImplementedError(f"{who}: use_dcn={cfg.use_dcn!r} -- only the DCNv3 encoder (use_dcn='dcnv3') has a backward, the plain "
                                      "3x3 stride-2 conv encoder does not")

    def _module_params_f32(self, module, keys, device):
        """{key: fp32 device tensor} of `module`'s parameters from the state_dict, kept until one changes (keyed on storage and version
        counter, as _xyz_params_f32)."""
        device = torch.device(device)
        sd = self.state_dict()
        src = [sd[f"{module}.{k}"] for k in keys]
        key = (device, tuple((t.data_ptr(), t._version) for t in src))
        hit = self._enc_f32.get(module)
        if hit is None or hit[0] != key:
            hit = (key, {k: t.detach().to(device=device, dtype=torch.float32).contiguous() for k, t in zip(keys, src)})
            self._enc_f32[module] = hit
        return hit[1]

    def _enc_groups(self, B, groups):
        """The coupling batches of a forward over B crops: `groups` as given, else the forward's rule (dcn_couple chunks)."""
        if groups is not None:
            return [int(g) for g in groups]
        if self.dcn_couple and B > self.dcn_couple:
            if B % self.dcn_couple:
                raise ValueError(f"batch {B} is not a multiple of dcn_couple = {self.dcn_couple}")
            return [self.dcn_couple] * (B // self.dcn_couple)
        return [B]

    @torch.no_grad()
    def map_encoder_backward(self, coor, g_nocs_feat, groups=None, device="cuda", return_saved=False):
        """Backward of the map encoder (MAPEncoder with DCNv3 layers, network/conv_pnp_net.py:254-332) in fp32 on the device: the
        encoder is recomputed in fp32 from coor (B,3,R,R), R a multiple of 8 (64 in the network), saving what the backward needs
        (gpe_map_encoder_forward_save), then differentiated at that point from g_nocs_feat (B,256,R/8,R/8) (gpe_map_encoder_backward).
        groups: the coupling batches -- the crops whose DCNv3 layers shared one flat offset / mask buffer in the forward that ran
        (SURVEY.md 0.3); None is the forward's own rule: chunks of dcn_couple if that is set and B exceeds it, else one batch.
        -> {"param_grads": {state_dict name: fp32 gradient in that parameter's own shape} for the 48 differentiated nocs_encoder.*
            tensors (features.N.dcnv3.bn.* is never applied and has no entry, as its .grad stays None in the reference),
            "coor": (B,3,R,R), the gradient of the map, "outputs": {"nocs_feat": (B,256,R/8,R/8)} of the fp32 recompute};
        return_saved adds "saved", the list of the batches' saved activations (givepose_amd.enc_grad.saved_shapes).
        With `encoder_scatter` "atomic" (the default) d xp is scattered with fp32 atomics: two calls agree to rounding, not bit for
        bit (include/givepose_encgrad.h).  After `set_encoder_scatter("ordered")` d xp is an ordered sum and two calls give equal
        bits in every entry (include/givepose_encgrad_ordered.h)."""
        from . import enc_grad
        self._enc_backward_supported("map_encoder_backward")
        dev = torch.device(device)
        _lib.load()
        P = self._module_params_f32("nocs_encoder", enc_grad.PARAM_KEYS, dev)
        coor = torch.as_tensor(coor).to(dev).to(torch.float32).contiguous()
        groups = self._enc_groups(coor.shape[0], groups)
        saved = enc_grad.enc_forward_save(coor, P, groups=groups)
        grads, g_coor = enc_grad.enc_backward(P, saved, coor, torch.as_tensor(g_nocs_feat).to(dev), scatter=self._encoder_scatter)
        res = {"param_grads": {"nocs_encoder." + k: v for k, v in grads.items()}, "coor": g_coor,
               "outputs": {"nocs_feat": torch.cat([s["act"][2] for s in saved])}}
        if return_saved:
            res["saved"] = saved
        return res

    @torch.no_grad()
    def feat_reducer_backward(self, feat, g_conv_feat256, device="cuda"):
        """Backward of feat_reducer (a 1x1 conv with bias, Cfeat -> 256; network/PoseNet.py:191): feat (B,Cfeat,8,8) NCHW and
        g_conv_feat256 (B,256,8,8) -> {"param_grads": {"feat_reducer.weight", "feat_reducer.bias"}, "feat": (B,Cfeat,8,8)}."""
        from . import enc_grad
        dev = torch.device(device)
        _lib.load()
        P = self._module_params_f32("feat_reducer", ("weight", "bias"), dev)
        out = enc_grad.conv1x1_backward(torch.as_tensor(g_conv_feat256).to(dev), torch.as_tensor(feat).to(dev), P["weight"])
        return {"param_grads": {"feat_reducer.weight": out["dW"], "feat_reducer.bias": out["db"]}, "feat": out["dX"]}

    @_size_head_keyword("_head_grads_feat")
    def head_grads_feat(self, data, pose_loss, device="cuda", gout=None, groups=None):
        """`head_grads_xyz` carried on to the backbone's output: every entry the two share is the same bits, and
          * "param_grads" also holds the gradient of feat_reducer.*, of the 48 differentiated nocs_encoder.* tensors and of all 35
            names of xyz_nocs_head.*: every parameter outside the backbone and size_head;
          * grads["nocs_coor_direct"] keeps the loss's own part of d nocs_coor, grads["nocs_coor_from_encoder"] is what comes back
            through nocs_encoder from d nocs_feat (the reference does not detach the map, network/PoseNet.py:191-194) and
            grads["nocs_coor"] becomes the total: the two added in that order;
          * grads gains "feat_from_reducer" (feat_reducer's backward of d conv_feat256), "feat_from_nocs_head" (xyz_nocs_head's backward
            of the total d nocs_coor) and "feat", their sum in that order: (B,Cfeat,8,8) NCHW, the gradient at the backbone's output.
        Keyword-only option size_head= (`_size_head_keyword`).
        size_head=None (the default): the size head's contribution to d feat is NOT included and size_head.* has no gradient -- in train
        mode its BatchNorm1d normalises with batch statistics and its Dropout is random, neither of which the eval-mode forward computes,
        so a gradient at the forward that ran would not be the reference's.
        size_head={"seed": s} or {"keep": (B,F) uint8 mask}: the size head runs in TRAIN mode on the forward's feat before the loss
        (batch-statistics BatchNorm1d, Dropout(0.2) with that mask: `size_head_backward`), output["size"] and the Size term are taken at
        that prediction, and its backward is applied to grads["size"] (gps_size_backward on what the train-mode forward saved):
        "param_grads" gains the six size_head.* entries, grads gains "feat_from_size_head", grads["feat"] is reducer + nocs head + size
        head, added in that order, and the result gains "size_head": {"outputs": {"size_raw", "keep"}, "stats": {"mean",
        "var_unbiased"}}.
        `head_grads_backbone` carries the chain on through the backbone.
        The inputs are the forward's own tensors in fp32 (nocs_coor, and feat, which the forward keeps NHWC); `groups` is used for the
        forward and for the encoder's backward alike."""
        return self._head_grads_feat(data, pose_loss, device, gout, groups)

    @torch.no_grad()
    def _head_grads_feat(self, data, pose_loss, device="cuda", gout=None, groups=None, size_head=None):
        self._enc_backward_supported("head_grads_feat")
        res, raw = self._head_grads_xyz(data, pose_loss, device, gout, groups, size_head)
        g, out = res["grads"], res["output"]
        if raw["feat"] is None:
            raise NotImplementedError(f"head_grads_feat: main_backbone={self.cfg.main_backbone!r} -- the forward returns the backbone's "
                                      "output for the ConvNeXt backbone only")
        B = out["nocs_coor"].shape[0]
        enc =self.map_encoder_backward(out["nocs_coor"], g["nocs_feat"], groups=self._enc_groups(B, groups), device=device)
        g["nocs_coor_direct"], g["nocs_coor_from_encoder"] = g["nocs_coor"], enc["coor"]
        g["nocs_coor"] = g["nocs_coor"] + enc["coor"]
        feat = raw["feat"].permute(0, 3, 1, 2).float().contiguous()
        red = self.feat_reducer_backward(feat, g["conv_feat256"], device=device)
        head = self.xyz_head_backward("xyz_nocs_head", feat, g["nocs_coor"], device=device)
        for part in (red, enc, head):
            res["param_grads"].update(part["param_grads"])
        g["feat_from_reducer"], g["feat_from_nocs_head"] = red["feat"], head["feat"]
        g["feat"] = red["feat"] + head["feat"]
        if size_head is not None:
            from . import size_grad
            P = self._module_params_f32("size_head", size_grad.PARAM_KEYS, torch.device(device))
            sgrads, sfeat = size_grad.size_backward(P, raw["size_saved"], g["size"], feat.shape)
            res["param_grads"].update({"size_head." + k: v for k, v in sgrads.items()})
            g["feat_from_size_head"] = sfeat
            g["feat"] = g["feat"] + sfeat
        return res

    # ------------------------------------------------------------------ backward through the backbone
    def _backbone_backward_supported(self, who):
        """The ConvNeXt backbone is what gpb_backbone_backward differentiates."""
        if self.cfg.main_backbone != "convnext":
            raise NotImplementedError(f"{who}: main_backbone={self.cfg.main_backbone!r} -- only the ConvNeXt backbone (main_backbone='convnext') "
                                      "has a backward, the resnet34 throughput variant does not")

    @torch.no_grad()
    def backbone_backward(self, img, g_feat, device="cuda", return_saved=False):
        """Backward of the ConvNeXt backbone (timm convnext_base as called by network/backbone.py:36-46) in fp32 on the device: the
        backbone is recomputed in fp32 from img (B,3,S,S), S a multiple of 32 (256 in the network), saving what the backward needs
        (gpb_backbone_forward_save), then differentiated at that point from g_feat (B,Cfeat,S/32,S/32) (gpb_backbone_backward).
        drop_path is 0 and the backbone has neither BatchNorm nor Dropout: train mode computes this forward.
        -> {"param_grads": {state_dict name: fp32 gradient in that parameter's own shape} for every backbone.* tensor, in state_dict
            order, "img": (B,3,S,S), the gradient of the image, "outputs": {"feat": (B,Cfeat,S/32,S/32)} of the fp32 recompute};
        return_saved adds "saved" (givepose_amd.bb_grad.saved_shapes: 176.7 MB per crop for ConvNeXt-Base at 256 x 256).
        There is no atomic on this path: two calls give equal bits.  The fp32 parameters are cached as `_module_params_f32` caches them.
        Under set_backward_precision("bf16") the block contractions of both passes take bf16-rounded operands (fp32 sums); parameters,
        saved tensors and results stay fp32."""
        from . import bb_grad
        self._backbone_backward_supported("backbone_backward")
        dev = torch.device(device)
        _lib.load()
        P = self._module_params_f32("backbone", bb_grad.PARAM_KEYS(self.cfg), dev)
        img = torch.as_tensor(img).to(dev).to(torch.float32).contiguous()
        g_feat = torch.as_tensor(g_feat).to(dev).to(torch.float32).contiguous()
        saved, feat = bb_grad.backbone_forward_save(img, P, self.cfg, precision=self._backward_precision)
        grads, d_img = bb_grad.backbone_backward(P, saved, img, g_feat, self.cfg, precision=self._backward_precision)
        res = {"param_grads": {"backbone." + k: v for k, v in grads.items()}, "img": d_img, "outputs": {"feat": feat}}
        if return_saved:
            res["saved"] = saved
        return res

    @_size_head_keyword("_head_grads_backbone")
    def head_grads_backbone(self, data, pose_loss, device="cuda", gout=None, groups=None):
        """`head_grads_feat` carried on through the backbone to the image: every entry the two share is the same bits, and
          * "param_grads" also holds the gradient of every backbone.* parameter: with it every parameter outside size_head (and the
            never-applied nocs_encoder.features.N.bn.*) has its gradient;
          * grads gains "roi_img" (B,3,S,S), the gradient of the image crop.
        The upstream gradient is grads["feat"].  The backbone is differentiated at its own fp32 recompute from data["roi_img"]
        (`backbone_backward`), while the heads were differentiated at the forward's feat, which for an fp16 network is the fp16
        forward's: the two agree to the forward's precision, not bit for bit.
        Keyword-only option size_head=, as in `head_grads_feat`.  With None the size head's contribution to d feat is NOT included, for the reason given there;
        with a mask every parameter but the never-applied bn.* has its gradient and d feat is the reference's."""
        return self._head_grads_backbone(data, pose_loss, device, gout, groups)

    @torch.no_grad()
    def _head_grads_backbone(self, data, pose_loss, device="cuda", gout=None, groups=None, size_head=None):
        self._backbone_backward_supported("head_grads_backbone")
        self._enc_backward_supported("head_grads_backbone")
        option = {} if size_head is None else {"size_head": size_head}
        res = self.head_grads_feat(data, pose_loss, device, gout=gout, groups=groups, **option)
        back = self.backbone_backward(data["roi_img"], res["grads"]["feat"], device=device)
        res["param_grads"].update(back["param_grads"])
        res["grads"]["roi_img"] = back["img"]
        return res

    # ------------------------------------------------------------------ one training step
    @_accumulator_keywords("_train_step_accumulated")
    @torch.no_grad()
    def train_step(self, data, pose_loss, optimizer, device="cuda", groups=None, clip_norm=5.0, lr=None, size_head=None):
        """One iteration of the reference's loop (engine/train.py:113-129) for a single batch: `head_grads_backbone` (forward, the six
        loss terms, the backward chain to the image), then optimizer.step(param_grads, clip_norm=clip_norm, lr=lr) with a
        givepose_amd.optim.Ranger, Adam or AdamW built over this model (the only thing checked is `optimizer.model is self`, so any
        object with Ranger's `step` serves): clip_grad_norm_ at clip_norm (None: no clipping) fused into one optimiser step on
        the device.  The step ends with `params_updated()`, so the next forward repacks the updated weights (on the host: `_pack`).
        -> what `head_grads_backbone` returns (res["loss"] holds the six terms; the gradients in res["param_grads"] are left as computed,
        not scaled by the clip coefficient, which is in optimizer.scalars[1] next to the norm in optimizer.scalars[0]).
        The never-applied nocs_encoder.features.N.dcnv3.bn.* are not updated.  size_head=None (the default): the size head gets no
        gradient and is NOT updated, and its contribution to d feat is not included (`head_grads_feat`).
        size_head={"seed": s} or {"keep": mask}: the reference's iteration -- the size head runs in train mode, the Size term is taken at
        its prediction, size_head.* is stepped with everything else, and after the optimiser step size_head.bn1.running_mean /
        running_var / num_batches_tracked are updated on the device as nn.BatchNorm1d(momentum=0.1) updates them
        (gps_bn_running_update), followed by `params_updated()`, so the next eval-mode forward folds the new statistics.  A fresh seed
        per step is the caller's business.
        Keyword-only options accumulator=None, accumulate=1, micro_step=0, group=None (`_accumulator_keywords`).
        accumulator=None (the default): the body above, one batch and one rank; accumulate, micro_step and group must keep their defaults.
        accumulator=a givepose_amd.optim.GradAccumulator built over `optimizer`: the reference's loop with FLAGS.accumulate, to the
        letter (engine/train.py:117-131) -- the gradients are added to the accumulator with scale 1 / accumulate and clip_grad_norm_ at
        clip_norm is applied to the ACCUMULATED gradients, in place, on every micro-step (GradAccumulator.add), so a later micro-step
        adds to an already clipped buffer; when micro_step % accumulate == 0 the optimiser steps from the accumulator without a second
        clip and the accumulator is zeroed (res["stepped"] is True), otherwise no parameter moves and `params_updated()` is not called
        (res["stepped"] is False).  The caller passes micro_step = global_step; as in the reference, whose global_step starts at 0, the
        very first micro-step steps on one micro-batch.  res["param_grads"] stays unscaled.  With size_head= the running statistics
        move on EVERY micro-step (the reference's BatchNorm is in train mode on every forward), followed by `params_updated()`.
        group: a torch.distributed process group: the gradients are averaged over its ranks by one all_reduce of the accumulator's
        staging buffer before they are added (DDP's average); every rank must call with the same names, i.e. the same size_head= choice.
        With size_head= the three bn1 buffers are broadcast from rank 0 of the group after their update and before `params_updated()`
        (DDP's broadcast_buffers), so that the replicas' eval-mode forwards stay the same.  The all-reduce starts after the whole backward
        chain; there is no SyncBatchNorm: the batch statistics stay per rank and per micro-batch."""
        if getattr(optimizer, "model", None) is not self:
            raise ValueError("train_step: the optimizer must be a givepose_amd.optim.Ranger built over this model")
        if size_head is not None:
            self._size_head_mask(size_head, "train_step")
        res = self.head_grads_backbone(data, pose_loss, device, groups=groups, **({} if size_head is None else {"size_head": size_head}))
        optimizer.step(res["param_grads"], clip_norm=clip_norm, lr=lr)
        if size_head is not None:
            from . import size_grad
            sd, stats = self.state_dict(), res["size_head"]["stats"]
            size_grad.bn_running_update(sd["size_head.bn1.running_mean"], sd["size_head.bn1.running_var"],
                                        sd.get("size_head.bn1.num_batches_tracked"), stats["mean"], stats["var_unbiased"])
            self.params_updated()      # the step's own call came before the buffers moved
        return res

    @torch.no_grad()
    def _train_step_accumulated(self, data, pose_loss, optimizer, device="cuda", groups=None, clip_norm=5.0, lr=None, size_head=None,
                                accumulator=None, accumulate=1, micro_step=0, group=None):
        """train_step with an accumulator: one micro-step of the reference's loop."""
        if getattr(optimizer, "model", None) is not self:
            raise ValueError("train_step: the optimizer must be a givepose_amd.optim.Ranger built over this model")
        if size_head is not None:
            self._size_head_mask(size_head, "train_step")
        if getattr(accumulator, "optimizer", None) is not optimizer:
            raise ValueError("train_step: the accumulator must be a givepose_amd.optim.GradAccumulator built over this optimizer")
        if int(accumulate) != accumulate or accumulate < 1 or int(micro_step) != micro_step or micro_step < 0:
            raise ValueError(f"train_step: accumulate {accumulate} must be a positive and micro_step {micro_step} a non-negative integer")
        res = self.head_grads_backbone(data, pose_loss, device, groups=groups, **({} if size_head is None else {"size_head": size_head}))
        accumulator.add(res["param_grads"], scale=1.0 / accumulate, clip_norm=clip_norm, group=group)
        res["stepped"] = micro_step % accumulate == 0
        if res["stepped"]:
            optimizer.step(accumulator.grads, clip_norm=None, lr=lr)
            accumulator.zero()
        if size_head is not None:
            from . import size_grad
            sd, stats = self.state_dict(), res["size_head"]["stats"]
            buffers = [sd["size_head.bn1.running_mean"], sd["size_head.bn1.running_var"], sd.get("size_head.bn1.num_batches_tracked")]
            size_grad.bn_running_update(*buffers, stats["mean"], stats["var_unbiased"])
            if group is not None:
                import torch.distributed as dist
                src = dist.get_global_rank(group, 0)
                for b in buffers:
                    if b is not None:
                        dist.broadcast(b, src=src, group=group)
            self.params_updated()
        return res
