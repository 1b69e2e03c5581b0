"""The weight-repack family (include/givepose_repack.h, gpr_*): PoseNet._pack on the device, in place.

`plan(cfg, compute_dtype, split_gemm)` is a symbolic description of `_pack`, key by key: which strided view of which state-dict tensor
(or of which fold result) goes, in which storage kind, to which element offset of which packed tensor.  It holds names and numbers only
and needs no GPU; tests/repack_ref.py interprets it with torch on the host and compares it with `_pack` itself.

`DeviceRepack` binds a plan to a model: it allocates the packed tensors (the keys, shapes and dtypes of `_pack`, a `SplitW` where `_pack`
makes one), the fold scratch and the device tables, sends the tables once, and `run()` is then gpr_repack: at most
_lib.GPR_REPACK_LAUNCHES launches on the current stream, no allocation, no copy, no synchronisation.  Every packed tensor keeps its
address, which is what lets `PoseNet.params_updated()` keep the forward's plans and captured hipGraphs (PoseNet.set_repack("device")).
"""
import ctypes
import os
from collections import OrderedDict, namedtuple

import torch

from . import _lib, synth
from .ops import SPLIT_SHIFT, SplitW

OM_LD = 128     # posenet.OM_LD: row count of the zero-padded offset | mask projection
F32, F16, SPLIT = "f32", "f16", "split"
_KIND = {F32: _lib.GPR_KIND_F32, F16: _lib.GPR_KIND_F16, SPLIT: _lib.GPR_KIND_SPLIT}
FOLD = "@"      # first character of a fold result's name (a state-dict name never starts with it)

# src: a state-dict name or a fold result (FOLD + key); dims / strides (source elements) / offset: the view, outermost first;
# dst, dst_off: the packed tensor and the element offset (inside each plane for SPLIT) the view's first element goes to
Entry = namedtuple("Entry", "src dims strides offset dst dst_off kind")
# eval BatchNorm1d folded into the 1x1 conv in front of it; w_out / b_out: fold results (fp32, (C, K) and (C,))
BnFold = namedtuple("BnFold", "w b bn_w bn_b mean var w_out b_out C K eps")
# out[m, n] = sum_k A[a_off + m a_rs + k] B[b_off + k b_rs + n] (+ add[m]) in float64, rounded once into out32[o32_off + m ld32 + n];
# out64 (level 0 only): the unrounded result, which a level-1 fold may name as its B (b_f64)
MatFold = namedtuple("MatFold", "A a_off a_rs B b_off b_rs b_f64 add out32 o32_off ld32 out64 o64_off ld64 M N K level")
# the fold results whose summation order the host's BLAS does not fix: held to float64 by the tests, not to _pack's bits
MATRIX_FOLD_KEYS = tuple(f"enc{li}.{k}" for li in range(3) for k in ("fold_w", "fold_b")) + ("enc0.xyz_m",)


CONV3_WCM_LAYERS = (6, 7, 9, 10)      # the xyz heads' 3x3 convs on 32 x 32 and 64 x 64 maps: the layers the wide window conv can take


class Plan:
    def __init__(self):
        self.entries, self.bnfolds, self.matfolds = [], [], []
        self.dst = OrderedDict()        # packed key -> (shape, kind); SPLIT: shape (N, K) of the (2, N, K) planes
        self.scratch = OrderedDict()    # fold result -> (shape, "f32" | "f64")
        self.sources = OrderedDict()    # state-dict name -> shape, every tensor the plan reads
        self.zero_filled = set()        # packed keys with rows no entry writes (the padding of om_w / om_b): zeroed at allocation


class _View:
    """A strided view of one source, built with the tensor methods `_pack` uses.  reshape() of a view that is no longer contiguous only
    renames the shape: the element order, row-major over the view, is what reaches the (dense) destination."""

    def __init__(self, src, shape, strides=None, offset=0, final=None):
        self.src, self.dims, self.offset, self.final = src, tuple(int(d) for d in shape), int(offset), final
        if strides is None:
            strides, run = [], 1
            for d in reversed(self.dims):
                strides.insert(0, run)
                run *= d
        self.strides = tuple(int(s) for s in strides)

    @property
    def shape(self):
        return self.dims if self.final is None else self.final

    def numel(self):
        n = 1
        for d in self.dims:
            n *= d
        return n

    def _contiguous(self):
        run = 1
        for d, s in zip(reversed(self.dims), reversed(self.strides)):
            if d != 1 and s != run:
                return False
            run *= d
        return True

    def reshape(self, *shape):
        shape, n = list(shape), self.numel()
        if -1 in shape:
            known = 1
            for d in shape:
                known *= d if d != -1 else 1
            shape[shape.index(-1)] = n // known
        prod = 1
        for d in shape:
            prod *= d
        assert prod == n, (self.src, self.shape, shape)
        if self.final is None and self._contiguous():
            return _View(self.src, shape, None, self.offset)
        return _View(self.src, self.dims, self.strides, self.offset, final=tuple(shape))

    def permute(self, *p):
        assert self.final is None and sorted(p) == list(range(len(self.dims))), (self.src, p)
        return _View(self.src, [self.dims[i] for i in p], [self.strides[i] for i in p], self.offset)

    def t(self):
        assert len(self.dims) == 2
        return self.permute(1, 0)

    def squeeze_last(self):
        assert self.final is None and self.dims[-1] == 1
        return _View(self.src, self.dims[:-1], self.strides[:-1], self.offset)

    def canonical(self):
        """(dims, strides) with size-1 dims dropped and mergeable neighbours merged, padded in front to GPR_MAX_DIMS."""
        dims, strides = [], []
        for d, s in zip(self.dims, self.strides):
            if d == 1:
                continue
            if dims and strides[-1] == s * d:
                dims[-1], strides[-1] = dims[-1] * d, s
            else:
                dims.append(d)
                strides.append(s)
        if len(dims) > _lib.GPR_MAX_DIMS:
            raise ValueError(f"{self.src}: a view of {len(dims)} dims after merging, {_lib.GPR_MAX_DIMS} are supported")
        pad = _lib.GPR_MAX_DIMS - len(dims)
        return (1,) * pad + tuple(dims), (0,) * pad + tuple(strides)


def check_supported(cfg):
    """The configurations the device repack serves are those `train_step` accepts; the others are refused by name."""
    if cfg.main_backbone != "convnext":
        raise NotImplementedError(f"device repack: main_backbone={cfg.main_backbone!r} (the 'resnet34' BatchNorm folds) is not built; use set_repack('host')")
    if cfg.nocsmap_encoder != "conv":
        raise NotImplementedError(f"device repack: nocsmap_encoder={cfg.nocsmap_encoder!r} (the 'att' encoder: its plans hold position-embedding rows "
                                  "copied from the packed weights) is not built; use set_repack('host')")
    if cfg.pnp_head != "conv":
        raise NotImplementedError(f"device repack: pnp_head={cfg.pnp_head!r} (the 'att' head: its plans hold position-embedding rows copied from "
                                  "the packed weights) is not built; use set_repack('host')")
    if cfg.use_dcn != "dcnv3":
        raise NotImplementedError(f"device repack: use_dcn={cfg.use_dcn!r} (the plain-conv encoder, use_dcn='') is not built; use set_repack('host')")
    if cfg.defer_ln:
        raise NotImplementedError("device repack: defer_ln=True (LayerNorm folded into fc1: fc1_wg / fc1_cs / fc1_cb) is not built; use set_repack('host')")


def plan(cfg, compute_dtype=torch.float16, split_gemm=False):
    """The entries that reproduce PoseNet(cfg, dtype=compute_dtype, split_gemm=split_gemm)._pack key by key.  No pointers, no GPU."""
    check_supported(cfg)
    if compute_dtype not in (torch.float16, torch.float32):
        raise TypeError(f"unsupported dtype {compute_dtype} (float16 / float32)")
    if split_gemm and compute_dtype != torch.float32:
        raise ValueError("split_gemm is a float32-storage mode")
    manifest = synth.param_manifest(cfg)
    fp16 = compute_dtype == torch.float16
    P = Plan()

    def sd(name):
        P.sources[name] = tuple(manifest[name])
        return _View(name, manifest[name])

    def fold(key, shape, dtype="f32"):
        P.scratch[key] = (tuple(shape), dtype)
        return _View(FOLD + key, shape)

    def put(key, view, kind, dst_off=0, shape=None):
        """view -> P.dst[key]; shape: the whole destination's, where the view is one part of a concatenation."""
        shape = tuple(view.shape if shape is None else shape)
        assert kind != SPLIT or len(shape) == 2, key        # ops.split_weights: (N, K) -> planes (2, N, K)
        if key in P.dst:
            assert P.dst[key] == (shape, kind), key
        else:
            P.dst[key] = (shape, kind)
        dims, strides = view.canonical()
        P.entries.append(Entry(view.src, dims, strides, view.offset, key, int(dst_off), kind))

    f32 = lambda key, v, **k: put(key, v, F32, **k)
    lowp = lambda key, v, **k: put(key, v, F16 if fp16 else F32, **k)
    gw = (lambda key, v, **k: put(key, v, SPLIT, **k)) if split_gemm else lowp

    g = lambda k: sd("backbone." + k)
    for s, (d, n) in enumerate(zip(cfg.convnext_dims, cfg.convnext_depths)):
        if s == 0:
            f32("stem.w", g("stem_0.weight").reshape(-1, 48).t())
            f32("stem.b", g("stem_0.bias"))
            f32("stem.ln_w", g("stem_1.weight"))
            f32("stem.ln_b", g("stem_1.bias"))
        if s > 0:
            p = f"stages_{s}.downsample."
            f32(f"ds{s}.ln_w", g(p + "0.weight"))
            f32(f"ds{s}.ln_b", g(p + "0.bias"))
            gw(f"ds{s}.w", g(p + "1.weight").permute(0, 2, 3, 1).reshape(d, -1))
            f32(f"ds{s}.b", g(p + "1.bias"))
        for b in range(n):
            p, q = f"stages_{s}.blocks.{b}.", f"s{s}b{b}."
            lowp(q + "dw_w", g(p + "conv_dw.weight").reshape(d, 49).t())
            f32(q + "dw_b", g(p + "conv_dw.bias"))
            f32(q + "ln_w", g(p + "norm.weight"))
            f32(q + "ln_b", g(p + "norm.bias"))
            gw(q + "fc1_w", g(p + "mlp.fc1.weight"))
            f32(q + "fc1_b", g(p + "mlp.fc1.bias"))
            gw(q + "fc2_w", g(p + "mlp.fc2.weight"))
            f32(q + "fc2_b", g(p + "mlp.fc2.bias"))
            f32(q + "gamma", g(p + "gamma"))
            fuse512 = d == 512 and (cfg.fuse_mlp512 or os.environ.get("GP_FUSE_MLP512") == "1")
            if fp16 and (d in (128, 256) or fuse512) and cfg.fuse_mlp:
                # gp_convnext_mlp_pack_w2 as a view of fc2.weight (d, 4 d): inside every block of 32 hidden units, k-slot fq 8 + nt 4 + j takes unit
                # nt 16 + fq 4 + j -- the dims (row and block, fq, nt, j) with the source strides (32, 4, 16, 1)
                put(q + "fc2_wp", _View("backbone." + p + "mlp.fc2.weight", (d * 4 * d // 32, 4, 2, 4), (32, 4, 16, 1)).reshape(d, 4 * d), F16)
    for head in ("xyz_nocs_head", "xyz_deform_head"):
        h = lambda k: sd(f"{head}.{k}")
        gw(head + ".deconv_w", h("features.0.weight").permute(2, 3, 1, 0).reshape(9 * 256, -1))
        f32(head + ".gn0_w", h("features.1.weight"))
        f32(head + ".gn0_b", h("features.1.bias"))
        for i in (3, 4, 6, 7, 9, 10):
            gw(f"{head}.c{i}_w", h(f"features.{i}.conv.weight").permute(0, 2, 3, 1).reshape(256, -1))
            if fp16 and i in CONV3_WCM_LAYERS:
                # ops.conv3_pack_wcm (gpw_conv3_pack_wcm) as a view of the conv weight (256, Cin, 3, 3): [n][ci / 32][tap][ci % 32], the chunk-major
                # copy the eight-phase window conv reads (gp_gemm_desc.W_cm) -- the dims (n, chunk, tap, ci % 32) with the source strides
                cin = int(manifest[f"{head}.features.{i}.conv.weight"][1])
                put(f"{head}.c{i}_wcm", _View(f"{head}.features.{i}.conv.weight", (256, cin // 32, 9, 32), (cin * 9, 32 * 9, 1, 9)).reshape(256, -1), F16)
            f32(f"{head}.c{i}_gw", h(f"features.{i}.norm.weight"))
            f32(f"{head}.c{i}_gb", h(f"features.{i}.norm.bias"))
        f32(head + ".out_w", h("out_layer.weight").reshape(3, 256))
        f32(head + ".out_b", h("out_layer.bias"))
    # SizeHead: eval BatchNorm1d folded into conv1
    C, K = manifest["size_head.conv1.weight"][:2]
    for n in ("conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var"):
        sd("size_head." + n)
    P.bnfolds.append(BnFold("size_head.conv1.weight", "size_head.conv1.bias", "size_head.bn1.weight", "size_head.bn1.bias",
                            "size_head.bn1.running_mean", "size_head.bn1.running_var", "size.w1", "size.b1", int(C), int(K), 1e-5))
    f32("size.w1", fold("size.w1", (C, K)))
    f32("size.b1", fold("size.b1", (C,)))
    f32("size.w2", sd("size_head.conv2.weight").squeeze_last())
    f32("size.b2", sd("size_head.conv2.bias"))
    for li, i in enumerate((0, 3, 6)):
        p, q = f"nocs_encoder.features.{i}.", f"enc{li}."
        d = p + "dcnv3."
        cw = sd(p + "conv.weight").reshape(256, -1)
        Kc = cw.shape[1]
        (f32 if li == 0 else gw)(q + "conv_w", cw)
        f32(q + "conv_b", sd(p + "conv.bias"))
        lowp(q + "dw_w", sd(d + "dw_conv.0.weight").reshape(256, 9).t())
        f32(q + "dw_b", sd(d + "dw_conv.0.bias"))
        f32(q + "ln_w", sd(d + "dw_conv.1.1.weight"))
        f32(q + "ln_b", sd(d + "dw_conv.1.1.bias"))
        ow, mw = sd(d + "offset.weight"), sd(d + "mask.weight")
        gw(q + "om_w", ow, shape=(OM_LD, 256))
        gw(q + "om_w", mw, shape=(OM_LD, 256), dst_off=ow.numel())
        f32(q + "om_b", sd(d + "offset.bias"), shape=(OM_LD,))
        f32(q + "om_b", sd(d + "mask.bias"), shape=(OM_LD,), dst_off=ow.shape[0])
        P.zero_filled.update((q + "om_w", q + "om_b"))
        gw(q + "in_w", sd(d + "input_proj.weight"))
        f32(q + "in_b", sd(d + "input_proj.bias"))
        # input_proj(conv1x1(x)) as one linear map: fold_w = in_w @ conv_w, fold_b = in_w @ conv_b + in_b
        xyz = li == 0 and fp16 and not split_gemm
        if xyz:
            P.scratch["enc0.fold64"] = ((256, 4), "f64")       # [fold_w | fold_b] unrounded: what enc0_xyz_pack contracts output_proj with
        P.matfolds.append(MatFold(d + "input_proj.weight", 0, 256, p + "conv.weight", 0, Kc, False, None, q + "fold_w", 0, Kc,
                                  "enc0.fold64" if xyz else None, 0, 4, 256, Kc, 256, 0))
        P.matfolds.append(MatFold(d + "input_proj.weight", 0, 256, p + "conv.bias", 0, 1, False, d + "input_proj.bias", q + "fold_b", 0, 1,
                                  "enc0.fold64" if xyz else None, 3, 4, 256, 1, 256, 0))
        (f32 if li == 0 else gw)(q + "fold_w", fold(q + "fold_w", (256, Kc)))
        f32(q + "fold_b", fold(q + "fold_b", (256,)))
        gw(q + "out_w", sd(d + "output_proj.weight"))
        f32(q + "out_b", sd(d + "output_proj.bias"))
        if xyz:     # layer 0 as one gather + one 256 x 16 matrix: M[:, 4 g + c] = out_w[:, 64 g : 64 g + 64] @ fold64[64 g : 64 g + 64, c]
            assert Kc == 3
            for grp in range(4):
                P.matfolds.append(MatFold(d + "output_proj.weight", 64 * grp, 256, FOLD + "enc0.fold64", 64 * grp * 4, 4, True, None,
                                          "enc0.xyz_m", 4 * grp, 16, None, 0, 0, 256, 4, 64, 1))
            f32(q + "xyz_m", fold("enc0.xyz_m", (256, 16)))
            f32(q + "xyz_b", sd(d + "output_proj.bias"))
        f32(q + "gn_w", sd(f"nocs_encoder.features.{i + 1}.weight"))
        f32(q + "gn_b", sd(f"nocs_encoder.features.{i + 1}.bias"))
    gw("red.w", sd("feat_reducer.weight").reshape(256, -1))
    f32("red.b", sd("feat_reducer.bias"))
    f32("pnp.c0_w", sd("pnp_net.features.0.weight").reshape(128, -1).t())
    for li, i in enumerate((0, 3, 6)):
        if li > 0:
            gw(f"pnp.c{li}_w", sd(f"pnp_net.features.{i}.weight").permute(0, 2, 3, 1).reshape(128, -1))
        f32(f"pnp.g{li}_w", sd(f"pnp_net.features.{i + 1}.weight"))
        f32(f"pnp.g{li}_b", sd(f"pnp_net.features.{i + 1}.bias"))
    # fc1 || fc1_z as one GEMM; flat_op 'flatten': columns from the reference's NCHW flatten (c 64 + hw) to the channels-last one (hw 128 + c)
    if cfg.flat_op == "flatten":
        perm = lambda w: w.reshape(-1, 128, 64).permute(0, 2, 1).reshape(-1, 8192)
    else:
        perm = lambda w: w
    w1, w1z = perm(sd("pnp_net.fc1.weight")), perm(sd("pnp_net.fc1_z.weight"))
    rows, cols = w1.shape[0] + w1z.shape[0], w1.shape[1]
    gw("pnp.fc1_w", w1, shape=(rows, cols))
    gw("pnp.fc1_w", w1z, shape=(rows, cols), dst_off=w1.numel())
    f32("pnp.fc1_b", sd("pnp_net.fc1.bias"), shape=(rows,))
    f32("pnp.fc1_b", sd("pnp_net.fc1_z.bias"), shape=(rows,), dst_off=w1.shape[0])
    gw("pnp.fc2_w", sd("pnp_net.fc2.weight"))
    f32("pnp.fc2_b", sd("pnp_net.fc2.bias"))
    gw("pnp.fc2z_w", sd("pnp_net.fc2_z.weight"))
    f32("pnp.fc2z_b", sd("pnp_net.fc2_z.bias"))
    for n in ("fc_r", "fc_t", "fc_z"):
        f32(n + ".w", sd(f"pnp_net.{n}.weight"))
        f32(n + ".b", sd(f"pnp_net.{n}.bias"))
    for f in P.matfolds:
        for name in (f.A, f.B, f.add):
            if name is not None and not name.startswith(FOLD):
                P.sources[name] = tuple(manifest[name])
    return P


def _prod(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _describe(t):
    return f"{tuple(t.shape)} {t.dtype} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}"


class DeviceRepack:
    """A plan bound to one device: the packed tensors, the fold scratch and the device tables.  `packed` is what `_pack` would return.
    alloc(key, shape, dtype, zero): optional hook that supplies the packed tensors (default torch.empty / torch.zeros)."""

    def __init__(self, plan, device, alloc=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the device repack runs on the HIP device only")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.plan = P = plan
        if alloc is None:
            alloc = lambda key, shape, dtype, zero: (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
        self.packed, self._dst = OrderedDict(), {}
        for key, (shape, kind) in P.dst.items():
            if kind == SPLIT:
                planes = alloc(key, (2,) + tuple(shape), torch.float16, key in P.zero_filled)
                self.packed[key], self._dst[key] = SplitW(planes, SPLIT_SHIFT), planes
            else:
                self.packed[key] = self._dst[key] = alloc(key, tuple(shape), torch.float16 if kind == F16 else torch.float32, key in P.zero_filled)
        self._scratch = {key: torch.empty(shape, dtype=torch.float64 if dt == "f64" else torch.float32, device=self.device)
                         for key, (shape, dt) in P.scratch.items()}
        self._tables, self._info, self._ptrs, self._stages = None, _lib.RepackInfo(), None, []
        self.uploads = 0

    def sources_of(self, net):
        """The tensors of `net` the plan reads, by state-dict name."""
        sd = net.state_dict(keep_vars=True)
        return {name: sd[name] for name in self.plan.sources}

    def _check(self, src):
        for name, shape in self.plan.sources.items():
            t = src[name]
            if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"device repack: {name}: {_describe(t)}, expected contiguous float32 {shape} on {self.device} "
                                 "(move the model to the device first)")

    def _build(self, src):
        """The host tables with this model's pointers, checked by gpr_tables_upload and sent to the device: once per set of pointers."""
        P, lib = self.plan, _lib.load()

        def tensor(name):
            return self._scratch[name[len(FOLD):]] if name.startswith(FOLD) else src[name]

        def ptr(name, off=0):
            if name is None:
                return None
            t = tensor(name)
            assert 0 <= off < t.numel(), (name, off)
            return t.data_ptr() + off * t.element_size()

        E = (_lib.RepackEntry * len(P.entries))()
        for e, r in zip(P.entries, E):
            s, d = tensor(e.src), self._dst[e.dst]
            shape, kind = P.dst[e.dst]
            r.src, r.dst, r.src_numel, r.dst_numel = s.data_ptr(), d.data_ptr(), s.numel(), _prod(shape)
            r.src_off, r.dst_off, r.plane_stride = e.offset, e.dst_off, _prod(shape) if kind == SPLIT else 0
            r.strides[:], r.dims[:], r.kind = e.strides, e.dims, _KIND[kind]
        B = (_lib.RepackBnFold * max(len(P.bnfolds), 1))()
        for f, r in zip(P.bnfolds, B):
            for field in ("w", "b", "bn_w", "bn_b", "mean", "var"):
                t = src[getattr(f, field)]
                assert t.numel() == (f.C * f.K if field == "w" else f.C), (field, tuple(t.shape))
                setattr(r, field, t.data_ptr())
            assert self._scratch[f.w_out].numel() == f.C * f.K and self._scratch[f.b_out].numel() == f.C
            r.w_numel, r.c_numel = src[f.w].numel(), f.C      # (the asserts above: every tensor has exactly these counts; the entry point checks C, K against them)
            r.w_out, r.b_out, r.C, r.K, r.eps = self._scratch[f.w_out].data_ptr(), self._scratch[f.b_out].data_ptr(), f.C, f.K, f.eps
        M = (_lib.RepackMatFold * max(len(P.matfolds), 1))()
        for f, r in zip(P.matfolds, M):
            # every index the kernel forms lies inside its tensor
            assert f.a_off + (f.M - 1) * f.a_rs + f.K <= tensor(f.A).numel() and f.b_off + (f.K - 1) * f.b_rs + f.N <= tensor(f.B).numel(), f
            assert f.add is None or tensor(f.add).numel() >= f.M, f
            assert f.o32_off + (f.M - 1) * f.ld32 + f.N <= self._scratch[f.out32].numel(), f
            assert f.out64 is None or f.o64_off + (f.M - 1) * f.ld64 + f.N <= self._scratch[f.out64].numel(), f
            assert tensor(f.B).dtype == (torch.float64 if f.b_f64 else torch.float32), f
            r.A, r.B, r.add = ptr(f.A, f.a_off), ptr(f.B, f.b_off), ptr(f.add)
            r.out32, r.out64 = ptr(FOLD + f.out32, f.o32_off), (None if f.out64 is None else ptr(FOLD + f.out64, f.o64_off))
            # what lies behind each pointer: the entry point checks the kernel's index expressions against these
            r.a_numel, r.b_numel, r.add_numel = tensor(f.A).numel() - f.a_off, tensor(f.B).numel() - f.b_off, 0 if f.add is None else tensor(f.add).numel()
            r.out32_numel = self._scratch[f.out32].numel() - f.o32_off
            r.out64_numel = 0 if f.out64 is None else self._scratch[f.out64].numel() - f.o64_off
            r.M, r.N, r.K, r.a_rs, r.b_rs, r.ld32, r.ld64, r.b_f64, r.level = f.M, f.N, f.K, f.a_rs, f.b_rs, f.ld32, f.ld64, int(f.b_f64), f.level
        args = (E, len(P.entries), B, len(P.bnfolds), M, len(P.matfolds))
        nbytes = lib.gpr_tables_bytes(*args)
        if nbytes <= 0:
            _lib.check(-1, "gpr_tables_bytes")
        if self._tables is None or self._tables.numel() < nbytes:
            self._tables = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        # a pinned staging buffer per upload, kept until an event recorded behind the copy has completed (never waited for: only polled)
        self._stages = [(t, ev) for t, ev in self._stages if not ev.query()]
        stage = torch.empty(self._tables.numel(), dtype=torch.uint8).pin_memory()
        cur = torch.cuda.current_stream(self.device)
        _lib.check(lib.gpr_tables_upload(*args, ctypes.c_void_p(stage.data_ptr()), ctypes.c_void_p(self._tables.data_ptr()), self._tables.numel(),
                                         ctypes.byref(self._info), ctypes.c_void_p(cur.cuda_stream)), "gpr_tables_upload")
        ev = torch.cuda.Event()
        ev.record(cur)
        self._stages.append((stage, ev))
        self.uploads += 1

    def run(self, src):
        """One repack on the current stream from the tensors `src` ({name: contiguous fp32 tensor on the device}).  The tables are rebuilt
        only when a tensor's data_ptr differs from the one they hold."""
        self._check(src)
        ptrs = tuple(src[name].data_ptr() for name in self.plan.sources)
        if ptrs != self._ptrs:
            self._build(src)
            self._ptrs = ptrs
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(_lib.load().gpr_repack(ctypes.c_void_p(self._tables.data_ptr()), ctypes.byref(self._info), stream), "gpr_repack")

    def launches(self):
        """Launches of one run(): _lib.GPR_REPACK_LAUNCHES in the fp16 mode, _lib.GPR_REPACK_LAUNCHES_F32 otherwise."""
        return 2 + bool(self.plan.bnfolds) + any(f.level == 1 for f in self.plan.matfolds)
