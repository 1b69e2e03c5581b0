"""The map-encoder backward family (include/givepose_encgrad.h, gpe_*): MAPEncoder's fp32 forward-that-saves and its backward (use_dcn
'dcnv3'), the operators they are made of, and the 1x1 conv backward with any number of output channels (feat_reducer).

Everything runs on the device in this library's HIP kernels; there is no CPU path.  Parameters and their gradients are fp32 in the
reference's own shapes; the coordinate map, the result and the GroupNorm tensors are NCHW, what a layer saves in between is
channels-last as the reference's module is (`saved_shapes`).

A coupling batch is the set of crops whose DCNv3 layers share one flat offset / mask buffer: `groups` lists the batch
sizes of the forward that ran (None: one batch).  The batches are run one after the other and their parameter gradients are added
in batch order.

d xp is scattered with fp32 atomics by default (`scatter="atomic"`): results are repeatable to rounding, not bit for bit, except
where the header says so.  `scatter="ordered"` (include/givepose_encgrad_ordered.h, gpeo_*) adds the same terms per element in
ascending order of their source id, without any floating-point atomic: two calls give equal bits in every output.

`alloc(name, shape)` -- an optional hook every function takes -- supplies the output and workspace buffers (fp32, contiguous, on
the device; workspaces 256-byte aligned); the default is torch.empty.  The tests use it to put sentinels around every buffer.
"""
import ctypes

import torch

from . import _lib
from .pnp_grad import _default_alloc, _f32, _stream, _ws

LAYER_IDS = (0, 3, 6)
_LAYER_KEYS = [f"{m}.{p}" for m in ("conv", "dcnv3.dw_conv.0", "dcnv3.dw_conv.1.1", "dcnv3.offset", "dcnv3.mask", "dcnv3.input_proj",
                                    "dcnv3.output_proj") for p in ("weight", "bias")]
# the 48 tensors in the order of gpe_enc_params, named as in the reference's state_dict (without the prefix); dcnv3's bn.* is never
# applied in the forward and has no gradient
PARAM_KEYS = [k for i in LAYER_IDS for k in [f"features.{i}.{n}" for n in _LAYER_KEYS] + [f"features.{i + 1}.weight", f"features.{i + 1}.bias"]]
SAVED_KEYS = _lib.EncLayerSaved.FIELDS
# of the last layer, what no scatter feeds (equal bits between runs)
ATOMIC_FREE_KEYS = [f"features.6.dcnv3.{m}.{p}" for m in ("dw_conv.0", "dw_conv.1.1", "offset", "mask", "output_proj") for p in ("weight", "bias")] \
    + ["features.7.weight", "features.7.bias"]
# with scatter="ordered" no floating-point atomic feeds anything: all 48 gradients and d coor are equal bits between runs
ORDERED_FREE_KEYS = PARAM_KEYS
SCATTER_MODES = {"atomic": _lib.GPE_SCATTER_ATOMIC, "ordered": _lib.GPE_SCATTER_ORDERED}


def scatter_mode(scatter):
    """"atomic" / "ordered" -> GPE_SCATTER_*; anything else raises ValueError naming the value."""
    if not isinstance(scatter, str) or scatter not in SCATTER_MODES:
        raise ValueError(f"scatter {scatter!r}: expected one of {tuple(SCATTER_MODES)}")
    return SCATTER_MODES[scatter]


def param_shapes():
    """name -> shape of every differentiated parameter of the encoder."""
    s = {}
    for i in LAYER_IDS:
        q = f"features.{i}."
        s[q + "conv.weight"] = (256, 3 if i == 0 else 256, 1, 1)
        s[q + "dcnv3.dw_conv.0.weight"] = (256, 1, 3, 3)
        s[q + "dcnv3.offset.weight"], s[q + "dcnv3.offset.bias"] = (72, 256), (72,)
        s[q + "dcnv3.mask.weight"], s[q + "dcnv3.mask.bias"] = (36, 256), (36,)
        s[q + "dcnv3.input_proj.weight"] = s[q + "dcnv3.output_proj.weight"] = (256, 256)
    return {k: s.get(k, (256,)) for k in PARAM_KEYS}


def saved_shapes(N, R):
    """name -> the three layers' shapes of what enc_forward_save writes for one coupling batch of N crops at resolution R
    (gpe_layer_saved).  x, xp: NHWC; dwout, x1, y, offset, mask, ln_*: the N (H/2)^2 prefix rows; pre, act, gn_*: NCHW."""
    out = {k: [] for k in SAVED_KEYS}
    for l in range(3):
        H = R >> l
        Ho = H // 2
        n = N * Ho * Ho
        for k, s in (("x", (N, H, H, 256)), ("xp", (N, H, H, 256)), ("dwout", (n, 256)), ("ln_mean", (n,)), ("ln_rstd", (n,)), ("x1", (n, 256)),
                     ("offset", (n, 72)), ("mask", (n, 36)), ("y", (n, 256)), ("pre", (N, 256, Ho, Ho)), ("gn_mean", (N, 32)),
                     ("gn_rstd", (N, 32)), ("act", (N, 256, Ho, Ho))):
            out[k].append(s)
    return out


def _dev(t):
    if t.device.type != "cuda":
        raise _lib.GivePoseHipError("the map-encoder backward runs on a HIP device only: there is no CPU path")
    return t.device


def _call(dev, fn, name, *args):
    with torch.cuda.device(dev):
        _lib.check(fn(*args), name)


def _params_struct(tensors, what):
    shapes = param_shapes()
    st = _lib.EncParams()
    for n, k in enumerate(PARAM_KEYS):
        t = tensors[k]
        if tuple(t.shape) != shapes[k] or t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != "cuda":
            raise ValueError(f"{what}[{k}]: {tuple(t.shape)} {t.dtype} on {t.device}, expected contiguous float32 {shapes[k]} on the device")
        setattr(st.layer[n // 16], _lib.EncLayerParams.FIELDS[n % 16], t.data_ptr())
    return st


def _saved_struct(saved, N, R):
    st = _lib.EncSaved()
    for k, shp in saved_shapes(N, R).items():
        for l, s in enumerate(shp):
            t = saved[k][l]
            if tuple(t.shape) != tuple(s) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"saved[{k}][{l}]: {tuple(t.shape)} {t.dtype}, expected contiguous float32 {tuple(s)}")
            setattr(st.layer[l], k, t.data_ptr())
    return st


def _groups(groups, B):
    if groups is None:
        return [B]
    groups = [int(g) for g in groups]
    if not groups or min(groups) < 1 or sum(groups) != B:
        raise ValueError(f"groups {groups} must be positive batch sizes summing to the {B} crops")
    return groups


# ------------------------------------------------------------------------------------------------ the pieces
@torch.no_grad()
def linear_forward(X, W, b=None, alloc=None):
    """F.linear(X, W, b) over rows in fp32: X (rows,Cin), W (Cout,Cin) -> (rows,Cout)."""
    dev = _dev(X)
    rows, Cin = X.shape
    Cout = W.shape[0]
    X, W = _f32(X, dev), _f32(W, dev, (Cout, Cin), "W")
    b = None if b is None else _f32(b, dev, (Cout,), "b")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    Y = alloc("Y", (rows, Cout))
    nbytes = L.gpe_linear_workspace(rows, Cin, Cout)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpe_linear_forward, "gpe_linear_forward", X.data_ptr(), W.data_ptr(), None if b is None else b.data_ptr(), rows, Cin, Cout,
          Y.data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return Y


@torch.no_grad()
def linear_backward(dY, X, W, alloc=None):
    """Backward of F.linear(X, W, b): dY (rows,Cout) -> {"dX": (rows,Cin), "dW": (Cout,Cin), "db": (Cout,)}."""
    dev = _dev(dY)
    rows, Cin = X.shape
    Cout = W.shape[0]
    dY, X, W = _f32(dY, dev, (rows, Cout), "dY"), _f32(X, dev), _f32(W, dev, (Cout, Cin), "W")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    dX, dW, db = alloc("dX", (rows, Cin)), alloc("dW", (Cout, Cin)), alloc("db", (Cout,))
    nbytes = L.gpe_linear_workspace(rows, Cin, Cout)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpe_linear_backward, "gpe_linear_backward", dY.data_ptr(), X.data_ptr(), W.data_ptr(), rows, Cin, Cout, dX.data_ptr(),
          dW.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return {"dX": dX, "dW": dW, "db": db}


@torch.no_grad()
def dwln_forward_save(xin, dw_w, dw_b, ln_w, ln_b, n_pixels, alloc=None):
    """GELU(LayerNorm_eps1e-6(dw3x3(xin) + dw_b)) on the first n_pixels rows of xin (N,H,W,C)
    -> {"dwout", "x1": (n_pixels,C), "mean", "rstd": (n_pixels,)}."""
    dev = _dev(xin)
    N, H, W, C = xin.shape
    xin = _f32(xin, dev)
    dw_w, dw_b, ln_w, ln_b = _f32(dw_w, dev, (C, 1, 3, 3), "dw_w"), _f32(dw_b, dev, (C,), "dw_b"), _f32(ln_w, dev, (C,), "ln_w"), _f32(ln_b, dev, (C,), "ln_b")
    alloc = alloc or _default_alloc(dev)
    out = {"dwout": alloc("dwout", (n_pixels, C)), "mean": alloc("mean", (n_pixels,)), "rstd": alloc("rstd", (n_pixels,)),
           "x1": alloc("x1", (n_pixels, C))}
    L = _lib.load()
    _call(dev, L.gpe_dwln_forward_save, "gpe_dwln_forward_save", xin.data_ptr(), dw_w.data_ptr(), dw_b.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(),
          N, H, W, C, n_pixels, out["dwout"].data_ptr(), out["mean"].data_ptr(), out["rstd"].data_ptr(), out["x1"].data_ptr(), _stream(dev))
    return out


@torch.no_grad()
def dwln_backward(dx1, xin, saved, dw_w, ln_w, ln_b, alloc=None):
    """Backward of dwln_forward_save: d x1 (n_pixels,C), xin and what the forward saved for it
    -> {"dxin": (N,H,W,C), "d_dw_w": (C,1,3,3), "d_dw_b", "d_ln_w", "d_ln_b": (C,)}."""
    dev = _dev(dx1)
    N, H, W, C = xin.shape
    n = dx1.shape[0]
    xin, dx1 = _f32(xin, dev), _f32(dx1, dev, (n, C), "dx1")
    dwout, mean, rstd = _f32(saved["dwout"], dev, (n, C), "dwout"), _f32(saved["mean"], dev, (n,), "mean"), _f32(saved["rstd"], dev, (n,), "rstd")
    dw_w, ln_w, ln_b = _f32(dw_w, dev, (C, 1, 3, 3), "dw_w"), _f32(ln_w, dev, (C,), "ln_w"), _f32(ln_b, dev, (C,), "ln_b")
    alloc = alloc or _default_alloc(dev)
    out = {"dxin": alloc("dxin", (N, H, W, C)), "d_dw_w": alloc("d_dw_w", (C, 1, 3, 3)), "d_dw_b": alloc("d_dw_b", (C,)),
           "d_ln_w": alloc("d_ln_w", (C,)), "d_ln_b": alloc("d_ln_b", (C,))}
    L = _lib.load()
    nbytes = L.gpe_dwln_backward_workspace(N, H, W, C, n)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpe_dwln_backward, "gpe_dwln_backward", dx1.data_ptr(), xin.data_ptr(), dwout.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
          dw_w.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), N, H, W, C, n, *(out[k].data_ptr() for k in ("dxin", "d_dw_w", "d_dw_b", "d_ln_w", "d_ln_b")),
          ws.data_ptr(), nbytes, _stream(dev))
    return out


def _core_rows(N, H, W):
    return N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)


@torch.no_grad()
def dcnv3_core_forward(xp, offset, mask_logits, alloc=None):
    """The DCNv3 core (3x3, stride 2, pad 1, 4 groups of 64) on xp (N,H,W,256) with the first rows = N Ho Wo rows of the flat offset
    (.,72) and mask-logit (.,36) buffers -> {"mask": (rows,36) softmax probabilities, "y": (rows,256)}."""
    dev = _dev(xp)
    N, H, W, _ = xp.shape
    rows = _core_rows(N, H, W)
    xp = _f32(xp, dev, (N, H, W, 256), "xp")
    offset, mask_logits = _f32(offset, dev).reshape(-1, 72), _f32(mask_logits, dev).reshape(-1, 36)
    if offset.shape[0] < rows or mask_logits.shape[0] < rows:
        raise ValueError(f"offset / mask hold fewer than the {rows} rows the core consumes")
    alloc = alloc or _default_alloc(dev)
    out = {"mask": alloc("mask", (rows, 36)), "y": alloc("y", (rows, 256))}
    L = _lib.load()
    _call(dev, L.gpe_dcnv3_core_forward, "gpe_dcnv3_core_forward", xp.data_ptr(), offset.data_ptr(), mask_logits.data_ptr(), N, H, W,
          out["mask"].data_ptr(), out["y"].data_ptr(), _stream(dev))
    return out


@torch.no_grad()
def dcnv3_core_backward(xp, offset, mask, dy, alloc=None, scatter="atomic"):
    """Backward of dcnv3_core_forward given its probabilities `mask`: dy (rows,256)
    -> {"dxp": (N,H,W,256), "doffset": (rows,72), "dmask_logits": (rows,36)}.  scatter "atomic": d xp by fp32 atomic adds, equal
    to rounding between runs; "ordered": the same terms added in ascending source id, equal bits between runs (a workspace is
    allocated).  doffset and dmask_logits are the same bits in both."""
    mode = scatter_mode(scatter)
    dev = _dev(xp)
    N, H, W, _ = xp.shape
    rows = _core_rows(N, H, W)
    xp, dy = _f32(xp, dev, (N, H, W, 256), "xp"), _f32(dy, dev, (rows, 256), "dy")
    offset, mask = _f32(offset, dev).reshape(-1, 72), _f32(mask, dev, (rows, 36), "mask")
    if offset.shape[0] < rows:
        raise ValueError(f"offset holds fewer than the {rows} rows the core consumes")
    alloc = alloc or _default_alloc(dev)
    out = {"dxp": alloc("dxp", (N, H, W, 256)), "doffset": alloc("doffset", (rows, 72)), "dmask_logits": alloc("dmask_logits", (rows, 36))}
    L = _lib.load()
    if mode == _lib.GPE_SCATTER_ATOMIC:
        _call(dev, L.gpe_dcnv3_core_backward, "gpe_dcnv3_core_backward", xp.data_ptr(), offset.data_ptr(), mask.data_ptr(), dy.data_ptr(), N, H, W,
              out["dxp"].data_ptr(), out["doffset"].data_ptr(), out["dmask_logits"].data_ptr(), _stream(dev))
        return out
    nbytes = L.gpeo_dcnv3_core_backward_workspace(N, H, W, mode)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpeo_dcnv3_core_backward, "gpeo_dcnv3_core_backward", xp.data_ptr(), offset.data_ptr(), mask.data_ptr(), dy.data_ptr(), N, H, W,
          out["dxp"].data_ptr(), out["doffset"].data_ptr(), out["dmask_logits"].data_ptr(), _stream(dev), mode, ws.data_ptr(), nbytes)
    return out


@torch.no_grad()
def gn_relu_forward(x, gamma, beta, groups=32, alloc=None):
    """ReLU(GroupNorm_groups(x)) on (B,C,H,W) or (B,C,HW) -> {"out", "mean", "rstd": (B,groups)}."""
    dev = _dev(x)
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    x, gamma, beta = _f32(x, dev), _f32(gamma, dev, (C,), "gamma"), _f32(beta, dev, (C,), "beta")
    alloc = alloc or _default_alloc(dev)
    out = {"out": alloc("out", tuple(x.shape)), "mean": alloc("mean", (B, groups)), "rstd": alloc("rstd", (B, groups))}
    L = _lib.load()
    _call(dev, L.gpe_gn_relu_forward, "gpe_gn_relu_forward", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), B, C, HW, groups,
          out["out"].data_ptr(), out["mean"].data_ptr(), out["rstd"].data_ptr(), _stream(dev))
    return out


@torch.no_grad()
def gn_relu_backward(dout, x, mean, rstd, gamma, beta, groups=32, alloc=None):
    """Backward of out = ReLU(GroupNorm_groups(x)) given the saved x, mean and rstd (B,groups) -> {"dx", "dgamma", "dbeta"}."""
    dev = _dev(dout)
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    dout, x = _f32(dout, dev, x.shape, "dout"), _f32(x, dev)
    mean, rstd = _f32(mean, dev, (B, groups), "mean"), _f32(rstd, dev, (B, groups), "rstd")
    gamma, beta = _f32(gamma, dev, (C,), "gamma"), _f32(beta, dev, (C,), "beta")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    dx, dg, db = alloc("dx", tuple(x.shape)), alloc("dgamma", (C,)), alloc("dbeta", (C,))
    nbytes = L.gpe_gn_relu_backward_workspace(B, C)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpe_gn_relu_backward, "gpe_gn_relu_backward", dout.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
          beta.data_ptr(), B, C, HW, groups, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return {"dx": dx, "dgamma": dg, "dbeta": db}


@torch.no_grad()
def conv1x1_backward(dY, X, W, alloc=None):
    """Backward of F.conv2d(X, W, bias) with a 1x1 kernel and any Cout: dY (B,Cout,...), X (B,Cin,...), W (Cout,Cin[,1,1])
    -> {"dX": like X, "dW": like W, "db": (Cout,)}."""
    dev = _dev(dY)
    B, Cin = X.shape[:2]
    Cout = W.shape[0]
    HW = X[0, 0].numel()
    X, W = _f32(X, dev), _f32(W, dev)
    if W.numel() != Cout * Cin:
        raise ValueError(f"W: shape {tuple(W.shape)}, expected ({Cout},{Cin}[,1,1])")
    dY = _f32(dY, dev, (B, Cout) + tuple(X.shape[2:]), "dY")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    dX, dW, db = alloc("dX", tuple(X.shape)), alloc("dW", tuple(W.shape)), alloc("db", (Cout,))
    nbytes = L.gpe_conv1x1_backward_workspace(B, Cin, Cout, HW)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpe_conv1x1_backward, "gpe_conv1x1_backward", dY.data_ptr(), X.data_ptr(), W.data_ptr(), B, Cin, Cout, HW, dX.data_ptr(),
          dW.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return {"dX": dX, "dW": dW, "db": db}


# ------------------------------------------------------------------------------------------------ the encoder
def _check_coor(coor, dev):
    if coor.dim() != 4 or coor.shape[1] != 3 or coor.shape[2] != coor.shape[3] or coor.shape[2] % 8 or coor.shape[0] == 0:
        raise ValueError(f"coor {tuple(coor.shape)}, expected (B,3,R,R) with R a multiple of 8")
    return _f32(coor, dev)


@torch.no_grad()
def enc_forward_save(coor, params, groups=None, alloc=None):
    """MAPEncoder.forward in fp32 (gpe_map_encoder_forward_save): coor (B,3,R,R), params {name: fp32 device tensor} over PARAM_KEYS
    -> the list of the coupling batches' saved activations (saved_shapes), in batch order; saved["act"][2] (N,256,R/8,R/8) is a
    batch's result."""
    dev = _dev(coor)
    coor = _check_coor(coor, dev)
    B, R = coor.shape[0], coor.shape[2]
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    pw = _params_struct(params, "params")
    out, i0 = [], 0
    for N in _groups(groups, B):
        saved = {k: [alloc(f"{k}{l}", s) for l, s in enumerate(v)] for k, v in saved_shapes(N, R).items()}
        nbytes = L.gpe_map_encoder_forward_workspace(N, R)
        ws = _ws(alloc, nbytes)
        sv = _saved_struct(saved, N, R)
        _call(dev, L.gpe_map_encoder_forward_save, "gpe_map_encoder_forward_save", coor[i0:i0 + N].data_ptr(), ctypes.byref(pw), N, R,
              ctypes.byref(sv), ws.data_ptr(), nbytes, _stream(dev))
        out.append(saved)
        i0 += N
    return out


@torch.no_grad()
def enc_backward(params, saved, coor, g_feat, alloc=None, scatter="atomic"):
    """gpe_map_encoder_backward per coupling batch: from d nocs_feat (B,256,R/8,R/8), coor and what enc_forward_save returned for it
    (and the same params) -> ({name: gradient} over PARAM_KEYS, the batches' gradients added in batch order, d coor (B,3,R,R)).
    scatter "atomic": equal to rounding between runs outside ATOMIC_FREE_KEYS; "ordered" (gpeo_map_encoder_backward): equal bits in
    all of ORDERED_FREE_KEYS and d coor."""
    mode = scatter_mode(scatter)
    dev = _dev(coor)
    coor = _check_coor(coor, dev)
    B, R = coor.shape[0], coor.shape[2]
    groups = [s["act"][2].shape[0] for s in saved]
    if sum(groups) != B:
        raise ValueError(f"saved holds batches of {groups} crops, coor {B}")
    g_feat = _f32(g_feat, dev, (B, 256, R // 8, R // 8), "g_feat")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    pw = _params_struct(params, "params")
    g_coor = alloc("coor", (B, 3, R, R))
    total, i0 = None, 0
    for N, sv_t in zip(groups, saved):
        grads = {k: alloc(k, s) for k, s in param_shapes().items()}
        ordered = mode != _lib.GPE_SCATTER_ATOMIC
        nbytes = L.gpeo_map_encoder_backward_workspace(N, R, mode) if ordered else L.gpe_map_encoder_backward_workspace(N, R)
        ws = _ws(alloc, nbytes)
        sv, pg = _saved_struct(sv_t, N, R), _params_struct(grads, "grads")
        args = (ctypes.byref(pw), ctypes.byref(sv), coor[i0:i0 + N].data_ptr(), g_feat[i0:i0 + N].data_ptr(), N, R, ctypes.byref(pg),
                g_coor[i0:i0 + N].data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
        if ordered:
            _call(dev, L.gpeo_map_encoder_backward, "gpeo_map_encoder_backward", *args, mode)
        else:
            _call(dev, L.gpe_map_encoder_backward, "gpe_map_encoder_backward", *args)
        total = grads if total is None else {k: total[k] + grads[k] for k in PARAM_KEYS}
        i0 += N
    return total, g_coor
