"""The coordinate-head backward family (include/givepose_xyzgrad.h, gpx_*): TopDownXyzHead's fp32 forward-that-saves and its
backward, and the operators they are made of.

Everything runs on the device in this library's HIP kernels; there is no CPU path.  Tensors are fp32 in the reference's own
layouts (NCHW activations, OIHW conv weights, the transposed conv's weight (Cin,256,3,3) as nn.ConvTranspose2d stores it), so a
gradient lies under the index of its parameter and nothing has to be permuted back.

`alloc(name, shape)` -- an optional hook every function takes -- supplies the output and workspace buffers (fp32, contiguous, on
the device; workspaces 256-byte aligned); the default is torch.empty.  The tests use it to put sentinels around every buffer.

`precision="fp32"` (the default) is the gpx_ entry points themselves.  `precision="bf16"` on the 3x3 convs, the transposed conv and
the head (include/givepose_xyzgrad_bf16.h, gpxm_*) multiplies bf16-rounded operands and adds in fp32 in the 21 contractions of the
3x3 layers; GroupNorm + GELU, the bilinear x2 and the 1x1 output conv stay fp32, and so does everything in memory.
"""
import ctypes

import torch

from . import _lib
from .pnp_grad import _default_alloc, _f32, _stream, _ws

CONV_IDS = (3, 4, 6, 7, 9, 10)
# the 23 tensors of one head in the order of gpx_xyz_params, named as in the reference's state_dict (without the prefix)
PARAM_KEYS = (["features.0.weight"] + [f"features.{i}.conv.weight" for i in CONV_IDS]
              + ["features.1.weight"] + [f"features.{i}.norm.weight" for i in CONV_IDS]
              + ["features.1.bias"] + [f"features.{i}.norm.bias" for i in CONV_IDS]
              + ["out_layer.weight", "out_layer.bias"])
# ConvModule registers its norm twice: features.N.gn.* is the same Parameter as features.N.norm.*
ALIASES = {f"features.{i}.gn.{p}": f"features.{i}.norm.{p}" for i in CONV_IDS for p in ("weight", "bias")}
SAVED_KEYS = ("pre", "mean", "rstd", "act", "up", "coor")
LAYER_MUL = (2, 2, 2, 4, 4, 8, 8)      # layer l runs at H0 * LAYER_MUL[l]


def param_shapes(Cin):
    """name -> shape of every parameter of a TopDownXyzHead with in_dim Cin (1024: xyz_nocs_head, 512: xyz_deform_head)."""
    s = {"features.0.weight": (Cin, 256, 3, 3), "out_layer.weight": (3, 256, 1, 1), "out_layer.bias": (3,)}
    for k in PARAM_KEYS:
        if k.endswith("conv.weight"):
            s[k] = (256, 256, 3, 3)
        elif k not in s:
            s[k] = (256,)
    return {k: s[k] for k in PARAM_KEYS}


def saved_shapes(B, Cin, H0):
    """name -> shape(s) of what xyz_forward_save writes (gpx_xyz_saved); Cin does not enter: the input feature is not saved."""
    maps = [(B, 256, H0 * m, H0 * m) for m in LAYER_MUL]
    return {"pre": maps, "mean": [(B, 32)] * 7, "rstd": [(B, 32)] * 7, "act": list(maps),
            "up": [(B, 256, 4 * H0, 4 * H0), (B, 256, 8 * H0, 8 * H0)], "coor": (B, 3, 8 * H0, 8 * H0)}


def _dev(t):
    if t.device.type != "cuda":
        raise _lib.GivePoseHipError("the coordinate-head backward runs on a HIP device only: there is no CPU path")
    return t.device


def _params_struct(tensors, Cin, what):
    shapes = param_shapes(Cin)
    for k in PARAM_KEYS:
        t = tensors[k]
        if tuple(t.shape) != shapes[k] or t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != "cuda":
            raise ValueError(f"{what}[{k}]: {tuple(t.shape)} {t.dtype} on {t.device}, expected contiguous float32 {shapes[k]} on the device")
    st = _lib.XyzParams()
    ptr = [tensors[k].data_ptr() for k in PARAM_KEYS]
    st.deconv_w = ptr[0]
    for i in range(6):
        st.conv_w[i] = ptr[1 + i]
    for i in range(7):
        st.gn_w[i], st.gn_b[i] = ptr[7 + i], ptr[14 + i]
    st.out_w, st.out_b = ptr[21], ptr[22]
    return st


def _saved_struct(saved, B, Cin, H0):
    st = _lib.XyzSaved()
    for k, shp in saved_shapes(B, Cin, H0).items():
        v = saved[k]
        for i, (t, s) in enumerate(zip(v, shp) if isinstance(shp, list) else [(v, shp)]):
            if tuple(t.shape) != tuple(s) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"saved[{k}]: {tuple(t.shape)} {t.dtype}, expected contiguous float32 {tuple(s)}")
            if isinstance(shp, list):
                getattr(st, k)[i] = t.data_ptr()
            else:
                setattr(st, k, t.data_ptr())
    return st


PRECISIONS = {"fp32": _lib.GPX_PREC_F32, "bf16": _lib.GPX_PREC_BF16}


def _prec(precision):
    """The GPX_PREC_* value of "fp32" or "bf16" (include/givepose_xyzgrad_bf16.h)."""
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"precision: {precision!r}, expected 'fp32' or 'bf16'")
    return PRECISIONS[precision]


def _entry(L, stem, prec):
    """(function, its name, trailing arguments) of gpx_<stem> in a precision: "fp32" is the gpx_ entry point itself."""
    if prec == _lib.GPX_PREC_F32:
        return getattr(L, "gpx_" + stem), "gpx_" + stem, ()
    return getattr(L, "gpxm_" + stem), "gpxm_" + stem, (prec,)


def _query(L, stem, prec, *args):
    fn, _, tail = _entry(L, stem, prec)
    return fn(*args, *tail)


def _call(dev, fn, name, *args):
    with torch.cuda.device(dev):
        _lib.check(fn(*args), name)


# ------------------------------------------------------------------------------------------------ the pieces
def _conv_args(X, W, transposed):
    dev = _dev(X)
    B, Cin, H = X.shape[0], X.shape[1], X.shape[2]
    Cout = W.shape[1] if transposed else W.shape[0]
    X = _f32(X, dev, (B, Cin, H, H), "X")
    W = _f32(W, dev, (Cin, Cout, 3, 3) if transposed else (Cout, Cin, 3, 3), "W")
    return dev, B, Cin, Cout, H, X, W


@torch.no_grad()
def conv3x3s1_forward(X, W, alloc=None, precision="fp32"):
    """F.conv2d(X, W, padding=1) without bias: X (B,Cin,H,H), W (Cout,Cin,3,3) -> (B,Cout,H,H), fp32.
    precision="bf16": the contraction multiplies bf16-rounded operands and adds in fp32 (gpxm_conv3x3s1_forward)."""
    prec = _prec(precision)
    dev, B, Cin, Cout, H, X, W = _conv_args(X, W, False)
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    Y = alloc("Y", (B, Cout, H, H))
    nbytes = _query(L, "conv3x3s1_workspace", prec, B, Cin, Cout, H)
    ws = _ws(alloc, nbytes)
    fn, name, tail = _entry(L, "conv3x3s1_forward", prec)
    _call(dev, fn, name, X.data_ptr(), W.data_ptr(), B, Cin, Cout, H, Y.data_ptr(), ws.data_ptr(), nbytes, _stream(dev), *tail)
    return Y


@torch.no_grad()
def conv3x3s1_backward(dY, X, W, alloc=None, precision="fp32"):
    """Backward of F.conv2d(X, W, padding=1) without bias: dY (B,Cout,H,H) -> {"dX": (B,Cin,H,H), "dW": (Cout,Cin,3,3)}.
    precision="bf16": both contractions multiply bf16-rounded operands and add in fp32 (gpxm_conv3x3s1_backward)."""
    prec = _prec(precision)
    dev, B, Cin, Cout, H, X, W = _conv_args(X, W, False)
    dY = _f32(dY, dev, (B, Cout, H, H), "dY")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    dX, dW = alloc("dX", (B, Cin, H, H)), alloc("dW", (Cout, Cin, 3, 3))
    nbytes = _query(L, "conv3x3s1_workspace", prec, B, Cin, Cout, H)
    ws = _ws(alloc, nbytes)
    fn, name, tail = _entry(L, "conv3x3s1_backward", prec)
    _call(dev, fn, name, dY.data_ptr(), X.data_ptr(), W.data_ptr(), B, Cin, Cout, H, dX.data_ptr(), dW.data_ptr(), ws.data_ptr(), nbytes,
          _stream(dev), *tail)
    return {"dX": dX, "dW": dW}


@torch.no_grad()
def deconv3x3s2_forward(X, W, alloc=None, precision="fp32"):
    """F.conv_transpose2d(X, W, stride=2, padding=1, output_padding=1) without bias: X (B,Cin,H,H), W (Cin,Cout,3,3)
    -> (B,Cout,2H,2H), fp32.  precision="bf16": bf16-rounded operands, fp32 sums (gpxm_deconv3x3s2_forward)."""
    prec = _prec(precision)
    dev, B, Cin, Cout, H, X, W = _conv_args(X, W, True)
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    Y = alloc("Y", (B, Cout, 2 * H, 2 * H))
    nbytes = _query(L, "deconv3x3s2_workspace", prec, B, Cin, Cout, H)
    ws = _ws(alloc, nbytes)
    fn, name, tail = _entry(L, "deconv3x3s2_forward", prec)
    _call(dev, fn, name, X.data_ptr(), W.data_ptr(), B, Cin, Cout, H, Y.data_ptr(), ws.data_ptr(), nbytes, _stream(dev), *tail)
    return Y


@torch.no_grad()
def deconv3x3s2_backward(dY, X, W, alloc=None, precision="fp32"):
    """Backward of the transposed conv: dY (B,Cout,2H,2H) -> {"dX": (B,Cin,H,H), "dW": (Cin,Cout,3,3)}.
    precision="bf16": both contractions multiply bf16-rounded operands and add in fp32 (gpxm_deconv3x3s2_backward)."""
    prec = _prec(precision)
    dev, B, Cin, Cout, H, X, W = _conv_args(X, W, True)
    dY = _f32(dY, dev, (B, Cout, 2 * H, 2 * H), "dY")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    dX, dW = alloc("dX", (B, Cin, H, H)), alloc("dW", (Cin, Cout, 3, 3))
    nbytes = _query(L, "deconv3x3s2_workspace", prec, B, Cin, Cout, H)
    ws = _ws(alloc, nbytes)
    fn, name, tail = _entry(L, "deconv3x3s2_backward", prec)
    _call(dev, fn, name, dY.data_ptr(), X.data_ptr(), W.data_ptr(), B, Cin, Cout, H, dX.data_ptr(), dW.data_ptr(), ws.data_ptr(), nbytes,
          _stream(dev), *tail)
    return {"dX": dX, "dW": dW}


@torch.no_grad()
def gn_gelu_backward(dout, x, mean, rstd, gamma, beta, groups=32, alloc=None):
    """Backward of out = GELU(GroupNorm_groups(x)) on (B,C,H,W) or (B,C,HW) given the saved x, mean and rstd (B,groups)
    -> {"dx", "dgamma", "dbeta"}."""
    dev = _dev(dout)
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    dout, x = _f32(dout, dev, x.shape, "dout"), _f32(x, dev)
    mean, rstd = _f32(mean, dev, (B, groups), "mean"), _f32(rstd, dev, (B, groups), "rstd")
    gamma, beta = _f32(gamma, dev, (C,), "gamma"), _f32(beta, dev, (C,), "beta")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    dx, dg, db = alloc("dx", tuple(x.shape)), alloc("dgamma", (C,)), alloc("dbeta", (C,))
    nbytes = L.gpx_gn_gelu_backward_workspace(B, C)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpx_gn_gelu_backward, "gpx_gn_gelu_backward", dout.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
          beta.data_ptr(), B, C, HW, groups, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return {"dx": dx, "dgamma": dg, "dbeta": db}


@torch.no_grad()
def upsample_bilinear2x_forward(x, alloc=None):
    """UpsamplingBilinear2d(scale_factor=2) (align_corners=True) in fp32: (B,C,H,H) -> (B,C,2H,2H)."""
    dev = _dev(x)
    B, C, H = x.shape[:3]
    x = _f32(x, dev, (B, C, H, H), "x")
    y = (alloc or _default_alloc(dev))("y", (B, C, 2 * H, 2 * H))
    L = _lib.load()
    _call(dev, L.gpx_upsample_bilinear2x_forward, "gpx_upsample_bilinear2x_forward", x.data_ptr(), B, C, H, y.data_ptr(), _stream(dev))
    return y


@torch.no_grad()
def upsample_bilinear2x_backward(dy, alloc=None):
    """The transpose of upsample_bilinear2x_forward: dy (B,C,2H,2H) -> (B,C,H,H)."""
    dev = _dev(dy)
    B, C, H2 = dy.shape[:3]
    if H2 % 2:
        raise ValueError(f"dy: {tuple(dy.shape)} is not the shape of a x2 upsampled map")
    dy = _f32(dy, dev, (B, C, H2, H2), "dy")
    dx = (alloc or _default_alloc(dev))("dx", (B, C, H2 // 2, H2 // 2))
    L = _lib.load()
    _call(dev, L.gpx_upsample_bilinear2x_backward, "gpx_upsample_bilinear2x_backward", dy.data_ptr(), B, C, H2 // 2, dx.data_ptr(), _stream(dev))
    return dx


@torch.no_grad()
def conv1x1_backward(dY, X, W, alloc=None):
    """Backward of F.conv2d(X, W, bias) with a 1x1 kernel: dY (B,Cout,...), X (B,Cin,...), W (Cout,Cin[,1,1])
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
    nbytes = L.gpx_conv1x1_backward_workspace(B, Cin, Cout, HW)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpx_conv1x1_backward, "gpx_conv1x1_backward", dY.data_ptr(), X.data_ptr(), W.data_ptr(), B, Cin, Cout, HW, dX.data_ptr(),
          dW.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return {"dX": dX, "dW": dW, "db": db}


# ------------------------------------------------------------------------------------------------ the head
@torch.no_grad()
def xyz_forward_save(feat, params, alloc=None, precision="fp32"):
    """TopDownXyzHead.forward in fp32 (gpx_xyz_forward_save): feat (B,Cin,H0,H0), params {name: fp32 device tensor} over PARAM_KEYS
    -> the saved activations (saved_shapes); saved["coor"] (B,3,8 H0,8 H0) is the head's result.
    precision="bf16": the transposed conv and the six 3x3 convs multiply bf16-rounded operands and add in fp32
    (gpxm_xyz_forward_save); what is saved has the same shapes and dtypes."""
    prec = _prec(precision)
    dev = _dev(feat)
    B, Cin, H0 = feat.shape[:3]
    if B == 0:
        raise ValueError("empty batch")
    feat = _f32(feat, dev, (B, Cin, H0, H0), "feat")
    alloc = alloc or _default_alloc(dev)
    saved = {k: [alloc(f"{k}{i}", s) for i, s in enumerate(v)] if isinstance(v, list) else alloc(k, v)
             for k, v in saved_shapes(B, Cin, H0).items()}
    L = _lib.load()
    nbytes = _query(L, "xyz_forward_workspace", prec, B, Cin, H0)
    ws = _ws(alloc, nbytes)
    pw, sv = _params_struct(params, Cin, "params"), _saved_struct(saved, B, Cin, H0)
    fn, name, tail = _entry(L, "xyz_forward_save", prec)
    _call(dev, fn, name, feat.data_ptr(), ctypes.byref(pw), B, Cin, H0, ctypes.byref(sv), ws.data_ptr(), nbytes, _stream(dev), *tail)
    return saved


@torch.no_grad()
def xyz_backward(params, saved, feat, g_coor, alloc=None, precision="fp32"):
    """gpx_xyz_backward: from d coor (B,3,8 H0,8 H0), the head's input feat and what xyz_forward_save returned for it (and the same
    params) -> ({name: gradient} over PARAM_KEYS, d feat (B,Cin,H0,H0)).
    precision="bf16": dX and dW of the transposed conv and of the six 3x3 convs multiply bf16-rounded operands and add in fp32
    (gpxm_xyz_backward); `saved` may come from a forward of either precision."""
    prec = _prec(precision)
    dev = _dev(feat)
    B, Cin, H0 = feat.shape[:3]
    feat = _f32(feat, dev, (B, Cin, H0, H0), "feat")
    g_coor = _f32(g_coor, dev, (B, 3, 8 * H0, 8 * H0), "g_coor")
    alloc = alloc or _default_alloc(dev)
    grads = {k: alloc(k, s) for k, s in param_shapes(Cin).items()}
    g_feat = alloc("feat", (B, Cin, H0, H0))
    L = _lib.load()
    nbytes = _query(L, "xyz_backward_workspace", prec, B, Cin, H0)
    ws = _ws(alloc, nbytes)
    pw, sv, pg = _params_struct(params, Cin, "params"), _saved_struct(saved, B, Cin, H0), _params_struct(grads, Cin, "grads")
    fn, name, tail = _entry(L, "xyz_backward", prec)
    _call(dev, fn, name, ctypes.byref(pw), ctypes.byref(sv), feat.data_ptr(), g_coor.data_ptr(), B, Cin, H0, ctypes.byref(pg),
          g_feat.data_ptr(), ws.data_ptr(), nbytes, _stream(dev), *tail)
    return grads, g_feat
