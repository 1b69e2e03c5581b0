"""The pose-head backward family (include/givepose_headgrad.h, gph_*): ConvPnPNet's fp32 forward-that-saves and its backward.

Everything runs on the device in this library's HIP kernels; there is no CPU path.  Tensors are fp32 in the reference's own
layouts (NCHW activations, OIHW conv weights, (out, in) linear weights with fc1's columns in the NCHW flatten order), so a
gradient lies under the index of its parameter and nothing has to be permuted back.

`alloc(name, shape)` -- an optional hook every function takes -- supplies the output and workspace buffers (fp32, contiguous, on
the device; workspaces 256-byte aligned); the default is torch.empty.  The tests use it to put sentinels around every buffer.
"""
import ctypes

import torch

from . import _lib

# the 23 tensors of pnp_net in the order of gph_pnp_params, named as in the reference's state_dict (without the prefix)
PARAM_KEYS = ([f"features.{i}.weight" for i in (0, 3, 6)] + [f"features.{i}.weight" for i in (1, 4, 7)]
              + [f"features.{i}.bias" for i in (1, 4, 7)]
              + [f"{n}.{p}" for n in ("fc1", "fc1_z", "fc2", "fc2_z", "fc_r", "fc_t", "fc_z") for p in ("weight", "bias")])
SAVED_KEYS = ("x0", "conv", "mean", "rstd", "act", "h1", "h2", "h2z", "pred_rot", "pred_t")


def param_shapes(rot_dim=6):
    """name -> shape of every pnp_net parameter (ConvPnPNet, flat_op 'flatten', five input channels)."""
    s = {"features.0.weight": (128, 5, 3, 3), "features.3.weight": (128, 128, 3, 3), "features.6.weight": (128, 128, 3, 3)}
    for i in (1, 4, 7):
        s[f"features.{i}.weight"] = s[f"features.{i}.bias"] = (128,)
    for n, (o, i) in {"fc1": (1024, 8192), "fc1_z": (1024, 8192), "fc2": (256, 1024), "fc2_z": (256, 1024), "fc_r": (rot_dim, 256),
                      "fc_t": (2, 256), "fc_z": (1, 256)}.items():
        s[n + ".weight"], s[n + ".bias"] = (o, i), (o,)
    return {k: s[k] for k in PARAM_KEYS}


def _default_alloc(dev):
    return lambda name, shape: torch.empty(shape, device=dev, dtype=torch.float32)


def _dev(t):
    if t.device.type != "cuda":
        raise _lib.GivePoseHipError("the pose-head backward runs on a HIP device only: there is no CPU path")
    return t.device


def _f32(t, dev, shape=None, name="tensor"):
    t = torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _ws(alloc, nbytes):
    ws = alloc("workspace", (max(int(nbytes) // 4, 64),))
    assert ws.data_ptr() % 256 == 0, "workspace buffers must be 256-byte aligned"
    return ws


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _params_struct(tensors, rot_dim, what):
    shapes = param_shapes(rot_dim)
    st = _lib.PnpParams()
    for idx, (k, field) in enumerate(zip(PARAM_KEYS, _lib.PnpParams.FIELDS)):
        t = tensors[k]
        if tuple(t.shape) != shapes[k] or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what}[{k}]: {tuple(t.shape)} {t.dtype}, expected contiguous float32 {shapes[k]}")
        if idx < 9:
            getattr(st, field)[idx % 3] = t.data_ptr()
        else:
            setattr(st, field, t.data_ptr())
    return st


def saved_shapes(B, rot_dim=6):
    return {"x0": (B, 5, 64, 64), "conv": [(B, 128, r, r) for r in (32, 16, 8)], "mean": [(B, 32)] * 3, "rstd": [(B, 32)] * 3,
            "act": [(B, 128, r, r) for r in (32, 16, 8)], "h1": (B, 2048), "h2": (B, 256), "h2z": (B, 256), "pred_rot": (B, rot_dim),
            "pred_t": (B, 3)}


def _saved_struct(saved):
    st = _lib.PnpSaved()
    for k in SAVED_KEYS:
        v = saved[k]
        if isinstance(v, (list, tuple)):
            for i in range(3):
                getattr(st, k)[i] = v[i].data_ptr()
        else:
            setattr(st, k, v.data_ptr())
    return st


# ------------------------------------------------------------------------------------------------ the pieces
@torch.no_grad()
def linear_backward(dY, W, X, Y=None, accumulate_into=None, alloc=None):
    """Backward of Y = LeakyReLU_0.1(X W^T + b) (no activation when Y is None): dY (M,N), W (N,K), X (M,K), Y the saved output
    -> {"dX": (M,K), "dW": (N,K), "db": (N,)}.  accumulate_into (M,K): dX is added to it, in place."""
    dev = _dev(dY)
    M, N = dY.shape
    K = W.shape[1]
    dY, W, X = _f32(dY, dev), _f32(W, dev, (N, K), "W"), _f32(X, dev, (M, K), "X")
    Y = None if Y is None else _f32(Y, dev, (M, N), "Y")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    dX = accumulate_into if accumulate_into is not None else alloc("dX", (M, K))
    dW, db = alloc("dW", (N, K)), alloc("db", (N,))
    nbytes = L.gph_linear_backward_workspace(M, N, K)
    ws = _ws(alloc, nbytes)
    with torch.cuda.device(dev):
        _lib.check(L.gph_linear_backward(dY.data_ptr(), N, Y.data_ptr() if Y is not None else 0, N, W.data_ptr(), X.data_ptr(), K, M, N, K,
                                         int(accumulate_into is not None), dX.data_ptr(), K, dW.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                         nbytes, _stream(dev)), "gph_linear_backward")
    return {"dX": dX, "dW": dW, "db": db}


@torch.no_grad()
def gn_relu_backward(dout, out, x, mean, rstd, gamma, alloc=None):
    """Backward of out = ReLU(GroupNorm_32x4(x)) on (B,C,H,W) given the saved output, mean and rstd (B,C/4)
    -> {"dx", "dgamma", "dbeta"}."""
    dev = _dev(dout)
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    dout, out, x = _f32(dout, dev, x.shape, "dout"), _f32(out, dev, x.shape, "out"), _f32(x, dev)
    mean, rstd, gamma = _f32(mean, dev, (B, C // 4), "mean"), _f32(rstd, dev, (B, C // 4), "rstd"), _f32(gamma, dev, (C,), "gamma")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    dx, dg, db = alloc("dx", tuple(x.shape)), alloc("dgamma", (C,)), alloc("dbeta", (C,))
    nbytes = L.gph_gn_relu_backward_workspace(B, C)
    ws = _ws(alloc, nbytes)
    with torch.cuda.device(dev):
        _lib.check(L.gph_gn_relu_backward(dout.data_ptr(), out.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                          B, C, HW, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, _stream(dev)),
                   "gph_gn_relu_backward")
    return {"dx": dx, "dgamma": dg, "dbeta": db}


@torch.no_grad()
def conv3x3s2_backward(dY, X, W, mask=None, cin_dx=None, alloc=None):
    """Backward of F.conv2d(X, W, stride=2, padding=1) without bias: dY (B,Cout,H/2,H/2), X (B,Cin,H,H), W (Cout,Cin,3,3)
    -> {"dX": (B,cin_dx,H,H) -- the first cin_dx (default all) input channels, times mask (B,1,H,H) when given --, "dW"}."""
    dev = _dev(dY)
    B, Cin, H = X.shape[0], X.shape[1], X.shape[2]
    Cout = W.shape[0]
    cin_dx = Cin if cin_dx is None else int(cin_dx)
    dY, X, W = _f32(dY, dev, (B, Cout, H // 2, H // 2), "dY"), _f32(X, dev, (B, Cin, H, H), "X"), _f32(W, dev, (Cout, Cin, 3, 3), "W")
    mask = None if mask is None else _f32(mask, dev, (B, 1, H, H), "mask")
    alloc = alloc or _default_alloc(dev)
    L = _lib.load()
    dX, dW = alloc("dX", (B, cin_dx, H, H)), alloc("dW", (Cout, Cin, 3, 3))
    nbytes = L.gph_conv3x3s2_backward_workspace(B, Cin, Cout, H, cin_dx)
    ws = _ws(alloc, nbytes)
    with torch.cuda.device(dev):
        _lib.check(L.gph_conv3x3s2_backward(dY.data_ptr(), X.data_ptr(), W.data_ptr(), mask.data_ptr() if mask is not None else 0, B, Cin,
                                            Cout, H, cin_dx, dX.data_ptr(), dW.data_ptr(), ws.data_ptr(), nbytes, _stream(dev)),
                   "gph_conv3x3s2_backward")
    return {"dX": dX, "dW": dW}


# ------------------------------------------------------------------------------------------------ the head
@torch.no_grad()
def pnp_forward_save(ivfc, roi_coord_2d, params, mask=None, rot_dim=6, alloc=None):
    """ConvPnPNet.forward in fp32 (gph_pnp_forward_save): ivfc (B,3,64,64), roi_coord_2d (B,2,64,64), mask (B,1,64,64) or None
    (mask_attention_type 'mul'), params {name: fp32 device tensor} over PARAM_KEYS -> the saved activations (saved_shapes)."""
    dev = _dev(ivfc)
    B = ivfc.shape[0]
    if B == 0:
        raise ValueError("empty batch")
    ivfc, coord = _f32(ivfc, dev, (B, 3, 64, 64), "ivfc_coor"), _f32(roi_coord_2d, dev, (B, 2, 64, 64), "roi_coord_2d")
    mask = None if mask is None else _f32(mask, dev, (B, 1, 64, 64), "mask")
    alloc = alloc or _default_alloc(dev)
    saved = {k: [alloc(f"{k}{i}", s) for i, s in enumerate(v)] if isinstance(v, list) else alloc(k, v) for k, v in saved_shapes(B, rot_dim).items()}
    L = _lib.load()
    nbytes = L.gph_pnp_forward_workspace(B, rot_dim)
    ws = _ws(alloc, nbytes)
    pw, sv = _params_struct(params, rot_dim, "params"), _saved_struct(saved)
    with torch.cuda.device(dev):
        _lib.check(L.gph_pnp_forward_save(ivfc.data_ptr(), coord.data_ptr(), mask.data_ptr() if mask is not None else 0, ctypes.byref(pw), B,
                                          rot_dim, ctypes.byref(sv), ws.data_ptr(), nbytes, _stream(dev)), "gph_pnp_forward_save")
    return saved


@torch.no_grad()
def pnp_backward(params, saved, g_pred_rot, g_pred_t, mask=None, alloc=None):
    """gph_pnp_backward: from d pred_rot (B,rot_dim), d pred_t (B,3) and what pnp_forward_save returned (for the same params and mask)
    -> ({name: gradient} over PARAM_KEYS, the head's part of d ivfc_coor (B,3,64,64))."""
    dev = _dev(saved["x0"])
    B, rot_dim = saved["pred_rot"].shape
    g_rot, g_t = _f32(g_pred_rot, dev, (B, rot_dim), "g_pred_rot"), _f32(g_pred_t, dev, (B, 3), "g_pred_t")
    mask = None if mask is None else _f32(mask, dev, (B, 1, 64, 64), "mask")
    alloc = alloc or _default_alloc(dev)
    grads = {k: alloc(k, s) for k, s in param_shapes(rot_dim).items()}
    g_ivfc = alloc("ivfc_coor", (B, 3, 64, 64))
    L = _lib.load()
    nbytes = L.gph_pnp_backward_workspace(B, rot_dim)
    ws = _ws(alloc, nbytes)
    pw, sv, pg = _params_struct(params, rot_dim, "params"), _saved_struct(saved), _params_struct(grads, rot_dim, "grads")
    with torch.cuda.device(dev):
        _lib.check(L.gph_pnp_backward(ctypes.byref(pw), ctypes.byref(sv), mask.data_ptr() if mask is not None else 0, g_rot.data_ptr(),
                                      g_t.data_ptr(), B, rot_dim, ctypes.byref(pg), g_ivfc.data_ptr(), ws.data_ptr(), nbytes, _stream(dev)),
                   "gph_pnp_backward")
    return grads, g_ivfc
