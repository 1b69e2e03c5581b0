"""The backbone backward family (include/givepose_bbgrad.h, gpb_*): the ConvNeXt backbone's fp32 forward-that-saves and its backward,
and the operators they are made of (depth-wise 7x7, LayerNorm over channels, the patch convs, the block).

Everything runs on the device in this library's HIP kernels; there is no CPU path.  Parameters and their gradients are fp32 in the
reference's own shapes under their state_dict names (without the "backbone." prefix); the image, feat and their gradients are NCHW,
what is saved in between is channels-last rows (b,h,w) x C (`saved_shapes`).

`cfg` is anything with `convnext_dims` and `convnext_depths` (a PoseNetConfig), or the pair (dims, depths).  Every dim must be a
multiple of 64, the image side a multiple of 4 * 2^(stages - 1).

There is no atomic in this family: equal inputs give equal bits, and the gradients are linear in g_feat bit for bit under a
scaling by a power of two.

Unlike the conversions of the earlier families, every tensor argument is checked, not converted: fp32, contiguous, on the device, of
the stated shape.  `alloc(name, shape)` -- an optional hook every function takes -- supplies the output and workspace buffers; the
default is torch.empty.  The tests use it to put sentinels around every buffer.
"""
import ctypes

import torch

from . import _lib
from .pnp_grad import _default_alloc, _stream, _ws

BLOCK_KEYS = ("gamma", "conv_dw.weight", "conv_dw.bias", "norm.weight", "norm.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
              "mlp.fc2.bias")
BLOCK_SAVED = ("x", "dwout", "mean", "rstd", "h", "y2")
NORM_SAVED = ("pre", "mean", "rstd")


def _dd(cfg):
    dims, depths = (cfg.convnext_dims, cfg.convnext_depths) if hasattr(cfg, "convnext_dims") else cfg
    dims, depths = tuple(int(d) for d in dims), tuple(int(d) for d in depths)
    if len(dims) != len(depths) or not 1 <= len(dims) <= _lib.GPB_MAX_STAGES:
        raise ValueError(f"dims {dims} and depths {depths} must list the same 1 .. {_lib.GPB_MAX_STAGES} stages")
    for s, d in enumerate(dims):
        if d <= 0 or d % 64:
            raise ValueError(f"dims[{s}] = {d} is not a multiple of 64: the depth-wise kernels hold a channel per lane of a 64-lane wavefront")
    if min(depths) < 1:
        raise ValueError(f"depths {depths}: every stage needs at least one block")
    return dims, depths


def block_shapes(C):
    """name -> shape of the nine tensors of a block with C channels, in state_dict order."""
    return dict(zip(BLOCK_KEYS, ((C,), (C, 1, 7, 7), (C,), (C,), (C,), (4 * C, C), (4 * C,), (C, 4 * C), (C,))))


def param_shapes(cfg):
    """name -> shape of every backbone parameter, in state_dict order (the order of a gpb parameter table)."""
    dims, depths = _dd(cfg)
    s = {"stem_0.weight": (dims[0], 3, 4, 4), "stem_0.bias": (dims[0],), "stem_1.weight": (dims[0],), "stem_1.bias": (dims[0],)}
    for i, (C, n) in enumerate(zip(dims, depths)):
        if i:
            q = f"stages_{i}.downsample."
            s[q + "0.weight"] = s[q + "0.bias"] = (dims[i - 1],)
            s[q + "1.weight"], s[q + "1.bias"] = (C, dims[i - 1], 2, 2), (C,)
        for b in range(n):
            s.update({f"stages_{i}.blocks.{b}.{k}": v for k, v in block_shapes(C).items()})
    return s


def PARAM_KEYS(cfg):
    """The backbone's parameter names in state_dict order, without the "backbone." prefix."""
    return list(param_shapes(cfg))


def _side(S, n):
    if S <= 0 or S % (4 << (n - 1)):
        raise ValueError(f"image side {S} is not a multiple of {4 << (n - 1)}")
    return [S // (4 << s) for s in range(n)]


def saved_shapes(cfg, B, S):
    """name -> shape of what backbone_forward_save keeps for B crops of side S, in the order of a gpb saved table: the stem's and every
    downsample's pre-norm map and statistics, and per block the input x, the depth-wise output with its LayerNorm's mean / rstd, the fc1
    pre-activation h and the fc2 output y2."""
    dims, depths = _dd(cfg)
    side = _side(S, len(dims))
    out = {}

    def norm(q, rows, C):
        out.update({q + "pre": (rows, C), q + "mean": (rows,), q + "rstd": (rows,)})

    norm("stem.", B * side[0] ** 2, dims[0])
    for i, (C, n) in enumerate(zip(dims, depths)):
        if i:
            norm(f"stages_{i}.downsample.", B * side[i - 1] ** 2, dims[i - 1])
        rows = B * side[i] ** 2
        for b in range(n):
            q = f"stages_{i}.blocks.{b}."
            out.update({q + "x": (rows, C), q + "dwout": (rows, C), q + "mean": (rows,), q + "rstd": (rows,), q + "h": (rows, 4 * C), q + "y2": (rows, C)})
    return out


def saved_bytes(cfg, B, S):
    n = 0
    for s in saved_shapes(cfg, B, S).values():
        k = 4
        for d in s:
            k *= d
        n += k
    return n


def _dev(t):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise _lib.GivePoseHipError("the backbone backward runs on a HIP device only: there is no CPU path")
    return t.device


def _chk(t, dev, shape, name):
    if not torch.is_tensor(t) or t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{name}: {got}, expected contiguous float32 {tuple(shape)} on {dev}")
    return t


def _call(dev, fn, name, *args):
    with torch.cuda.device(dev):
        _lib.check(fn(*args), name)


def _c64(C, name="C"):
    if C <= 0 or C % 64:
        raise ValueError(f"{name} = {C} is not a multiple of 64")


def _table(tensors, shapes, dev, what):
    t = (ctypes.c_void_p * len(shapes))()
    for i, (k, s) in enumerate(shapes.items()):
        if k not in tensors:
            raise ValueError(f"{what}: {k} is missing")
        t[i] = _chk(tensors[k], dev, s, f"{what}[{k}]").data_ptr()
    return t


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


PRECISIONS = {"fp32": _lib.GPB_PREC_F32, "bf16": _lib.GPB_PREC_BF16}


def _prec(precision):
    """The GPB_PREC_* value of "fp32" or "bf16" (include/givepose_bbgrad_bf16.h)."""
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"precision: {precision!r}, expected 'fp32' or 'bf16'")
    return PRECISIONS[precision]


def _entry(L, stem, prec):
    """(function, its name, trailing arguments) of gpb_<stem> in a precision: "fp32" is the gpb_ entry point itself."""
    if prec == _lib.GPB_PREC_F32:
        return getattr(L, "gpb_" + stem), "gpb_" + stem, ()
    return getattr(L, "gpbm_" + stem), "gpbm_" + stem, (prec,)


def _query(L, stem, prec, *args):
    fn, _, tail = _entry(L, stem, prec)
    return fn(*args, *tail)


def _block_struct(tensors, C, dev, what):
    st = _lib.BbBlockParams()
    for f, (k, s) in zip(_lib.BbBlockParams.FIELDS, block_shapes(C).items()):
        setattr(st, f, _chk(tensors[k], dev, s, f"{what}[{k}]").data_ptr())
    return st


# ------------------------------------------------------------------------------------------------ the pieces
@torch.no_grad()
def dw7_forward(x, w, b, alloc=None):
    """Depth-wise 7x7, pad 3, on x (N,H,W,C) channels-last with w (C,1,7,7), b (C) -> (N,H,W,C)."""
    dev = _dev(x)
    if x.dim() != 4:
        raise ValueError(f"x: {tuple(x.shape)}, expected (N,H,W,C)")
    N, H, W, C = x.shape
    _c64(C)
    _chk(x, dev, (N, H, W, C), "x"), _chk(w, dev, (C, 1, 7, 7), "w"), _chk(b, dev, (C,), "b")
    y = (alloc or _default_alloc(dev))("y", (N, H, W, C))
    _call(dev, _lib.load().gpb_dw7_forward, "gpb_dw7_forward", x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, C, y.data_ptr(), _stream(dev))
    return y


@torch.no_grad()
def dw7_backward(dy, x, w, alloc=None):
    """Backward of dw7_forward -> {"dx": (N,H,W,C), "dw": (C,1,7,7), "db": (C,)}."""
    dev = _dev(dy)
    if x.dim() != 4:
        raise ValueError(f"x: {tuple(x.shape)}, expected (N,H,W,C)")
    N, H, W, C = x.shape
    _c64(C)
    _chk(dy, dev, (N, H, W, C), "dy"), _chk(x, dev, (N, H, W, C), "x"), _chk(w, dev, (C, 1, 7, 7), "w")
    alloc = alloc or _default_alloc(dev)
    out = {"dx": alloc("dx", (N, H, W, C)), "dw": alloc("dw", (C, 1, 7, 7)), "db": alloc("db", (C,))}
    L = _lib.load()
    nbytes = L.gpb_dw7_backward_workspace(N, H, W, C)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpb_dw7_backward, "gpb_dw7_backward", dy.data_ptr(), x.data_ptr(), w.data_ptr(), N, H, W, C, out["dx"].data_ptr(),
          out["dw"].data_ptr(), out["db"].data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return out


@torch.no_grad()
def layernorm_forward_save(x, w, b, alloc=None):
    """LayerNorm over channels (eps 1e-6) of x (rows,C) -> {"y": (rows,C), "mean", "rstd": (rows,)}."""
    dev = _dev(x)
    rows, C = x.shape
    _c64(C)
    _chk(x, dev, (rows, C), "x"), _chk(w, dev, (C,), "w"), _chk(b, dev, (C,), "b")
    alloc = alloc or _default_alloc(dev)
    out = {"y": alloc("y", (rows, C)), "mean": alloc("mean", (rows,)), "rstd": alloc("rstd", (rows,))}
    _call(dev, _lib.load().gpb_layernorm_forward_save, "gpb_layernorm_forward_save", x.data_ptr(), w.data_ptr(), b.data_ptr(), rows, C,
          out["y"].data_ptr(), out["mean"].data_ptr(), out["rstd"].data_ptr(), _stream(dev))
    return out


@torch.no_grad()
def layernorm_backward(dy, x, mean, rstd, w, alloc=None):
    """Backward of layernorm_forward_save at the saved statistics -> {"dx": (rows,C), "dw", "db": (C,)}."""
    dev = _dev(dy)
    rows, C = x.shape
    _c64(C)
    _chk(dy, dev, (rows, C), "dy"), _chk(x, dev, (rows, C), "x"), _chk(mean, dev, (rows,), "mean"), _chk(rstd, dev, (rows,), "rstd")
    _chk(w, dev, (C,), "w")
    alloc = alloc or _default_alloc(dev)
    out = {"dx": alloc("dx", (rows, C)), "dw": alloc("dw", (C,)), "db": alloc("db", (C,))}
    L = _lib.load()
    nbytes = L.gpb_layernorm_backward_workspace(rows, C)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpb_layernorm_backward, "gpb_layernorm_backward", dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(),
          rows, C, out["dx"].data_ptr(), out["dw"].data_ptr(), out["db"].data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return out


def _patch_geometry(x, w, nchw):
    if x.dim() != 4 or w.dim() != 4 or w.shape[2] != w.shape[3]:
        raise ValueError(f"x {tuple(x.shape)}, w {tuple(w.shape)}: expected a 4-d input and an OIHW weight with a square kernel")
    N, Cin, H, W = x.shape if nchw else (x.shape[0], x.shape[3], x.shape[1], x.shape[2])
    Cout, p = w.shape[0], w.shape[2]
    if w.shape[1] != Cin or H % p or W % p:
        raise ValueError(f"x {tuple(x.shape)}, w {tuple(w.shape)}: the channels disagree or the map is no multiple of the patch")
    return N, H, W, Cin, Cout, p


@torch.no_grad()
def patch_conv_forward(x, w, b, nchw, alloc=None):
    """conv2d(x, w, b, stride = kernel) with non-overlapping patches: x (N,Cin,H,W) if nchw else (N,H,W,Cin), w (Cout,Cin,p,p)
    -> rows (N H/p W/p, Cout)."""
    dev = _dev(x)
    N, H, W, Cin, Cout, p = _patch_geometry(x, w, nchw)
    _chk(x, dev, x.shape, "x"), _chk(w, dev, (Cout, Cin, p, p), "w"), _chk(b, dev, (Cout,), "b")
    alloc = alloc or _default_alloc(dev)
    y = alloc("y", (N * (H // p) * (W // p), Cout))
    L = _lib.load()
    nbytes = L.gpb_patch_conv_workspace(N, H, W, Cin, Cout, p, int(bool(nchw)))
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpb_patch_conv_forward, "gpb_patch_conv_forward", x.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, Cin, Cout, p,
          int(bool(nchw)), y.data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return y


@torch.no_grad()
def patch_conv_backward(dy, x, w, nchw, alloc=None):
    """Backward of patch_conv_forward: dy rows (N H/p W/p, Cout) -> {"dX": like x, "dW": like w, "db": (Cout,)}."""
    dev = _dev(dy)
    N, H, W, Cin, Cout, p = _patch_geometry(x, w, nchw)
    _chk(dy, dev, (N * (H // p) * (W // p), Cout), "dy"), _chk(x, dev, x.shape, "x"), _chk(w, dev, (Cout, Cin, p, p), "w")
    alloc = alloc or _default_alloc(dev)
    out = {"dX": alloc("dX", tuple(x.shape)), "dW": alloc("dW", (Cout, Cin, p, p)), "db": alloc("db", (Cout,))}
    L = _lib.load()
    nbytes = L.gpb_patch_conv_workspace(N, H, W, Cin, Cout, p, int(bool(nchw)))
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpb_patch_conv_backward, "gpb_patch_conv_backward", dy.data_ptr(), x.data_ptr(), w.data_ptr(), N, H, W, Cin, Cout, p,
          int(bool(nchw)), out["dX"].data_ptr(), out["dW"].data_ptr(), out["db"].data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return out


@torch.no_grad()
def block_forward_save(x, params, alloc=None, precision="fp32"):
    """One ConvNeXt block on x (N,H,W,C): params {name over BLOCK_KEYS: tensor}
    -> {"dwout": (rows,C), "mean", "rstd": (rows,), "h": (rows,4C), "y2": (rows,C), "out": (N,H,W,C)}, rows = N H W.
    precision="bf16": fc1 and fc2 multiply bf16-rounded operands and add in fp32 (gpbm_block_forward_save); everything else, and
    every shape and dtype, is as in "fp32", which is gpb_block_forward_save bit for bit."""
    prec = _prec(precision)
    dev = _dev(x)
    if x.dim() != 4:
        raise ValueError(f"x: {tuple(x.shape)}, expected (N,H,W,C)")
    N, H, W, C = x.shape
    _c64(C)
    _chk(x, dev, (N, H, W, C), "x")
    st = _block_struct(params, C, dev, "params")
    alloc = alloc or _default_alloc(dev)
    rows = N * H * W
    out = {"dwout": alloc("dwout", (rows, C)), "mean": alloc("mean", (rows,)), "rstd": alloc("rstd", (rows,)), "h": alloc("h", (rows, 4 * C)),
           "y2": alloc("y2", (rows, C)), "out": alloc("out", (N, H, W, C))}
    L = _lib.load()
    nbytes = _query(L, "block_workspace", prec, N, H, W, C)
    ws = _ws(alloc, nbytes)
    fn, name, tail = _entry(L, "block_forward_save", prec)
    _call(dev, fn, name, x.data_ptr(), ctypes.byref(st), N, H, W, C,
          *(out[k].data_ptr() for k in ("dwout", "mean", "rstd", "h", "y2", "out")), ws.data_ptr(), nbytes, _stream(dev), *tail)
    return out


@torch.no_grad()
def block_backward(g, x, params, saved, alloc=None, precision="fp32"):
    """Backward of block_forward_save from g = d out (N,H,W,C) and what the forward saved
    -> {"dx": (N,H,W,C)} and the nine parameter gradients under BLOCK_KEYS.
    precision="bf16": the four contractions (d W2, d h, d W1, fc1's dX) multiply bf16-rounded operands and add in fp32; `saved` may
    come from a forward of either precision."""
    prec = _prec(precision)
    dev = _dev(g)
    if x.dim() != 4:
        raise ValueError(f"x: {tuple(x.shape)}, expected (N,H,W,C)")
    N, H, W, C = x.shape
    _c64(C)
    rows = N * H * W
    _chk(g, dev, (N, H, W, C), "g"), _chk(x, dev, (N, H, W, C), "x")
    for k, s in (("dwout", (rows, C)), ("mean", (rows,)), ("rstd", (rows,)), ("h", (rows, 4 * C)), ("y2", (rows, C))):
        _chk(saved[k], dev, s, f"saved[{k}]")
    st = _block_struct(params, C, dev, "params")
    alloc = alloc or _default_alloc(dev)
    out = {"dx": alloc("dx", (N, H, W, C)), **{k: alloc(k, s) for k, s in block_shapes(C).items()}}
    gs = _block_struct(out, C, dev, "grads")
    L = _lib.load()
    nbytes = _query(L, "block_workspace", prec, N, H, W, C)
    ws = _ws(alloc, nbytes)
    fn, name, tail = _entry(L, "block_backward", prec)
    _call(dev, fn, name, g.data_ptr(), x.data_ptr(), ctypes.byref(st),
          *(saved[k].data_ptr() for k in ("dwout", "mean", "rstd", "h", "y2")), N, H, W, C, ctypes.byref(gs), out["dx"].data_ptr(), ws.data_ptr(),
          nbytes, _stream(dev), *tail)
    return out


@torch.no_grad()
def matmul_bf16(a, b, trans_a=False, trans_b=False, alloc=None):
    """The bf16 contraction of the "bf16" precision as a piece of its own (gpbm_matmul_bf16): C (M,N) fp32 = op(a) op(b) with every
    element of a and b rounded to bf16 (nearest even) and the products added in fp32.  a is (M,K), or (K,M) with trans_a; b is (K,N),
    or (N,K) with trans_b; both contiguous float32 on the device.  No atomic: equal inputs give equal bits."""
    dev = _dev(a)
    if not torch.is_tensor(b) or a.dim() != 2 or b.dim() != 2:
        raise ValueError("a and b must be matrices")
    (K, M) = a.shape if trans_a else a.shape[::-1]
    (N, Kb) = b.shape if trans_b else b.shape[::-1]
    if K != Kb or min(M, N, K) < 1:
        raise ValueError(f"a {tuple(a.shape)} (trans_a={bool(trans_a)}) and b {tuple(b.shape)} (trans_b={bool(trans_b)}) do not contract")
    _chk(a, dev, a.shape, "a"), _chk(b, dev, b.shape, "b")
    alloc = alloc or _default_alloc(dev)
    c = alloc("c", (M, N))
    L = _lib.load()
    nbytes = L.gpbm_matmul_bf16_workspace(M, N, K)
    ws = _ws(alloc, nbytes)
    _call(dev, L.gpbm_matmul_bf16, "gpbm_matmul_bf16", a.data_ptr(), b.data_ptr(), M, N, K, int(bool(trans_a)), int(bool(trans_b)), c.data_ptr(),
          ws.data_ptr(), nbytes, _stream(dev))
    return c


# ------------------------------------------------------------------------------------------------ the backbone
def _check_img(img, dev, n):
    if not torch.is_tensor(img) or img.dim() != 4 or img.shape[0] < 1 or img.shape[1] != 3 or img.shape[2] != img.shape[3]:
        raise ValueError(f"img {tuple(img.shape) if torch.is_tensor(img) else img}, expected (B,3,S,S)")
    _side(img.shape[2], n)
    return _chk(img, dev, img.shape, "img")


@torch.no_grad()
def backbone_forward_save(img, params, cfg, alloc=None, precision="fp32"):
    """The ConvNeXt backbone in fp32 (gpb_backbone_forward_save): img (B,3,S,S), params {name: fp32 device tensor} over PARAM_KEYS(cfg)
    -> (saved {name: tensor} over saved_shapes(cfg, B, S), feat (B,C_last,S/32,S/32) NCHW for four stages).
    precision="bf16": fc1 and fc2 of every block multiply bf16-rounded operands and add in fp32 (gpbm_backbone_forward_save); the
    saved table has the same shapes and dtypes."""
    prec = _prec(precision)
    dev = _dev(img)
    dims, depths = _dd(cfg)
    n = len(dims)
    _check_img(img, dev, n)
    B, S = img.shape[0], img.shape[2]
    pt = _table(params, param_shapes(cfg), dev, "params")
    alloc = alloc or _default_alloc(dev)
    saved = {k: alloc(k, s) for k, s in saved_shapes(cfg, B, S).items()}
    vt = _table(saved, saved_shapes(cfg, B, S), dev, "saved")
    last = S // (4 << (n - 1))
    feat = alloc("feat", (B, dims[-1], last, last))
    L = _lib.load()
    nbytes = _query(L, "backbone_forward_workspace", prec, _ints(dims), _ints(depths), n, B, S)
    ws = _ws(alloc, nbytes)
    fn, name, tail = _entry(L, "backbone_forward_save", prec)
    _call(dev, fn, name, img.data_ptr(), pt, _ints(dims), _ints(depths), n, B, S, vt,
          feat.data_ptr(), ws.data_ptr(), nbytes, _stream(dev), *tail)
    return saved, feat


@torch.no_grad()
def backbone_backward(params, saved, img, g_feat, cfg, alloc=None, precision="fp32"):
    """gpb_backbone_backward: from g_feat (like feat), img and what backbone_forward_save returned for it (and the same params)
    -> ({name: gradient} over PARAM_KEYS(cfg), each in its parameter's shape, d img (B,3,S,S)).
    precision="bf16": the four backward contractions of every block multiply bf16-rounded operands and add in fp32
    (gpbm_backbone_backward); `saved` may come from a forward of either precision."""
    prec = _prec(precision)
    dev = _dev(img)
    dims, depths = _dd(cfg)
    n = len(dims)
    _check_img(img, dev, n)
    B, S = img.shape[0], img.shape[2]
    last = S // (4 << (n - 1))
    _chk(g_feat, dev, (B, dims[-1], last, last), "g_feat")
    shapes = param_shapes(cfg)
    pt = _table(params, shapes, dev, "params")
    vt = _table(saved, saved_shapes(cfg, B, S), dev, "saved")
    alloc = alloc or _default_alloc(dev)
    grads = {k: alloc(k, s) for k, s in shapes.items()}
    gt = _table(grads, shapes, dev, "grads")
    d_img = alloc("img", (B, 3, S, S))
    L = _lib.load()
    nbytes = _query(L, "backbone_backward_workspace", prec, _ints(dims), _ints(depths), n, B, S)
    ws = _ws(alloc, nbytes)
    fn, name, tail = _entry(L, "backbone_backward", prec)
    _call(dev, fn, name, pt, vt, img.data_ptr(), g_feat.data_ptr(), _ints(dims), _ints(depths), n, B, S,
          gt, d_img.data_ptr(), ws.data_ptr(), nbytes, _stream(dev), *tail)
    return grads, d_img
