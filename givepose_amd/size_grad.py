"""The train-mode size head (include/givepose_sizegrad.h, gps_*): SizeHead as the training loop runs it -- BatchNorm1d on the
statistics of the batch, Dropout(0.2) with an explicit or seeded mask --, its fp32 forward-that-saves, its backward and the update of
the running statistics.

Everything runs on the device in this library's HIP kernels; there is no CPU path.  Parameters and gradients are fp32 in the
reference's own shapes (conv*.weight keeps its trailing 1), so a gradient lies under the index of its parameter.

`alloc(name, shape)` -- an optional hook every function takes -- supplies the output and workspace buffers (fp32, contiguous, on
the device; workspaces 256-byte aligned); the default is torch.empty.  The tests use it to put sentinels around every buffer.  The
two buffers that are not fp32 are views of fp32 storage from the same hook: `arg` (int32) and `keep` (uint8, B F / 4 floats).
"""
import ctypes

import torch

from . import _lib
from .pnp_grad import _default_alloc, _f32, _stream, _ws

# size_head's six tensors in the order of gps_params, named as in the reference's state_dict (without the prefix)
PARAM_KEYS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "bn1.weight", "bn1.bias")
BUFFER_KEYS = ("bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked")
SAVED_KEYS = _lib.SizeSaved.FIELDS
DROP_P, BN_EPS, BN_MOMENTUM = 0.2, 1e-5, 0.1


def param_shapes(C, F):
    """name -> shape of every size_head parameter for a backbone feature of C channels and F = feat_ts hidden channels."""
    return {"conv1.weight": (F, C, 1), "conv1.bias": (F,), "conv2.weight": (3, F, 1), "conv2.bias": (3,), "bn1.weight": (F,), "bn1.bias": (F,)}


def saved_shapes(B, C, F):
    """name -> shape of what size_forward_save writes (gps_saved).  All float32 but arg (int32) and keep (uint8)."""
    return {"pooled": (B, C), "arg": (B, C), "h": (B, F), "mean": (F,), "mean_lo": (F,), "rstd": (F,), "rstd_lo": (F,), "d": (B, F),
            "keep": (B, F), "out": (B, 3), "var_unbiased": (F,)}


SAVED_DTYPES = {"arg": torch.int32, "keep": torch.uint8}


def _dev(t):
    if t.device.type != "cuda":
        raise _lib.GivePoseHipError("the train-mode size head runs on a HIP device only: there is no CPU path")
    return t.device


def _params_struct(tensors, C, F, what):
    shapes = param_shapes(C, F)
    st = _lib.SizeParams()
    for k, field in zip(PARAM_KEYS, _lib.SizeParams.FIELDS):
        t = tensors[k]
        if tuple(t.shape) != shapes[k] or t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != "cuda":
            raise ValueError(f"{what}[{k}]: {tuple(t.shape)} {t.dtype} on {t.device}, expected contiguous float32 {shapes[k]} on the device")
        setattr(st, field, t.data_ptr())
    return st


def _saved_struct(saved, B, C, F):
    st = _lib.SizeSaved()
    for k, shp in saved_shapes(B, C, F).items():
        t, dt = saved[k], SAVED_DTYPES.get(k, torch.float32)
        if tuple(t.shape) != shp or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"saved[{k}]: {tuple(t.shape)} {t.dtype}, expected contiguous {dt} {shp}")
        setattr(st, k, t.data_ptr())
    return st


def _sizes(params):
    w1 = params["conv1.weight"]
    if w1.dim() != 3 or w1.shape[2] != 1:
        raise ValueError(f"params[conv1.weight]: {tuple(w1.shape)}, expected (F,C,1)")
    return int(w1.shape[1]), int(w1.shape[0])


def _call(dev, fn, name, *args):
    with torch.cuda.device(dev):
        _lib.check(fn(*args), name)


@torch.no_grad()
def size_forward_save(feat, params, keep=None, seed=None, nhwc=False, mean_size=None, alloc=None):
    """SizeHead.forward in train mode in fp32 (gps_size_forward_save, GPS_FORWARD_LAUNCHES launches).
    feat: (B,C,H,W) float32 (nhwc=False), or (B,H,W,C) float16 / float32 as the network's forward holds it (nhwc=True); it is read in
    place, without a converted or transposed copy.  params {name: fp32 device tensor} over PARAM_KEYS.
    The dropout mask: exactly one of keep, a (B,F) uint8 / bool tensor (non-zero = kept), and seed, an int in [0, 2^64) for the
    counter-based rule of the header.  mean_size (B,3): also returns "size" = out + mean_size / |mean_size|.
    -> the saved tensors (saved_shapes): saved["out"] (B,3) is the head's result, saved["keep"] the mask that was used."""
    if (keep is None) == (seed is None):
        raise ValueError("size_forward_save: exactly one of keep and seed must be given")
    dev = _dev(feat)
    C, F = _sizes(params)
    if feat.dim() != 4 or feat.shape[3 if nhwc else 1] != C:
        raise ValueError(f"feat: {tuple(feat.shape)}, expected {'(B,H,W,C)' if nhwc else '(B,C,H,W)'} with C = {C}")
    if feat.dtype not in ((torch.float16, torch.float32) if nhwc else (torch.float32,)):
        raise ValueError(f"feat: {feat.dtype}, expected float32{' or float16' if nhwc else ''}")
    feat = feat.contiguous()
    B, HW = int(feat.shape[0]), int(feat.numel() // max(feat.shape[0] * C, 1))
    if keep is not None:
        keep = torch.as_tensor(keep).to(dev)
        if tuple(keep.shape) != (B, F) or keep.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"keep: {tuple(keep.shape)} {keep.dtype}, expected (B,F) = ({B},{F}) uint8")
        keep = keep.to(torch.uint8).contiguous()
    else:
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed: {seed} is not in [0, 2^64)")
    L = _lib.load()
    pw = _params_struct(params, C, F, "params")      # before anything is allocated: a refused call leaves nothing behind
    alloc = alloc or _default_alloc(dev)
    saved = {}
    for k, shp in saved_shapes(B, C, F).items():
        n = 1
        for s in shp:
            n *= s
        if k == "arg":
            saved[k] = alloc(k, shp).view(torch.int32)
        elif k == "keep":
            saved[k] = alloc(k, ((n + 3) // 4,)).view(torch.uint8)[:n].view(shp)
        else:
            saved[k] = alloc(k, shp)
    size = None
    if mean_size is not None:
        mean_size = _f32(mean_size, dev, (B, 3), "mean_size")
        size = alloc("size", (B, 3))
    sv = _saved_struct(saved, B, C, F)
    _call(dev, L.gps_size_forward_save, "gps_size_forward_save", feat.data_ptr(), _lib.GP_F16 if feat.dtype == torch.float16 else _lib.GP_F32,
          int(bool(nhwc)), ctypes.byref(pw), None if keep is None else keep.data_ptr(), 0 if seed is None else seed,
          None if size is None else mean_size.data_ptr(), B, C, HW, F, ctypes.byref(sv), None if size is None else size.data_ptr(), _stream(dev))
    if size is not None:
        saved["size"] = size
    return saved


@torch.no_grad()
def size_backward(params, saved, g_out, feat_shape, alloc=None):
    """gps_size_backward (GPS_BACKWARD_LAUNCHES launches): from d out (B,3) and what size_forward_save returned (and the same params)
    -> ({name: gradient} over PARAM_KEYS, d feat (B,C,H,W) float32 NCHW, every element written).  feat_shape: (B,C,H,W)."""
    dev = _dev(saved["pooled"])
    C, F = _sizes(params)
    B = int(saved["pooled"].shape[0])
    feat_shape = tuple(int(s) for s in feat_shape)
    if len(feat_shape) != 4 or feat_shape[:2] != (B, C):
        raise ValueError(f"feat_shape: {feat_shape}, expected ({B},{C},H,W)")
    HW = feat_shape[2] * feat_shape[3]
    g_out = _f32(g_out, dev, (B, 3), "g_out")
    L = _lib.load()
    pw = _params_struct(params, C, F, "params")
    sv = _saved_struct({k: saved[k] for k in SAVED_KEYS}, B, C, F)
    nbytes = L.gps_size_backward_workspace(B, C, HW, F)
    if nbytes == 0:
        _lib.check(-1, "gps_size_backward_workspace")
    alloc = alloc or _default_alloc(dev)
    grads = {k: alloc(k, s) for k, s in param_shapes(C, F).items()}
    g_feat = alloc("feat", feat_shape)
    ws = _ws(alloc, nbytes)
    pg = _params_struct(grads, C, F, "grads")
    _call(dev, L.gps_size_backward, "gps_size_backward", ctypes.byref(pw), ctypes.byref(sv), g_out.data_ptr(), B, C, HW, F, ctypes.byref(pg),
          g_feat.data_ptr(), ws.data_ptr(), nbytes, _stream(dev))
    return grads, g_feat


@torch.no_grad()
def bn_running_update(running_mean, running_var, num_batches_tracked, mean, var_unbiased, momentum=BN_MOMENTUM):
    """nn.BatchNorm1d's train-mode update of its buffers, in place on the device (gps_bn_running_update): running_mean and running_var
    (F,) float32 move by `momentum` towards mean and var_unbiased; num_batches_tracked (an int64 scalar tensor, or None) += 1."""
    dev = _dev(running_mean)
    F = running_mean.numel()
    for n, t in (("running_mean", running_mean), ("running_var", running_var), ("mean", mean), ("var_unbiased", var_unbiased)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != F or t.device != dev:
            raise ValueError(f"{n}: {tuple(t.shape)} {t.dtype} on {t.device}, expected contiguous float32 ({F},) on {dev}")
    nbt = None
    if num_batches_tracked is not None:
        if num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1 or num_batches_tracked.device != dev:
            raise ValueError(f"num_batches_tracked: {tuple(num_batches_tracked.shape)} {num_batches_tracked.dtype} on {num_batches_tracked.device}")
        nbt = num_batches_tracked.data_ptr()
    L = _lib.load()
    _call(dev, L.gps_bn_running_update, "gps_bn_running_update", running_mean.data_ptr(), running_var.data_ptr(), nbt, mean.data_ptr(),
          var_unbiased.data_ptr(), F, float(momentum), _stream(dev))

