"""The validation loss on the device: the reference's `PoseLoss` (losses/pose_loss.py:13-196) and the train-time pose decode
`pose_from_predictions_train` (network/pose_utils/pose_from_pred_centroid_z.py:160-249).  Host side of gpl_pose_decode_train /
gpl_pose_loss_partials / gpl_pose_loss_reduce (include/givepose_loss.h).

Forward values only: nothing returned here carries a gradient.  The reference's loop -- per crop a `.cpu().numpy()` round trip and
a search over 360 symmetric rotations -- is two launches for the whole batch, with no copy to the host; `LossAccumulator` keeps the
running sums of a validation sweep on the device and copies one vector at the end.

Every value is float64 computed from the float32 inputs (the reference works in float32; its search in NumPy float64); the float32
results are the float64 ones rounded once.  Two calls on the same inputs give the same bits.

One documented difference: with a 'sym' r_type the reference zeroes the x and z coordinates of the symmetric crops' points in the
CALLER's `data['model_point']` (through a permuted view, pose_loss.py:163-168).  Here `model_point` is only read.

The gradients of these values live in their own family (include/givepose_grad.h, gpg_*): `PoseLoss.value_and_grad`,
`PoseLoss.with_grad` (the autograd binding a training loop calls) and `pose_decode_train_backward` below.

HIP devices only; there is no CPU fallback.
"""
import dataclasses

import numpy as np
import torch

from . import _lib
from .config import ROT_TYPES

KEYS = ("Rot1", "Tran", "Size", "Point_matching", "nocs_coor", "sp2d_coor")
RECORD_COLUMNS = ("index", "re_best", "re", "te", "rot1_sum", "tran_sum", "size_sum", "branch")
GRAD_KEYS = ("rot", "trans", "size", "nocs_coor", "ivfc_coor")


@dataclasses.dataclass(frozen=True)
class LossConfig:
    """The reference FLAGS PoseLoss reads (config/config.py), with their defaults."""
    pose_loss_type: str = "l1"        # 'l1' | 'smoothl1' (beta 0.5)
    r_loss: str = "l1"                # 'l1' | 'angle'
    r_type: str = "allo_rot6d"        # a name holding 'sym' switches the search off and masks the x / z axes instead
    coor_gt_sym: str = "rot"
    rot_1_w: float = 1.0
    tran_w: float = 1.0
    size_w: float = 1.0
    prop_pm_w: float = 1.0
    coor_w: float = 0.1

    def __post_init__(self):
        if self.pose_loss_type not in ("l1", "smoothl1"):
            raise ValueError(f"pose_loss_type must be 'l1' or 'smoothl1', not {self.pose_loss_type!r}")
        if self.r_loss not in ("l1", "angle"):
            raise ValueError(f"r_loss must be 'l1' or 'angle', not {self.r_loss!r}")
        if self.coor_gt_sym not in ("rot", "coor", "radius"):
            raise ValueError(f"coor_gt_sym must be 'rot', 'coor' or 'radius', not {self.coor_gt_sym!r}")
        if self.coor_gt_sym != "rot":
            raise NotImplementedError("coor_gt_sym != 'rot': the reference asserts it (losses/pose_loss.py:61)")
        if not isinstance(self.r_type, str) or self.r_type not in ROT_TYPES:
            raise ValueError(f"unknown r_type {self.r_type!r}")
        for k in ("rot_1_w", "tran_w", "size_w", "prop_pm_w", "coor_w"):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
                raise ValueError(f"{k} must be a finite number, not {v!r}")


_sym_tables = {}


def _sym_table(dev):
    """cos / sin of symmetry_rotation_matrix_y(360) (pose_loss.py:319-326) as NumPy gives them on the host, uploaded once per device."""
    t = _sym_tables.get(str(dev))
    if t is None:
        th = np.array([2 * np.pi / _lib.GPL_SYM * i for i in range(_lib.GPL_SYM)])
        t = _sym_tables[str(dev)] = torch.from_numpy(np.stack([np.cos(th), np.sin(th)], 1)).to(dev)
    return t


def _f32(t, dev, shape, name):
    t = torch.as_tensor(t)
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must be {shape}, not {tuple(t.shape)}")
    t = t.detach().to(dev, torch.float32).contiguous()
    if t.data_ptr() % 16:             # a view into a larger buffer at an odd offset: the kernels load 16 bytes per lane
        t = t.clone()
    return t


def pose_decode_train(pred_t, rot_allo, cam_K, bbox_center, resize_ratio, roi_wh, t_site=True, is_allo=True, eps=1e-4, return_details=False):
    """pose_from_predictions_train on a (B,3,3) rotation -> (rot_ego (B,3,3), translation (B,3)) float32 on the device of `rot_allo`;
    return_details: a third value, the dict of the float64 `rot` / `trans`."""
    rot_allo = torch.as_tensor(rot_allo)
    dev = rot_allo.device
    if dev.type != "cuda":
        raise _lib.GivePoseHipError("pose_decode_train runs on a HIP device only: there is no CPU path")
    B = rot_allo.shape[0]
    if B == 0:
        raise ValueError("empty batch")
    pt, Ra, K = _f32(pred_t, dev, (B, 3), "pred_t"), _f32(rot_allo, dev, (B, 3, 3), "rot_allo"), _f32(cam_K, dev, (B, 3, 3), "cam_K")
    ce, wh = _f32(bbox_center, dev, (B, 2), "bbox_center"), _f32(roi_wh, dev, (B, 2), "roi_wh")
    ra = _f32(torch.as_tensor(resize_ratio).reshape(-1), dev, (B,), "resize_ratio")
    rot32, trans32 = torch.empty(B, 3, 3, device=dev), torch.empty(B, 3, device=dev)
    rot64, trans64 = torch.empty(B, 3, 3, device=dev, dtype=torch.float64), torch.empty(B, 3, device=dev, dtype=torch.float64)
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.gpl_pose_decode_train(pt.data_ptr(), Ra.data_ptr(), K.data_ptr(), ce.data_ptr(), ra.data_ptr(), wh.data_ptr(),
                                           int(bool(t_site)), int(bool(is_allo)), float(eps), B, rot32.data_ptr(), trans32.data_ptr(),
                                           rot64.data_ptr(), trans64.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "gpl_pose_decode_train")
    if return_details:
        return rot32, trans32, {"rot": rot64, "trans": trans64}
    return rot32, trans32


def pose_decode_train_backward(g_rot_ego, g_trans, pred_t, rot_allo, cam_K, bbox_center, resize_ratio, roi_wh, rot6d=None, t_site=True,
                               is_allo=True, eps=1e-4, return_details=False):
    """Backward of `pose_decode_train` (gpg_pose_decode_train_backward): the upstream gradients of its two results, then its own
    inputs -> {"rot_allo": (B,3,3), "pred_t": (B,3)} float32 on the device of `rot_allo`.  rot6d (B,6): the raw vector `rot_allo`
    was decoded from by rot6d_to_mat_batch; the dict then also holds its gradient, "rot6d" (B,6).
    return_details: a second value, the (B,18) float64 record (d rot_allo, d pred_t, d rot6d)."""
    rot_allo = torch.as_tensor(rot_allo)
    dev = rot_allo.device
    if dev.type != "cuda":
        raise _lib.GivePoseHipError("pose_decode_train_backward runs on a HIP device only: there is no CPU path")
    B = rot_allo.shape[0]
    if B == 0:
        raise ValueError("empty batch")
    ge, gt = _f32(g_rot_ego, dev, (B, 3, 3), "g_rot_ego"), _f32(g_trans, dev, (B, 3), "g_trans")
    pt, Ra, K = _f32(pred_t, dev, (B, 3), "pred_t"), _f32(rot_allo, dev, (B, 3, 3), "rot_allo"), _f32(cam_K, dev, (B, 3, 3), "cam_K")
    ce, wh = _f32(bbox_center, dev, (B, 2), "bbox_center"), _f32(roi_wh, dev, (B, 2), "roi_wh")
    ra = _f32(torch.as_tensor(resize_ratio).reshape(-1), dev, (B,), "resize_ratio")
    r6 = None if rot6d is None else _f32(rot6d, dev, (B, 6), "rot6d")
    out = {"rot_allo": torch.empty(B, 3, 3, device=dev), "pred_t": torch.empty(B, 3, device=dev)}
    if r6 is not None:
        out["rot6d"] = torch.empty(B, 6, device=dev)
    g64 = torch.empty(B, _lib.GPG_DECODE, device=dev, dtype=torch.float64)
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.gpg_pose_decode_train_backward(ge.data_ptr(), gt.data_ptr(), pt.data_ptr(), Ra.data_ptr(), K.data_ptr(), ce.data_ptr(),
                                                    ra.data_ptr(), wh.data_ptr(), r6.data_ptr() if r6 is not None else 0,
                                                    int(bool(t_site)), int(bool(is_allo)), float(eps), B, out["rot_allo"].data_ptr(),
                                                    out["pred_t"].data_ptr(), out["rot6d"].data_ptr() if r6 is not None else 0,
                                                    g64.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "gpg_pose_decode_train_backward")
    return (out, g64) if return_details else out


class _PoseLossFunction(torch.autograd.Function):
    """The six terms as one node of the autograd graph: five differentiable inputs, six outputs."""

    @staticmethod
    def forward(ctx, loss, data, *pred):
        a, dims = loss._inputs(dict(zip(GRAD_KEYS, pred)), data)
        out64, out32, record, slabs = loss._forward(a, dims)
        ctx.loss, ctx.dims, ctx.like = loss, dims, [(p.dtype, p.device) for p in pred]
        ctx.save_for_backward(*a, slabs, record)
        return tuple(out32[i].clone() for i in range(len(KEYS)))

    @staticmethod
    def backward(ctx, *gouts):
        *a, slabs, record = ctx.saved_tensors
        dev = record.device
        gout = torch.stack([torch.zeros((), device=dev, dtype=torch.float64) if g is None else g.to(dev, torch.float64).reshape(())
                            for g in gouts])
        grads, _ = ctx.loss._backward(a, ctx.dims, slabs, record, gout)
        return (None, None) + tuple(grads[k].to(device=d, dtype=t) for k, (t, d) in zip(GRAD_KEYS, ctx.like))


class PoseLoss:
    """`PoseLoss()(pred_dict, data)` of the reference: a dict of 0-dim float32 device tensors with the keys Rot1, Tran, Size,
    Point_matching, nocs_coor, sp2d_coor, in that order.  pred_dict: rot (B,3,3), trans, size (B,3), nocs_coor, ivfc_coor
    (B,3,64,64); data: rotation, translation, real_size, roi_mask_output, roi_ivfc_mask_output (B,1,64,64), sym_info (B,4),
    nocs_scale (B), nocs_coord, ivfc_coord, model_point (B,P,3).  Host or device tensors; everything runs on the device of
    pred_dict['rot'], asynchronously on its current stream.

    return_details=True: a second value, the dict of `terms` (6) and `mean_re` / `mean_te` in float64, `out32` (8), and the per-crop
    (B,8) float64 `record` with its columns by name (RECORD_COLUMNS: `index` is the chosen candidate, -1 = the unrotated ground
    truth; `re_best` its rotation error in degrees; `re` / `te` the crop's errors against the unrotated ground truth)."""

    def __init__(self, cfg: LossConfig = LossConfig()):
        if not isinstance(cfg, LossConfig):
            raise ValueError("PoseLoss needs a LossConfig")
        self.cfg = cfg

    def _inputs(self, pred_dict, data):
        """-> (the sixteen float32 / int32 device tensors of gpl_pose_loss_partials, (B, P, device))."""
        rot = torch.as_tensor(pred_dict["rot"])
        dev = rot.device
        if dev.type != "cuda":
            raise _lib.GivePoseHipError("PoseLoss runs on a HIP device only: there is no CPU path")
        if rot.dim() != 3 or rot.shape[0] == 0:
            raise ValueError(f"pred_dict['rot'] must be (B,3,3) with B >= 1, not {tuple(rot.shape)}")
        B, R = rot.shape[0], _lib.GPL_RES
        mp = torch.as_tensor(data["model_point"])
        if mp.dim() != 3 or mp.shape[1] < 1:
            raise ValueError(f"data['model_point'] must be (B,P,3) with P >= 1, not {tuple(mp.shape)}")
        P = mp.shape[1]
        sym = torch.as_tensor(data["sym_info"])
        if sym.dim() != 2 or sym.shape[0] != B:
            raise ValueError(f"data['sym_info'] must be ({B},4), not {tuple(sym.shape)}")
        f = lambda t, shape, name: _f32(t, dev, shape, name)
        a = [f(rot, (B, 3, 3), "rot"), f(pred_dict["trans"], (B, 3), "trans"), f(pred_dict["size"], (B, 3), "size"),
             f(pred_dict["nocs_coor"], (B, 3, R, R), "nocs_coor"), f(pred_dict["ivfc_coor"], (B, 3, R, R), "ivfc_coor"),
             f(data["rotation"], (B, 3, 3), "rotation"), f(data["translation"], (B, 3), "translation"),
             f(data["real_size"], (B, 3), "real_size"), f(torch.as_tensor(data["nocs_scale"]).reshape(-1), (B,), "nocs_scale"),
             (sym[:, 0] == 1).to(dev, torch.int32).contiguous(),
             f(data["roi_mask_output"], (B, 1, R, R), "roi_mask_output"), f(data["roi_ivfc_mask_output"], (B, 1, R, R), "roi_ivfc_mask_output"),
             f(data["nocs_coord"], (B, 3, R, R), "nocs_coord"), f(data["ivfc_coord"], (B, 3, R, R), "ivfc_coord"),
             f(mp, (B, P, 3), "model_point"), _sym_table(dev)]
        return a, (B, P, dev)

    def _forward(self, a, dims, acc=None):
        cfg, R = self.cfg, _lib.GPL_RES
        B, P, dev = dims
        slabs = torch.empty(B, _lib.GPL_SPLIT, _lib.GPL_PART, device=dev, dtype=torch.float64)
        record = torch.empty(B, _lib.GPL_RECORD, device=dev, dtype=torch.float64)
        out64 = torch.empty(_lib.GPL_OUT, device=dev, dtype=torch.float64)
        out32 = torch.empty(_lib.GPL_OUT, device=dev, dtype=torch.float32)
        angle = int(cfg.r_loss == "angle")
        L = _lib.load()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(L.gpl_pose_loss_partials(*[t.data_ptr() for t in a], B, P, R, int("sym" in cfg.r_type), angle,
                                                int(cfg.pose_loss_type == "smoothl1"), slabs.data_ptr(), record.data_ptr(), stream),
                       "gpl_pose_loss_partials")
            _lib.check(L.gpl_pose_loss_reduce(slabs.data_ptr(), record.data_ptr(), B, P, angle, float(cfg.rot_1_w), float(cfg.tran_w),
                                              float(cfg.size_w), float(cfg.prop_pm_w), float(cfg.coor_w), out64.data_ptr(), out32.data_ptr(),
                                              acc.data_ptr() if acc is not None else 0, stream), "gpl_pose_loss_reduce")
        return out64, out32, record, slabs

    def _backward(self, a, dims, slabs, record, gout):
        """One launch of gpg_pose_loss_grad -> (the five float32 gradients by GRAD_KEYS, the (B,15) float64 record of the small ones)."""
        cfg, R = self.cfg, _lib.GPL_RES
        B, P, dev = dims
        if gout is not None:
            gout = torch.as_tensor(gout)
            if tuple(gout.shape) != (_lib.GPG_TERMS,):
                raise ValueError(f"gout must be ({_lib.GPG_TERMS},), not {tuple(gout.shape)}")
            gout = gout.detach().to(dev, torch.float64).contiguous()
        g = {"rot": torch.empty(B, 3, 3, device=dev), "trans": torch.empty(B, 3, device=dev), "size": torch.empty(B, 3, device=dev),
             "nocs_coor": torch.empty(B, 3, R, R, device=dev), "ivfc_coor": torch.empty(B, 3, R, R, device=dev)}
        small = torch.empty(B, _lib.GPG_SMALL, device=dev, dtype=torch.float64)
        L = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(L.gpg_pose_loss_grad(*[t.data_ptr() for t in a], slabs.data_ptr(), record.data_ptr(),
                                            gout.data_ptr() if gout is not None else 0, B, P, R, int("sym" in cfg.r_type),
                                            int(cfg.r_loss == "angle"), int(cfg.pose_loss_type == "smoothl1"), float(cfg.rot_1_w),
                                            float(cfg.tran_w), float(cfg.size_w), float(cfg.prop_pm_w), float(cfg.coor_w),
                                            *[g[k].data_ptr() for k in GRAD_KEYS], small.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "gpg_pose_loss_grad")
        return g, small

    def _launch(self, pred_dict, data, acc=None):
        a, dims = self._inputs(pred_dict, data)
        return self._forward(a, dims, acc)[:3]

    def _details(self, out64, out32, record):
        details = {"terms": out64[:6], "mean_re": out64[6], "mean_te": out64[7], "out32": out32, "record": record}
        details.update({k: record[:, i] for i, k in enumerate(RECORD_COLUMNS)})
        return details

    @torch.no_grad()
    def value_and_grad(self, pred_dict, data, gout=None, return_details=False):
        """-> (the loss dict of `__call__`, {rot, trans, size, nocs_coor, ivfc_coor}: the float32 gradients of
        sum_k gout[k] * term_k with respect to the five predictions).  gout: six weights in KEYS order (a device tensor stays on
        the device), None = ones: the gradient of the total loss.  Two forward launches and one gradient launch, no host sync.
        The closest ground truth and the rotated ground-truth maps are constants, as in the reference.
        return_details: a third value, the details of `__call__` plus `small64`, the (B,15) float64 d rot / d trans / d size."""
        a, dims = self._inputs(pred_dict, data)
        out64, out32, record, slabs = self._forward(a, dims)
        grads, small = self._backward(a, dims, slabs, record, gout)
        loss = {k: out32[i] for i, k in enumerate(KEYS)}
        if not return_details:
            return loss, grads
        return loss, grads, {**self._details(out64, out32, record), "small64": small}

    def with_grad(self, pred_dict, data):
        """The loss dict of `__call__`, attached to the autograd graph: `sum(d.values()).backward()` (or any other function of
        the six terms) fills `.grad` of the five prediction tensors through gpg_pose_loss_grad, as the reference's
        `total_loss.backward()` does.  The predictions must be device tensors."""
        pred = [pred_dict[k] for k in GRAD_KEYS]
        if not all(torch.is_tensor(p) and p.device.type == "cuda" for p in pred):
            raise _lib.GivePoseHipError("PoseLoss runs on a HIP device only: there is no CPU path")
        return dict(zip(KEYS, _PoseLossFunction.apply(self, data, *pred)))

    @torch.no_grad()
    def __call__(self, pred_dict, data, return_details=False):
        out64, out32, record = self._launch(pred_dict, data)
        loss = {k: out32[i] for i, k in enumerate(KEYS)}
        if not return_details:
            return loss
        return loss, self._details(out64, out32, record)


class LossAccumulator:
    """The running means of a validation sweep: `add(pred_dict, data)` per batch (no host sync: the sums stay on the device),
    `result()` once at the end -- the crop-weighted means of the six terms, their `total`, and `mean_re` [deg] / `mean_te`."""

    def __init__(self, cfg: LossConfig = LossConfig()):
        self.loss = PoseLoss(cfg)
        self._acc = None

    @torch.no_grad()
    def add(self, pred_dict, data):
        dev = torch.as_tensor(pred_dict["rot"]).device
        if dev.type != "cuda":
            raise _lib.GivePoseHipError("LossAccumulator runs on a HIP device only: there is no CPU path")
        if self._acc is None:
            self._acc = torch.zeros(_lib.GPL_ACC, device=dev, dtype=torch.float64)
        elif self._acc.device != dev:
            raise ValueError(f"this accumulator lives on {self._acc.device}, the batch on {dev}")
        self.loss._launch(pred_dict, data, acc=self._acc)

    def result(self):
        if self._acc is None:
            raise ValueError("no batch was added")
        a = self._acc.cpu().numpy()           # the one D->H copy of the sweep
        out = {k: float(a[i] / a[8]) for i, k in enumerate(KEYS)}
        out["total"] = float(sum(out[k] for k in KEYS))
        out.update(mean_re=float(a[6] / a[8]), mean_te=float(a[7] / a[8]), crops=int(a[8]), batches=int(a[9]))
        return out
