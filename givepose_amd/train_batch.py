"""The training batch on the device: uint8 frames + labels -> the `data` dict forward(do_loss=True), PoseLoss and train_step read.

Host side of `gpt_crop_train` and `gpt_mask_deform` (include/givepose_traindata.h).  Mirrors datasets/load_data_nocs.py:180-386 of the
reference, which builds a sample with CPU work: a 640x480 coordinate grid, float conversions of three full frames, seven
cv2.warpAffine calls and defor_2D.  Here the host computes a few dozen scalars per sample with the reference's roundings -- the DZI box
of tools/dataset_utils.py:32-82, the inverse maps of the two crops (preprocess.crop_params_from_center_scale), roi_wh / bbox_center /
resize_ratio -- and one (3,256) value table per sample: every value of the reference's float arithmetic on a NOCS or IVFC frame is a
function of (sample, channel, byte).  The frames travel as uint8 and two launches, whatever the batch size, write every map.

Not produced: `full_img`, `one_hot`, `roi_img_origin`, `img_scale` and `info_2d` (the training path of this library reads none of
them).  The colour augmentation of the frame comes before this builder: color_aug.ColorAugmenter maps `frames` to augmented frames
on the device, and its output is what is passed here.  Instance and frame selection and PNG decoding stay with the caller's loader;
`fs_net_scale` and `sym_info` let it fill `labels` without the reference on the path.

The mask deformation draws a uniform random floor(l/2)-subset of the band, the distribution of defor_2D's
np.random.choice(l, l // 2, replace=False); the STREAM of numpy's legacy generator cannot be reproduced and is not: the subset is the
floor(l/2) band pixels that come first by (key, pixel index), with explicit keys or the counter hash of a seed.  cv2's arithmetic
(warpAffine's fixed-point walk, the 2x2 MORPH_ELLIPSE element [[0,1],[1,1]] with anchor (1,1), erode / dilate ignoring what lies
outside the image, and one iteration, since the reference passes its radius in the position of `dst`) is restated from the published
algorithm; OpenCV is not installed where this library is tested, so that parity is unpinned, as for the warp (oracle/preprocess_ref.py).
"""
import numpy as np
import torch

from . import _lib
from .preprocess import crop_params_from_center_scale, luts

DZI_TYPES = ("uniform", "uniform_sr", "none")
DZI_REFUSED = {"roi10d": "the reference's roi10d collapses x2 onto x1 (tools/dataset_utils.py:69), so its boxes have no width",
               "truncnorm": "the reference raises NotImplementedError for truncnorm (tools/dataset_utils.py:74-75)"}
DRAW_TAG = 0x7462          # Philox key [seed, DRAW_TAG]: the host draws of a seeded call
LABEL_KEYS = ("rotation", "translation", "real_size", "mean_size", "sym_info", "nocs_scale", "model_point", "cam_K")
MAP_KEYS = ("roi_img", "roi_mask", "roi_mask_deform", "roi_mask_output", "roi_ivfc_mask_output", "roi_coord_2d", "nocs_coord", "ivfc_coord")
MUG = 5                    # cat_id (0-based) whose coordinates are moved by mug_meta

_UNIT_SIZE = {"bottle": (87, 220, 89), "bowl": (165, 80, 165), "camera": (88, 128, 156), "can": (68, 146, 72), "laptop": (346, 200, 335),
              "mug": (146, 83, 114), "02876657": (324 / 4, 874 / 4, 321 / 4), "02880940": (675 / 4, 271 / 4, 675 / 4),
              "02942699": (464 / 4, 487 / 4, 702 / 4), "02946921": (450 / 4, 753 / 4, 460 / 4), "03642806": (581 / 4, 445 / 4, 672 / 4),
              "03797390": (670 / 4, 540 / 4, 497 / 4)}
_SYM = {1: (1, 1, 0, 1), 2: (1, 1, 0, 1), 3: (0, 0, 0, 0), 4: (1, 1, 1, 1), 5: (0, 1, 0, 0), (6, 1): (0, 1, 0, 0), (6, 0): (1, 0, 0, 0)}


def fs_net_scale(cat_name, model, nocs_scale):
    """get_fs_net_scale (datasets/load_data_nocs.py:403-470): model (P,3) -> (real_size, mean_size) in millimetres; the loader divides
    both by 1000."""
    if cat_name not in _UNIT_SIZE:
        raise NotImplementedError(f"fs_net_scale: category {cat_name!r} is not recorded")
    model = np.asarray(model)
    lx = 2 * max(np.max(model[:, 0]), -np.min(model[:, 0]))
    ly = np.max(model[:, 1]) - np.min(model[:, 1])
    lz = np.max(model[:, 2]) - np.min(model[:, 2])
    return np.array([lx * nocs_scale * 1000, ly * nocs_scale * 1000, lz * nocs_scale * 1000]), np.array(_UNIT_SIZE[cat_name])


def sym_info(cat_id_1_based, mug_handle=1):
    """get_sym_info (datasets/load_data_nocs.py:472-489)."""
    key = (6, mug_handle) if cat_id_1_based == 6 else cat_id_1_based
    if key not in _SYM:
        raise NotImplementedError(f"sym info {cat_id_1_based}")
    return np.array(_SYM[key], dtype=int)


def dzi_center_scale(bboxes, u, im_H, im_W, dzi_type="uniform", pad_scale=1.5, scale_ratio=0.25, shift_ratio=0.25):
    """aug_bbox_DZI (tools/dataset_utils.py:32-82) for n boxes (y1,x1,y2,x2) with the draws u (n,3) in [0,1) in the place of
    np.random.random_sample() (u0: scale, u1 / u2: shift in x / y) -> cx, cy, scale (float64, the reference's operation order)."""
    bboxes = np.asarray(bboxes, dtype=np.float64).reshape(-1, 4)
    u = np.asarray(u, dtype=np.float64).reshape(-1, 3)
    y1, x1, y2, x2 = bboxes[:, 0], bboxes[:, 1], bboxes[:, 2], bboxes[:, 3]
    cx, cy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
    bh, bw = y2 - y1, x2 - x1
    ext = np.maximum(bh, bw)
    if dzi_type in ("uniform", "uniform_sr"):
        sr = 1 + scale_ratio * (2 * u[:, 0] - 1) if dzi_type == "uniform" else 1 - 0.25 * u[:, 0]
        shift = shift_ratio * (2 * u[:, 1:3] - 1)
        cx, cy = cx + bw * shift[:, 0], cy + bh * shift[:, 1]
        scale = ext * sr * pad_scale
    elif dzi_type == "none":
        scale = ext
    else:
        raise ValueError(f"dzi_type {dzi_type!r}: one of {DZI_TYPES}")
    return cx, cy, np.minimum(scale, max(im_H, im_W)) * 1.0


def coord_tables(cat_id, mug_meta):
    """(B,3,256) fp32: the value of a NOCS or IVFC byte per (sample, channel), as load_data_nocs.py:257-266 / 312-323 compute it on the
    whole frame: float32(v) / 255, channel 2 mirrored to 1 - x, then - 0.5, all in float32; for a mug s0 * (x + T0) in the dtype numpy
    promotes to, rounded to fp32 once at the end (the loader's torch.as_tensor(..., dtype=float32)).  Both maps share the arithmetic."""
    x = np.array(np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256)), dtype=np.float32) / 255
    x[2] = 1 - x[2]
    x = x - 0.5
    out = np.empty((len(cat_id), 3, 256), np.float32)
    for b, c in enumerate(cat_id):
        if c == MUG:
            if mug_meta[b] is None:
                raise ValueError(f"mug_meta[{b}]: a mug (cat_id 5) needs (T0, s0)")
            T0, s0 = mug_meta[b]
            T0 = np.asarray(T0)
            if T0.shape != (3,):
                raise ValueError(f"mug_meta[{b}]: T0 must be (3,), not {T0.shape}")
            out[b] = (s0 * (x + T0[:, None])).astype(np.float32)
        else:
            out[b] = x
    return out


def host_draws(seed, B, mask_pro):
    """The host draws of a seeded call: dzi (B,3) and deform (B,) = (u <= mask_pro), from Philox(key=[seed, DRAW_TAG])."""
    g = np.random.Generator(np.random.Philox(key=[seed, DRAW_TAG]))
    dzi = g.random((B, 3))
    return dzi, g.random(B) <= mask_pro


class TrainBatchBuilder:
    """Device-side replacement of the reference's train-time `__getitem__` + collate.

        builder = TrainBatchBuilder(480, 640, device)
        data = builder(frames, inst_masks, nocs_png, ivfc_png, frame_idx, ivfc_idx, inst_id, bbox, cat_id, mug_meta, labels, seed=step)
        net.train_step(data, PoseLoss(), optimizer)

    Output (fp32, contiguous, on the device): roi_img (B,3,S,S), roi_mask, roi_mask_deform (B,1,S,S), roi_mask_output,
    roi_ivfc_mask_output (B,1,R,R), roi_coord_2d (B,2,R,R), nocs_coord, ivfc_coord (B,3,R,R), roi_wh, bbox_center (B,2), resize_ratio
    (B,), and `labels` passed through.  full_img, one_hot, roi_img_origin, img_scale and info_2d are NOT produced: the training path
    reads none of them.  See the module docstring for what the mask deformation reproduces of defor_2D and what it cannot."""

    def __init__(self, im_H, im_W, device, img_size=256, out_res=64, dzi_type="uniform", pad_scale=1.5, scale_ratio=0.25, shift_ratio=0.25,
                 mask_pro=0.5):
        dzi_type = str(dzi_type).lower()
        if dzi_type in DZI_REFUSED:
            raise ValueError(f"dzi_type {dzi_type!r} is not supported: {DZI_REFUSED[dzi_type]}")
        if dzi_type not in DZI_TYPES:
            raise ValueError(f"dzi_type {dzi_type!r}: one of {DZI_TYPES}")
        if img_size * img_size > _lib.GPT_MAX_PIXELS or not 0 < out_res <= img_size:
            raise ValueError(f"img_size {img_size} / out_res {out_res}: img_size^2 <= {_lib.GPT_MAX_PIXELS} and 0 < out_res <= img_size")
        self.H, self.W, self.S, self.R = im_H, im_W, img_size, out_res
        self.dzi_type, self.pad, self.scale_ratio, self.shift_ratio, self.mask_pro = dzi_type, pad_scale, scale_ratio, shift_ratio, mask_pro
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TrainBatchBuilder runs on a HIP device only (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        il, xl, yl = luts(im_H, im_W)
        self.img_lut = torch.from_numpy(il).to(self.device)
        self.xlut = torch.from_numpy(xl).to(self.device)
        self.ylut = torch.from_numpy(yl).to(self.device)

    def host_params(self, bbox, cat_id, mug_meta, dzi):
        """The host's share of a batch: bbox (B,4) as (y1,x1,y2,x2), cat_id (B,), mug_meta (B entries), dzi (B,3) -> inv_img, inv_out
        (B,6) float64, roi_wh (from the un-augmented box, get_real_hw), bbox_center (the augmented centre), resize_ratio, table."""
        bbox = np.asarray(bbox, dtype=np.float64).reshape(-1, 4)
        y1, x1, y2, x2 = bbox[:, 0], bbox[:, 1], bbox[:, 2], bbox[:, 3]
        ok = np.isfinite(bbox).all(1) & (np.maximum(y2 - y1, x2 - x1) > 0)
        if not ok.all():
            bad = np.nonzero(~ok)[0]
            raise ValueError(f"TrainBatchBuilder: degenerate box(es) at index {bad.tolist()}: (y1,x1,y2,x2) = {bbox[bad].tolist()}")
        cx, cy, scale = dzi_center_scale(bbox, dzi, self.H, self.W, self.dzi_type, self.pad, self.scale_ratio, self.shift_ratio)
        P = crop_params_from_center_scale(cx, cy, scale, self.S, self.R)
        P["roi_wh"] = np.stack([np.minimum(self.W, x2) - np.maximum(0, x1), np.minimum(self.H, y2) - np.maximum(0, y1)], 1).astype(np.float32)
        P["table"] = coord_tables(cat_id, mug_meta)
        return P

    def __call__(self, frames, inst_masks, nocs_png, ivfc_png, frame_idx, ivfc_idx, inst_id, bbox, cat_id, mug_meta, labels,
                 draws=None, seed=None, out=None):
        """frames (F,H,W,3), inst_masks (F,H,W), nocs_png (F,H,W,3), ivfc_png (NI,H,W,3): uint8, on the device (or host: copied as
        uint8).  frame_idx, ivfc_idx, inst_id, bbox, cat_id (0-based), mug_meta ((T0 (3,), s0) for a mug, else None): host sequences of
        length B.  labels: host arrays under LABEL_KEYS, (B, ...) each, uploaded as fp32.  Exactly one of
            draws = {"dzi": (B,3) float64 in [0,1), "deform": (B,) bool, "keys": (B,S,S) uint32}
            seed  = an int in [0, 2^64): dzi and deform from host_draws(seed, B, mask_pro), keys hashed on the device.
        Writes into `out` (caller-owned buffers, e.g. the model's static inputs) or fresh tensors; returns the dict."""
        dev, S, R, H, W = self.device, self.S, self.R, self.H, self.W
        if (draws is None) == (seed is None):
            raise ValueError("TrainBatchBuilder: exactly one of draws and seed must be given")
        u8 = lambda a: torch.as_tensor(a).to(dev, torch.uint8).contiguous()
        frames, inst_masks, nocs_png, ivfc_png = u8(frames), u8(inst_masks), u8(nocs_png), u8(ivfc_png)
        F, NI = frames.shape[0], ivfc_png.shape[0]
        for name, t, shape in (("frames", frames, (F, H, W, 3)), ("inst_masks", inst_masks, (F, H, W)), ("nocs_png", nocs_png, (F, H, W, 3)),
                               ("ivfc_png", ivfc_png, (NI, H, W, 3))):
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} {tuple(t.shape)} does not match {shape}")
        fi, ii, idn, cat = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (frame_idx, ivfc_idx, inst_id, cat_id))
        B = len(fi)
        if B == 0 or not (len(ii) == len(idn) == len(cat) == len(bbox) == len(mug_meta) == B):
            raise ValueError("frame_idx, ivfc_idx, inst_id, bbox, cat_id and mug_meta must have one entry per sample (B >= 1)")
        if fi.min() < 0 or fi.max() >= F or ii.min() < 0 or ii.max() >= NI:
            raise ValueError("frame_idx / ivfc_idx out of range")      # the kernel trusts them
        if idn.min() < 0 or idn.max() > 255 or cat.min() < 0 or cat.max() > 5:
            raise ValueError("inst_id must lie in [0, 255] and cat_id in [0, 5]")
        if set(labels) != set(LABEL_KEYS):
            raise ValueError(f"labels must hold exactly {LABEL_KEYS}, got {sorted(labels)}")
        lab = {k: np.ascontiguousarray(np.asarray(labels[k], dtype=np.float32)) for k in LABEL_KEYS}
        for k, v in lab.items():
            if v.ndim < 1 or v.shape[0] != B:
                raise ValueError(f"labels[{k!r}] {v.shape}: the leading dimension must be B = {B}")
        keys = None
        if seed is not None:
            seed = int(seed)
            if not 0 <= seed < 1 << 64:
                raise ValueError(f"seed: {seed} is not in [0, 2^64)")
            dzi, deform = host_draws(seed, B, self.mask_pro)
        else:
            if not isinstance(draws, dict) or set(draws) != {"dzi", "deform", "keys"}:
                raise ValueError("draws must be {'dzi': (B,3), 'deform': (B,), 'keys': (B,S,S) uint32}")
            dzi, deform = np.asarray(draws["dzi"], dtype=np.float64), np.asarray(draws["deform"])
            if dzi.shape != (B, 3) or not ((dzi >= 0) & (dzi < 1)).all():
                raise ValueError(f"draws['dzi'] must be ({B},3) in [0,1)")
            if deform.shape != (B,):
                raise ValueError(f"draws['deform'] must be ({B},)")
            keys = np.asarray(draws["keys"])
            if keys.shape != (B, S, S) or keys.dtype != np.uint32:
                raise ValueError(f"draws['keys'] must be ({B},{S},{S}) uint32, not {keys.shape} {keys.dtype}")
            keys = torch.from_numpy(np.ascontiguousarray(keys).view(np.int32)).to(dev)
        P = self.host_params(bbox, cat, mug_meta, dzi)
        if out is None:
            out = {}

        def buf(name, shape):
            t = out.get(name)
            if t is None:
                t = out[name] = torch.empty(shape, device=dev, dtype=torch.float32)
            if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"out[{name!r}] must be a contiguous fp32 {tuple(shape)} tensor on {dev}")
            return t
        shapes = {"roi_img": (B, 3, S, S), "roi_mask": (B, 1, S, S), "roi_mask_deform": (B, 1, S, S), "roi_mask_output": (B, 1, R, R),
                  "roi_ivfc_mask_output": (B, 1, R, R), "roi_coord_2d": (B, 2, R, R), "nocs_coord": (B, 3, R, R), "ivfc_coord": (B, 3, R, R)}
        m = {k: buf(k, shapes[k]) for k in MAP_KEYS}
        small = {k: buf(k, P[k].shape) for k in ("roi_wh", "bbox_center", "resize_ratio")}
        small.update({k: buf(k, v.shape) for k, v in lab.items()})      # every buffer is checked before anything is written
        if m["roi_mask"].data_ptr() == m["roi_mask_deform"].data_ptr():
            raise ValueError("out['roi_mask'] and out['roi_mask_deform'] must be two buffers")
        up = lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)
        inv = up(np.concatenate([P["inv_img"].reshape(-1), P["inv_out"].reshape(-1)]))
        idx = up(np.concatenate([fi, ii, idn]).astype(np.int32))
        table = up(P["table"])
        dfm = up(np.ascontiguousarray(deform != 0).view(np.uint8))
        L = _lib.load()
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.gpt_crop_train(frames.data_ptr(), inst_masks.data_ptr(), nocs_png.data_ptr(), ivfc_png.data_ptr(), idx.data_ptr(),
                                    idx.data_ptr() + 4 * B, idx.data_ptr() + 8 * B, inv.data_ptr(), inv.data_ptr() + 8 * 6 * B,
                                    self.img_lut.data_ptr(), self.xlut.data_ptr(), self.ylut.data_ptr(), table.data_ptr(), table.data_ptr(),
                                    m["roi_img"].data_ptr(), m["roi_mask"].data_ptr(), m["roi_mask_output"].data_ptr(),
                                    m["roi_ivfc_mask_output"].data_ptr(), m["roi_coord_2d"].data_ptr(), m["nocs_coord"].data_ptr(),
                                    m["ivfc_coord"].data_ptr(), B, F, NI, H, W, S, R, stream), "gpt_crop_train")
        _lib.check(L.gpt_mask_deform(m["roi_mask"].data_ptr(), dfm.data_ptr(), None if keys is None else keys.data_ptr(),
                                     0 if seed is None else seed, m["roi_mask_deform"].data_ptr(), B, S, stream), "gpt_mask_deform")
        for k in ("roi_wh", "bbox_center", "resize_ratio"):
            small[k].copy_(torch.from_numpy(P[k]).pin_memory(), non_blocking=True)
        for k, v in lab.items():
            small[k].copy_(torch.from_numpy(v).pin_memory(), non_blocking=True)
        return out
