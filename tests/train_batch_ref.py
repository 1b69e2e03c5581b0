"""TEST INFRASTRUCTURE ONLY: numpy restatement of the reference's train-time sample (datasets/load_data_nocs.py:238-386), written from
its arithmetic on full-frame float arrays -- it uses none of the product's tables, maps or kernels.

Follows, line for line: the NOCS / IVFC conversions (257-266, 311-324), aug_bbox_DZI (tools/dataset_utils.py:32-82) with the draws
handed in, get_real_hw (tools/eval_utils.py:243-249), the seven NEAREST crops (277-331) through oracle/preprocess_ref.py's restatement
of get_affine_transform / cv2.warpAffine, and defor_2D (datasets/data_augmentation.py:11-33).

defor_2D's cv2 calls are restated from the published algorithm, as the warp is in oracle/preprocess_ref.py and with the same caveat
(OpenCV is not installed here: **parity unpinned**): getStructuringElement(MORPH_ELLIPSE, (2,2)) is [[0,1],[1,1]] with the default
anchor (1,1), so erode / dilate take the min / max over (x,y), (x,y-1), (x-1,y); the default border value of a morphological
operation leaves pixels outside the image out of the min / max; `cv2.erode(mask, kernel, rand_r)` passes rand_r as `dst`, so ONE
iteration runs.  np.random.choice(l, l // 2, replace=False) is replaced by explicit keys: the l // 2 band pixels that come first in
a stable argsort of the keys (ties: the lower pixel index) become 0 -- the same distribution for independent uniform keys, another
stream.  Also here: the numpy form of the key hash of a seeded call (include/givepose_sizegrad.h's counter hash).
"""
import numpy as np

from oracle.preprocess_ref import get_2d_coord_ref, get_affine_transform_ref, warp_affine_nearest_ref

IMG_MEAN = (0.485, 0.456, 0.406)
IMG_STD = (0.229, 0.224, 0.225)


def hash_keys(seed, B, S):
    """(B,S,S) uint32: the device's key of pixel i of sample b under `seed` (idx = b S S + i)."""
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    idx = np.arange(B * S * S, dtype=np.uint64)
    x = (idx * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    x = x.astype(np.uint32) ^ lo ^ ((hi << np.uint32(16)) | (hi >> np.uint32(16)))
    mul = lambda a, c: ((a.astype(np.uint64) * np.uint64(c)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    x ^= x >> np.uint32(16)
    x = mul(x, 0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x = mul(x, 0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x.reshape(B, S, S)


def aug_bbox_dzi_ref(bbox_xyxy, u, im_H, im_W, dzi_type, scale_ratio=0.25, shift_ratio=0.25, pad_scale=1.5):
    """tools/dataset_utils.py:32-82; u = the three values np.random.random_sample() would return, in call order."""
    x1, y1, x2, y2 = [float(v) for v in bbox_xyxy]
    cx = 0.5 * (x1 + x2)
    cy = 0.5 * (y1 + y2)
    bh = y2 - y1
    bw = x2 - x1
    if dzi_type == "uniform":
        sr = 1 + scale_ratio * (2 * float(u[0]) - 1)
        shift = shift_ratio * (2 * np.array([u[1], u[2]], dtype=np.float64) - 1)
        center = np.array([cx + bw * shift[0], cy + bh * shift[1]])
        scale = max(y2 - y1, x2 - x1) * sr * pad_scale
    elif dzi_type == "uniform_sr":
        sr = 1 - 0.25 * float(u[0])
        shift = shift_ratio * (2 * np.array([u[1], u[2]], dtype=np.float64) - 1)
        center = np.array([cx + bw * shift[0], cy + bh * shift[1]])
        scale = max(y2 - y1, x2 - x1) * sr * pad_scale
    elif dzi_type == "none":
        center = np.array([cx, cy])
        scale = max(y2 - y1, x2 - x1)
    else:
        raise NotImplementedError(dzi_type)
    scale = min(scale, max(im_H, im_W)) * 1.0
    return center, scale


def coord_frame_ref(png, cat_id, mug_meta):
    """load_data_nocs.py:257-266 (and 312-323): (H,W,3) uint8 RGB -> the float coordinate frame, before any masking."""
    c = np.array(png, dtype=np.float32) / 255
    c[:, :, 2] = 1 - c[:, :, 2]
    c = c - 0.5
    if cat_id == 5:
        T0, s0 = mug_meta
        c = s0 * (c + T0)
    return c


def defor_2d_ref(roi_mask, deform, keys):
    """datasets/data_augmentation.py:11-33 with `deform` in the place of (np.random.rand() <= rand_pro) and keys (S,S) uint32 in the
    place of np.random.choice."""
    roi_mask = roi_mask.copy().squeeze()
    if not deform:
        return roi_mask
    S0, S1 = roi_mask.shape

    def morph(op, fill):
        p = np.full((S0 + 1, S1 + 1), fill, dtype=roi_mask.dtype)
        p[1:, 1:] = roi_mask
        return op(op(p[1:, 1:], p[:-1, 1:]), p[1:, :-1])          # (x,y), (x,y-1), (x-1,y)
    band = morph(np.minimum, np.inf) != morph(np.maximum, -np.inf)
    change_list = roi_mask[band]
    l_list = change_list.size
    if l_list < 1.0:
        return roi_mask
    order = np.argsort(np.asarray(keys)[band], kind="stable")     # boolean indexing walks the pixels in index order
    choose = order[: l_list // 2]
    change_list = np.ones_like(change_list)
    change_list[choose] = 0.0
    roi_mask[band] = change_list
    roi_mask[roi_mask > 0.0] = 1.0
    return roi_mask


def sample_ref(image, mask, nocs_png, ivfc_png, inst_id, bbox, cat_id, mug_meta, u, deform, keys, img_size=256, out_res=64,
               dzi_type="uniform", pad_scale=1.5, scale_ratio=0.25, shift_ratio=0.25):
    """One sample of __getitem__ from decoded uint8 arrays: image (H,W,3) RGB, mask (H,W) instance ids, nocs_png / ivfc_png (H,W,3) RGB;
    bbox (y1,x1,y2,x2)."""
    im_H, im_W = image.shape[:2]
    coord_2d = get_2d_coord_ref(im_W, im_H)
    nocs_coord = coord_frame_ref(nocs_png, cat_id, mug_meta)
    y1, x1, y2, x2 = bbox
    center, scale = aug_bbox_dzi_ref(np.array([x1, y1, x2, y2]), u, im_H, im_W, dzi_type, scale_ratio, shift_ratio, pad_scale)
    bw, bh = min(im_W, x2) - max(0, x1), min(im_H, y2) - max(0, y1)
    M_img = get_affine_transform_ref(center, scale, img_size)
    M_out = get_affine_transform_ref(center, scale, out_res)

    roi_img = warp_affine_nearest_ref(image, M_img, img_size)
    roi_img = (roi_img / 255.0 - IMG_MEAN) / IMG_STD
    roi_img = roi_img.transpose(2, 0, 1)
    roi_coord_2d = warp_affine_nearest_ref(coord_2d, M_out, out_res).transpose(2, 0, 1)

    mask_target = mask.copy().astype(np.float32)
    mask_target[mask != inst_id] = 0.0
    mask_target[mask == inst_id] = 1.0
    nocs_coord[mask_target == 0] = 0
    roi_mask = warp_affine_nearest_ref(mask_target, M_img, img_size)[None]
    roi_mask_output = warp_affine_nearest_ref(mask_target, M_out, out_res)[None]
    roi_nocs_coord = warp_affine_nearest_ref(nocs_coord, M_out, out_res).transpose(2, 0, 1)

    ivfc_f = np.array(ivfc_png, dtype=np.float32) / 255
    mask_target_ivfc = np.ones_like(mask_target)
    mask_target_ivfc[ivfc_f[:, :, 0] == 0] = 0
    ivfc_coord = coord_frame_ref(ivfc_png, cat_id, mug_meta)
    ivfc_coord[mask_target_ivfc == 0] = 0
    roi_ivfc_coord = warp_affine_nearest_ref(ivfc_coord, M_out, out_res).transpose(2, 0, 1)
    roi_ivfc_mask_output = warp_affine_nearest_ref(mask_target_ivfc, M_out, out_res)[None]

    roi_mask_def = defor_2d_ref(roi_mask, deform, keys)
    f = lambda a: np.array(np.asarray(a).astype(np.float32), order="C")       # torch.as_tensor(..., dtype=float32).contiguous(); a scalar stays 0-d
    return {"roi_img": f(roi_img), "roi_mask": f(roi_mask), "roi_mask_deform": f(roi_mask_def)[None], "roi_mask_output": f(roi_mask_output),
            "roi_ivfc_mask_output": f(roi_ivfc_mask_output), "roi_coord_2d": f(roi_coord_2d), "nocs_coord": f(roi_nocs_coord),
            "ivfc_coord": f(roi_ivfc_coord), "roi_wh": f([bw, bh]), "bbox_center": f(center), "resize_ratio": f(out_res / scale)}


def batch_ref(frames, inst_masks, nocs_png, ivfc_png, frame_idx, ivfc_idx, inst_id, bbox, cat_id, mug_meta, draws, **kw):
    """The collated batch: sample_ref per sample, stacked."""
    rows = [sample_ref(frames[frame_idx[b]], inst_masks[frame_idx[b]], nocs_png[frame_idx[b]], ivfc_png[ivfc_idx[b]], inst_id[b],
                       [float(v) for v in bbox[b]], cat_id[b], mug_meta[b], draws["dzi"][b], bool(draws["deform"][b]), draws["keys"][b], **kw)
            for b in range(len(frame_idx))]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}
