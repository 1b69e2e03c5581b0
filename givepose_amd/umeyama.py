"""Pose from the NOCS map and depth on the device: the reference's `pose_from_umeyama` (tools/umeyama.py:17-60; the RANSAC and
the Umeyama fit: tools/align_utils.py:10-104).  Host side of gpa_backproject / gpa_umeyama (include/givepose_align.h).

The camera-space points of a crop are back-projected from its depth and aligned to the crop's predicted NOCS coordinates by a
similarity transform: 128 RANSAC hypotheses of 5 points each, evaluated in parallel, the reference's sequential acceptance and
early-stop rule replayed on their inlier counts, then one fit on the inliers of the winner.

The reference draws its samples from NumPy's global generator.  Here the draws are an explicit (B, 128, 5) uint32 table
(`draws`; hypothesis i of crop b fits the points `draws[b, i] mod n_points[b]`), by default filled from
`np.random.RandomState(seed)` and uploaded once per (B, seed, device): the documented substitute that makes a run reproducible.

One documented departure: a sample or inlier set whose covariance has rank < 2 (sigma_2 <= 1e-12 sigma_1) or no source variance
has no defined fit -- the reference's result there is LAPACK's choice of null-space vectors.  Such a hypothesis counts zero
inliers; such a final set fails with status DEGENERATE.  A failed crop returns (1, I, 0), as tools/umeyama.py:30-33 does.

HIP devices only; there is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib

OK, NO_POINTS, LOW_INLIERS, DEGENERATE = _lib.GPA_OK, _lib.GPA_NO_POINTS, _lib.GPA_LOW_INLIERS, _lib.GPA_DEGENERATE
STATUS_NAMES = {OK: "ok", NO_POINTS: "no masked point", LOW_INLIERS: "best inlier ratio < 0.1", DEGENERATE: "rank-deficient inlier set"}
RES, MAX_POINTS, MAX_ITER, SAMPLE = _lib.GPA_RES, _lib.GPA_MAX_POINTS, _lib.GPA_MAX_ITER, _lib.GPA_SAMPLE

_draw_cache = {}


def make_draws(B, seed=0):
    """The default draw table: (B, 128, 5) uint32 from np.random.RandomState(seed) (host array)."""
    return np.random.RandomState(seed).randint(0, 2 ** 32, size=(B, MAX_ITER, SAMPLE), dtype=np.uint64).astype(np.uint32)


def _default_draws(B, seed, dev):
    key = (B, seed, str(dev))
    t = _draw_cache.get(key)
    if t is None:
        if len(_draw_cache) > 16:
            _draw_cache.clear()
        t = _draw_cache[key] = torch.from_numpy(make_draws(B, seed).view(np.int32)).to(dev)
    return t


def _as_draws(draws, B, dev):
    if isinstance(draws, np.ndarray):
        if draws.dtype != np.uint32:
            raise ValueError(f"draws must be uint32, not {draws.dtype}")
        draws = torch.from_numpy(np.ascontiguousarray(draws).view(np.int32))
    if hasattr(torch, "uint32") and draws.dtype == torch.uint32:
        draws = draws.view(torch.int32)
    if tuple(draws.shape) != (B, MAX_ITER, SAMPLE):
        raise ValueError(f"draws must be ({B}, {MAX_ITER}, {SAMPLE}), not {tuple(draws.shape)}")
    if draws.dtype != torch.int32:
        raise ValueError(f"draws must be a uint32 table (or its int32 view), not {draws.dtype}")
    return draws.to(dev).contiguous()


def pose_from_umeyama_device(xyz_coor, coor_2d, camK, Depth, obj_mask, draws=None, seed=0, valid_depth_only=False,
                             return_details=False):
    """xyz_coor (B,3,64,64) fp32 or fp16, coor_2d (B,2,64,64) pixel x / y, camK (B,3,3), Depth (B,1,64,64), obj_mask (B,1,64,64)
    (non-zero = object) -> (scales (B,), rots (B,3,3), trans (B,3)) float32 on the device; asynchronous on the current stream.

    valid_depth_only: also require depth > 0 (backproject, align_utils.py:116-117); off = the reference's pose_from_umeyama.
    return_details: a fourth value, the dict of float64 `scale` / `R` / `t` / `sRT` (B,4,4) / `sigma` (singular values of the
    final covariance, the last signed), the int32 `record` columns (`n_points`, `n_inliers`, `best_iteration`, `iterations_run`,
    `status`), `counts` (B,128) of every hypothesis, `inlier` (B,4096) flags of the winner over the compacted points, `index`
    (B,4096) pixel of each compacted point (-1 past the end), `points` (B,6,4096) and `PC` (B,4096,3) (the back-projection of
    every pixel)."""
    xyz_coor = torch.as_tensor(xyz_coor)
    dev = xyz_coor.device
    if dev.type != "cuda":
        raise _lib.GivePoseHipError("pose_from_umeyama_device runs on a HIP device only: there is no CPU path")
    if xyz_coor.dim() != 4:
        raise ValueError(f"xyz_coor must be (B,3,{RES},{RES}), not {tuple(xyz_coor.shape)}")
    B, R = xyz_coor.shape[0], xyz_coor.shape[-1]
    shapes = {"xyz_coor": (xyz_coor, (B, 3, R, R)), "coor_2d": (coor_2d, (B, 2, R, R)), "camK": (camK, (B, 3, 3)),
              "Depth": (Depth, (B, 1, R, R)), "obj_mask": (obj_mask, (B, 1, R, R))}
    for name, (t, shape) in shapes.items():
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, not {tuple(t.shape)}")
    if B == 0:
        raise ValueError("empty batch")
    f32 = lambda t: torch.as_tensor(t).to(dev, torch.float32).contiguous()      # fp16 map: widened first
    xyz, c2d, K, D = f32(xyz_coor), f32(coor_2d), f32(camK), f32(Depth)
    mask = (torch.as_tensor(obj_mask).to(dev) != 0).to(torch.uint8).contiguous()   # .bool() of the reference
    draws = _default_draws(B, seed, dev) if draws is None else _as_draws(draws, B, dev)
    e = lambda shape, dt: torch.empty(shape, device=dev, dtype=dt)
    points, index, n_points = e((B, 6, MAX_POINTS), torch.float32), e((B, MAX_POINTS), torch.int32), e((B,), torch.int32)
    pc = e((B, MAX_POINTS, 3), torch.float32) if return_details else None
    hyp, counts = e((B, MAX_ITER, _lib.GPA_HYP_STRIDE), torch.float64), e((B, MAX_ITER), torch.int32)
    inlier, fit64, sRT = e((B, MAX_POINTS), torch.uint8), e((B, _lib.GPA_FIT_STRIDE), torch.float64), e((B, 4, 4), torch.float64)
    record, fit32 = e((B, _lib.GPA_RECORD), torch.int32), e((B, _lib.GPA_FIT32_STRIDE), torch.float32)
    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        # R goes to the library as it is: a map of another size is refused there (GP_ERR_INVALID), before any launch
        _lib.check(L.gpa_backproject(xyz.data_ptr(), c2d.data_ptr(), K.data_ptr(), D.data_ptr(), mask.data_ptr(), int(bool(valid_depth_only)),
                                     B, R, points.data_ptr(), index.data_ptr(), n_points.data_ptr(), pc.data_ptr() if pc is not None else 0,
                                     stream), "gpa_backproject")
        _lib.check(L.gpa_umeyama(points.data_ptr(), n_points.data_ptr(), draws.data_ptr(), B, hyp.data_ptr(), counts.data_ptr(),
                                 inlier.data_ptr(), fit64.data_ptr(), sRT.data_ptr(), record.data_ptr(), fit32.data_ptr(), stream),
                   "gpa_umeyama")
    scales, rots, trans = fit32[:, 0].contiguous(), fit32[:, 1:10].reshape(B, 3, 3).contiguous(), fit32[:, 10:13].contiguous()
    if not return_details:
        return scales, rots, trans
    details = {"scale": fit64[:, 0], "R": fit64[:, 1:10].reshape(B, 3, 3), "t": fit64[:, 10:13], "sigma": fit64[:, 13:16], "sRT": sRT,
               "record": record, "n_points": record[:, 0], "n_inliers": record[:, 1], "best_iteration": record[:, 2],
               "iterations_run": record[:, 3], "status": record[:, 4], "counts": counts, "inlier": inlier, "index": index,
               "points": points, "PC": pc}
    return scales, rots, trans, details


def pose_from_umeyama(xyz_coor, coor_2d, camK, Depth, obj_mask, draws=None, seed=0, valid_depth_only=False, return_details=False):
    """The reference's signature and return (tools/umeyama.py:17,37): float32 CPU tensors (scales, rots, trans).  The inputs go to
    the HIP device they are on, or to the current one; the arithmetic runs there."""
    xyz_coor = torch.as_tensor(xyz_coor)
    if xyz_coor.device.type != "cuda":
        if not torch.cuda.is_available():
            raise _lib.GivePoseHipError("pose_from_umeyama needs a HIP device: there is no CPU path")
        xyz_coor = xyz_coor.to(torch.device("cuda", torch.cuda.current_device()))
    out = pose_from_umeyama_device(xyz_coor, coor_2d, camK, Depth, obj_mask, draws=draws, seed=seed, valid_depth_only=valid_depth_only,
                                   return_details=return_details)
    host = tuple(t.cpu().contiguous() for t in out[:3])
    if return_details:
        return host + ({k: (v.cpu() if v is not None else None) for k, v in out[3].items()},)
    return host
