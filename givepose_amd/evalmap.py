"""Degree-cm / 3D-IoU mAP of a run on the device: the drop-in for `compute_degree_cm_mAP` of the reference
(evaluation/eval_utils_cass.py:490-820, called twice by evaluation/evaluate.py:160, 234).

    pairs of a frame and class --gp_eval_pair_overlaps--> IoU (float32), (degree, cm) (float64)
                               --gp_eval_match----------> matched flags per (threshold cell, prediction / ground truth)
    classes x cells            --gp_eval_ap-------------> AP per class and cell, and the mean over the classes

The host only groups: it sorts the predictions of every (frame, class) by score, builds the CSR-style offset tables the kernels
walk, and sorts each class's predictions of the whole run by score once.  All arithmetic is float64 HIP (csrc/evalmap.hip); there
is no NumPy fallback.  Not built: eval_size, eval_recon, plot_figure (NotImplementedError), the `phone / eggbox / glue` branch of the
reference (unreachable with the NOCS classes; such a `synset_names` is refused), the legacy real_iou=False boxes.

Where this differs from the reference on purpose:
  * float32 poses are widened to float64 and everything is float64; the reference, handed float32 arrays, takes det / cbrt in float32.
  * the IoU is rounded to float32 as there, and the thresholds are compared against that value widened to float64.
  * equal scores inside one class: the reference leaves their order to `np.argsort(...)[::-1]`; here the earlier prediction goes first.
  * more than 64 predictions or ground truths of one class in one frame are refused (the reference asserts at most 48 per frame).
  * `pred_bboxes` is not read (the reference only trims all-zero rows from it, and asserts that there are none).
"""
import numpy as np
import torch

from . import _lib

SYMMETRIC = ("bottle", "bowl", "can")          # rotation about y is free (eval_utils_cass.py:75, 148); `mug` when its handle is hidden
UNSUPPORTED = ("phone", "eggbox", "glue")      # eval_utils_cass.py:161-166
MAX_PER_GROUP = 64                             # GP_EVAL_MAX_PER_GROUP
_AP_WORKGROUPS = 2048


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev_float(x, dev):
    """(n, ...) poses or sizes as float32 / float64: a device tensor stays where it is; a host array stays on the host until `_cat`
    uploads the whole run in one copy."""
    if isinstance(x, torch.Tensor):
        t = x.detach()
        if t.dtype not in (torch.float32, torch.float64):
            t = t.double()
        return t.to(dev).contiguous()
    a = np.asarray(x)
    return a if a.dtype == np.float32 else a.astype(np.float64)


def _numel(t):
    return t.numel() if isinstance(t, torch.Tensor) else t.size


def _host(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).reshape(-1).astype(dtype)


def _cat(ts, tail, dev):
    ts = [t.reshape(-1, *tail) for t in ts if _numel(t)]
    if not ts:
        return torch.zeros((0, *tail), dtype=torch.float64, device=dev)
    f64 = len({str(t.dtype).split(".")[-1] for t in ts}) > 1
    if all(isinstance(t, np.ndarray) for t in ts):
        a = np.concatenate([t.astype(np.float64) for t in ts] if f64 else ts, 0)
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ts = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) if isinstance(t, np.ndarray) else t for t in ts]
    return torch.cat([t.double() for t in ts] if f64 else ts, 0).contiguous()


class MapAccumulator:
    """Collects the frames of a run; `compute` evaluates them in three launches."""

    def __init__(self, synset_names, device="cuda"):
        bad = [n for n in synset_names if n in UNSUPPORTED]
        if bad:
            raise NotImplementedError(f"the 180-degree symmetric classes {bad} of the reference are not built")
        self.names, self.dev = list(synset_names), torch.device(device)
        if self.dev.type != "cuda":
            raise _lib.GivePoseHipError("the mAP evaluation runs on the GPU only: there is no CPU path")
        self._p_rt, self._p_size, self._g_rt, self._g_size = [], [], [], []
        self._p_cls, self._p_score, self._p_frame, self._g_cls, self._g_hv, self._g_frame = [], [], [], [], [], []
        self.n_frames = 0

    def add_frame(self, pred_RT, pred_size, pred_class_ids, pred_scores, gt_RTs, gt_scales, gt_class_ids, gt_handle_visibility):
        """One frame.  pred_RT (n,4,4) / pred_size (n,3): the device tensors `FramePipeline` returns (or arrays); gt_RTs (m,4,4) /
        gt_scales (m,3); class ids index `synset_names` (0 = BG is ignored, as in the reference); scores (n,); handle visibility (m,)."""
        pc, ps = _host(pred_class_ids, np.int64), _host(pred_scores, np.float64)
        gc, gh = _host(gt_class_ids, np.int64), _host(gt_handle_visibility, np.int64)
        if len(ps) != len(pc) or len(gh) != len(gc):
            raise ValueError("add_frame: class ids, scores and handle visibilities do not line up")
        f = self.n_frames
        self.n_frames += 1
        if len(pc):
            rt, sz = _dev_float(pred_RT, self.dev), _dev_float(pred_size, self.dev)
            if _numel(rt) != len(pc) * 16 or _numel(sz) != len(pc) * 3:
                raise ValueError(f"add_frame: {len(pc)} predictions but pred_RT {tuple(rt.shape)}, pred_size {tuple(sz.shape)}")
            self._p_rt.append(rt); self._p_size.append(sz)
            self._p_cls.append(pc); self._p_score.append(ps); self._p_frame.append(np.full(len(pc), f, np.int64))
        if len(gc):
            rt, sz = _dev_float(gt_RTs, self.dev), _dev_float(gt_scales, self.dev)
            if _numel(rt) != len(gc) * 16 or _numel(sz) != len(gc) * 3:
                raise ValueError(f"add_frame: {len(gc)} ground truths but gt_RTs {tuple(rt.shape)}, gt_scales {tuple(sz.shape)}")
            self._g_rt.append(rt); self._g_size.append(sz)
            self._g_cls.append(gc); self._g_hv.append(gh); self._g_frame.append(np.full(len(gc), f, np.int64))

    def _tensors(self):
        return (_cat(self._p_rt, (4, 4), self.dev), _cat(self._p_size, (3,), self.dev),
                _cat(self._g_rt, (4, 4), self.dev), _cat(self._g_size, (3,), self.dev))

    def normalised(self):
        """The scale-normalised view evaluate.py:215-227 evaluates a second time: rows 0..2 of every pose divided by cbrt(det R)."""
        L = _lib.load()
        out = MapAccumulator(self.names, self.dev)
        for k in ("_p_size", "_g_size", "_p_cls", "_p_score", "_p_frame", "_g_cls", "_g_hv", "_g_frame"):
            setattr(out, k, list(getattr(self, k)))
        out.n_frames = self.n_frames
        p_rt, _, g_rt, _ = self._tensors()
        for src, dst in ((p_rt, out._p_rt), (g_rt, out._g_rt)):
            if src.shape[0]:
                o = torch.empty(src.shape, dtype=torch.float64, device=self.dev)
                _lib.check(L.gp_eval_normalise(src.data_ptr(), _lib.GP_F64 if src.dtype == torch.float64 else _lib.GP_F32, o.data_ptr(),
                                               src.shape[0], _stream(self.dev)), "gp_eval_normalise")
                dst.append(o)
        return out

    def compute(self, degree_thresholds=(360,), shift_thresholds=(100,), iou_3d_thresholds=(0.1,), iou_pose_thres=0.1,
                use_matches_for_pose=False, return_details=False):
        """-> (iou_3d_aps (len(names) + 1, n_iou), pose_aps (len(names) + 1, n_deg + 1, n_shift + 1)), float64 NumPy, rows as in the
        reference: 0 = BG (zeros), the classes, last = their mean.  `return_details`: also a dict of the intermediate arrays."""
        L, dev = _lib.load(), self.dev
        deg = np.asarray(list(degree_thresholds) + [360], np.float64)
        shift = np.asarray(list(shift_thresholds) + [100000], np.float64)
        iou_thr = np.asarray(list(iou_3d_thresholds), np.float64)
        n_deg, n_shift, n_iou = len(deg), len(shift), len(iou_thr)
        if n_iou == 0:
            raise ValueError("iou_3d_thresholds is empty")
        gate = -1
        if use_matches_for_pose:
            if iou_pose_thres not in list(iou_3d_thresholds):
                raise ValueError(f"use_matches_for_pose: iou_pose_thres {iou_pose_thres} is not one of iou_3d_thresholds")
            gate = list(iou_3d_thresholds).index(iou_pose_thres)
        num_classes = len(self.names)
        n_cls = num_classes - 1
        if n_cls < 1:
            raise ValueError("synset_names needs BG and at least one class")
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
        p_cls, p_score, p_frame = cat(self._p_cls, np.int64), cat(self._p_score, np.float64), cat(self._p_frame, np.int64)
        g_cls, g_hv, g_frame = cat(self._g_cls, np.int64), cat(self._g_hv, np.int64), cat(self._g_frame, np.int64)
        p_rt, p_size, g_rt, g_size = self._tensors()
        # ---- grouping (host): slots = the kept predictions / ground truths, group-major; predictions by descending score inside a group
        p_keep, g_keep = np.flatnonzero((p_cls >= 1) & (p_cls < num_classes)), np.flatnonzero((g_cls >= 1) & (g_cls < num_classes))
        p_key, g_key = p_frame[p_keep] * num_classes + p_cls[p_keep], g_frame[g_keep] * num_classes + g_cls[g_keep]
        o = np.lexsort((-p_score[p_keep], p_key))
        p_rows, p_key = p_keep[o], p_key[o]
        o = np.argsort(g_key, kind="stable")
        g_rows, g_key = g_keep[o], g_key[o]
        n_pred, n_gt = len(p_rows), len(g_rows)
        keys = np.union1d(p_key, g_key)
        G = len(keys)
        pred_off = np.searchsorted(p_key, np.append(keys, np.iinfo(np.int64).max)).astype(np.int64)
        gt_off = np.searchsorted(g_key, np.append(keys, np.iinfo(np.int64).max)).astype(np.int64)
        if G:
            pred_off[-1], gt_off[-1] = n_pred, n_gt
        npg, ngg = np.diff(pred_off), np.diff(gt_off)
        biggest = int(max(npg.max(initial=0), ngg.max(initial=0)))
        if biggest > MAX_PER_GROUP:
            raise ValueError(f"{biggest} predictions or ground truths of one class in one frame: at most {MAX_PER_GROUP} are supported")
        pair_off = np.concatenate([[0], np.cumsum(npg * ngg)]).astype(np.int64)
        P = int(pair_off[-1])
        if max(P, n_pred, n_gt) >= 2 ** 22:
            raise ValueError("run too large for one evaluation (2^22 predictions, ground truths or pairs)")
        grp = np.repeat(np.arange(G), npg * ngg)
        loc = np.arange(P) - pair_off[grp]
        pair_pred = p_rows[pred_off[grp] + loc // np.maximum(ngg[grp], 1)]
        pair_gt_slot = gt_off[grp] + loc % np.maximum(ngg[grp], 1)
        names = np.asarray(self.names)
        g_sym = np.isin(names[g_cls[g_rows]], SYMMETRIC) | ((names[g_cls[g_rows]] == "mug") & (g_hv[g_rows] == 0))
        # ---- the class-wise score order of the whole run (one per class, shared by every cell)
        slot_cls, slot_score = p_cls[p_rows], p_score[p_rows]
        order = np.lexsort((-slot_score, slot_cls))
        cls_off = np.searchsorted(slot_cls[order], np.arange(1, num_classes + 1))
        cls_ngt = np.bincount(g_cls[g_rows], minlength=num_classes)[1:num_classes]
        work_stride = int(np.diff(cls_off).max(initial=0)) + 2

        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev) if len(a) else torch.zeros(1, dtype=getattr(torch, np.dtype(dt).name), device=dev)
        d_pair_pred, d_pair_gt = up(pair_pred, np.int32), up(g_rows[pair_gt_slot] if P else np.zeros(0), np.int32)
        d_pair_sym = up(g_sym[pair_gt_slot].astype(np.uint8) if P else np.zeros(0), np.uint8)
        d_pred_off, d_gt_off, d_pair_off = up(pred_off, np.int32), up(gt_off, np.int32), up(pair_off, np.int32)
        d_order, d_cls_off, d_cls_ngt = up(order, np.int32), up(cls_off, np.int32), up(cls_ngt, np.int32)
        ang = 2 * np.pi * np.arange(20) / float(20)
        d_cs, d_iou_thr, d_deg, d_shift = up(np.concatenate([np.cos(ang), np.sin(ang)]), np.float64), up(iou_thr, np.float64), up(deg, np.float64), up(shift, np.float64)
        z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt, device=dev)
        iou = z(max(P, 1), dt=torch.float32)
        deg_cm = z(max(P, 1), 2, dt=torch.float64)
        n_pose = n_deg * n_shift
        f_ip, f_ig = z(n_iou, max(n_pred, 1)), z(n_iou, max(n_gt, 1))
        f_pp, f_pg = z(n_pose, max(n_pred, 1)), z(n_pose, max(n_gt, 1))
        status = z(1, dt=torch.int32)
        iou_ap, pose_ap = z(n_cls + 1, n_iou, dt=torch.float64), z(n_cls + 1, n_pose, dt=torch.float64)
        work = z(_AP_WORKGROUPS * work_stride, dt=torch.float64)
        st = _stream(dev)
        dt_of = lambda t: _lib.GP_F64 if t.dtype == torch.float64 else _lib.GP_F32
        if p_size.dtype != p_rt.dtype:
            p_size = p_size.to(p_rt.dtype)
        if g_size.dtype != g_rt.dtype:
            g_size = g_size.to(g_rt.dtype)
        if P:
            _lib.check(L.gp_eval_pair_overlaps(p_rt.data_ptr(), p_size.data_ptr(), dt_of(p_rt), g_rt.data_ptr(), g_size.data_ptr(), dt_of(g_rt),
                                               d_pair_pred.data_ptr(), d_pair_gt.data_ptr(), d_pair_sym.data_ptr(), d_cs.data_ptr(),
                                               iou.data_ptr(), deg_cm.data_ptr(), P, st), "gp_eval_pair_overlaps")
        if G:
            _lib.check(L.gp_eval_match(iou.data_ptr(), deg_cm.data_ptr(), d_pred_off.data_ptr(), d_gt_off.data_ptr(), d_pair_off.data_ptr(), G,
                                       biggest, d_iou_thr.data_ptr(), n_iou, d_deg.data_ptr(), n_deg, d_shift.data_ptr(), n_shift, gate,
                                       max(n_pred, 1), max(n_gt, 1), f_ip.data_ptr(), f_ig.data_ptr(), f_pp.data_ptr(), f_pg.data_ptr(),
                                       status.data_ptr(), st), "gp_eval_match")
        # np.mean over the class rows: a column-wise sum for the IoU table, a strided 1-D sum per cell for the pose table
        _lib.check(L.gp_eval_ap(f_ip.data_ptr(), 0, max(n_pred, 1), d_order.data_ptr(), d_cls_off.data_ptr(), d_cls_ngt.data_ptr(), n_cls,
                                n_iou, work.data_ptr(), work_stride, _AP_WORKGROUPS, 0, iou_ap.data_ptr(), st), "gp_eval_ap")
        _lib.check(L.gp_eval_ap(f_pp.data_ptr(), f_ip[gate].data_ptr() if gate >= 0 else 0, max(n_pred, 1), d_order.data_ptr(),
                                d_cls_off.data_ptr(), d_cls_ngt.data_ptr(), n_cls, n_pose, work.data_ptr(), work_stride, _AP_WORKGROUPS, 1,
                                pose_ap.data_ptr(), st), "gp_eval_ap")
        iou_h, pose_h = iou_ap.cpu().numpy(), pose_ap.cpu().numpy()      # the D->H copies synchronise
        if int(status.cpu()[0]):
            raise _lib.GivePoseHipError("gp_eval_match: a group exceeds 64 predictions or ground truths")
        iou_3d_aps = np.zeros((num_classes + 1, n_iou))
        pose_aps = np.zeros((num_classes + 1, n_deg, n_shift))
        iou_3d_aps[1:num_classes], iou_3d_aps[-1] = iou_h[:n_cls], iou_h[n_cls]
        pose_aps[1:num_classes], pose_aps[-1] = pose_h[:n_cls].reshape(n_cls, n_deg, n_shift), pose_h[n_cls].reshape(n_deg, n_shift)
        if not return_details:
            return iou_3d_aps, pose_aps
        det = dict(group_frame=keys // num_classes, group_class=keys % num_classes, pred_off=pred_off, gt_off=gt_off, pair_off=pair_off,
                   pred_rows=p_rows, gt_rows=g_rows, iou=iou.cpu().numpy()[:P], deg_cm=deg_cm.cpu().numpy()[:P],
                   iou_pred_flag=f_ip.cpu().numpy()[:, :n_pred], iou_gt_flag=f_ig.cpu().numpy()[:, :n_gt],
                   pose_pred_flag=f_pp.cpu().numpy()[:, :n_pred].reshape(n_deg, n_shift, n_pred),
                   pose_gt_flag=f_pg.cpu().numpy()[:, :n_gt].reshape(n_deg, n_shift, n_gt))
        return iou_3d_aps, pose_aps, det


def compute_degree_cm_mAP(final_results, synset_names, log_dir=None, degree_thresholds=[360], shift_thresholds=[100],
                          iou_3d_thresholds=[0.1], iou_pose_thres=0.1, use_matches_for_pose=False, eval_recon=False, plot_figure=False,
                          eval_size=False, device="cuda"):
    """The reference's signature, defaults and `final_results` (a list of dicts with gt_class_ids, gt_RTs, gt_scales,
    gt_handle_visibility, pred_class_ids, pred_scales, pred_scores, pred_RTs) -> (iou_3d_aps, pose_aps).  `log_dir` is unused (it
    only serves the plots there)."""
    if eval_recon or plot_figure or eval_size:
        raise NotImplementedError("eval_recon, eval_size and plot_figure of the reference are not built")
    acc = MapAccumulator(synset_names, device)
    for r in final_results:
        if len(r["gt_class_ids"]) == 0 and len(r["pred_class_ids"]) == 0:      # eval_utils_cass.py:558
            continue
        acc.add_frame(r["pred_RTs"], r["pred_scales"], r["pred_class_ids"], r["pred_scores"], r["gt_RTs"], r["gt_scales"],
                      r["gt_class_ids"], r["gt_handle_visibility"])
    return acc.compute(degree_thresholds, shift_thresholds, iou_3d_thresholds, iou_pose_thres, use_matches_for_pose)


def paper_table(iou_aps, pose_aps, synset_names, iou_thres_list, degree_thres_list, shift_thres_list, normalised=False, per_obj=None):
    """The lines evaluate.py logs after each of its two evaluations (:170-203 in centimetres; :245-280, `normalised`, in per cent of
    the object's scale).  `per_obj`: a class name -> that class's block only (FLAGS.per_obj)."""
    i25, i50, i75 = (list(iou_thres_list).index(t) for t in (0.25, 0.5, 0.75))
    d05, d10 = list(degree_thres_list).index(5), list(degree_thres_list).index(10)
    a, b = (20, 50) if normalised else (5, 10)
    sa, sb = list(shift_thres_list).index(a), list(shift_thres_list).index(b)
    ua, ub = (f"{a}%", f"{b}%") if normalised else (f"{a}cm", f"{b}cm")

    def block(idx, tail):
        out = ["3D IoU at 25: {:.1f}".format(iou_aps[idx, i25] * 100), "3D IoU at 50: {:.1f}".format(iou_aps[idx, i50] * 100),
               "3D IoU at 75: {:.1f}".format(iou_aps[idx, i75] * 100),
               "5 degree, {}: {:.1f}".format(ua, pose_aps[idx, d05, sa] * 100), "10 degree, {}: {:.1f}".format(ua, pose_aps[idx, d10, sa] * 100),
               "10 degree, {}: {:.1f}".format(ub, pose_aps[idx, d10, sb] * 100)]
        if tail:
            out.append("10 degree: {:.1f}".format(pose_aps[idx, d10, -1] * 100))
            out += ["{}: {:.1f}".format(ua, pose_aps[idx, -1, sa] * 100), "{}: {:.1f}".format(ub, pose_aps[idx, -1, sb] * 100)] if normalised else \
                   ["{}: {:.1f}".format(ub, pose_aps[idx, -1, sb] * 100)]
        return out

    names = list(synset_names)
    if per_obj in names:
        return ["mAP:"] + block(names.index(per_obj), True)
    msgs = ["average mAP:"] + block(-1, True)
    for idx in range(1, len(names)):
        msgs += ["category {}".format(names[idx]), "mAP:"] + block(idx, normalised)
    return msgs
