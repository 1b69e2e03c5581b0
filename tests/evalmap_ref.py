"""NumPy restatement of the reference's degree-cm / 3D-IoU mAP (evaluation/eval_utils_cass.py:35-175, 260-362, 445-733) in this project's
own words: the checker of givepose_amd.evalmap on the GPU box, where the reference does not exist.  tests/test_evalmap_cpu.py pins it
against fixtures recorded from the reference itself (tests/golden/evalmap_*.npz, scripts/gen_golden_evalmap.py).

Vectorised where the reference loops: the pair values of a whole run in one batch, the greedy matchings of a (frame, class) over all
threshold cells at once.  Float64 throughout (float32 inputs are widened first, which the reference does not do for det / cbrt).

Also here: the per-pair bounds and the `decisive` filter that say when equal DECISIONS can be demanded of two implementations whose
floats differ in the last bits (used by the fixture generator on the reference's values and by the GPU test on this file's).
"""
import numpy as np

SYMMETRIC = ("bottle", "bowl", "can")

# Per-pair bounds between two float64 implementations of the same formulas (other summation order, other acos / cbrt / det).
EPS = np.finfo(np.float64).eps
# IoU: the float64 value carries a few ulp (coordinates ~1 m, extents ~0.1 m: relative 1e-14); rounding it to float32 can then land on the
# neighbouring float32.  One float32 ulp at 1.0 covers every IoU in [0, 1].
B_IOU = float(np.finfo(np.float32).eps)                  # 1.19e-7, absolute
# degrees: the arccos argument is a sum of 9 products of entries <= 1 over a product of norms: <= 16 eps.  Away from the endpoints the
# angle error is that over sin(theta); at them it is sqrt(2 * 16 eps) rad = 8.4e-8 rad = 4.8e-6 degree -- the bound, in absolute degrees.
B_DEG = float(np.degrees(np.sqrt(32 * EPS)))             # 4.83e-6 degree
# centimetres: |T1 - T2| * 100 with operands up to ~10 (scale-normalised translations) -> magnitude 1e3; 16 eps of that.
B_CM = float(16 * EPS * 1e3)                             # 3.6e-12 cm
# arccos argument within 16 eps of +-1  <=>  angle within B_DEG of 0 or 180 degrees
B_END = B_DEG


def pair_values(rt1, size1, rt2, size2, sym):
    """P pairs at once: rt (P,4,4), size (P,3), sym (P,) bool -> (iou float32 (P,), deg_cm float64 (P,2))."""
    rt1, size1, rt2, size2 = (np.asarray(a, np.float64) for a in (rt1, size1, rt2, size2))
    sym = np.asarray(sym, bool)
    P = len(rt1)
    if P == 0:
        return np.zeros(0, np.float32), np.zeros((0, 2))
    signs = np.array([[sx, sy, sz] for sy in (1, -1) for sx in (1, -1) for sz in (1, -1)], np.float64)      # the 8 corners

    def extent(M, size):            # M (..., 4, 4), size (..., 3) -> lo, hi (..., 3): the transformed corners' bounding box
        c = signs * (size[..., None, :] / 2)                                   # (..., 8, 3)
        h = np.concatenate([c, np.ones(c.shape[:-1] + (1,))], -1)              # homogeneous
        t = np.matmul(M[..., None, :, :], h[..., None])[..., 0]                # (..., 8, 4)
        xyz = t[..., :3] / t[..., 3:4]
        return xyz.min(-2), xyz.max(-2)

    def iou_of(M1, s1, lo2, hi2):
        lo1, hi1 = extent(M1, s1)
        d = np.minimum(hi1, hi2) - np.maximum(lo1, lo2)
        inter = np.where(d.min(-1) < 0, 0.0, d.prod(-1))
        return inter / ((hi1 - lo1).prod(-1) + (hi2 - lo2).prod(-1) - inter)

    lo2, hi2 = extent(rt2, size2)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = iou_of(rt1, size1, lo2, hi2)
        if sym.any():
            ang = 2 * np.pi * np.arange(20) / float(20)
            Ry = np.zeros((20, 4, 4))
            Ry[:, 0, 0], Ry[:, 0, 2], Ry[:, 2, 0], Ry[:, 2, 2], Ry[:, 1, 1], Ry[:, 3, 3] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang), 1, 1
            rot = np.matmul(rt1[sym][:, None], Ry[None])                           # (S, 20, 4, 4)
            v = iou_of(rot, size1[sym][:, None], lo2[sym][:, None], hi2[sym][:, None])
            iou[sym] = np.fmax.reduce(v, axis=1, initial=0.0)                      # max from 0; a NaN never wins a Python max()
        R1 = rt1[:, :3, :3] / np.cbrt(np.linalg.det(rt1[:, :3, :3]))[:, None, None]
        R2 = rt2[:, :3, :3] / np.cbrt(np.linalg.det(rt2[:, :3, :3]))[:, None, None]
        y1, y2 = R1[:, :, 1], R2[:, :, 1]
        arg_y = (y1 * y2).sum(-1) / (np.sqrt((y1 * y1).sum(-1)) * np.sqrt((y2 * y2).sum(-1)))
        arg_r = (np.einsum("pij,pij->p", R1, R2) - 1) / 2
        theta = np.arccos(np.where(sym, arg_y, arg_r)) * (180 / np.pi)
    d = rt1[:, :3, 3] - rt2[:, :3, 3]
    return iou.astype(np.float32), np.stack([theta, np.sqrt((d * d).sum(-1)) * 100], -1)


def match_iou(iou, thr):
    """One (frame, class): iou (np, ng) float32, predictions in descending score order -> pred (T, np), gt (T, ng) bool, all T thresholds at once."""
    n_p, n_g = iou.shape
    thr = np.asarray(thr, np.float64)
    pm, gm = np.zeros((len(thr), n_p), bool), np.zeros((len(thr), n_g), bool)
    for i in range(n_p):
        alive = np.ones(len(thr), bool)
        for j in np.argsort(-iou[i].astype(np.float64), kind="stable"):
            v = float(iou[i, j])
            if v != v:
                continue
            free = alive & ~gm[:, j]
            hit = free & (v > thr)
            gm[hit, j] = True
            pm[hit, i] = True
            alive &= ~(hit | (free & (v < thr)))
    return pm, gm


def match_pose(deg_cm, enters, deg_thr, shift_thr):
    """deg_cm (np, ng, 2); enters (np,) bool: the predictions that take part -> pred (D, S, np), gt (D, S, ng) bool."""
    n_p, n_g = deg_cm.shape[:2]
    deg_thr, shift_thr = np.asarray(deg_thr, np.float64), np.asarray(shift_thr, np.float64)
    D, S = len(deg_thr), len(shift_thr)
    pm, gm = np.zeros((D, S, n_p), bool), np.zeros((D, S, n_g), bool)
    if n_g == 0:
        return pm, gm
    with np.errstate(invalid="ignore"):
        for i in np.flatnonzero(enters):
            order = np.argsort(deg_cm[i].sum(-1), kind="stable")                    # ascending degree + cm, NaN last
            ok = ~(deg_cm[i, order, 0][None, None, :] > deg_thr[:, None, None]) & ~(deg_cm[i, order, 1][None, None, :] > shift_thr[None, :, None])
            cand = ok & ~gm[:, :, order]
            has = cand.any(-1)
            d, s = np.nonzero(has)
            gm[d, s, order[cand.argmax(-1)[d, s]]] = True
            pm[:, :, i] = has
    return pm, gm


def average_precision(flags, n_gt):
    """flags: the match flags of a class's predictions in descending score order -> AP (the VOC form of the reference, recall kept in float32)."""
    flags = np.asarray(flags, bool)
    hits = np.cumsum(flags)
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = hits / (np.arange(len(flags)) + 1)
        recall = hits.astype(np.float32) / n_gt
        p = np.concatenate([[0], precision, [0]])
        r = np.concatenate([[0], recall, [1]])
        p = np.maximum.accumulate(p[::-1])[::-1]
        steps = np.flatnonzero(r[:-1] != r[1:]) + 1
        return np.sum((r[steps] - r[steps - 1]) * p[steps])


def groups_of(final_results, synset_names):
    """-> list of dict(frame, cls, pred (indices into the frame, descending score), gt (indices), sym (per gt))."""
    names = list(synset_names)
    out = []
    for f, r in enumerate(final_results):
        g_cls, p_cls = np.asarray(r["gt_class_ids"]).astype(np.int64), np.asarray(r["pred_class_ids"]).astype(np.int64)
        for c in range(1, len(names)):
            gi, pi = np.flatnonzero(g_cls == c), np.flatnonzero(p_cls == c)
            if len(gi) == 0 and len(pi) == 0:
                continue
            pi = pi[np.argsort(-np.asarray(r["pred_scores"], np.float64)[pi], kind="stable")]
            hv = np.asarray(r["gt_handle_visibility"])[gi] if len(gi) else np.zeros(0)
            sym = np.full(len(gi), names[c] in SYMMETRIC) | ((names[c] == "mug") & (hv == 0))
            out.append(dict(frame=f, cls=c, pred=pi, gt=gi, sym=sym))
    return out


def all_pair_values(final_results, groups):
    """The pair values of every group in one batch: fills g['iou'] (np, ng) float32 and g['deg_cm'] (np, ng, 2)."""
    a, b, sa, sb, sy = [], [], [], [], []
    for g in groups:
        r = final_results[g["frame"]]
        if len(g["pred"]) and len(g["gt"]):
            ii, jj = np.repeat(g["pred"], len(g["gt"])), np.tile(g["gt"], len(g["pred"]))
            a.append(np.asarray(r["pred_RTs"], np.float64)[ii]); sa.append(np.asarray(r["pred_scales"], np.float64)[ii])
            b.append(np.asarray(r["gt_RTs"], np.float64)[jj]); sb.append(np.asarray(r["gt_scales"], np.float64)[jj])
            sy.append(np.tile(g["sym"], len(g["pred"])))
    if a:
        iou, dc = pair_values(np.concatenate(a), np.concatenate(sa), np.concatenate(b), np.concatenate(sb), np.concatenate(sy))
    k = 0
    for g in groups:
        n_p, n_g = len(g["pred"]), len(g["gt"])
        g["iou"], g["deg_cm"] = np.zeros((n_p, n_g), np.float32), np.zeros((n_p, n_g, 2))
        if n_p and n_g:
            g["iou"], g["deg_cm"] = iou[k:k + n_p * n_g].reshape(n_p, n_g), dc[k:k + n_p * n_g].reshape(n_p, n_g, 2)
            k += n_p * n_g


def normalised_results(final_results):
    """The scale-normalised copy evaluate.py:214-227 evaluates a second time (rows 0..2 of both poses over cbrt(det R)), in float64."""
    out = []
    for r in final_results:
        r = dict(r)
        for k in ("gt_RTs", "pred_RTs"):
            rt = np.array(r[k], np.float64).reshape(-1, 4, 4)
            if len(rt):
                rt[:, :3, :] = rt[:, :3, :] / np.cbrt(np.linalg.det(rt[:, :3, :3]))[:, None, None]
            r[k] = rt
        out.append(r)
    return out


def compute_degree_cm_mAP(final_results, synset_names, degree_thresholds=(360,), shift_thresholds=(100,), iou_3d_thresholds=(0.1,),
                          iou_pose_thres=0.1, use_matches_for_pose=False, details=False):
    """-> (iou_3d_aps, pose_aps[, groups]) as the reference returns them; `groups` carry the pair values and the match flags."""
    names = list(synset_names)
    deg, shift, iou_thr = list(degree_thresholds) + [360], list(shift_thresholds) + [100000], list(iou_3d_thresholds)
    gate = iou_thr.index(iou_pose_thres) if use_matches_for_pose else None
    groups = groups_of(final_results, names)
    all_pair_values(final_results, groups)
    n_cls = len(names)
    per = {c: dict(score=[], iou=[], pose=[], enters=[], n_gt=0) for c in range(1, n_cls)}
    for g in groups:
        g["iou_pred"], g["iou_gt"] = match_iou(g["iou"], iou_thr)
        enters = g["iou_pred"][gate] if gate is not None else np.ones(len(g["pred"]), bool)
        g["pose_pred"], g["pose_gt"] = match_pose(g["deg_cm"], enters, deg, shift)
        p = per[g["cls"]]
        p["score"].append(np.asarray(final_results[g["frame"]]["pred_scores"], np.float64)[g["pred"]])
        p["iou"].append(g["iou_pred"]); p["pose"].append(g["pose_pred"]); p["enters"].append(enters)
        p["n_gt"] += len(g["gt"])
    iou_aps, pose_aps = np.zeros((n_cls + 1, len(iou_thr))), np.zeros((n_cls + 1, len(deg), len(shift)))
    for c, p in per.items():
        score = np.concatenate(p["score"]) if p["score"] else np.zeros(0)
        order = np.argsort(-score, kind="stable")
        fi = np.concatenate(p["iou"], -1)[:, order] if p["iou"] else np.zeros((len(iou_thr), 0), bool)
        fp = np.concatenate(p["pose"], -1)[:, :, order] if p["pose"] else np.zeros((len(deg), len(shift), 0), bool)
        keep = np.concatenate(p["enters"])[order] if p["enters"] else np.zeros(0, bool)
        for t in range(len(iou_thr)):
            iou_aps[c, t] = average_precision(fi[t], p["n_gt"])
        for d in range(len(deg)):
            for s in range(len(shift)):
                pose_aps[c, d, s] = average_precision(fp[d, s][keep], p["n_gt"])
    iou_aps[-1] = np.mean(iou_aps[1:-1], axis=0)
    for d in range(len(deg)):
        for s in range(len(shift)):
            pose_aps[-1, d, s] = np.mean(pose_aps[1:-1, d, s])
    return (iou_aps, pose_aps, groups) if details else (iou_aps, pose_aps)


def indecisive(iou, deg_cm, iou_thr, deg_thr, shift_thr):
    """One (frame, class), pair values iou (np, ng), deg_cm (np, ng, 2) -> the reason why two implementations that differ by the per-pair
    bounds might DECIDE differently here, or None: a value within its bound of a threshold it is compared with, two ground truths of one
    prediction tied within the bound (in IoU, or in degree + cm), an arccos argument within the bound of +-1, a NaN.  An IoU of exactly
    0.0 (disjoint boxes: the same bits on both sides) is no violation, against a threshold or against another 0.0."""
    iou, deg_cm = np.asarray(iou, np.float64), np.asarray(deg_cm, np.float64)
    if iou.size == 0:
        return None
    if np.isnan(iou).any() or np.isnan(deg_cm).any():
        return "nan"
    nz = iou != 0
    if (nz[..., None] & (np.abs(iou[..., None] - np.asarray(iou_thr, np.float64)) < B_IOU)).any():
        return "iou at a threshold"
    if (np.abs(deg_cm[..., 0, None] - np.asarray(list(deg_thr) + [360], np.float64)) < B_DEG).any():
        return "degree at a threshold"
    if (np.abs(deg_cm[..., 1, None] - np.asarray(list(shift_thr) + [100000], np.float64)) < B_CM).any():
        return "cm at a threshold"
    if ((deg_cm[..., 0] < B_END) | (deg_cm[..., 0] > 180 - B_END)).any():
        return "arccos argument at +-1"
    if iou.shape[1] > 1:
        a, b = np.triu_indices(iou.shape[1], 1)
        if ((np.abs(iou[:, a] - iou[:, b]) < B_IOU) & (nz[:, a] | nz[:, b])).any():
            return "iou tie"
        s = deg_cm.sum(-1)
        if (np.abs(s[:, a] - s[:, b]) < B_DEG + B_CM).any():
            return "degree + cm tie"
    return None


def np_sum_order(a):
    """The order np.sum adds a 1-D float64 array in, spelt out -- the model of the summation in csrc/evalmap.hip, checked against np.sum
    itself in tests/test_evalmap_cpu.py: pieces of 8192 (the ufunc buffer size) added in turn, each piece pairwise."""
    res = _pairwise(a[:8192])
    for i in range(8192, len(a), 8192):
        res += _pairwise(a[i:i + 8192])
    return res


def _pairwise(a):
    """numpy's pairwise sum: 8 accumulators per block of at most 128, halves (the first a multiple of 8 long) above that."""
    n = len(a)
    if n < 8:
        res = 0.0
        for x in a:
            res += x
        return res
    if n <= 128:
        r = [float(x) for x in a[:8]]
        i = 8
        while i < n - n % 8:
            for k in range(8):
                r[k] += a[i + k]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res += a[i]
            i += 1
        return res
    h = n // 2
    h -= h % 8
    return _pairwise(a[:h]) + _pairwise(a[h:])


# ------------------------------------------------------------------------------------------ fixtures
def load_golden(name):
    """tests/golden/evalmap_<name>.npz -> (final_results as the reference takes them, the recorded arrays, the manifest entry, the manifest)."""
    import json
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    manifest = json.load(open(os.path.join(gold, "evalmap_manifest.json")))
    z = dict(np.load(os.path.join(gold, f"evalmap_{name}.npz")))
    frames, p, g = [], 0, 0
    for n_p, n_g in zip(z["frame_npred"], z["frame_ngt"]):
        frames.append(dict(gt_class_ids=z["gt_class_ids"][g:g + n_g], gt_RTs=z["gt_RTs"][g:g + n_g], gt_scales=z["gt_scales"][g:g + n_g],
                           gt_handle_visibility=z["gt_handle_visibility"][g:g + n_g], pred_bboxes=z["pred_bboxes"][p:p + n_p],
                           pred_class_ids=z["pred_class_ids"][p:p + n_p], pred_scales=z["pred_scales"][p:p + n_p],
                           pred_scores=z["pred_scores"][p:p + n_p], pred_RTs=z["pred_RTs"][p:p + n_p]))
        p, g = p + n_p, g + n_g
    return frames, z, manifest["sets"][name], manifest


def golden_match_flags(z, k, cfg, groups, match_frames):
    """Unpack match_flags_<k> (gen_golden_evalmap.py) along `groups` (groups_of order) -> list of (iou_pred, iou_gt, pose_pred, pose_gt) bool arrays
    for the groups of the first `match_frames` frames."""
    flat, at, out = z[f"match_flags_{k}"].astype(bool), 0, []
    T, D, S = len(cfg["iou"]), len(cfg["degree"]) + 1, len(cfg["shift"]) + 1
    for g in groups:
        if g["frame"] >= match_frames:
            break
        n_p, n_g, parts = len(g["pred"]), len(g["gt"]), []
        for shape in ((T, n_p), (T, n_g), (D, S, n_p), (D, S, n_g)):
            n = int(np.prod(shape))
            parts.append(flat[at:at + n].reshape(shape))
            at += n
        out.append(tuple(parts))
    assert at == len(flat)
    return out
