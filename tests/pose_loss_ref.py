"""Float64 NumPy restatement of the reference's PoseLoss.forward (losses/pose_loss.py:30-196, the closest-symmetric-rotation
search of :329-353, :401-428, :451-466) and of its train-time pose decode (pose_from_predictions_train,
network/pose_utils/pose_from_pred_centroid_z.py:160-249 with allo_to_ego_mat_torch, network/pose_utils/utils.py:198-229), plus the
seeded inputs of the fixtures tests/golden/pose_loss_*.npz (scripts/gen_golden_pose_loss.py stores the reference's OUTPUTS only; the
inputs are regenerated here and checked against a CRC).

Test helper: the package never imports this file.

Everything is float64 computed from the float32 inputs.  The one float32 rounding inside is the reference's own: the winning
gt_rot . S_k goes through torch.tensor(..., dtype=float32) (pose_loss.py:427).  The scalar arithmetic is written operation by
operation (no np.dot, no BLAS) in the order givepose_amd/csrc/loss.hip uses, so the device reproduces every element and differs
only in the order of the long sums.
"""
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("Rot1", "Tran", "Size", "Point_matching", "nocs_coor", "sp2d_coor")
DEFAULTS = dict(pose_loss_type="l1", r_loss="l1", r_type="allo_rot6d", coor_gt_sym="rot", rot_1_w=1.0, tran_w=1.0, size_w=1.0,
                prop_pm_w=1.0, coor_w=0.1)
SYM_ROWS = ([1, 1, 0, 1], [0, 0, 0, 0], [1, 1, 1, 1], [0, 1, 0, 0], [1, 0, 0, 0])
HUBER = 0.03
REAL_K = np.array([[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]], np.float32)

# name -> B, P, seed, sym rows ("cycle" / "none" / "all"), mask kinds per crop (cycled), crop with pred == gt (or None), flags
CASES = {
    "b1": dict(B=1, P=1, seed=1, sym="cycle", masks=("binary",), equal=None, cfg={}),
    "b3": dict(B=3, P=1000, seed=2, sym="cycle", masks=("binary", "zero", "one"), equal=None, cfg={}),
    "b5": dict(B=5, P=1024, seed=3, sym="cycle", masks=("full", "soft", "binary", "zero", "one"), equal=2, cfg={}),
    "nosym": dict(B=3, P=1000, seed=4, sym="none", masks=("binary", "soft", "full"), equal=None, cfg={}),
    "allsym": dict(B=3, P=1, seed=5, sym="all", masks=("soft", "binary", "one"), equal=1, cfg={}),
    "angle": dict(B=3, P=1024, seed=6, sym="cycle", masks=("binary", "soft", "full"), equal=1, cfg=dict(r_loss="angle")),
    "smoothl1": dict(B=3, P=1000, seed=7, sym="cycle", masks=("binary", "full", "soft"), equal=None, cfg=dict(pose_loss_type="smoothl1")),
    "symtype": dict(B=5, P=1000, seed=8, sym="cycle", masks=("binary", "soft", "full", "one", "zero"), equal=None,
                    cfg=dict(r_type="allo_rot6d_sym")),
}
# the decode fixtures: r_type (allo / ego), t_type; crop 0 of each sits exactly on the optical axis
DECODE_CASES = {"allo_site": ("allo_rot6d", "site"), "allo_center": ("allo_rot6d", "center"), "ego_site": ("ego_rot6d", "site"),
                "ego_center": ("ego_rot6d", "center")}


def crc_of(arrays):
    c = 0
    for k in sorted(arrays):
        c = zlib.crc32(np.ascontiguousarray(arrays[k]).tobytes(), c)
    return int(c)


def _rotations(r, n):
    q = r.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def _mask(r, kind):
    if kind == "binary":
        return (r.random((1, 64, 64)) > 0.5).astype(np.float32)
    if kind == "soft":
        return r.random((1, 64, 64)).astype(np.float32)            # masks are float and need not be binary
    m = np.full((1, 64, 64), 1.0 if kind == "full" else 0.0, np.float32)
    if kind == "one":
        m[0, 37, 21] = 1.0
    return m


def make_inputs(B, P, seed, sym="cycle", masks=("binary",), equal=None, **_):
    """(pred_dict, data) of float32 / int64 NumPy arrays with the keys PoseLoss.forward reads."""
    r = np.random.Generator(np.random.Philox(key=[seed, 0x105E]))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    gt_rot = f(_rotations(r, B))
    rot = f(_rotations(r, B) + 0.02 * r.standard_normal((B, 3, 3)))      # a network's output is not exactly orthonormal
    if equal is not None:
        rot[equal] = gt_rot[equal]
    scale = f(r.uniform(0.2, 0.6, B))
    gt_trans = f(r.normal(0, 0.2, (B, 3)) + [0, 0, 1.0])
    trans = f(gt_trans / scale[:, None] + r.normal(0, 0.3, (B, 3)))
    gt_size = f(r.uniform(0.05, 0.4, (B, 3)))
    size = f(gt_size / scale[:, None] + r.normal(0, 0.3, (B, 3)))
    maps = {}
    for k in ("nocs", "ivfc"):
        gt = r.uniform(-0.5, 0.5, (B, 3, 64, 64))
        noise = r.normal(0, 1, (B, 3, 64, 64)) * np.where(r.random((B, 3, 64, 64)) < 0.5, 0.01, 0.08)    # both Huber branches
        maps[k] = (f(gt + noise), f(gt))
    kinds = [masks[i % len(masks)] for i in range(B)]
    gm, gms = f(np.stack([_mask(r, k) for k in kinds])), f(np.stack([_mask(r, k) for k in kinds]))
    rows = {"cycle": [SYM_ROWS[i % 5] for i in range(B)], "none": [[0, 1, 0, 0]] * B, "all": [[1, 1, 0, 1]] * B}[sym]
    pred = {"rot": rot, "trans": trans, "size": size, "nocs_coor": maps["nocs"][0], "ivfc_coor": maps["ivfc"][0]}
    data = {"rotation": gt_rot, "translation": gt_trans, "real_size": gt_size, "roi_mask_output": gm, "roi_ivfc_mask_output": gms,
            "sym_info": np.array(rows, np.int64), "nocs_scale": scale, "nocs_coord": maps["nocs"][1], "ivfc_coord": maps["ivfc"][1],
            "model_point": f(r.uniform(-0.3, 0.3, (B, P, 3)))}
    return pred, data


def case_inputs(name):
    return make_inputs(**CASES[name])


def case_cfg(name):
    return {**DEFAULTS, **CASES[name]["cfg"]}


def make_decode_inputs(seed=21, B=4):
    r = np.random.Generator(np.random.Philox(key=[seed, 0xDEC0]))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    K = np.broadcast_to(REAL_K, (B, 3, 3)).copy()
    off = r.uniform(60, 200, (B, 2)) * np.where(r.random((B, 2)) < 0.5, -1, 1)
    center = f(K[:, :2, 2] + off)
    wh = f(r.uniform(40, 200, (B, 2)))
    pred_t = f(np.concatenate([r.normal(0, 0.05, (B, 2)), 1.0 + 0.3 * r.random((B, 1))], 1))
    center[0] = K[0, :2, 2]         # crop 0: exactly on the optical axis for both t_types (tx = ty = 0; only eps shapes the result)
    pred_t[0, :2] = 0
    return {"pred_t": pred_t, "rot_allo": f(_rotations(r, B) + 0.01 * r.standard_normal((B, 3, 3))), "cam_K": f(K), "bbox_center": center,
            "resize_ratio": f(64.0 / (1.5 * wh.max(1))), "roi_wh": wh}


# ------------------------------------------------------------------------------------------------ the restatement
def sym_table():
    """cos / sin of symmetry_rotation_matrix_y(360) (pose_loss.py:319-326), the reference's expression for theta."""
    th = np.array([2 * np.pi / 360 * i for i in range(360)])
    return np.stack([np.cos(th), np.sin(th)], 1)


def _trace_abt(A, B):
    """sum_ij A_ij B_ij, row by row (A, B: (..., 3, 3) float64)."""
    a, b = A.reshape(A.shape[:-2] + (9,)), B.reshape(B.shape[:-2] + (9,))
    t = a[..., 0] * b[..., 0]
    for i in range(1, 9):
        t = t + a[..., i] * b[..., i]
    return t


def re_deg(A, B):
    t = np.minimum(_trace_abt(A, B), 3.0)
    return np.arccos(np.minimum(1.0, np.maximum(-1.0, 0.5 * (t - 1.0)))) * (180.0 / np.pi)


def _times_sym_y(G, c, s):
    """G (3,3) . S_k for arrays c, s (K,) -> (K,3,3)."""
    o = np.empty((len(c), 3, 3))
    for i in range(3):
        o[:, i, 0] = G[i, 0] * c - G[i, 2] * s
        o[:, i, 1] = G[i, 1]
        o[:, i, 2] = G[i, 0] * s + G[i, 2] * c
    return o


def _smooth_l1(a, b, beta):
    d = np.abs(a - b)
    return np.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)


def candidates_re(rot, gt_rot):
    """re of the 360 candidates of one crop (float64)."""
    tab = sym_table()
    return re_deg(np.float64(rot)[None], _times_sym_y(np.float64(gt_rot), tab[:, 0], tab[:, 1]))


def pose_loss_ref(pred, data, pose_loss_type="l1", r_loss="l1", r_type="allo_rot6d", coor_gt_sym="rot", rot_1_w=1.0, tran_w=1.0,
                  size_w=1.0, prop_pm_w=1.0, coor_w=0.1):
    """-> dict: `terms` (6,) float64 in KEYS order, per crop `index`, `re_best`, `re`, `te`, `closest` (B,3,3), `gap` (best against
    second-best candidate re, inf for a crop that is not searched), `branch`, `mean_re`, `mean_te`."""
    assert coor_gt_sym == "rot"
    d = lambda a: np.asarray(a, np.float32).astype(np.float64)
    rot, gt_rot = d(pred["rot"]), d(data["rotation"])
    B = rot.shape[0]
    sym1 = np.asarray(data["sym_info"])[:, 0] == 1
    r_sym = "sym" in r_type
    branch = bool(sym1.any()) and not r_sym
    term = (lambda a, b: np.abs(a - b)) if pose_loss_type == "l1" else (lambda a, b: _smooth_l1(a, b, 0.5))
    tab = sym_table()
    closest, index, re_best, gap = gt_rot.copy(), np.full(B, -1), np.zeros(B), np.full(B, np.inf)
    re0 = re_deg(rot, gt_rot)
    for b in range(B):
        re_best[b] = re0[b]
        if branch and sym1[b]:
            cand = _times_sym_y(gt_rot[b], tab[:, 0], tab[:, 1])
            res = re_deg(rot[b][None], cand)
            k = int(np.argmin(res))                      # the first smallest: a tie keeps the earlier candidate
            gap[b] = np.sort(np.unique(res))[1] - res[k] if len(np.unique(res)) > 1 else 0.0
            if res[k] < re0[b]:                           # strict: a tie keeps the unrotated ground truth
                index[b], re_best[b] = k, res[k]
                closest[b] = cand[k].astype(np.float32).astype(np.float64)
    # rot_sym = closest^T gt_rot, applied to every crop's maps when the branch runs
    rs = np.empty((B, 3, 3))
    for i in range(3):
        for j in range(3):
            rs[:, i, j] = (closest[:, 0, i] * gt_rot[:, 0, j] + closest[:, 1, i] * gt_rot[:, 1, j]) + closest[:, 2, i] * gt_rot[:, 2, j]

    def coor(p, g, m):
        p, g, m = d(p), d(g), d(m)
        if branch:
            g = np.stack([(rs[:, c, 0, None, None] * g[:, 0] + rs[:, c, 1, None, None] * g[:, 1]) + rs[:, c, 2, None, None] * g[:, 2]
                          for c in range(3)], 1)
        diff = np.abs(p * m - g * m)
        l = m * np.where(diff > HUBER, diff - HUBER / 2.0, diff * diff / (2.0 * HUBER))
        return (l.reshape(B, -1).sum(1) / (m.reshape(B, -1).sum(1) + 1e-5)).sum() / B

    zero = r_sym & sym1
    if r_loss == "angle":
        c = np.minimum(0.99999, np.maximum(-0.99999, (_trace_abt(closest, rot) - 1.0) / 2.0))
        rot1 = _smooth_l1(np.arccos(c), 0.0, 0.2).sum() / B
    else:
        mk = np.ones((B, 3, 3))
        mk[zero, :, 0] = 0
        mk[zero, :, 2] = 0
        rot1 = term(rot * mk, closest * mk).sum() / (9.0 * B)
    sc = d(data["nocs_scale"])[:, None]
    gtn = d(data["translation"]) / sc
    tran = term(d(pred["trans"]), gtn).sum() / (3.0 * B)
    size = term(d(pred["size"]), d(data["real_size"]) / sc).sum() / (3.0 * B)
    pts = d(data["model_point"]).copy()                   # the reference zeroes these in the caller's tensor, through a permuted view
    pts[zero, :, 0] = 0
    pts[zero, :, 2] = 0
    P = pts.shape[1]
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    pm = 0.0
    for c in range(3):
        pp = (rot[:, c, 0, None] * x + rot[:, c, 1, None] * y) + rot[:, c, 2, None] * z
        gp = (closest[:, c, 0, None] * x + closest[:, c, 1, None] * y) + closest[:, c, 2, None] * z
        pm = pm + term(pp, gp).sum()
    pm = pm / (3.0 * B * P)
    dt = gtn - d(pred["trans"])
    te = np.sqrt((dt[:, 0] * dt[:, 0] + dt[:, 1] * dt[:, 1]) + dt[:, 2] * dt[:, 2])
    terms = np.array([rot_1_w * rot1, tran_w * tran, size_w * size, prop_pm_w * pm,
                      coor_w * coor(pred["nocs_coor"], data["nocs_coord"], data["roi_mask_output"]),
                      coor_w * coor(pred["ivfc_coor"], data["ivfc_coord"], data["roi_ivfc_mask_output"])])
    return {"terms": terms, "index": index, "re_best": re_best, "re": re0, "te": te, "closest": closest, "gap": gap, "branch": branch,
            "mean_re": re0.sum() / B, "mean_te": te.sum() / B}


def decode_train_ref(pred_t, rot_allo, cam_K, bbox_center, resize_ratio, roi_wh, t_site=True, is_allo=True, eps=1e-4):
    """-> (rot_ego (B,3,3), translation (B,3)) float64."""
    d = lambda a: np.asarray(a, np.float32).astype(np.float64)
    pt, R, K, ce, ra, wh = d(pred_t), d(rot_allo), d(cam_K), d(bbox_center), d(resize_ratio).reshape(-1), d(roi_wh)
    o = pt[:, :2] if t_site else pt[:, :2] * 0.0
    cx, cy = o[:, 0] * wh[:, 0] + ce[:, 0], o[:, 1] * wh[:, 1] + ce[:, 1]
    z = pt[:, 2] * ra
    t = np.stack([z * (cx - K[:, 0, 2]) / K[:, 0, 0], z * (cy - K[:, 1, 2]) / K[:, 1, 1], z], 1)
    if not is_allo:
        return R, t
    n = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]) + eps
    rx, ry, rz = t[:, 0] / n, t[:, 1] / n, t[:, 2] / n
    angle = np.arccos(rz)
    ax, ay, az = 0.0 * rz - ry, rx - 0.0 * rz, 0.0 * ry - 0.0 * rx
    an = np.sqrt((ax * ax + ay * ay) + az * az) + eps
    ax, ay, az = ax / an, ay / an, az / an
    h = angle / 2.0
    sh = np.sin(h)
    qw, qx, qy, qz = np.cos(h), ax * sh, ay * sh, az * sh
    qn = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
    qw, qx, qy, qz = qw / qn, qx / qn, qy / qn, qz / qn
    X, Y, Z = qx * 2.0, qy * 2.0, qz * 2.0
    wX, wY, wZ, xX, xY, xZ, yY, yZ, zZ = qw * X, qw * Y, qw * Z, qx * X, qx * Y, qx * Z, qy * Y, qy * Z, qz * Z
    M = np.stack([1.0 - (yY + zZ), xY - wZ, xZ + wY, xY + wZ, 1.0 - (xX + zZ), yZ - wX, xZ - wY, yZ + wX, 1.0 - (xX + yY)], 1).reshape(-1, 3, 3)
    E = np.empty_like(R)
    for i in range(3):
        for j in range(3):
            E[:, i, j] = (M[:, i, 0] * R[:, 0, j] + M[:, i, 1] * R[:, 1, j]) + M[:, i, 2] * R[:, 2, j]
    return E, t


def off_axis_angle(t):
    return np.arccos(t[:, 2] / np.linalg.norm(t, axis=1))


# ------------------------------------------------------------------------------------------------ fixtures
def load_fixture(name):
    """-> (pred, data, cfg, fixture arrays); the regenerated inputs are checked against the recorded CRC."""
    z = np.load(os.path.join(GOLDEN, f"pose_loss_{name}.npz"))
    pred, data = case_inputs(name)
    assert crc_of({**pred, **data}) == int(z["input_crc"]), f"inputs of fixture {name} do not regenerate"
    return pred, data, case_cfg(name), z


def load_decode_fixture():
    z = np.load(os.path.join(GOLDEN, "pose_loss_decode.npz"))
    inp = make_decode_inputs()
    assert crc_of(inp) == int(z["input_crc"])
    return inp, z


def manifest():
    with open(os.path.join(GOLDEN, "pose_loss_manifest.json")) as f:
        return json.load(f)
