"""Float64 NumPy restatement of the two backward chains of givepose_amd/csrc/lossgrad.hip: the gradient of the reference's total loss
(losses/pose_loss.py:30-196 under autograd) with respect to rot, trans, size and the two coordinate maps, and the backward of the
train-time pose decode (pose_from_predictions_train with allo_to_ego_mat_torch, then rot6d_to_mat_batch, rot_reps.py:34-55).
Scalar operation by operation in the kernels' order; only the order of the P-point sum and of the mask sum differs.  Also the
seeded extras of the fixtures tests/golden/pose_loss_grad_*.npz (scripts/gen_golden_pose_loss_grad.py stores the reference's OUTPUTS
only): the non-uniform gout, the rot6d vectors and upstream gradients of the decode cases, the sampled pixels.

Test helper: the package never imports this file.  The forward restatement (tests/pose_loss_ref.py) is imported, not edited.

Derivative conventions (torch's): d|x| = sign(x), sign(0) = 0; SmoothL1(beta)' = x / beta where |x| < beta, else sign; clamp
passes the gradient on the closed interval; the norm of a zero vector has gradient 0.

`mutate` switches ONE deliberate mistake on (tests/test_pose_loss_grad_cpu.py shows that the fixtures reject each of them).
"""
import json
import os

import numpy as np

import pose_loss_ref as R

GRAD_KEYS = ("rot", "trans", "size", "nocs_coor", "ivfc_coor")
DECODE_KEYS = ("rot_allo", "pred_t", "rot6d")
MUTATIONS = ("mask_once", "sign0_one", "no_eps", "div3", "clip_pass", "huber_swap", "pm_to_trans")
GOUT_SEED, DECODE_SEED, SAMPLE_SEED, SAMPLE = 0x6007, 0xD6, 0x5A3, 256
H = R.HUBER
# The bounds of the float64 comparisons, |difference| / max|reference| over one tensor (tests/test_pose_loss_grad_cpu.py derives them)
U = 2.0 ** -53
F64_BOUND = (4096 + 24) * U                     # 24 roundings per element and one long sum (4096 mask values) in another order
DECODE_BOUND = 200 * U                          # the decode chain: at most 200 roundings ...
DECODE_COND_OFF, DECODE_COND_ON = 20.0, 1e4     # ... times its conditioning: 1 / sin(0.05 rad) off the optical axis, 1 / eps on it
F32_BOUND = 8 * 2.0 ** -24 / 0.03 + 8 * 2.0 ** -24


def make_gout():
    """Six seeded upstream weights, one of them 0 (Size)."""
    r = np.random.Generator(np.random.Philox(key=[GOUT_SEED, 6]))
    g = r.uniform(0.25, 2.0, 6) * np.where(r.random(6) < 0.5, -1.0, 1.0)
    g[2] = 0.0
    return g


def make_decode_grad_inputs(B=4):
    """rot6d (B,6) float32 and the upstream gradients g_rot_ego (B,3,3), g_trans (B,3) float32 of the decode cases."""
    r = np.random.Generator(np.random.Philox(key=[DECODE_SEED, B]))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"rot6d": f(r.standard_normal((B, 6))), "g_rot_ego": f(r.standard_normal((B, 3, 3))), "g_trans": f(r.standard_normal((B, 3)))}


def sample_pixels(name, B):
    """(B, SAMPLE) flat pixel indices of the stored map-gradient sample, seeded by the case's own seed."""
    r = np.random.Generator(np.random.Philox(key=[SAMPLE_SEED, R.CASES[name]["seed"]]))
    return np.stack([np.sort(r.choice(64 * 64, SAMPLE, replace=False)) for _ in range(B)])


def pose_loss_grad_ref(pred, data, gout=None, mutate=None, **cfg):
    """-> dict of the five float64 gradients of sum_k gout[k] * term_k (GRAD_KEYS), plus `forward` (pose_loss_ref's dict)."""
    assert mutate is None or mutate in MUTATIONS
    cfg = {**R.DEFAULTS, **cfg}
    fwd = R.pose_loss_ref(pred, data, **cfg)
    w = np.ones(6) if gout is None else np.asarray(gout, np.float64)
    d = lambda a: np.asarray(a, np.float32).astype(np.float64)
    rot, gt_rot, Rc = d(pred["rot"]), d(data["rotation"]), fwd["closest"]
    B = rot.shape[0]
    n = float(B)
    sym1 = np.asarray(data["sym_info"])[:, 0] == 1
    r_sym, branch = "sym" in cfg["r_type"], fwd["branch"]
    smooth = cfg["pose_loss_type"] == "smoothl1"
    sign = (lambda x: np.where(x >= 0, 1.0, -1.0)) if mutate == "sign0_one" else np.sign
    term_d = (lambda x: np.where(np.abs(x) < 0.5, x / 0.5, sign(x))) if smooth else sign
    rs = np.empty((B, 3, 3))
    for i in range(3):
        for j in range(3):
            rs[:, i, j] = (Rc[:, 0, i] * gt_rot[:, 0, j] + Rc[:, 1, i] * gt_rot[:, 1, j]) + Rc[:, 2, i] * gt_rot[:, 2, j]

    def coor(p, g, m, wk):
        p, g, m = d(p), d(g), d(m)
        if branch:
            g = np.stack([(rs[:, c, 0, None, None] * g[:, 0] + rs[:, c, 1, None, None] * g[:, 1]) + rs[:, c, 2, None, None] * g[:, 2]
                          for c in range(3)], 1)
        den = m.reshape(B, -1).sum(1)
        if mutate == "div3":
            den = 3.0 * den
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = ((wk * cfg["coor_w"]) / n) / (den + (0.0 if mutate == "no_eps" else 1e-5))
            x = p * m - g * m
            dd = np.abs(x)
            dl = np.where(dd >= H, 1.0, dd / (2.0 * H)) if mutate == "huber_swap" else np.where(dd > H, 1.0, (2.0 * dd) / (2.0 * H))
            out = (scale[:, None, None, None] * m) * (dl * np.sign(x))
            return out if mutate == "mask_once" else out * m

    zero = r_sym & sym1
    pts = d(data["model_point"]).copy()
    pts[zero, :, 0] = 0
    pts[zero, :, 2] = 0
    P = pts.shape[1]
    xyz = (pts[..., 0], pts[..., 1], pts[..., 2])
    pm, pm_t = np.zeros((B, 3, 3)), np.zeros((B, 3))
    for c in range(3):
        pp = (rot[:, c, 0, None] * xyz[0] + rot[:, c, 1, None] * xyz[1]) + rot[:, c, 2, None] * xyz[2]
        gp = (Rc[:, c, 0, None] * xyz[0] + Rc[:, c, 1, None] * xyz[1]) + Rc[:, c, 2, None] * xyz[2]
        t = term_d(pp - gp)
        pm_t[:, c] = t.sum(1)
        for j in range(3):
            pm[:, c, j] = (t * xyz[j]).sum(1)
    k_pm = (w[3] * cfg["prop_pm_w"]) / ((3.0 * n) * float(P))
    if cfg["r_loss"] == "angle":
        u = (R._trace_abt(Rc, rot) - 1.0) / 2.0
        c = np.minimum(0.99999, np.maximum(-0.99999, u))
        passed = np.ones(B) if mutate == "clip_pass" else ((u >= -0.99999) & (u <= 0.99999)).astype(np.float64)
        ang = np.arccos(c)
        ds = np.where(ang < 0.2, ang / 0.2, np.sign(ang))
        k = (((((w[0] * cfg["rot_1_w"]) / n) * ds) * (-1.0 / np.sqrt(1.0 - c * c))) * passed) * 0.5
        g_rot = k[:, None, None] * Rc + k_pm * pm
    else:
        k = (w[0] * cfg["rot_1_w"]) / (9.0 * n)
        mk = np.ones((B, 3, 3))
        mk[zero, :, 0] = 0
        mk[zero, :, 2] = 0
        x = rot * mk - Rc * mk if r_sym else rot - Rc
        g_rot = (k * term_d(x)) * mk + k_pm * pm
    sc = d(data["nocs_scale"])[:, None]
    k_t, k_s = (w[1] * cfg["tran_w"]) / (3.0 * n), (w[2] * cfg["size_w"]) / (3.0 * n)
    g_trans = k_t * term_d(d(pred["trans"]) - d(data["translation"]) / sc)
    if mutate == "pm_to_trans":
        g_trans = g_trans + k_pm * pm_t
    g_size = k_s * term_d(d(pred["size"]) - d(data["real_size"]) / sc)
    return {"rot": g_rot, "trans": g_trans, "size": g_size,
            "nocs_coor": coor(pred["nocs_coor"], data["nocs_coord"], data["roi_mask_output"], w[4]),
            "ivfc_coor": coor(pred["ivfc_coor"], data["ivfc_coord"], data["roi_ivfc_mask_output"], w[5]), "forward": fwd}


# ------------------------------------------------------------------------------------------------ the decode
def rot6d_to_mat_ref(d6):
    """rot6d_to_mat_batch (rot_reps.py:34-55), float64 from float32."""
    d6 = np.asarray(d6, np.float32).astype(np.float64)
    xr, yr = d6[:, :3], d6[:, 3:]
    x = xr / np.maximum(np.sqrt((xr[:, 0] * xr[:, 0] + xr[:, 1] * xr[:, 1]) + xr[:, 2] * xr[:, 2]), 1e-12)[:, None]
    zr = _cross(x, yr)
    z = zr / np.maximum(np.sqrt((zr[:, 0] * zr[:, 0] + zr[:, 1] * zr[:, 1]) + zr[:, 2] * zr[:, 2]), 1e-12)[:, None]
    return np.stack([x, _cross(z, x), z], -1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _div_norm_bwd(u, gv, nrm, den):
    """v = u / den, den = |u| + eps or max(|u|, eps): -> gu; the norm's own gradient is 0 where nrm is 0."""
    gden = -(((gv[:, 0] * u[:, 0] + gv[:, 1] * u[:, 1]) + gv[:, 2] * u[:, 2]) / (den * den))
    safe = np.where(nrm > 0.0, nrm, 1.0)
    return gv / den[:, None] + np.where(nrm > 0.0, gden, 0.0)[:, None] * (u / safe[:, None])


def decode_train_backward_ref(g_rot_ego, g_trans, pred_t, rot_allo, cam_K, bbox_center, resize_ratio, roi_wh, rot6d=None, t_site=True,
                              is_allo=True, eps=1e-4):
    """-> dict rot_allo (B,3,3), pred_t (B,3), rot6d (B,6) (zeros without rot6d), float64.  With rot6d, rot_allo's values are not read."""
    d = lambda a: np.asarray(a, np.float32).astype(np.float64)
    gE, gt = d(g_rot_ego), d(g_trans).copy()
    pt, Ra, K, ce, ra, wh = d(pred_t), d(rot_allo), d(cam_K), d(bbox_center), d(resize_ratio).reshape(-1), d(roi_wh)
    B = pt.shape[0]
    if rot6d is not None:            # the chain starts from the raw vector in float64; rot_allo's float32 rounding stays out
        Ra = rot6d_to_mat_ref(rot6d)
    o = pt[:, :2] if t_site else pt[:, :2] * 0.0
    cx, cy = o[:, 0] * wh[:, 0] + ce[:, 0], o[:, 1] * wh[:, 1] + ce[:, 1]
    z = pt[:, 2] * ra
    fx, fy = K[:, 0, 0], K[:, 1, 1]
    ux, uy = cx - K[:, 0, 2], cy - K[:, 1, 2]
    t = np.stack([z * ux / fx, z * uy / fy, z], 1)
    gR = gE.copy()
    if is_allo:
        tn = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
        n = tn + eps
        r = t / n[:, None]
        angle = np.arccos(r[:, 2])
        ar = np.stack([0.0 * r[:, 2] - r[:, 1], r[:, 0] - 0.0 * r[:, 2], 0.0 * r[:, 1] - 0.0 * r[:, 0]], 1)
        arn = np.sqrt((ar[:, 0] * ar[:, 0] + ar[:, 1] * ar[:, 1]) + ar[:, 2] * ar[:, 2])
        an = arn + eps
        ax = ar / an[:, None]
        h = angle / 2.0
        sh, ch = np.sin(h), np.cos(h)
        u = np.stack([ch, ax[:, 0] * sh, ax[:, 1] * sh, ax[:, 2] * sh], 1)
        qn = np.sqrt(((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]) + u[:, 3] * u[:, 3])
        qw, qx, qy, qz = (u / qn[:, None]).T
        X, Y, Z = qx * 2.0, qy * 2.0, qz * 2.0
        wX, wY, wZ, xX, xY, xZ, yY, yZ, zZ = qw * X, qw * Y, qw * Z, qx * X, qx * Y, qx * Z, qy * Y, qy * Z, qz * Z
        M = np.stack([1.0 - (yY + zZ), xY - wZ, xZ + wY, xY + wZ, 1.0 - (xX + zZ), yZ - wX, xZ - wY, yZ + wX, 1.0 - (xX + yY)], 1).reshape(-1, 3, 3)
        gM = np.empty((B, 3, 3))
        for i in range(3):
            for k in range(3):
                gM[:, i, k] = (gE[:, i, 0] * Ra[:, k, 0] + gE[:, i, 1] * Ra[:, k, 1]) + gE[:, i, 2] * Ra[:, k, 2]
                gR[:, i, k] = (M[:, 0, i] * gE[:, 0, k] + M[:, 1, i] * gE[:, 1, k]) + M[:, 2, i] * gE[:, 2, k]
        m = gM.reshape(B, 9).T
        g_yY, g_zZ, g_xX = -m[0] - m[8], -m[0] - m[4], -m[4] - m[8]
        g_xY, g_wZ, g_xZ, g_wY, g_yZ, g_wX = m[1] + m[3], m[3] - m[1], m[2] + m[6], m[2] - m[6], m[5] + m[7], m[7] - m[5]
        g_X = g_wX * qw + g_xX * qx
        g_Y = (g_wY * qw + g_xY * qx) + g_yY * qy
        g_Z = ((g_wZ * qw + g_xZ * qx) + g_yZ * qy) + g_zZ * qz
        gq = np.stack([(g_wX * X + g_wY * Y) + g_wZ * Z, ((g_xX * X + g_xY * Y) + g_xZ * Z) + g_X * 2.0, (g_yY * Y + g_yZ * Z) + g_Y * 2.0,
                       g_zZ * Z + g_Z * 2.0], 1)
        gqn = -((((gq[:, 0] * u[:, 0] + gq[:, 1] * u[:, 1]) + gq[:, 2] * u[:, 2]) + gq[:, 3] * u[:, 3]) / (qn * qn))
        gu = gq / qn[:, None] + gqn[:, None] * (u / qn[:, None])
        g_h = ((gu[:, 1] * ax[:, 0] + gu[:, 2] * ax[:, 1]) + gu[:, 3] * ax[:, 2]) * ch - gu[:, 0] * sh
        g_angle = g_h / 2.0
        gax = gu[:, 1:] * sh[:, None]
        gar = _div_norm_bwd(ar, gax, arn, an)
        gr = np.stack([gar[:, 1], -gar[:, 0], g_angle * (-1.0 / np.sqrt(1.0 - r[:, 2] * r[:, 2]))], 1)
        gt = gt + _div_norm_bwd(t, gr, tn, n)
    g_z = (gt[:, 0] * ux / fx + gt[:, 1] * uy / fy) + gt[:, 2]
    g_cx, g_cy = gt[:, 0] * z / fx, gt[:, 1] * z / fy
    g_pt = np.stack([g_cx * wh[:, 0] if t_site else (g_cx * wh[:, 0]) * 0.0, g_cy * wh[:, 1] if t_site else (g_cy * wh[:, 1]) * 0.0, g_z * ra], 1)
    g6 = np.zeros((B, 6))
    if rot6d is not None:
        d6 = d(rot6d)
        xr, yr = d6[:, :3], d6[:, 3:]
        xn = np.sqrt((xr[:, 0] * xr[:, 0] + xr[:, 1] * xr[:, 1]) + xr[:, 2] * xr[:, 2])
        xd = np.maximum(xn, 1e-12)
        x = xr / xd[:, None]
        zr = _cross(x, yr)
        zn = np.sqrt((zr[:, 0] * zr[:, 0] + zr[:, 1] * zr[:, 1]) + zr[:, 2] * zr[:, 2])
        zd = np.maximum(zn, 1e-12)
        zz = zr / zd[:, None]
        gx, gy, gz = gR[:, :, 0], gR[:, :, 1], gR[:, :, 2]
        gz = gz + _cross(x, gy)
        gx = gx + _cross(gy, zz)
        gzr = _div_norm_bwd(zr, gz, np.where(zn >= 1e-12, zn, 0.0), zd)
        gx = gx + _cross(yr, gzr)
        g6 = np.concatenate([_div_norm_bwd(xr, gx, np.where(xn >= 1e-12, xn, 0.0), xd), _cross(gzr, x)], 1)
    return {"rot_allo": gR, "pred_t": g_pt, "rot6d": g6}


# ------------------------------------------------------------------------------------------------ fixtures
def load_grad_fixture(name):
    """-> (pred, data, cfg, fixture arrays); the regenerated inputs and extras are checked against the recorded CRCs."""
    z = np.load(os.path.join(R.GOLDEN, f"pose_loss_grad_{name}.npz"))
    pred, data = R.case_inputs(name)
    assert R.crc_of({**pred, **data}) == int(z["input_crc"]), f"inputs of fixture {name} do not regenerate"
    assert R.crc_of({"gout": make_gout(), "pix": sample_pixels(name, pred["rot"].shape[0])}) == int(z["extra_crc"])
    return pred, data, R.case_cfg(name), z


def load_decode_grad_fixture():
    z = np.load(os.path.join(R.GOLDEN, "pose_loss_grad_decode.npz"))
    inp, extra = R.make_decode_inputs(), make_decode_grad_inputs()
    assert R.crc_of(inp) == int(z["input_crc"]) and R.crc_of(extra) == int(z["extra_crc"])
    return inp, extra, z


def sampled(g, pix):
    """(B,3,64,64) map gradient -> its values at the sampled pixels (B,3,SAMPLE), and the per-(crop, channel) sum and sum of |.|."""
    B = g.shape[0]
    flat = np.asarray(g).reshape(B, 3, -1)
    return np.take_along_axis(flat, pix[:, None, :].repeat(3, 1), 2), flat.sum(2), np.abs(flat).sum(2)


def manifest():
    with open(os.path.join(R.GOLDEN, "pose_loss_grad_manifest.json")) as f:
        return json.load(f)
