"""NumPy restatement of the reference's pose_from_umeyama (tools/umeyama.py:17-60; tools/align_utils.py:10-104) in this project's
words, with the draw table as an argument, and the bounds the alignment kernels (csrc/align.hip) are held to.

What is compared exactly (DECISIONS): the back-projection (float32, bit for bit), the compaction order, the inlier count of every
iteration the reference ran, the iterations run, the best iteration, the final inlier set, the status.

What is compared within a bound (VALUES): float64 scale, R, t, sRT.  The bounds come from the number formats, not from any
implementation's output.  With u = 2^-53, n the size of the final inlier set, C its covariance (mean of (tgt - mean)(src - mean)^T),
var_s / var_t the mean squared distances of the source / target points from their centroids, sigma_1 >= sigma_2 >= |sigma_3| the
singular values of C, the last signed (negative in the reflection case, det C < 0):

  dC   every entry of C is a sum of n products whose absolute values add up to at most n sqrt(var_s var_t) (Cauchy-Schwarz).  A
       pairwise or tree sum of n terms loses at most ceil(log2 n) u per level relative to that, the centring and the product 3 u more.
       The kernel adds 16 terms per thread in turn, then an 8-level tree (24 levels at most); numpy's mean is pairwise and its matmul
       accumulates in blocks.  Budget for BOTH sides together: K(n) = 8 ceil(log2 n) + 32 roundings, so
           dC = K(n) u sqrt(var_s var_t)   per entry,   3 dC in the Frobenius norm.
  R    the rotation is the polar factor of C restricted to proper rotations.  It moves by at most 2 |dC|_F / (sigma_2 + sigma_3)
       (sigma_3 signed: sigma_2 - |sigma_3| in the reflection case), plus 16 u for forming it from the factors:
           B_R = 2 * 3 dC / (sigma_2 + sigma_3) + 16 u           (per entry, as the Frobenius bound)
  s    sum of the signed singular values = max over proper rotations Q of trace(Q^T C), which is sqrt(3)-Lipschitz in the Frobenius
       norm; var_s is a sum of n non-negative terms (relative K(n) u):
           B_s = s * (sqrt(3) 3 dC / (sigma_1 + sigma_2 + sigma_3) + K(n) u)
  t    t = mean_t - s R mean_s with the centroids good to K(n) u relative:
           B_t = K(n) u (|mean_t| + s |mean_s|) + B_s |mean_s| + s B_R sqrt(3) |mean_s|
  sRT  s R entries: B_s + s B_R; last column: B_t.
The fixtures' final sets have comparable singular values, so B_R comes out at 1e-13 .. 3e-13.

Decisiveness (judged on THIS module's values, never on the kernel's): a crop is decisive when no residual of an evaluated hypothesis
lies within a relative MARGIN_RESIDUAL of its threshold, no early-stop value within MARGIN_STOP of 0.99, and every evaluated sample
has sigma_2 / sigma_1 >= MIN_SAMPLE_RANK and sigma_1 / (sigma_2 + sigma_3) <= MAX_SAMPLE_COND (a sample fit moves by about
u * that factor, 1e-11 relative at the limit: a hundredth of the residual margin).  The generator of the fixtures asserts the same on
the reference's own values.

The documented departure (include/givepose_align.h, GPA_RANK_TOL): a sample whose covariance has sigma_2 <= 1e-12 sigma_1 or no
source variance counts zero inliers; a final set like that fails with DEGENERATE.
"""
import numpy as np

U = 2.0 ** -53
MAX_ITER, SAMPLE, RES = 128, 5, 64
OK, NO_POINTS, LOW_INLIERS, DEGENERATE = 0, 1, 2, 3
RANK_TOL = 1e-12
MARGIN_RESIDUAL, MARGIN_STOP, MIN_SAMPLE_RANK, MAX_SAMPLE_COND = 1e-9, 1e-9, 1e-6, 1e5


def back_project(coor_2d, camK, depth):
    """get_PC_nocs (tools/umeyama.py:53-59): (x_label - ux) * depth / fx in float32, in exactly this order.
    coor_2d (B,2,R,R), camK (B,3,3), depth (B,1,R,R) -> PC (B,R*R,3) float32."""
    f = np.float32
    coor_2d, camK, depth = np.asarray(coor_2d, f), np.asarray(camK, f), np.asarray(depth, f)
    B = coor_2d.shape[0]
    d = depth[:, 0]
    fx, fy, ux, uy = camK[:, 0, 0], camK[:, 1, 1], camK[:, 0, 2], camK[:, 1, 2]
    x = ((coor_2d[:, 0] - ux[:, None, None]).astype(f) * d).astype(f) / fx[:, None, None]
    y = ((coor_2d[:, 1] - uy[:, None, None]).astype(f) * d).astype(f) / fy[:, None, None]
    return np.stack([x.astype(f), y.astype(f), d], -1).reshape(B, -1, 3)


def compact(mask, depth, valid_depth_only=False):
    """Pixels kept, in row-major order (obj_mask.bool() of tools/umeyama.py:45; depth > 0 of align_utils.py:116-117 when asked)."""
    keep = np.asarray(mask).reshape(-1) != 0
    if valid_depth_only:
        keep &= np.asarray(depth, np.float32).reshape(-1) > 0
    return np.nonzero(keep)[0]


def umeyama(src, tgt):
    """estimateSimilarityUmeyama (align_utils.py:10-41) on (n,3) float64 sets -> dict.  `sigma` has the last value signed."""
    n = src.shape[0]
    ms, mt = src.mean(0), tgt.mean(0)
    cs, ct = src - ms, tgt - mt
    C = ct.T @ cs / n
    Uu, D, Vh = np.linalg.svd(C)
    if np.linalg.det(Uu) * np.linalg.det(Vh) < 0:
        D = D.copy()
        D[-1] = -D[-1]
        Uu = Uu.copy()
        Uu[:, -1] = -Uu[:, -1]
    var = (cs ** 2).sum() / n
    ok = bool(np.isfinite(C).all() and D[0] > 0 and D[1] > RANK_TOL * D[0] and var > 0)
    R = Uu @ Vh
    with np.errstate(all="ignore"):
        scale = D.sum() / var
        t = mt - scale * (R @ ms)
    sRT = np.eye(4)
    sRT[:3, :3] = scale * R
    sRT[:3, 3] = t
    return {"scale": scale, "R": R, "t": t, "sRT": sRT, "sigma": D, "ok": ok, "mean_s": ms, "mean_t": mt, "var_s": var,
            "var_t": (ct ** 2).sum() / n, "n": n}


def residuals(fit, src, tgt):
    return np.linalg.norm(tgt - (src @ fit["sRT"][:3, :3].T + fit["t"]), axis=1)


def ransac(src, tgt, draws):
    """estimateSimilarityTransform (align_utils.py:44-104) on (n,3) sets; draws (128,5) uint32, reduced mod n.  Returns the
    decisions, the final fit and the decisiveness margins."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    n = src.shape[0]
    out = {"n_points": n, "counts": [], "iterations_run": 0, "best_iteration": -1, "inlier_idx": np.zeros(0, np.int64),
           "margin_residual": np.inf, "margin_stop": np.inf, "min_sample_rank": np.inf, "max_sample_cond": 0.0, "fit": None}
    if n == 0:
        out["status"] = NO_POINTS
        return out
    inlier_t = 2 * np.linalg.norm(src - src.mean(0), axis=1).max() / 10.0
    best, best_idx = 0, np.zeros(0, np.int64)
    for i in range(MAX_ITER):
        idx = (np.asarray(draws[i], np.uint32) % np.uint32(n)).astype(np.int64)
        f = umeyama(src[idx], tgt[idx])
        s = f["sigma"]
        if f["ok"]:
            out["min_sample_rank"] = min(out["min_sample_rank"], s[1] / s[0])
            out["max_sample_cond"] = max(out["max_sample_cond"], s[0] / (s[1] + s[2]) if s[1] + s[2] > 0 else np.inf)
            thr = f["scale"] * inlier_t
            res = residuals(f, src, tgt)
            if thr > 0:
                out["margin_residual"] = min(out["margin_residual"], np.abs(res / thr - 1).min())
            ins = np.nonzero(res < thr)[0]
        else:
            ins = np.zeros(0, np.int64)              # the departure: a rank-deficient sample counts nothing
        out["counts"].append(len(ins))
        if len(ins) > best:
            best, best_idx = len(ins), ins
            out["best_iteration"] = i
        out["iterations_run"] = i + 1
        stop = 1 - (1 - (best / n) ** 5) ** i
        out["margin_stop"] = min(out["margin_stop"], abs(stop - 0.99))
        if stop > 0.99:
            break
    out["n_inliers"] = best
    out["inlier_idx"] = best_idx
    if best / n < 0.1:
        out["status"] = LOW_INLIERS
        return out
    f = umeyama(src[best_idx], tgt[best_idx])
    out["status"] = OK if f["ok"] else DEGENERATE
    out["fit"] = f
    return out


def decisive(r):
    return (r["margin_residual"] >= MARGIN_RESIDUAL and r["margin_stop"] >= MARGIN_STOP and r["min_sample_rank"] >= MIN_SAMPLE_RANK
            and r["max_sample_cond"] <= MAX_SAMPLE_COND)


def pose_from_umeyama_ref(xyz_coor, coor_2d, camK, Depth, obj_mask, draws, valid_depth_only=False):
    """The whole of tools/umeyama.py:17-37 per crop -> list of ransac() dicts (with `index`: the compacted pixels) and PC."""
    xyz = np.asarray(xyz_coor, np.float32)
    B = xyz.shape[0]
    PC = back_project(coor_2d, camK, Depth)
    nocs = xyz.transpose(0, 2, 3, 1).reshape(B, -1, 3)
    out = []
    for b in range(B):
        idx = compact(np.asarray(obj_mask)[b], np.asarray(Depth)[b], valid_depth_only)
        r = ransac(nocs[b][idx], PC[b][idx], np.asarray(draws)[b])
        r["index"] = idx
        out.append(r)
    return out, PC


def result_arrays(r):
    """(scale, R, t, sRT) a crop returns: the fit, or (1, I, 0) on any failure (tools/umeyama.py:30-33)."""
    if r["status"] != OK:
        return 1.0, np.eye(3), np.zeros(3), np.eye(4)
    f = r["fit"]
    return f["scale"], f["R"], f["t"], f["sRT"]


def K(n):
    return 8 * int(np.ceil(np.log2(max(n, 2)))) + 32


def bounds(n, sigma, var_s, var_t, mean_s, mean_t, scale):
    """B_s, B_R, B_t and the (4,4) bound on sRT of the module docstring."""
    sigma = np.asarray(sigma, np.float64)
    dC = 3 * K(n) * U * np.sqrt(var_s * var_t)                       # Frobenius
    b_R = 2 * dC / (sigma[1] + sigma[2]) + 16 * U
    b_s = abs(scale) * (np.sqrt(3) * dC / sigma.sum() + K(n) * U)
    nms, nmt = np.linalg.norm(mean_s), np.linalg.norm(mean_t)
    b_t = K(n) * U * (nmt + abs(scale) * nms) + b_s * nms + abs(scale) * b_R * np.sqrt(3) * nms
    b_srt = np.zeros((4, 4))
    b_srt[:3, :3] = b_s + abs(scale) * b_R
    b_srt[:3, 3] = b_t
    return b_s, b_R, b_t, b_srt


def fit_bounds(f):
    return bounds(f["n"], f["sigma"], f["var_s"], f["var_t"], f["mean_s"], f["mean_t"], f["scale"])


# ------------------------------------------------------------------------------------------------ synthetic crops
def synth_crop(rng, n_points, outlier_share, noise=2e-3, flat=False, mirror=False, zero_depth=0):
    """One 64x64 crop: a scattered mask of n_points pixels whose NOCS coordinates lie on an ellipsoid (plus noise), camera points
    = s R x + t of a known similarity, pixel coordinates and depth that back-project to them; outlier_share of the masked pixels
    get a NOCS coordinate drawn from the cube instead.  flat: a thin object (z extent 2 %); mirror: the camera points see the
    MIRRORED object, which with a thin object makes the final covariance a reflection case that still fits within the inlier
    threshold; zero_depth: that many masked pixels have depth 0."""
    f = np.float32
    npix = RES * RES
    pix = np.sort(rng.choice(npix, n_points, replace=False))
    a = rng.normal(size=(npix, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    x = a * np.array([0.45, 0.3, 0.006 if flat else 0.2]) * rng.uniform(0.6, 1.0, (npix, 1))
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    q = q * np.sign(np.linalg.det(q))
    s, t = rng.uniform(0.15, 0.5), np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.8, 1.5)])
    xm = x * np.array([1, 1, -1.0]) if mirror else x
    P = s * xm @ q.T + t
    fx, fy, ux, uy = 577.5, 577.5, 319.5, 239.5
    K3 = np.array([[fx, 0, ux], [0, fy, uy], [0, 0, 1]], f)
    depth = P[:, 2].astype(f)
    cx = (P[:, 0] / P[:, 2] * fx + ux).astype(f)
    cy = (P[:, 1] / P[:, 2] * fy + uy).astype(f)
    nocs = (x + rng.normal(size=x.shape) * noise).astype(f)
    n_out = int(round(outlier_share * n_points))
    if n_out:
        o = rng.choice(pix, n_out, replace=False)
        nocs[o] = rng.uniform(-0.5, 0.5, (n_out, 3)).astype(f)
    if zero_depth:
        depth[rng.choice(pix, zero_depth, replace=False)] = 0
    mask = np.zeros(npix, np.uint8)
    mask[pix] = 1
    off = mask == 0                                                   # unmasked pixels: plain values (they compress, and they are never read)
    nocs[off] = 0
    depth[off] = 1
    gy, gx = np.divmod(np.arange(npix), RES)
    cx[off], cy[off] = gx[off].astype(f), gy[off].astype(f)
    return {"xyz_coor": nocs.reshape(RES, RES, 3).transpose(2, 0, 1).copy(), "coor_2d": np.stack([cx, cy]).reshape(2, RES, RES),
            "camK": K3, "Depth": depth.reshape(1, RES, RES), "obj_mask": mask.reshape(1, RES, RES), "gt": (s, q, t)}


def stack_crops(crops):
    return {k: np.stack([c[k] for c in crops]) for k in ("xyz_coor", "coor_2d", "camK", "Depth", "obj_mask")}


# ------------------------------------------------------------------------------------------------ fixtures
def load_fixture(name):
    """tests/golden/umeyama_<name>.npz + its manifest entry -> (inputs dict, draws, PC, valid_depth_only, list of per-crop records)."""
    import json
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "umeyama_manifest.json")) as f:
        meta = json.load(f)[name]
    z = np.load(os.path.join(golden, f"umeyama_{name}.npz"))
    inputs = {k: z[k] for k in ("xyz_coor", "coor_2d", "camK", "Depth", "obj_mask")}
    crops = []
    for b, m in enumerate(meta["crops"]):
        c = dict(m)
        for k in ("index", "counts", "inlier_idx", "R", "t", "sRT", "sigma", "mean_s", "mean_t"):
            if f"{k}_{b}" in z.files:
                c[k] = z[f"{k}_{b}"]
        crops.append(c)
    return inputs, z["draws"], z["PC"], meta["valid_depth_only"], crops


FIXTURES = ("b1", "tiny", "waves", "special", "special_valid_depth")


def expected_status(c):
    """The status a fixture crop must get; None for the rank-deficient tiny crops (held to the documented departure instead)."""
    if c["expect"] == "tiny":
        return None
    if c["n_points"] == 0:
        return NO_POINTS
    return LOW_INLIERS if c["returned_none"] else OK


def check_crop_against_fixture(c, got, what):
    """`got`: dict with index, counts (>= iterations_run entries), iterations_run, best_iteration, n_inliers, inlier_idx, status and
    float64 scale, R, t, sRT.  Decisions exactly, values within the bounds; returns the deviations as ratios of their bounds."""
    assert np.array_equal(got["index"], c["index"]), (what, "compaction order")
    if c["expect"] == "tiny":
        return {}
    assert got["status"] == expected_status(c), (what, got["status"])
    assert got["iterations_run"] == c["iterations_run"], (what, got["iterations_run"], c["iterations_run"])
    if c["n_points"] == 0:
        return {}
    assert np.array_equal(np.asarray(got["counts"])[:c["iterations_run"]], c["counts"]), (what, "inlier counts")
    assert got["best_iteration"] == c["best_iteration"] and got["n_inliers"] == c["n_inliers"], what
    assert np.array_equal(got["inlier_idx"], c["inlier_idx"]), (what, "final inlier set")
    if c["returned_none"]:
        assert got["scale"] == 1 and np.array_equal(got["R"], np.eye(3)) and np.array_equal(got["t"], np.zeros(3)), what
        assert np.array_equal(got["sRT"], np.eye(4)), what
        return {}
    b_s, b_R, b_t, b_srt = bounds(c["n_inliers"], c["sigma"], c["var_s"], c["var_t"], c["mean_s"], c["mean_t"], c["scale"])
    dev = {"scale": abs(got["scale"] - c["scale"]), "R": np.abs(got["R"] - c["R"]).max(), "t": np.abs(got["t"] - c["t"]).max()}
    bnd = {"scale": b_s, "R": b_R, "t": b_t}
    print(f"{what}: n {c['n_inliers']}  |d scale| {dev['scale']:.2e} (bound {b_s:.2e})  |d R| {dev['R']:.2e} (bound {b_R:.2e})  "
          f"|d t| {dev['t']:.2e} (bound {b_t:.2e})")
    for k in dev:
        assert dev[k] <= bnd[k], (what, k, dev[k], bnd[k])
    assert (np.abs(got["sRT"] - c["sRT"]) <= b_srt).all(), (what, "sRT")
    return {k: dev[k] / bnd[k] for k in dev}


def restatement_as_got(r):
    s, Rm, t, srt = result_arrays(r)
    return {"index": r["index"], "counts": r["counts"], "iterations_run": r["iterations_run"], "best_iteration": r["best_iteration"],
            "n_inliers": r.get("n_inliers", 0), "inlier_idx": r["inlier_idx"], "status": r["status"], "scale": s, "R": Rm, "t": t, "sRT": srt}
