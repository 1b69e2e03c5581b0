"""Fixtures for the alignment kernels, recorded from the reference: tests/golden/umeyama_*.npz + umeyama_manifest.json.

    python scripts/gen_golden_umeyama.py --reference /path/to/GIVEPose

Runs on a CPU.  Imports the reference's tools/align_utils.py (NumPy only) and get_PC_nocs from its tools/umeyama.py (open3d,
matplotlib and PIL stubbed in sys.modules: the function uses none of them).  During a call np.random.randint is replaced by a
function that returns draws[b, i] % nPoints, and estimateSimilarityUmeyama by a wrapper that records what each call got and
returned; everything recorded below is computed by the reference's own expressions on the reference's own values.

Per crop: the inputs, PC, the inlier count of every iteration the reference ran, the iterations run, the best iteration, the final
inlier index set, scale / R / t / sRT (or the fact that it returned None) and, for the bounds of tests/umeyama_ref.py, the singular
values (last one signed), variances and centroids of the final set.

A seed is rejected (the next one is tried) unless, on the reference's values: no residual of an evaluated hypothesis lies within a
relative 1e-9 of its threshold; no early-stop value within 1e-9 of 0.99; every evaluated sample has sigma_2 / sigma_1 >= 1e-6 and
sigma_1 / (sigma_2 + sigma_3) <= 1e5; and the crop does what its case is there for (tests/umeyama_ref.py: MARGIN_*).  A best-count
tie cannot be decided by rounding: the ratios compared share their denominator, so the comparison is one of integers (asserted).
The 1- and 2-point crops are the dedicated rank-deficient cases: there the reference's result depends on LAPACK's null-space
vectors, nothing of it is recorded but the inputs, and the tests hold the kernels to the documented departure instead.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import umeyama_ref as R      # noqa: E402  (synthetic crops, margins)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def import_reference(path):
    for name in ("open3d", "matplotlib", "PIL", "PIL.Image"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["PIL"].Image = sys.modules["PIL.Image"]
    sys.modules["PIL.Image"].Image = object
    sys.path.insert(0, path)
    from tools import align_utils, umeyama
    return align_utils, umeyama


class Rejected(Exception):
    pass


def run_reference_crop(AU, src, tgt, draws_b):
    """estimateSimilarityTransform of the reference on one crop with the draws replaced; returns the record."""
    calls = []
    orig_fit, orig_randint = AU.estimateSimilarityUmeyama, np.random.randint
    state = {"i": 0}

    def fit(S, T):
        out = orig_fit(S, T)
        calls.append((S.copy(), T.copy(), out))
        return out

    def randint(n, size=None):
        assert size == 5
        v = (draws_b[state["i"]] % np.uint32(n)).astype(np.int64)
        state["i"] += 1
        return v

    AU.estimateSimilarityUmeyama, np.random.randint = fit, randint
    try:
        with np.errstate(all="ignore"):
            scale, rot, trans, srt = AU.estimateSimilarityTransform(src, tgt)
    finally:
        AU.estimateSimilarityUmeyama, np.random.randint = orig_fit, orig_randint
    n = src.shape[0]
    iters = state["i"]
    rec = {"n_points": n, "iterations_run": iters, "returned_none": scale is None}
    # the reference's own expressions (align_utils.py:49-59, 73-77) on the recorded transforms
    SourceHom = np.transpose(np.hstack([src, np.ones([n, 1])]))
    TargetHom = np.transpose(np.hstack([tgt, np.ones([n, 1])]))
    Centered = SourceHom[:3, :] - np.tile(np.mean(SourceHom[:3, :], axis=1), (n, 1)).transpose()
    InlierT = 2 * np.amax(np.linalg.norm(Centered, axis=0)) / 10.0
    counts, best, best_i, best_idx = [], 0, -1, np.arange(n)
    margin_res, margin_stop, min_rank, max_cond = np.inf, np.inf, np.inf, 0.0
    for i in range(iters):
        S, T, (Scale, _, _, Out) = calls[i]
        Cov = np.matmul(T[:3] - T[:3].mean(1, keepdims=True), (S[:3] - S[:3].mean(1, keepdims=True)).T) / 5
        sv = np.linalg.svd(Cov, compute_uv=False)
        sgn = -1.0 if np.linalg.det(Cov) < 0 else 1.0
        min_rank = min(min_rank, sv[1] / sv[0])
        max_cond = max(max_cond, sv[0] / (sv[1] + sgn * sv[2]))
        Pass = Scale * InlierT
        Res = np.linalg.norm((TargetHom - np.matmul(Out, SourceHom))[:3, :], axis=0)
        margin_res = min(margin_res, np.abs(Res / Pass - 1).min())
        Idx = np.where(Res < Pass)[0]
        counts.append(len(Idx))
        assert (len(Idx) / n > best / n) == (len(Idx) > best)      # a tie is never decided by rounding
        if len(Idx) / n > best / n:
            best, best_i, best_idx = len(Idx), i, Idx
        stop = 1 - (1 - (best / n) ** 5) ** i
        margin_stop = min(margin_stop, abs(stop - 0.99))
        if stop > 0.99:
            assert i == iters - 1, "replay of the early stop disagrees with the reference"
        else:
            assert i < iters - 1 or i == R.MAX_ITER - 1, "replay of the early stop disagrees with the reference"
    if not (margin_res >= R.MARGIN_RESIDUAL and margin_stop >= R.MARGIN_STOP and min_rank >= R.MIN_SAMPLE_RANK and max_cond <= R.MAX_SAMPLE_COND):
        raise Rejected(f"margins: residual {margin_res:.2e} stop {margin_stop:.2e} rank {min_rank:.2e} cond {max_cond:.2e}")
    assert (best / n < 0.1) == (scale is None)
    rec.update(counts=np.array(counts, np.int32), best_iteration=best_i, n_inliers=best, inlier_idx=best_idx.astype(np.int32),
               margins=[float(margin_res), float(margin_stop), float(min_rank), float(max_cond)])
    if scale is not None:
        S, T, (Scale, Rot, Trans, Out) = calls[-1]
        assert len(calls) == iters + 1 and np.array_equal(S, SourceHom[:, best_idx]) and np.array_equal(T, TargetHom[:, best_idx])
        assert Scale == scale
        cs, ct = S[:3] - S[:3].mean(1, keepdims=True), T[:3] - T[:3].mean(1, keepdims=True)
        Cov = np.matmul(ct, cs.T) / best
        sv = np.linalg.svd(Cov, compute_uv=False)
        if np.linalg.det(Cov) < 0:
            sv[2] = -sv[2]
        if sv[1] / sv[0] < 1e-3:
            raise Rejected("final set badly conditioned")
        rec.update(scale=float(scale), R=rot, t=trans, sRT=srt, sigma=sv, var_s=float((cs ** 2).sum() / best), var_t=float((ct ** 2).sum() / best),
                   mean_s=S[:3].mean(1), mean_t=T[:3].mean(1))
    return rec


# name -> list of crops: (n_points, outlier share, extra synth_crop arguments, expectation)
CASES = {
    "b1": dict(crops=[(700, 0.2, {}, "ok")], flag=False),
    "tiny": dict(crops=[(0, 0, {}, "none"), (1, 0, {}, "tiny"), (2, 0, {}, "tiny"), (5, 0, {}, "two"), (37, 0.2, {}, "ok")], flag=False),
    "waves": dict(crops=[(63, 0.2, {}, "ok"), (64, 0, {}, "two"), (65, 0.45, {}, "ok"), (2500, 0.45, {}, "ok"), (4096, 0.2, {}, "ok")], flag=False),
    "special": dict(crops=[(700, 0.95, {}, "none128"), (700, 0, {}, "two"), (700, 0.2, dict(flat=True, mirror=True), "reflection"),
                           (700, 0.2, dict(zero_depth=60), "ok"), (2500, 0.3, {}, "ok")], flag=False),
    "special_valid_depth": dict(same_inputs_as="special", flag=True),
}


def build_case(AU, UM, name, spec, inputs_of):
    seed = 0
    while True:
        seed += 1
        rng = np.random.RandomState(1000 * (sorted(CASES).index(name) + 1) + seed)
        if "same_inputs_as" in spec:
            inputs, crops_spec, draws = inputs_of[spec["same_inputs_as"]]
            draws = rng.randint(0, 2 ** 32, size=draws.shape, dtype=np.uint64).astype(np.uint32)
        else:
            crops_spec = spec["crops"]
            inputs = R.stack_crops([R.synth_crop(rng, n, share, **kw) for n, share, kw, _ in crops_spec])
            draws = rng.randint(0, 2 ** 32, size=(len(crops_spec), R.MAX_ITER, R.SAMPLE), dtype=np.uint64).astype(np.uint32)
        t = {k: torch.from_numpy(v) for k, v in inputs.items()}
        PC, nocs, mask = UM.get_PC_nocs(t["coor_2d"], t["camK"], t["Depth"], t["obj_mask"], t["xyz_coor"])
        out = {k: v for k, v in inputs.items()}
        out.update(draws=draws, PC=PC.astype(np.float32))
        assert PC.dtype == np.float32
        meta = []
        try:
            for b, (n, share, kw, expect) in enumerate(crops_spec):
                keep = mask[b].copy()
                if spec["flag"]:
                    keep &= inputs["Depth"][b].reshape(-1) > 0          # backproject, align_utils.py:116-117
                out[f"index_{b}"] = np.nonzero(keep)[0].astype(np.int32)
                src, tgt = nocs[b][keep, :], PC[b][keep, :]             # tools/umeyama.py:27-28
                if expect == "tiny":
                    meta.append({"n_points": int(keep.sum()), "expect": expect})
                    continue
                if keep.sum() == 0:
                    assert AU.estimateSimilarityTransform(src, tgt)[0] is None
                    meta.append({"n_points": 0, "expect": expect, "returned_none": True, "iterations_run": 0})
                    continue
                rec = run_reference_crop(AU, src, tgt, draws[b])
                if expect == "two" and not (rec["iterations_run"] == 2 and not rec["returned_none"]):
                    raise Rejected("clean crop did not stop after 2 iterations")
                if expect == "none128" and not (rec["iterations_run"] == 128 and rec["returned_none"]):
                    raise Rejected("95 % outliers did not fail after 128 iterations")
                if expect in ("ok", "reflection") and rec["returned_none"]:
                    raise Rejected("crop failed")
                if expect == "reflection" and not rec["sigma"][2] < 0:
                    raise Rejected("not a reflection case")
                if expect == "ok" and share >= 0.2 and n >= 63 and rec["iterations_run"] < 5:
                    raise Rejected("stopped too early to exercise the replay")
                m = {"expect": expect}
                for k, v in rec.items():
                    if isinstance(v, np.ndarray):
                        out[f"{k}_{b}"] = v
                    else:
                        m[k] = v
                meta.append(m)
        except Rejected as e:
            print(f"  {name}: seed {seed} rejected ({e})")
            if seed > 200:
                raise
            continue
        inputs_of[name] = (inputs, crops_spec, draws)
        return out, {"seed": seed, "valid_depth_only": spec["flag"], "crops": meta}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds tools/)")
    args = ap.parse_args()
    AU, UM = import_reference(args.reference)
    manifest, inputs_of = {}, {}
    for name, spec in CASES.items():
        arrays, meta = build_case(AU, UM, name, spec, inputs_of)
        path = os.path.join(GOLDEN, f"umeyama_{name}.npz")
        np.savez_compressed(path, **arrays)
        manifest[name] = meta
        print(name, os.path.getsize(path) // 1024, "KB", [(c.get("n_points"), c.get("iterations_run"), c.get("n_inliers")) for c in meta["crops"]])
    with open(os.path.join(GOLDEN, "umeyama_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)


if __name__ == "__main__":
    main()
