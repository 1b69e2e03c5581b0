#!/usr/bin/env python3
"""Generate tests/golden/size_head_train_<case>.npz from the REFERENCE's own network/pose_head.py:SizeHead in .train() (BatchNorm1d on
the statistics of the batch, Dropout(0.2) drawing from torch's generator), in float64 and in float32.

Run:  python scripts/gen_golden_size_head.py [REFERENCE_ROOT]       (build container only: needs the reference checkout, never a GPU)
      python scripts/gen_golden_size_head.py --search               (no reference needed: prints seeds for tests/size_head_ref.py)

Only the reference's OUTPUTS are stored; the inputs are the seeded arrays of tests/size_head_ref.py (golden_case), recorded by a CRC --
except the dropout mask, which the reference draws itself: a forward hook on drop1 records it (a unit whose input is 0 counts as kept:
it contributes nothing either way) from the float64 run, and the float32 run replays it through a hook that returns
input * keep / (1 - p) in the place of the module's own draw.  Per file, for the float64 run ("f64_") and the float32 run ("f32_"):
out, the six parameter gradients, d feat as its B C non-zero values ("feat_values") at "feat_arg" (the index within the map),
and the running statistics after one and after two calls of the module on the same input ("running_mean_1", "_2", ...;
num_batches_tracked is then 1 and 2).  The gradients are those of sum(out * g_out) with the seeded g_out.

--search walks seeds upward from 1 for every case of size_head_ref.SHAPES x SCALES and the golden cases and prints the first whose
float64 restatement keeps every y at least 2 GATE_MARGIN max|y| away from zero.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import size_head_ref as R  # noqa: E402


def search():
    def first(shape, scale):
        for seed in range(1, 2000):
            c = R.make_case(*shape, scale, seed)
            if R.gate_margin(R.reference(c, torch.float64)) > 2 * R.GATE_MARGIN and not R.has_ties(c["feat"]):
                return seed
        raise RuntimeError((shape, scale))
    print("CASES = {")
    for shape in R.SHAPES:
        print("    " + " ".join(f"({shape}, {scale!r}): {first(shape, scale)}," for scale in R.SCALES))
    print("}")
    print("GOLDEN_SEEDS = {" + ", ".join(f"{n!r}: {first(s, 'sqrt')}" for n, s in R.GOLDEN_CASES.items()) + "}")


def run_reference(SizeHead, FLAGS, case, dtype, keep=None):
    B, C, HW = case["feat"].shape
    F = case["keep"].shape[1]
    FLAGS.feat_ts = F
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    head = SizeHead(in_dim=C, out_dim=3).to(dtype).train()
    with torch.no_grad():
        for k, v in case["params"].items():
            mod, leaf = k.split(".")
            getattr(getattr(head, mod), leaf).copy_(T(v))
    seen = {}

    def hook(module, inp, out):
        if keep is None:
            seen["keep"] = ((out != 0) | (inp[0] == 0)).squeeze(2).to(torch.uint8).numpy()
            return None
        return inp[0] * T(keep)[:, :, None] / (1 - R.P_DROP)
    head.drop1.register_forward_hook(hook)
    feat = T(case["feat"]).reshape(B, C, 8 if HW == 64 else 2, -1).requires_grad_()
    res = {}
    for call in (1, 2):
        if call == 2:
            head.drop1._forward_hooks.clear()       # the second call only moves the running statistics
        out = head(feat)
        if call == 1:
            out.backward(T(case["g_out"]))
            res["out"] = out.detach().numpy()
            for k in R.PARAM_KEYS:
                mod, leaf = k.split(".")
                res[k] = getattr(getattr(head, mod), leaf).grad.numpy()
            g = feat.grad.reshape(B, C, HW)
            arg = g.abs().argmax(-1)
            assert int((g != 0).sum(-1).max()) <= 1
            res["feat_arg"] = arg.numpy().astype(np.int32)
            res["feat_values"] = g.gather(2, arg[:, :, None]).squeeze(2).numpy()
        res[f"running_mean_{call}"], res[f"running_var_{call}"] = head.bn1.running_mean.numpy().copy(), head.bn1.running_var.numpy().copy()
        assert int(head.bn1.num_batches_tracked) == call
    return res, seen.get("keep")


def generate():
    import ref_shim
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        ref_shim.REFERENCE_ROOT = os.path.abspath(args[0])
    FLAGS = ref_shim.install()
    from network.pose_head import SizeHead
    for name in R.GOLDEN_CASES:
        case = R.golden_case(name)
        torch.manual_seed(R.GOLDEN_SEEDS[name])
        r64, keep = run_reference(SizeHead, FLAGS, case, torch.float64)
        r32, _ = run_reference(SizeHead, FLAGS, case, torch.float32, keep=keep)
        assert 0 < keep.mean() < 1, "the mask of this seed drops nothing or everything"
        arrs = {"input_crc": R.case_crc(case), "keep": keep}
        for k, v in r64.items():
            arrs["f64_" + k] = v
            arrs["f32_" + k] = r32[k]
            if v.dtype == np.float64 and k != "conv1.bias":      # conv1.bias: analytically 0, no scale of its own
                scale = np.abs(v).max()
                print(f"  {name} {k:16s} float32 run against float64: {np.abs(r32[k] - v).max() / scale:.2e} of max|.|")
        assert (arrs["f64_feat_arg"] == arrs["f32_feat_arg"]).all()
        path = os.path.join(R.GOLDEN, f"size_head_train_{name}.npz")
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        print(f"  wrote size_head_train_{name}.npz ({size / 1024:.1f} KB), {int(keep.sum())} of {keep.size} units kept")
        assert size < 200 * 1024


if __name__ == "__main__":
    if "--search" in sys.argv:
        search()
    else:
        generate()
        print("done")
