"""Write tests/golden/color_aug_pil.npz: what Pillow itself gives for a few small seeded frames, so that the restatement in
tests/color_aug_ref.py stays pinned to Pillow's bytes where Pillow is not installed.  Needs Pillow; run from the repository root:

    python scripts/gen_golden_color_aug.py

    frames        (3,13,17,3) uint8   noise; a ramp with a little noise; flat blocks with hard edges
    factors       (5,) float32        0, an interior value, 1, two values above 1
    single        (3,4,5,13,17,3)     ImageEnhance.{Sharpness, Contrast, Brightness, Color} (codes 1..4) of frame i at factors[k]
    smooth        (3,13,17,3)         ImageFilter.SMOOTH
    plan_ops, plan_factors (P,4)      sequences of codes, with a "none" in the middle and a repeat
    plan_out      (3,P,13,17,3)       the sequences applied left to right, an enhance() call each
    pillow        the version that wrote the file
"""
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageFilter

ENHANCE = {1: ImageEnhance.Sharpness, 2: ImageEnhance.Contrast, 3: ImageEnhance.Brightness, 4: ImageEnhance.Color}
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "color_aug_pil.npz")


def enhance(a, code, f):
    return a if code == 0 else np.asarray(ENHANCE[code](Image.fromarray(a)).enhance(float(f)))


def main():
    r = np.random.Generator(np.random.Philox(key=[2024, 0x6361]))
    H, W = 13, 17
    noise = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ramp = (np.add.outer(np.arange(H) * 11, np.arange(W) * 7)[..., None] * np.array([1, 2, 3]) % 256 + r.integers(0, 9, (H, W, 3))).clip(0, 255).astype(np.uint8)
    blocks = np.repeat(np.repeat(r.integers(0, 2, (4, 5, 3)) * 255, 4, 0), 4, 1)[:H, :W].astype(np.uint8)
    frames = np.stack([noise, ramp, blocks])
    factors = np.array([0.0, 0.37, 1.0, 1.6, 2.9], dtype=np.float32)
    single = np.stack([np.stack([np.stack([enhance(a, code, f) for f in factors]) for code in (1, 2, 3, 4)]) for a in frames])
    smooth = np.stack([np.asarray(Image.fromarray(a).filter(ImageFilter.SMOOTH)) for a in frames])
    plan_ops = np.array([[1, 2, 3, 4], [4, 3, 2, 1], [2, 0, 2, 1], [3, 3, 0, 0]], dtype=np.int32)
    plan_factors = np.array([[1.8, 0.6, 1.3, 2.5], [0.2, 0.7, 1.45, 0.4], [1.5, 1.0, 0.5, 2.0], [1.5, 1.5, 1.0, 1.0]], dtype=np.float32)
    plan_out = np.empty((len(frames), len(plan_ops), H, W, 3), np.uint8)
    for i, a in enumerate(frames):
        for p, (codes, fs) in enumerate(zip(plan_ops, plan_factors)):
            b = a
            for code, f in zip(codes, fs):
                b = enhance(b, int(code), f)
            plan_out[i, p] = b
    np.savez_compressed(OUT, frames=frames, factors=factors, single=single, smooth=smooth, plan_ops=plan_ops, plan_factors=plan_factors,
                        plan_out=plan_out, pillow=np.array(PIL.__version__))
    print(OUT, os.path.getsize(OUT), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
