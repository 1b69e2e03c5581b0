"""GPU: givepose_amd.ColorAugmenter (gpca_luma_partials + gpca_apply, include/givepose_coloraug.h) against the numpy restatement of
PIL's enhance operations in tests/color_aug_ref.py, which tests/test_color_aug_cpu.py pins to Pillow.  Every comparison is
np.array_equal.  The references are computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

import color_aug_ref as R

pytestmark = pytest.mark.gpu
NONE, SHARP, CONTRAST, BRIGHT, COLOR = 0, 1, 2, 3, 4


def frames_for(F, H, W, seed):
    """Noise, with a dark and a bright band so that factors above 1 clip on both sides, and smooth blocks for SMOOTH's truncations."""
    r = np.random.Generator(np.random.Philox(key=[seed, 0x6362]))
    a = r.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    a[:, : H // 4] //= 8
    a[:, -(H // 4) or H:] |= 0xE0
    blocks = np.repeat(np.repeat(r.integers(0, 256, (F, (H + 3) // 4, (W + 3) // 4, 3), dtype=np.uint8), 4, 1), 4, 2)[:, :H, :W]
    return np.where((np.arange(W) % 8 < 3)[None, None, :, None], blocks, a)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "3x3":               # one interior pixel
        F, H, W = 1, 3, 3
        ops, fac = [[SHARP, CONTRAST, BRIGHT, COLOR]], [[1.9, 1.4, 0.8, 2.2]]
    elif name == "7x13":            # 39-byte rows, 273-byte frames: frames 1 and 2 start misaligned
        F, H, W = 3, 7, 13
        ops = [[SHARP, CONTRAST, BRIGHT, COLOR], [COLOR, BRIGHT, CONTRAST, SHARP], [CONTRAST, SHARP, COLOR, BRIGHT]]
        fac = [[0.3, 1.45, 1.2, 2.9], [0.0, 0.55, 0.5, 2.0], [1.0, 1.7, 3.0, 1.5]]
    elif name == "40x50":           # aligned 6000-byte frames, 150-byte rows; mixed plans
        F, H, W = 5, 40, 50
        ops = [[NONE, NONE, NONE, NONE],                    # must equal its input
               [NONE, NONE, COLOR, NONE],                   # one operation, not at the left
               [SHARP, CONTRAST, BRIGHT, COLOR],
               [COLOR, BRIGHT, CONTRAST, SHARP],            # the same four in another order
               [CONTRAST, CONTRAST, NONE, SHARP]]           # a repeat, and a gap
        fac = [[1, 1, 1, 1], [1, 1, 0.4, 1], [1.6, 0.7, 1.3, 2.4], [2.4, 1.3, 0.7, 1.6], [1.5, 1.5, 1, 0.25]]
    elif name == "19x32":           # 96-byte rows: the Sharpness strips, the last one of three rows
        F, H, W = 2, 19, 32
        ops, fac = [[SHARP, COLOR, SHARP, CONTRAST], [BRIGHT, SHARP, NONE, NONE]], [[2.0, 0.5, 0.6, 1.2], [1.4, 1.1, 1, 1]]
    elif name == "480x640":         # the real shape
        F, H, W = 2, 480, 640
        ops, fac = [[SHARP, CONTRAST, BRIGHT, COLOR], [COLOR, CONTRAST, SHARP, BRIGHT]], [[1.7, 1.3, 0.9, 2.6], [0.2, 0.6, 0.4, 1.45]]
    frames = frames_for(F, H, W, seed=H * W)
    plan = {"ops": np.array(ops, np.int32), "factors": np.array(fac, np.float32)}
    ref = R.run_plan(frames, plan["ops"], plan["factors"])
    for v in (frames, ref, plan["ops"], plan["factors"]):
        v.setflags(write=False)
    return frames, plan, ref


def aug_for(frames, **kw):
    from givepose_amd import ColorAugmenter
    return ColorAugmenter(frames.shape[1], frames.shape[2], "cuda", **kw)


@pytest.mark.parametrize("name", ["3x3", "7x13", "40x50", "19x32", "480x640"])
def test_plans_bit_equal(name):
    frames, plan, ref = case(name)
    dev = torch.from_numpy(frames.copy()).cuda()
    aug = aug_for(frames)
    got = aug(dev, plan=plan)
    assert got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous() and tuple(got.shape) == frames.shape
    got = got.cpu().numpy()
    for f in range(len(frames)):
        assert np.array_equal(got[f], ref[f]), (name, f, int((got[f] != ref[f]).sum()))
    assert np.array_equal(dev.cpu().numpy(), frames)                      # `frames` is never written
    assert (ref != frames).any()
    if name == "40x50":
        assert np.array_equal(ref[0], frames[0]) and not np.array_equal(ref[2], ref[3])
    # one apply launch per position of the plan, one reduction more where a frame's operation there is a Contrast: whatever F
    assert aug.launches == 4 + int((plan["ops"] == CONTRAST).any(0).sum())


def test_single_operations_on_every_walk():
    """Each operation alone, on an aligned and on a misaligned frame of one call (7 x 16: 48-byte rows, 336-byte frames; 9 x 11: 297-byte
    frames), at a factor inside [0, 1] and one above."""
    for H, W in ((7, 16), (9, 11)):
        frames = frames_for(4, H, W, seed=H)
        aug = aug_for(frames)
        for code in (SHARP, CONTRAST, BRIGHT, COLOR):
            plan = {"ops": np.full((4, 1), code, np.int32), "factors": np.array([[0.35], [1.0], [1.8], [2.75]], np.float32)}
            got = aug(frames, plan=plan).cpu().numpy()
            assert np.array_equal(got, R.run_plan(frames, plan["ops"], plan["factors"])), (H, W, code)
            assert aug.launches == (2 if code == CONTRAST else 1)


def test_seeded_form_equals_the_explicit_form():
    from givepose_amd import color_aug_draws
    frames, _, _ = case("40x50")
    big = np.concatenate([frames, frames[::-1], frames])[:12]
    aug = aug_for(frames)
    plan = color_aug_draws(4, 12)
    assert (plan["ops"] != 0).sum(1).max() >= 3 and ((plan["ops"] != 0).sum(1) == 0).any()
    a = aug(big, seed=4).cpu().numpy()
    assert np.array_equal(a, aug(big, plan=plan).cpu().numpy())
    assert np.array_equal(a, R.run_plan(big, plan["ops"], plan["factors"]))
    en = np.arange(12) % 2 == 0
    b = aug(big, seed=4, enable=en).cpu().numpy()
    assert np.array_equal(b[en], a[en]) and np.array_equal(b[~en], big[~en])
    assert np.array_equal(aug(big, plan=plan, enable=en).cpu().numpy(), b)
    # a plan without any operation is a copy, in one launch
    assert np.array_equal(aug(big, seed=4, enable=np.zeros(12, bool)).cpu().numpy(), big) and aug.launches == 1


def test_repeatable_out_honoured_and_a_larger_batch_after_a_smaller():
    frames, plan, ref = case("40x50")
    aug = aug_for(frames)
    dev = torch.from_numpy(frames.copy()).cuda()
    a = aug(dev[:2], plan={k: v[:2] for k, v in plan.items()})
    assert np.array_equal(a.cpu().numpy(), ref[:2])
    small = [t.data_ptr() if t is not None else None for t in aug._tmp]
    out = torch.full_like(dev, 7)
    b = aug(dev, plan=plan, out=out)                                      # F = 5 after F = 2: the buffers grow
    assert b is out and np.array_equal(out.cpu().numpy(), ref)
    grown = [t.data_ptr() for t in aug._tmp]
    c = aug(dev, plan=plan)
    assert np.array_equal(c.cpu().numpy(), ref) and c.data_ptr() != out.data_ptr()      # two calls, equal bits
    assert [t.data_ptr() for t in aug._tmp] == grown and all(t.shape[0] == 5 for t in aug._tmp)      # reused while F does not grow
    aug(dev[:3], plan={k: v[:3] for k, v in plan.items()})
    assert [t.data_ptr() for t in aug._tmp] == grown and small[0] is None                # two frames of one operation needed none
    assert np.array_equal(dev.cpu().numpy(), frames)


def test_refusals_before_any_launch():
    frames, plan, _ = case("7x13")
    aug = aug_for(frames)
    dev = torch.from_numpy(frames.copy()).cuda()
    bad = lambda **kw: {**plan, **kw}
    with pytest.raises(ValueError, match="exactly one"):
        aug(dev)
    with pytest.raises(ValueError, match="exactly one"):
        aug(dev, plan=plan, seed=1)
    with pytest.raises(ValueError, match="codes 0..4"):
        aug(dev, plan=bad(ops=np.full((3, 4), 5, np.int32)))
    with pytest.raises(ValueError, match="codes 0..4"):
        aug(dev, plan=bad(ops=np.full((3, 4), -1, np.int32)))
    with pytest.raises(ValueError, match="finite"):
        aug(dev, plan=bad(factors=np.full((3, 4), np.inf, np.float32)))
    with pytest.raises(ValueError, match="finite"):
        aug(dev, plan=bad(factors=np.full((3, 4), 1e300)))                # finite in float64, not in float32
    with pytest.raises(ValueError, match=r"plan\['ops'\]"):
        aug(dev, plan=bad(ops=plan["ops"][:2]))
    with pytest.raises(ValueError, match=r"plan\['factors'\]"):
        aug(dev, plan=bad(factors=plan["factors"][:, :3]))
    with pytest.raises(ValueError, match="uint8"):
        aug(dev.float(), plan=plan)
    with pytest.raises(ValueError, match="does not match"):
        aug(dev[:, :, :12], plan=plan)
    with pytest.raises(ValueError, match="alias"):
        aug(dev, plan=plan, out=dev)
    with pytest.raises(ValueError, match="out must be"):
        aug(dev, plan=plan, out=torch.empty_like(dev, dtype=torch.int8))
    assert np.array_equal(dev.cpu().numpy(), frames)


def test_augmented_frames_feed_the_train_batch_builder():
    """ColorAugmenter's output is TrainBatchBuilder's `frames`: roi_img equals the builder's on the restatement's frames (40 x 50, S = 32)."""
    from givepose_amd import TrainBatchBuilder
    from test_train_batch_gpu import run, small_case
    c, draws, _, labels, _, _, _ = small_case(32, 8)
    frames = c["frames"]
    r = np.random.Generator(np.random.Philox(key=[9, 0x6362]))
    plan = {"ops": np.stack([r.permutation(4) + 1 for _ in range(len(frames))]).astype(np.int32),
            "factors": r.uniform(0.3, 2.0, (len(frames), 4)).astype(np.float32)}
    aug = aug_for(frames)
    builder = TrainBatchBuilder(40, 50, "cuda", img_size=32, out_res=8, pad_scale=1.0)
    got = run(builder, {**c, "frames": aug(frames, plan=plan)}, labels, draws=draws)
    ref_frames = R.run_plan(frames, plan["ops"], plan["factors"])
    ref = run(builder, {**c, "frames": ref_frames}, labels, draws=draws)
    plain = run(builder, c, labels, draws=draws)
    assert torch.equal(got["roi_img"], ref["roi_img"]) and not torch.equal(got["roi_img"], plain["roi_img"])
    for k in ("roi_mask", "roi_mask_deform", "nocs_coord"):
        assert torch.equal(got[k], plain[k]), k
