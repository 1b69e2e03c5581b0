"""CPU: the host side of the training batch (givepose_amd/train_batch.py) against tests/train_batch_ref.py, the properties of the
restated defor_2D, and the ABI of the training-batch family: include/givepose_traindata.h == the library's gpt_* symbols ==
_lib.TRAINDATA_PROTOTYPES, none of them in givepose_hip.h (the check tests/test_umeyama_cpu.py makes for gpa_).  Every comparison is
np.array_equal: the host values are the reference's float64 / float32 operations in its order."""
import os
import re
import subprocess

import numpy as np
import pytest

import train_batch_ref as R
from oracle.preprocess_ref import get_affine_transform_ref, warp_affine_nearest_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 480, 640
# (y1,x1,y2,x2): an ordinary box; one whose padded side exceeds max(H,W) (the clip); one over the corner whose centre (2, 10) a shift
# moves off the frame; a tall one with fractional corners
BOXES = np.array([[100, 200, 220, 300], [10, 20, 470, 630], [-10, -28, 30, 32], [33.5, 411.25, 300.75, 500.0]], dtype=np.float64)
DRAWS = np.array([[0.3, 0.9, 0.1], [0.99, 0.5, 0.5], [0.5, 0.0, 0.01], [0.0, 0.999, 0.75]], dtype=np.float64)


def _walk(inv, size):
    """The source pixel index (+1; 0 outside the frame) of every destination pixel under the inverse map `inv` (6,), by
    cv::warpAffine's fixed-point walk -- what warp_src of csrc/common.hpp computes."""
    xs = np.arange(size, dtype=np.float64)
    X0 = np.rint((inv[1] * xs + inv[2]) * 1024).astype(np.int64) + 512
    Y0 = np.rint((inv[4] * xs + inv[5]) * 1024).astype(np.int64) + 512
    X = (X0[:, None] + np.rint(inv[0] * xs * 1024).astype(np.int64)[None, :]) >> 10
    Y = (Y0[:, None] + np.rint(inv[3] * xs * 1024).astype(np.int64)[None, :]) >> 10
    ok = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
    return np.where(ok, Y * W + X + 1, 0)


@pytest.mark.parametrize("dzi_type", ["uniform", "uniform_sr", "none"])
def test_dzi_parameters_and_crop_maps(dzi_type):
    from givepose_amd import preprocess as P, train_batch as TB
    cx, cy, scale = TB.dzi_center_scale(BOXES, DRAWS, H, W, dzi_type)
    params = P.crop_params_from_center_scale(cx, cy, scale, 256, 64)
    index = np.arange(1, H * W + 1, dtype=np.int64).reshape(H, W)
    for b, (y1, x1, y2, x2) in enumerate(BOXES):
        center, s = R.aug_bbox_dzi_ref(np.array([x1, y1, x2, y2]), DRAWS[b], H, W, dzi_type)
        assert (cx[b], cy[b], scale[b]) == (center[0], center[1], s), (dzi_type, b)
        assert np.array_equal(params["bbox_center"][b], center.astype(np.float32))
        assert params["resize_ratio"][b] == np.float32(64 / s)
        for key, size in (("inv_img", 256), ("inv_out", 64)):
            ref = warp_affine_nearest_ref(index, get_affine_transform_ref(center, s, size), size)
            assert np.array_equal(_walk(params[key][b], size), ref), (dzi_type, b, key)
    if dzi_type != "none":
        assert scale[1] == 640.0 and scale[0] < 640.0                                        # the max(H,W) clip binds on box 1 only
        assert cx[2] < 0 or cy[2] < 0                                                        # a centre off the frame
        assert (_walk(params["inv_out"][2], 64) == 0).any() and (_walk(params["inv_out"][2], 64) != 0).any()
    else:
        assert np.array_equal(scale, np.minimum(np.maximum(BOXES[:, 2] - BOXES[:, 0], BOXES[:, 3] - BOXES[:, 1]), 640))


def test_crop_params_is_the_centre_scale_form_of_the_padded_box():
    from givepose_amd import preprocess as P
    a = P.crop_params(BOXES, H, W)
    b = P.crop_params_loop(BOXES, H, W)
    cx, cy = 0.5 * (BOXES[:, 1] + BOXES[:, 3]), 0.5 * (BOXES[:, 0] + BOXES[:, 2])
    scale = np.minimum(np.maximum(BOXES[:, 2] - BOXES[:, 0], BOXES[:, 3] - BOXES[:, 1]) * 1.5, 640) * 1.0
    c = P.crop_params_from_center_scale(cx, cy, scale)
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k in c:
        assert np.array_equal(a[k], c[k]), k
    with pytest.raises(ValueError, match="scale"):
        P.crop_params_from_center_scale([1.0], [2.0], [0.0])


def test_value_tables_for_all_bytes():
    from givepose_amd import train_batch as TB
    meta = (np.array([0.013, -0.0625, 0.2071], dtype=np.float64), 0.9137)
    table = TB.coord_tables([5, 2], [meta, None])
    assert table.shape == (2, 3, 256) and table.dtype == np.float32
    png = np.stack([np.arange(256, dtype=np.uint8)] * 3, -1)[None]           # a (1,256,3) frame that holds every byte in every channel
    for b, (cat, m) in enumerate(((5, meta), (2, None))):
        frame = R.coord_frame_ref(png, cat, m)
        assert frame.dtype == (np.float64 if cat == 5 else np.float32)
        assert np.array_equal(table[b], frame[0].T.astype(np.float32)), cat
    assert table[1, 0, 0] == -0.5 and table[1, 2, 0] == 0.5 and table[1, 2, 255] == -0.5
    with pytest.raises(ValueError, match="mug"):
        TB.coord_tables([5], [None])


def _band(mask):
    """Where a pixel differs from its upper or its left neighbour: erode != dilate of the 3-pixel element, said another way."""
    m = mask != 0
    band = np.zeros(m.shape, bool)
    band[1:, :] |= m[1:, :] != m[:-1, :]
    band[:, 1:] |= m[:, 1:] != m[:, :-1]
    return band


def test_reference_deformation_properties():
    r = np.random.Generator(np.random.Philox(key=[7, 0x7B]))
    S = 24
    keys = r.integers(0, 1 << 32, (S, S), dtype=np.uint64).astype(np.uint32)
    blob = np.zeros((S, S), np.float32)
    blob[5:14, 3:11] = 1
    blob[9, 10] = 0
    noise = (r.random((S, S)) > 0.5).astype(np.float32)
    for name, mask in (("blob", blob), ("noise", noise)):
        band = _band(mask)
        l = int(band.sum())
        out = R.defor_2d_ref(mask[None], True, keys)
        assert out.shape == (S, S) and set(np.unique(out)) <= {0.0, 1.0}
        assert int((out[band] == 0).sum()) == l // 2, name                   # exactly floor(l/2) zeros in the band
        assert np.array_equal(out[~band], mask[~band]), name                 # pixels outside it keep their value
        assert np.array_equal(R.defor_2d_ref(mask[None], False, keys), mask)
        # duplicate keys: the lower pixel index goes first
        dup = R.defor_2d_ref(mask[None], True, np.zeros((S, S), np.uint32))
        assert np.array_equal(np.flatnonzero(dup[band] == 0), np.arange(l // 2)), name
    for flat in (np.zeros((S, S), np.float32), np.ones((S, S), np.float32)):     # l = 0: identity
        assert not _band(flat).any() and np.array_equal(R.defor_2d_ref(flat[None], True, keys), flat)
    # l = 1: a 0 at the corner of an image of ones has no neighbour up or left of it, and only itself differs from them
    one = np.ones((S, S), np.float32)
    one[S - 1, S - 1] = 0
    assert int(_band(one).sum()) == 1
    assert np.array_equal(R.defor_2d_ref(one[None], True, keys), np.ones((S, S), np.float32))
    # a single 1 inside: the band is the pixel and its right and lower neighbours, l = 3, one zero
    single = np.zeros((S, S), np.float32)
    single[7, 7] = 1
    band = _band(single)
    assert sorted(zip(*np.nonzero(band))) == [(7, 7), (7, 8), (8, 7)]
    assert int((R.defor_2d_ref(single[None], True, keys)[band] == 0).sum()) == 1


def test_hash_keys_is_the_size_heads_counter_hash():
    # x = lo ^ idx * 0x9E3779B9 ^ rotl(hi, 16), then the murmur3 finaliser: checked against a scalar restatement in Python integers
    seed = 0x0123456789ABCDEF
    got = R.hash_keys(seed, 2, 5)
    M = 0xFFFFFFFF
    for idx in (0, 1, 24, 25, 49):
        hi, lo = seed >> 32, seed & M
        x = lo ^ ((idx * 0x9E3779B9) & M) ^ (((hi << 16) | (hi >> 16)) & M)
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & M
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & M
        x ^= x >> 16
        assert int(got.reshape(-1)[idx]) == x, idx
    assert got.dtype == np.uint32 and len(np.unique(got)) == 50


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_traindata_header_equals_exported_symbols_and_prototypes():
    from givepose_amd import _lib, build
    assert "traindata.hip" in build.SOURCES
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (gpt_[a-z0-9_]+)", out))
    declared = set(re.findall(r"^int (gpt_[a-z0-9_]+)\s*\(", _header("givepose_traindata.h"), re.M))
    assert declared == {"gpt_crop_train", "gpt_mask_deform"} and declared == exported, (declared - exported, exported - declared)
    assert set(_lib.TRAINDATA_PROTOTYPES) == declared
    lib = _lib.load()
    for name, (argtypes, _) in _lib.TRAINDATA_PROTOTYPES.items():
        assert getattr(lib, name).argtypes == argtypes
        decl = re.search(rf"^int {name}\s*\((.*?)\);", _header("givepose_traindata.h"), re.M | re.S).group(1)
        assert len(decl.split(",")) == len(argtypes), name                      # one ctypes entry per declared parameter
    m = re.search(r"#define GP_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "givepose_hip.h")).read())
    assert int(m.group(1)) == _lib.ABI_VERSION == lib.gp_version() == 328
    for k in ("MAX_PIXELS", "TRAIN_BATCH_LAUNCHES"):
        v = re.search(rf"#define GPT_{k} (\d+)", _header("givepose_traindata.h")).group(1)
        assert int(v) == getattr(_lib, "GPT_" + k), k


def test_no_traindata_symbol_in_the_main_header():
    assert "gpt_" not in _header("givepose_hip.h")
    assert not re.search(r"^int gp_", _header("givepose_traindata.h"), re.M)


def test_fs_net_scale_and_sym_info():
    from givepose_amd import fs_net_scale, sym_info
    model = np.array([[-0.25, -0.125, 0.5], [0.125, 0.375, -0.25], [0.0, 0.0, 0.0]], dtype=np.float64)
    real, mean = fs_net_scale("laptop", model, 0.5)
    assert real.tolist() == [250.0, 250.0, 375.0] and mean.tolist() == [346, 200, 335]      # lx = 2 max(|x|): symmetric about x = 0
    assert fs_net_scale("02876657", model, 2.0)[1].tolist() == [81.0, 218.5, 80.25]
    assert fs_net_scale("mug", model, 1.0)[1].tolist() == [146, 83, 114]
    with pytest.raises(NotImplementedError, match="teapot"):
        fs_net_scale("teapot", model, 1.0)
    rows = {1: [1, 1, 0, 1], 2: [1, 1, 0, 1], 3: [0, 0, 0, 0], 4: [1, 1, 1, 1], 5: [0, 1, 0, 0], 6: [0, 1, 0, 0]}
    for c, row in rows.items():
        assert sym_info(c).tolist() == row and sym_info(c).dtype == np.dtype(int)
    assert sym_info(6, mug_handle=0).tolist() == [1, 0, 0, 0] and sym_info(5, mug_handle=0).tolist() == [0, 1, 0, 0]
    with pytest.raises(NotImplementedError, match="7"):
        sym_info(7)


def test_refusals_by_name():
    from givepose_amd import TrainBatchBuilder
    with pytest.raises(ValueError, match="roi10d.*x2 onto x1"):
        TrainBatchBuilder(H, W, "cuda", dzi_type="roi10d")
    with pytest.raises(ValueError, match="truncnorm.*NotImplementedError"):
        TrainBatchBuilder(H, W, "cuda", dzi_type="truncnorm")
    with pytest.raises(ValueError, match="gaussian"):
        TrainBatchBuilder(H, W, "cuda", dzi_type="gaussian")
    with pytest.raises(ValueError, match="img_size"):
        TrainBatchBuilder(H, W, "cuda", img_size=512)
    with pytest.raises(RuntimeError, match="HIP device only"):
        TrainBatchBuilder(H, W, "cpu")
