"""GPU: every gp_sn_* entry point (csrc/scalenet.hip) on its own against the float64 reference and the per-element bound of
tests/ops_reference.py, called the way givepose_amd/scale_net.py calls them.  Scale_net's own tests read one scalar per image behind two
global average pools and three Linear layers; here every output element of every kernel is checked, at odd maps, partial tiles and
image boundaries inside a tile.

Every case: the output buffer is NaN with one more row of sentinels behind it; every element within its bound (the worst ratio and its
index are printed on failure) and the sentinels intact; a second launch gives the same bits.  The inputs, cases and bounds are the ones
tests/test_ops_reference_cpu.py has already checked on the CPU.  The largest ratios of an MI355X run: profiles/op_conformance.txt."""
import ctypes

import pytest
import torch

import ops_reference as R

pytestmark = pytest.mark.gpu


def _lib():
    from givepose_amd import _lib as L
    return L


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(I):
    return {k: v.cuda().contiguous() for k, v in I.items()}


def run_case(what, v, bound, launch, dtype=torch.float32):
    """launch(buf) writes v.numel() values at the front of buf.  Returns the largest err / bound."""
    n, row = v.numel(), v.shape[-1] if v.dim() > 1 else 1
    bufs = []
    for _ in range(2):
        buf = torch.full((n + row,), R.NAN, dtype=dtype, device="cuda")
        buf[n:] = R.SENTINEL
        launch(buf)
        torch.cuda.synchronize()
        bufs.append(buf)
    ratio, msg = R.check_buffer(bufs[0], v, bound, what)
    print(f"GPU_RATIO {what} {ratio:.4f}")
    assert msg is None, msg
    ints = torch.int16 if dtype == torch.float16 else torch.int32
    assert torch.equal(bufs[0].view(ints), bufs[1].view(ints)), f"{what}: a second launch gives other bits"
    return ratio


def _refused(rc):
    assert rc == -1, rc          # GP_ERR_INVALID, before any launch
    assert _lib().load().gp_last_error()


# ------------------------------------------------------------------------------------------------ gp_sn_stem
@pytest.mark.parametrize("case", R.SN_STEM_CASES, ids=R.case_id)
def test_sn_stem(case):
    L, lib = _lib(), _lib().load()
    B, H, W = case
    I = R.sn_stem_inputs(case)
    assert all(R.act_branches(R.sn_stem_pre(I)[0], 2))
    v, bound = R.sn_stem_ref(I, case)
    D = _dev(I)
    run_case(f"gp_sn_stem {R.case_id(case)}", v, bound,
             lambda y: L.check(lib.gp_sn_stem(_p(D["img"]), _p(D["w"]), _p(D["b"]), _p(y), B, H, W, _st()), "gp_sn_stem"))


def test_sn_stem_refuses_odd_height():
    lib = _lib().load()
    D = _dev(R.sn_stem_inputs(R.SN_STEM_CASES[0]))
    y = torch.zeros(2 * 4 * 5 * 16, device="cuda")
    _refused(lib.gp_sn_stem(_p(D["img"]), _p(D["w"]), _p(D["b"]), _p(y), 1, 7, 10, _st()))


# ------------------------------------------------------------------------------------------------ gp_sn_pointwise
@pytest.mark.parametrize("case", R.SN_PW_CASES, ids=R.case_id)
def test_sn_pointwise(case):
    L, lib = _lib(), _lib().load()
    M, N, K, HW, act, se, res = case
    I = R.sn_pw_inputs(case)
    if M * N >= R.BRANCH_MIN_VALUES:
        assert all(R.act_branches(R.sn_pw_pre(I, case)[0], act))
    if se:
        assert float((I["se"][1:] - I["se"][:-1]).abs().max(1).values.min()) > 0.3       # the gates of neighbouring images differ clearly
    v, bound = R.sn_pw_ref(I, case)
    D = _dev(I)
    run_case(f"gp_sn_pointwise {R.case_id(case)}", v, bound,
             lambda y: L.check(lib.gp_sn_pointwise(_p(D["x"]), _p(D["w"]), _p(D["b"]), _p(D["se"]) if se else None, _p(D["res"]) if res else None, _p(y),
                                                   M, N, K, HW, act, _st()), "gp_sn_pointwise"))


@pytest.mark.parametrize("M,N,K,HW", [(70, 6, 16, 35), (70, 24, 5, 35), (70, 24, 16, 32)])
def test_sn_pointwise_refuses(M, N, K, HW):
    lib = _lib().load()
    x, w, b, y = (torch.zeros(s, device="cuda") for s in (M * 16, 24 * 16, 24, M * 24))
    _refused(lib.gp_sn_pointwise(_p(x), _p(w), _p(b), None, None, _p(y), M, N, K, HW, 0, _st()))


# ------------------------------------------------------------------------------------------------ gp_sn_depthwise
@pytest.mark.parametrize("case", R.SN_DW_CASES, ids=R.case_id)
def test_sn_depthwise(case):
    L, lib = _lib(), _lib().load()
    B, H, W, C, KS, stride, act = case
    I = R.sn_dw_inputs(case)
    v, bound = R.sn_dw_ref(I, case)
    assert tuple(v.shape) == (B, -(-H // stride), -(-W // stride), C)                   # ceil(H / stride)
    if v.numel() >= R.BRANCH_MIN_VALUES:
        assert all(R.act_branches(R.sn_dw_pre(I, case)[0], act))
    D = _dev(I)
    run_case(f"gp_sn_depthwise {R.case_id(case)}", v, bound,
             lambda y: L.check(lib.gp_sn_depthwise(_p(D["x"]), _p(D["w"]), _p(D["b"]), _p(y), B, H, W, C, KS, stride, act, _st()), "gp_sn_depthwise"))


@pytest.mark.parametrize("C,KS,stride", [(6, 3, 1), (4, 7, 1), (4, 3, 3)])
def test_sn_depthwise_refuses(C, KS, stride):
    lib = _lib().load()
    x, w, b, y = (torch.zeros(s, device="cuda") for s in (2 * 8 * 8 * 8, 49 * 8, 8, 2 * 8 * 8 * 8))
    _refused(lib.gp_sn_depthwise(_p(x), _p(w), _p(b), _p(y), 2, 8, 8, C, KS, stride, 0, _st()))


# ------------------------------------------------------------------------------------------------ gp_sn_avgpool
@pytest.mark.parametrize("case", R.SN_POOL_CASES, ids=R.case_id)
def test_sn_avgpool(case):
    L, lib = _lib(), _lib().load()
    B, HW, C = case
    I = R.sn_pool_inputs(case)
    v, bound = R.sn_pool_ref(I, case)
    D = _dev(I)
    run_case(f"gp_sn_avgpool {R.case_id(case)}", v, bound, lambda y: L.check(lib.gp_sn_avgpool(_p(D["x"]), _p(y), B, HW, C, _st()), "gp_sn_avgpool"))


# ------------------------------------------------------------------------------------------------ gp_sn_se
@pytest.mark.parametrize("case", R.SN_SE_CASES, ids=R.case_id)
def test_sn_se(case):
    L, lib = _lib(), _lib().load()
    B, C, S = case
    I = R.sn_se_inputs(case)
    v, bound = R.sn_se_ref(I, case)
    assert bool((v == 0).any()) and bool((v == 1).any()) and bool(((v > 0) & (v < 1)).any())     # closed, open and in between
    D = _dev(I)
    run_case(f"gp_sn_se {R.case_id(case)}", v, bound,
             lambda y: L.check(lib.gp_sn_se(_p(D["pooled"]), _p(D["w1"]), _p(D["b1"]), _p(D["w2"]), _p(D["b2"]), _p(y), B, C, S, _st()), "gp_sn_se"))


@pytest.mark.parametrize("C,S", [(580, 8), (16, 161)])
def test_sn_se_refuses(C, S):
    lib = _lib().load()
    t = torch.zeros(580 * 161, device="cuda")
    _refused(lib.gp_sn_se(_p(t), _p(t), _p(t), _p(t), _p(t), _p(t), 1, C, S, _st()))


# ------------------------------------------------------------------------------------------------ gp_sn_head
def _head(lib, D, y, B, F, FD, NC, use_hw):
    return lib.gp_sn_head(_p(D["f_roi"]), _p(D["f_full"]), _p(D["one_hot"]), _p(D["roi_wh"]), _p(D["mean_size"]), _p(D["w1"]), _p(D["b1"]), _p(D["w2"]),
                          _p(D["b2"]), _p(D["w3"]), _p(D["b3"]), _p(y), B, F, FD, NC, use_hw, _st())


@pytest.mark.parametrize("case", R.SN_HEAD_CASES, ids=R.case_id)
def test_sn_head(case):
    L, lib = _lib(), _lib().load()
    B, FD, NC, use_hw = case
    I = R.sn_head_inputs(case)
    if not use_hw:
        assert bool((I["roi_wh"] == 1e6).all())          # read by mistake, they would move the result by thousands
    v, bound = R.sn_head_ref(I, case)
    D = _dev(I)
    run_case(f"gp_sn_head {R.case_id(case)}", v, bound, lambda y: L.check(_head(lib, D, y, B, R.SN_HEAD_F, FD, NC, use_hw), "gp_sn_head"))


@pytest.mark.parametrize("F,FD,NC", [(512, 8, 6), (576, 65, 6), (576, 8, 17)])
def test_sn_head_refuses(F, FD, NC):
    lib = _lib().load()
    D = _dev(R.sn_head_inputs(R.SN_HEAD_CASES[0]))
    _refused(_head(lib, D, torch.zeros(4, device="cuda"), 3, F, FD, NC, 1))
