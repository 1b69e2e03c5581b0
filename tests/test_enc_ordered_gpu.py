"""GPU: the ordered d xp of the encoder's DCNv3 core (include/givepose_encgrad_ordered.h, gpeo_*; enc_grad's scatter="ordered";
PoseNet.set_encoder_scatter): bit-equal to the numpy float32 restatement of its contract (tests/enc_ordered_ref.py), equal bits between
two launches at every level up to train_step, and the same accuracy yardsticks as the atomic mode.

Bounds.  d xp of the two modes: both lie within the per-element grad_input bound of tests/dcnv3_backward_reference.py of float64 -- the
bound counts n - 1 additions in ANY order -- so they differ by at most twice that bound, and by exactly nothing where the bound is 0.
The encoder: the float64-at-the-device's-gates yardstick of tests/test_enc_backward_gpu.py::test_encoder_end_to_end (8 x the CPU float32
figure), and between the modes 16 fig32 max|.|, the bound that file uses between two atomic runs (each within 8 x of the reference).
"""
import functools

import numpy as np
import pytest
import torch

import dcnv3_backward_reference as DB
import dcnv3_reference as DR
import enc_backward_cases as C
import enc_backward_ref as R
import enc_ordered_ref as O
from test_enc_backward_gpu import CORE_EDGE_CASES, cuda, device_gates, device_params, yardstick
from test_xyz_backward_gpu import Guarded, bits, same_bits

pytestmark = pytest.mark.gpu
T = torch.from_numpy


# ------------------------------------------------------------------------------------------------ the core
def _edge(c):
    I = DR.inputs(c)
    rows = DR.n_rows(c)
    return (I["x"].numpy(), I["off"].view(rows, 72).numpy(), I["mask"].view(rows, 36).numpy(), DB.grad_output(c).numpy()), (c.N, c.H, c.W)


CORE_CASES = {
    "1x1x1": lambda: (O.random_case(1, 1, 1, seed=21), (1, 1, 1)),
    "edges-2x5x8": lambda: _edge(CORE_EDGE_CASES[0]),
    "c3-1x7x4": lambda: _edge(CORE_EDGE_CASES[1]),
    "random-3x8x8": lambda: (O.random_case(3, 8, 8, seed=22, scale=2.0), (3, 8, 8)),
    "pile-up-1x16x16": lambda: (O.pile_up_case(), (1, 16, 16)),
    "threshold-1x8x8": lambda: (O.threshold_case(), (1, 8, 8)),      # lists of exactly 64 and 65 ids: the gather's two paths meet
}


@pytest.mark.parametrize("name", list(CORE_CASES))
def test_core_ordered_is_the_restatement_bit_for_bit(name):
    from givepose_amd import enc_grad
    assert (CORE_EDGE_CASES[0].N, CORE_EDGE_CASES[0].H, CORE_EDGE_CASES[0].W, CORE_EDGE_CASES[0].iset) == (2, 5, 8, "edges")
    assert (CORE_EDGE_CASES[1].N, CORE_EDGE_CASES[1].H, CORE_EDGE_CASES[1].W) == (1, 7, 4)
    (xp, off, logits, dy), (N, H, W) = CORE_CASES[name]()
    guard = Guarded()
    xp_, off_, logits_, dy_ = cuda(xp, off, logits, dy)
    fw = enc_grad.dcnv3_core_forward(xp_, off_, logits_, alloc=guard)
    atomic = enc_grad.dcnv3_core_backward(xp_, off_, fw["mask"], dy_, alloc=guard)
    ordered = enc_grad.dcnv3_core_backward(xp_, off_, fw["mask"], dy_, alloc=guard, scatter="ordered")
    again = enc_grad.dcnv3_core_backward(xp_, off_, fw["mask"], dy_, alloc=guard, scatter="ordered")
    guard.check()      # every element of d xp written, nothing outside any buffer or the workspace
    mask = fw["mask"].cpu().numpy()      # the mask the device's forward saved
    want, lengths = O.ordered_dxp(off, mask, dy, N, H, W)
    got = ordered["dxp"].cpu().numpy()
    differ = int((got.view(np.int32) != want.view(np.int32)).sum())
    c = DR.mk(f"ordered-{name}", torch.float32, N=N, H=H, W=W, s=2, entry="any")
    v, bound = (t.numpy() for t in DB.ref(dict(x=T(xp), off=T(off).reshape(-1), mask=T(mask).reshape(-1), gout=T(dy)), c)["grad_input"])
    between = np.abs(got.astype(np.float64) - atomic["dxp"].cpu().numpy().astype(np.float64))
    err = np.abs(got.astype(np.float64) - v)
    print(f"ORDERED {name}: {differ} of {got.size} elements differ from the restatement; lists 0..{lengths.max()} ({(lengths == 0).sum()} empty, "
          f"{(lengths > 64).sum()} longer than 64); |ordered - atomic| / (2 bound) {np.max(between / np.maximum(2 * bound, 1e-300)):.3f}; "
          f"|ordered - float64| / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert differ == 0
    assert np.all(between <= 2 * bound) and np.all(err <= bound) and bool((bound > 0).any())
    for k in ("doffset", "dmask_logits"):      # the existing code's, the same bits in both modes
        assert torch.equal(bits(ordered[k]), bits(atomic[k])), k
    same_bits(ordered, again, "a second ordered launch")
    empty = np.repeat(lengths == 0, 64, axis=-1).reshape(got.shape)
    assert np.all(got[empty].view(np.int32) == 0)      # +0, not -0
    if name == "pile-up-1x16x16":
        assert lengths.max() == 576 > 64 and (lengths == 576).sum() == 16 and (lengths == 0).sum() == lengths.size - 16
        assert np.any(got[0, 2:4, 3:5] != 0) and not np.any(np.delete(got.reshape(256, 256), [2 * 16 + 3, 2 * 16 + 4, 3 * 16 + 3, 3 * 16 + 4], 0))
    if name == "random-3x8x8":
        assert (lengths == 1).any() and (lengths >= 2).any() and (lengths == 0).any() and lengths.max() <= 64
    if name == "1x1x1":
        assert lengths.shape == (1, 1, 1, 4)
    if name == "threshold-1x8x8":
        assert all(np.all(lengths[0, 2:4, 3:5, g] == n) for g, n in enumerate((64, 65, 63, 1))) and lengths.sum() == 4 * (64 + 65 + 63 + 1)


# ------------------------------------------------------------------------------------------------ the encoder
def run_encoder(case, groups=None, g_scale=1.0, guard=None, scatter="ordered"):
    from givepose_amd import enc_grad
    _, coor, g = R.case_inputs(case)
    c, gf = T(coor).cuda(), T(g).cuda() * g_scale
    saved = enc_grad.enc_forward_save(c, device_params(), groups=groups, alloc=guard)
    grads, g_coor = enc_grad.enc_backward(device_params(), saved, c, gf, alloc=guard, scatter=scatter)
    torch.cuda.synchronize()
    return {**grads, "coor": g_coor, "nocs_feat": torch.cat([s["act"][2] for s in saved])}, saved


@functools.lru_cache(maxsize=None)
def ordered_run(case, groups):
    """The ordered mode's result of a case, computed once and left unchanged."""
    guard = Guarded()
    got, saved = run_encoder(case, groups, guard=guard)
    guard.check()
    return got, saved


ENC_CASES = [(c, None) for c in R.CASES] + [R.GROUPED]
ids = lambda v: str(v).replace(" ", "")


@pytest.mark.parametrize("case,groups", ENC_CASES, ids=ids)
def test_encoder_ordered_repeats_and_is_linear_bit_for_bit(case, groups):
    from givepose_amd import enc_grad
    a, _ = ordered_run(case, groups)
    b, _ = run_encoder(case, groups)
    assert list(a) == enc_grad.ORDERED_FREE_KEYS + ["coor", "nocs_feat"] and len(a) == 50
    same_bits(a, b, f"{case} {groups} twice")
    twice, _ = run_encoder(case, groups, g_scale=2.0)
    zero, _ = run_encoder(case, groups, g_scale=0.0)
    for k in a:
        if k != "nocs_feat":
            assert torch.equal(bits(twice[k]), bits(a[k] * 2)), k      # every tensor x 2, bit for bit
            assert not bits(zero[k].abs()).any(), k                    # exact zeros
            assert bool(a[k].abs().max() > 0), k


@pytest.mark.parametrize("case,groups", ENC_CASES, ids=ids)
def test_encoder_ordered_against_float64_and_the_atomic_mode(case, groups):
    B, R_ = case
    r64, _, fig32, margins = C.reference(case, groups)
    got, saved = ordered_run(case, groups)
    glist = list(groups) if groups else [B]
    gates = device_gates(saved, glist, R_)
    total, inside, bad = C.gate_disagreements(gates, r64, margins)
    assert bad == 0
    params, coor, g = R.case_inputs(case)
    ref = R.enc_run(params, coor, g, groups=groups, gates=gates)
    want = {**ref["grads"], "coor": ref["coor"], "nocs_feat": ref["nocs_feat"]}
    worst = yardstick({k: v.cpu().numpy() for k, v in got.items()}, want, {k: want[k] * (1 + fig32[k]) for k in want}, f"ordered {case} {groups}")
    print(f"ordered {case} {groups}: largest ratio {worst:.2f}")
    atomic, asaved = run_encoder(case, groups, scatter="atomic")
    same_bits(saved, asaved, "saved")      # the forward is the same code
    far = 0.0
    for k in got:
        tol = 16 * fig32[k] * float(np.max(np.abs(want[k])))
        d = float((got[k] - atomic[k]).abs().max())
        far = max(far, d / tol)
        assert d <= tol, (k, d, tol)
    print(f"ordered {case} {groups}: largest |ordered - atomic| / (16 fig32 max|.|) {far:.3f}")


# ------------------------------------------------------------------------------------------------ the chain
def _chain_batch(n):
    from test_xyz_backward_gpu import loss_batch
    return {k: v[:n] if v.dim() and v.shape[0] == 4 else v for k, v in loss_batch().items()}


def _shapes(res):
    if isinstance(res, dict):
        return {k: _shapes(v) for k, v in res.items()}
    return tuple(res.shape) if torch.is_tensor(res) else type(res).__name__


def test_head_grads_feat_ordered_twice_and_back_to_atomic():
    import pose_loss_grad_ref as G
    from givepose_amd import PoseLoss, PoseNet, PoseNetConfig
    net = PoseNet(PoseNetConfig(), seed=R.WEIGHT_SEED, dtype=torch.float32).cuda()
    untouched = PoseNet(PoseNetConfig(), seed=R.WEIGHT_SEED, dtype=torch.float32).cuda()
    data, pl, w, groups = _chain_batch(3), PoseLoss(), T(G.make_gout()), [1, 2]
    assert net.set_encoder_scatter("ordered").encoder_scatter == "ordered"
    a = net.head_grads_feat(data, pl, "cuda", gout=w, groups=groups)
    b = net.head_grads_feat(data, pl, "cuda", gout=w, groups=groups)
    torch.cuda.synchronize()
    same_bits(a, b, "head_grads_feat")      # every entry: loss, output, grads, param_grads
    assert sum(k.startswith("nocs_encoder.") for k in a["param_grads"]) == 48
    net.set_encoder_scatter("atomic")
    back = net.head_grads_feat(data, pl, "cuda", gout=w, groups=groups)
    base = untouched.head_grads_feat(data, pl, "cuda", gout=w, groups=groups)
    torch.cuda.synchronize()
    assert _shapes(back) == _shapes(base) == _shapes(a)
    # the forward is the same code in both modes
    same_bits(back["loss"], base["loss"], "loss")
    same_bits(a["loss"], base["loss"], "loss")
    same_bits(a["output"], base["output"], "output")


def test_train_step_ordered_gives_equal_bits_from_the_same_state():
    """Two networks built from the same seed, each with its own Ranger, one train_step each on the same batch with the train-mode size
    head at a fixed seed: every parameter, every buffer, Ranger's state and the two clip scalars are equal bit for bit."""
    from givepose_amd import PoseLoss, Ranger
    from test_size_train_gpu import small_net_and_batch
    runs = []
    for _ in range(2):
        _, net, data = small_net_and_batch()
        assert data["roi_img"].shape[0] == 2
        opt = Ranger(net.set_encoder_scatter("ordered"))
        res = net.train_step(data, PoseLoss(), opt, "cuda", size_head={"seed": 7})
        torch.cuda.synchronize()
        runs.append(({k: v.detach().clone() for k, v in net.state_dict().items()}, opt.state_dict()["state"], opt.scalars.clone(),
                     res["param_grads"], res["loss"], res["grads"]))
    (sd_a, st_a, sc_a, pg_a, loss_a, g_a), (sd_b, st_b, sc_b, pg_b, loss_b, g_b) = runs
    same_bits(pg_a, pg_b, "param_grads")
    same_bits(g_a, g_b, "grads")
    same_bits(loss_a, loss_b, "loss")
    same_bits(sd_a, sd_b, "state_dict")
    assert list(st_a) == list(st_b) and len(st_a) > 100
    same_bits(st_a, st_b, "Ranger state")
    same_bits(sc_a, sc_b, "clip scalars")
    assert float(sc_a[0]) > 0 and any(k.startswith("nocs_encoder.") for k in pg_a)
