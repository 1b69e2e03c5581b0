"""GPU: the weight-repack family (include/givepose_repack.h, gpr_*; givepose_amd.repack; PoseNet.set_repack("device")).

Operator: one synthetic table through the entry point against the torch interpreter of tests/repack_ref.py, as bits.  Model: a
device-packed network against its host-packed twin, as bits but for the matrix folds (float64 rule) and for the
channels of the BatchNorm fold whose scale factor the host's torch.sqrt does not round correctly (the fold is held to the correctly
rounded operations' bits everywhere: repack_ref.check_against_host).  In place:
after params_updated() every packed tensor, plan and captured graph is the one it was, and the forward is that of a fresh host-packed
network with the new parameters.  train_step under "device".
"""
import pytest
import torch

import repack_ref as RR
from givepose_amd import PoseNet, PoseNetConfig, _lib, repack

pytestmark = pytest.mark.gpu

SMALL = dict(convnext_depths=(1, 1, 1, 1))
SENTINEL = -7.25
TAIL = 64
# 0, +- fp16 subnormals, +- values below fp16's subnormal range (half of the smallest subnormal, 2^-25, rounds to 0 or to 2^-24 by
# parity: 2^-25 itself ties to even = 0, 1.5 x 2^-25 rounds up), one value that rounds to fp16 infinity, the largest that does not
SPECIAL = [0.0, 3.0e-6, -3.0e-6, 6.1e-8, -6.1e-8, 2.0 ** -25, -(2.0 ** -25), 1.5 * 2.0 ** -25, 1.0e-9, -1.0e-9, 65520.0, 65519.0, -70000.0, -0.0]


def _values(n, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g) * torch.tensor([1.0, 1e-3, 30.0])[torch.arange(n) % 3]
    k = min(n, len(SPECIAL))
    v[:k] = torch.tensor(SPECIAL[:k])
    return v


def _operator_plan():
    """Every view of the issue in all three kinds; the sources, by name, and the plan over them."""
    C = _lib.GPR_CHUNK
    V = repack._View
    shapes = {"oihw": (5, 3, 3, 3), "deconv": (3, 7, 3, 3), "dw": (6, 49), "fc1": (4, 128, 64), "off": (72, 8), "mask": (36, 8),
              "one": (1,), "five": (5,), "long": (C + 1,), "shifted": (2 * C + 3,)}
    views = {"oihw": lambda: V("oihw", shapes["oihw"]).permute(0, 2, 3, 1).reshape(5, 27),
             "deconv": lambda: V("deconv", shapes["deconv"]).permute(2, 3, 1, 0).reshape(27, 7),
             "dw": lambda: V("dw", shapes["dw"]).t(),
             "fc1": lambda: V("fc1", shapes["fc1"]).permute(0, 2, 1).reshape(4, 8192),
             "one": lambda: V("one", (1, 1)), "five": lambda: V("five", (1, 5)), "long": lambda: V("long", (1, C + 1)),
             "shifted": lambda: V("shifted", (1, 2 * C + 3))}
    P = repack.Plan()
    P.sources.update(shapes)
    for kind in (repack.F32, repack.F16, repack.SPLIT):
        for name, make in views.items():
            v = make()
            dims, strides = v.canonical()
            key = f"{name}.{kind}"
            P.dst[key] = (tuple(v.shape), kind)
            P.entries.append(repack.Entry(name, dims, strides, v.offset, key, 0, kind))
        # five | one | long in one row: the long run lands 6 elements into the destination, off the 16-byte grid from an aligned source
        key = f"cat.{kind}"
        P.dst[key] = ((1, 6 + C + 1), kind)
        for name, off in (("five", 0), ("one", 5), ("long", 6)):
            dims, strides = V(name, shapes[name]).canonical()
            P.entries.append(repack.Entry(name, dims, strides, 0, key, off, kind))
        key = f"om.{kind}"
        P.dst[key] = ((128, 8), kind)
        P.zero_filled.add(key)
        for name, off in (("off", 0), ("mask", 72 * 8)):
            dims, strides = V(name, shapes[name]).canonical()
            P.entries.append(repack.Entry(name, dims, strides, 0, key, off, kind))
    return P, shapes


class _Tails:
    """alloc hook of repack.DeviceRepack: TAIL sentinel elements behind every destination."""

    def __init__(self):
        self.bufs = {}

    def __call__(self, key, shape, dtype, zero):
        n = repack._prod(shape)
        whole = torch.full((n + TAIL,), SENTINEL, dtype=dtype, device="cuda")
        if zero:
            whole[:n] = 0
        self.bufs[key] = whole
        return whole[:n].view(shape)

    def check(self):
        for key, whole in self.bufs.items():
            assert bool((whole[-TAIL:] == SENTINEL).all()), key


def test_operator_table_against_the_torch_expression():
    P, shapes = _operator_plan()
    host = {name: _values(repack._prod(shape), 100 + i).reshape(shape) for i, (name, shape) in enumerate(shapes.items())}
    dev = {}
    for name, t in host.items():
        if name == "shifted":                  # 4 bytes off the 16-byte grid
            base = torch.empty(t.numel() + 4, device="cuda")
            dev[name] = base[1:1 + t.numel()]
            dev[name].copy_(t)
            assert dev[name].data_ptr() % 16 == 4 and dev[name].is_contiguous()
        else:
            dev[name] = t.cuda()
            assert dev[name].data_ptr() % 16 == 0
    tails = _Tails()
    rp = repack.DeviceRepack(P, "cuda", alloc=tails)
    want = RR.interpret(P, host)
    assert any(bool(torch.isinf(want[f"long.{k}"].float()).any()) for k in (repack.F16, repack.SPLIT))          # the overflow case is in the data
    sub = want["long.f16"].float().abs()
    assert bool(((sub > 0) & (sub < 2.0 ** -14)).any()) and bool((want["long.f16"][:14] == 0).sum() >= 5)      # subnormals, and values flushed by rounding
    for rep in range(2):                       # the second run rewrites the same tensors from the same tables
        rp.run(dev)
        torch.cuda.synchronize()
        assert rp.uploads == 1
        tails.check()
        for key, (shape, kind) in P.dst.items():
            got = RR.raw(rp.packed[key]).cpu()
            assert got.shape == want[key].shape and got.dtype == want[key].dtype, key
            bits = torch.int16 if got.dtype == torch.float16 else torch.int32
            assert torch.equal(got.view(bits), want[key].view(bits)), (key, rep, int((got.view(bits) != want[key].view(bits)).sum()))
        for kind in (repack.F32, repack.F16, repack.SPLIT):      # the padding rows stay zero
            pad = RR.raw(rp.packed[f"om.{kind}"]).reshape(-1, 128, 8)[:, 108:]
            assert not bool(pad.any())
    # a source that moved: the tables are rebuilt, once
    dev["five"] = dev["five"].clone()
    rp.run(dev)
    rp.run(dev)
    assert rp.uploads == 2
    # refusals of the binding
    with pytest.raises(ValueError, match="device repack: dw"):
        rp.run({**dev, "dw": dev["dw"].t()})
    with pytest.raises(ValueError, match="device repack: one"):
        rp.run({**dev, "one": dev["one"].double()})
    with pytest.raises(ValueError, match="device repack: oihw"):
        rp.run({**dev, "oihw": host["oihw"]})


@pytest.mark.parametrize("mode", ["fp32", "split", "fp16"])
def test_device_packed_model_equals_its_host_packed_twin(mode):
    """Depths (1,1,1,1); the fp16 mode with the fused MLP, whose fc2_wp `_pack` makes with gp_convnext_mlp_pack_w2."""
    kw = {"fp32": dict(dtype=torch.float32), "split": dict(dtype=torch.float32, split_gemm=True), "fp16": dict(dtype=torch.float16)}[mode]
    cfg = PoseNetConfig(**SMALL)
    twin = PoseNet(cfg, seed=5, **kw).cuda()
    net = PoseNet(cfg, seed=None, **kw).cuda()
    net.load_state_dict(twin.state_dict())
    host = twin._pack(torch.device("cuda"))
    got = net.set_repack("device")._pack(torch.device("cuda"))
    torch.cuda.synchronize()
    assert net.repack_count == 1 and twin.repack_count == 0 and net._repacker.launches() == (4 if mode == "fp16" else 3)
    assert ("s0b0.fc2_wp" in host) == (mode == "fp16")
    P = net._repacker.plan
    figures = RR.check_against_host(P, got, host, RR.host_state(twin), where=mode)
    assert len(figures) == (7 if mode == "fp16" else 6)
    with pytest.raises(ValueError, match="device repack: backbone.stem_0.weight"):
        PoseNet(cfg, seed=None, **kw).set_repack("device")._pack(torch.device("cuda"))       # parameters still on the host


# ------------------------------------------------------------------------------------------------ in place, under a captured graph
def _batch():
    from test_xyz_backward_gpu import loss_batch
    data = {k: v[:2] if v.dim() and v.shape[0] == 4 else v for k, v in loss_batch().items()}
    return data, {**data, "roi_mask": data["roi_mask_deform"]}


def _tensors(out):
    return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}


@torch.no_grad()
def _move_parameters(net):
    """Changes every parameter and the BatchNorm statistics through their storage: data_ptr stays."""
    ptrs = [p.data_ptr() for p in net.parameters()]
    for i, p in enumerate(net.parameters()):
        p.mul_(1.0 + 0.01 * ((i % 5) - 2)).add_(1e-3)
    sd = net.state_dict()
    sd["size_head.bn1.running_var"].mul_(1.3).add_(0.1)
    sd["size_head.bn1.running_mean"].add_(0.05)
    assert ptrs == [p.data_ptr() for p in net.parameters()]


def _fresh_forward(net, cfg, fdata, **kw):
    """The forward of a fresh host-packed PoseNet loaded with net's state dict, after the matrix-fold keys were copied over from net."""
    fresh = PoseNet(cfg, seed=None, **kw).cuda()
    fresh.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    fresh._pack(torch.device("cuda"))
    assert fresh._repack_mode == "host" and set(fresh._packed) == set(net._packed)
    for key in repack.MATRIX_FOLD_KEYS:
        if key in fresh._packed:
            RR.raw(fresh._packed[key]).copy_(RR.raw(net._packed[key]))
    # the BatchNorm fold of the CURRENT statistics: the correctly rounded fold's bits, which are the fresh `_pack`'s in every channel whose scale
    # factor the host's torch.sqrt rounds correctly (repack_ref.host_exact_channels); the other channels are taken over like the matrix folds
    P, sd = net._repacker.plan, RR.host_state(net)
    ieee, exact = RR.bn_fold_ieee(P, sd), RR.host_exact_channels(P, sd)
    assert int(exact.sum()) > exact.numel() // 2
    for key in RR.BN_FOLD_KEYS:
        dev, host = net._packed[key].cpu(), fresh._packed[key].cpu()
        assert torch.equal(dev.view(torch.int32), ieee[key].reshape(dev.shape).view(torch.int32)), key
        assert torch.equal(dev[exact].view(torch.int32), host[exact].view(torch.int32)), key
        fresh._packed[key].copy_(net._packed[key])
    return _tensors(fresh.forward_device(fdata, "cuda"))


def _graph_state(net):
    return ({k: RR.raw(v).data_ptr() for k, v in net._packed.items()}, {k: id(p) for k, p in net._plans.items()},
            {k: p["graph"].value for k, p in net._plans.items()}, {k: {n: b.data_ptr() for n, b in p["buf"].items() if torch.is_tensor(b)} for k, p in net._plans.items()})


@pytest.mark.parametrize("inflight", [1, 2])
def test_params_updated_repacks_in_place_under_a_captured_graph(inflight):
    from test_xyz_backward_gpu import same_bits
    cfg = PoseNetConfig(**SMALL)
    kw = dict(dtype=torch.float16, use_graph=True, inflight=inflight)
    net = PoseNet(cfg, seed=9, **kw).cuda().set_repack("device")
    _, fdata = _batch()
    slots = list(range(inflight))
    for slot in slots:
        for _ in range(2):                     # the second forward captures the graph
            net.forward_device(fdata, "cuda", slot=slot)
    fwd0 = _tensors(net.forward_device(fdata, "cuda", slot=0))
    state = _graph_state(net)
    assert net.repack_count == 1 and len(net._plans) == inflight and all(g for g in state[2].values())
    if inflight == 2:                          # a forward still in flight on its slot stream when the weights are about to change
        pending = net.forward_device(fdata, "cuda", slot=0, wait=False)
    _move_parameters(net)
    net.params_updated()
    assert net.repack_count == 2 and _graph_state(net) == state and net._repacker.uploads == 1
    fwd1 = _tensors(net.forward_device(fdata, "cuda", slot=slots[-1]))
    if inflight == 2:
        torch.cuda.current_stream().wait_stream(net.stream(0))
        same_bits(_tensors(pending), fwd0, "the forward issued before the update")
    assert _graph_state(net) == state
    assert any(not torch.equal(fwd0[k], fwd1[k]) for k in fwd0)
    same_bits(_fresh_forward(net, cfg, fdata, **kw), fwd1, "forward after params_updated()")
    # load_state_dict still resets everything, and the next forward packs on the device again
    net.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
    assert net._packed is None and net._repacker is None and not net._plans and net._repack_mode == "device"
    same_bits(_tensors(net.forward_device(fdata, "cuda", slot=0)), fwd1, "forward after load_state_dict")
    assert net.repack_count == 3


# ------------------------------------------------------------------------------------------------ train_step
def test_train_step_with_the_size_head_repacks_on_the_device():
    """B = 2, fp32, size_head={"seed": s}: the step moves every parameter and bn1's running statistics (the BatchNorm fold); the forward
    after it is that of a fresh host-packed network with the new state dict."""
    import bb_backward_ref as B
    from givepose_amd import PoseLoss, Ranger
    from test_xyz_backward_gpu import same_bits
    cfg = PoseNetConfig(**SMALL)
    net = PoseNet(cfg, dtype=torch.float32, seed=B.WEIGHT_SEED).cuda().set_repack("device")
    data, fdata = _batch()
    opt = Ranger(net)
    fwd0 = _tensors(net.forward_device(fdata, "cuda"))
    ptrs = {k: RR.raw(v).data_ptr() for k, v in net._packed.items()}
    plans = {k: id(p) for k, p in net._plans.items()}
    mean0 = net.state_dict()["size_head.bn1.running_mean"].clone()
    assert net.repack_count == 1
    net.train_step(data, PoseLoss(), opt, "cuda", size_head={"seed": 7})
    assert net.repack_count == 3               # the step's own call, and the one after the running statistics moved
    assert not torch.equal(net.state_dict()["size_head.bn1.running_mean"], mean0)
    assert ptrs == {k: RR.raw(v).data_ptr() for k, v in net._packed.items()} and plans.items() <= {k: id(p) for k, p in net._plans.items()}.items()
    fwd1 = _tensors(net.forward_device(fdata, "cuda"))
    assert any(not torch.equal(fwd0[k], fwd1[k]) for k in fwd0)
    same_bits(_fresh_forward(net, cfg, fdata, dtype=torch.float32), fwd1, "forward after the step")


def test_a_micro_step_without_a_step_leaves_the_packed_weights_alone():
    import bb_backward_ref as B
    from givepose_amd import GradAccumulator, PoseLoss, Ranger
    from test_xyz_backward_gpu import same_bits
    cfg = PoseNetConfig(**SMALL)
    net = PoseNet(cfg, dtype=torch.float32, seed=B.WEIGHT_SEED).cuda().set_repack("device")
    data, fdata = _batch()
    opt = Ranger(net)
    acc = GradAccumulator(opt)
    net.forward_device(fdata, "cuda")
    packed0 = {k: RR.raw(v).clone() for k, v in net._packed.items()}
    res = net.train_step(data, PoseLoss(), opt, "cuda", accumulator=acc, accumulate=2, micro_step=1)
    assert res["stepped"] is False and net.repack_count == 1
    same_bits({k: RR.raw(v) for k, v in net._packed.items()}, packed0, "packed weights after the micro-step without a step")
    res = net.train_step(data, PoseLoss(), opt, "cuda", accumulator=acc, accumulate=2, micro_step=2)
    assert res["stepped"] is True and net.repack_count == 2
    assert any(not torch.equal(RR.raw(v), packed0[k]) for k, v in net._packed.items())
    same_bits(_fresh_forward(net, cfg, fdata, dtype=torch.float32), _tensors(net.forward_device(fdata, "cuda")), "forward after the step")
