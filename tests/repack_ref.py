"""A torch interpreter of givepose_amd.repack.plan: what the gpr_ kernels must compute, on the host.

Views are `as_strided`, the fp16 kind is `.half()` (round to nearest even), the split kind is the expression of ops.split_weights, the
BatchNorm fold is `_pack`'s fp32 expression with every operation correctly rounded, and a matrix fold is a float64 product rounded once.  `matrix_fold_refs` gives the
unrounded float64 value of every matrix-fold key, and `stored64` what a packed tensor holds, as float64.
"""
import torch

from givepose_amd import repack
from givepose_amd.ops import SPLIT_SHIFT, SplitW
from givepose_amd.posenet import enc0_xyz_pack


def host_state(net):
    return {k: v.detach().to(device="cpu", dtype=torch.float32).contiguous() for k, v in net.state_dict().items() if v.is_floating_point()}


def _flat_view(t, dims, strides, offset):
    return torch.as_strided(t.reshape(-1), tuple(dims), tuple(strides), offset)


def interpret(P, sd):
    """plan, {state-dict name: fp32 CPU tensor} -> {packed key: tensor}; a split key is its (2, N, K) fp16 planes."""
    scratch = {k: torch.zeros(shape, dtype=torch.float64 if dt == "f64" else torch.float32) for k, (shape, dt) in P.scratch.items()}

    def src(name):
        return scratch[name[len(repack.FOLD):]] if name.startswith(repack.FOLD) else sd[name]

    for f in P.bnfolds:             # `_pack`'s fp32 expression with every operation correctly rounded (see host_exact_channels)
        ieee = bn_fold_ieee(P, sd)
        scratch[f.w_out].copy_(ieee["size.w1"])
        scratch[f.b_out].copy_(ieee["size.b1"])
    for level in (0, 1):
        for f in P.matfolds:
            if f.level != level:
                continue
            assert src(f.B).dtype == (torch.float64 if f.b_f64 else torch.float32)
            a = _flat_view(src(f.A), (f.M, f.K), (f.a_rs, 1), f.a_off).double()
            b = _flat_view(src(f.B), (f.K, f.N), (f.b_rs, 1), f.b_off).double()
            r = a @ b
            if f.add is not None:
                r = r + src(f.add).double().reshape(-1)[:f.M, None]
            _flat_view(scratch[f.out32], (f.M, f.N), (f.ld32, 1), f.o32_off).copy_(r.float())
            if f.out64 is not None:
                _flat_view(scratch[f.out64], (f.M, f.N), (f.ld64, 1), f.o64_off).copy_(r)
    out = {}
    for key, (shape, kind) in P.dst.items():
        if kind == repack.SPLIT:
            out[key] = torch.zeros((2,) + tuple(shape), dtype=torch.float16)
        else:
            out[key] = torch.zeros(shape, dtype=torch.float16 if kind == repack.F16 else torch.float32)
    written = {key: torch.zeros(repack._prod(shape), dtype=torch.bool) for key, (shape, _) in P.dst.items()}
    for e in P.entries:
        v = _flat_view(src(e.src), e.dims, e.strides, e.offset).reshape(-1)
        n, o = v.numel(), e.dst_off
        assert not written[e.dst][o:o + n].any(), e          # no element of a destination is written twice
        written[e.dst][o:o + n] = True
        if e.kind == repack.F32:
            out[e.dst].view(-1)[o:o + n] = v
        elif e.kind == repack.F16:
            out[e.dst].view(-1)[o:o + n] = v.half()
        else:
            hi = v.half()
            planes = out[e.dst].view(2, -1)
            planes[0, o:o + n] = hi
            planes[1, o:o + n] = ((v - hi.float()) * float(2 ** SPLIT_SHIFT)).half()
    for key, w in written.items():
        assert bool(w.all()) != (key in P.zero_filled), key  # exactly the zero-filled keys keep unwritten (padding) elements
    return out


def raw(t):
    """A packed value as a plain tensor: the planes of a SplitW."""
    return t.planes if isinstance(t, SplitW) else t


def stored64(t):
    """What a packed tensor holds, as float64 on the host (split planes: hi + 2^-shift lo')."""
    t = raw(t).detach().cpu()
    if t.dim() == 3 and t.shape[0] == 2 and t.dtype == torch.float16:
        return t[0].double() + t[1].double() * 2.0 ** -SPLIT_SHIFT
    return t.double()


def is_split(P, key):
    return P.dst[key][1] == repack.SPLIT


def matrix_fold_refs(P, sd):
    """{matrix-fold key: unrounded float64 value} for the keys of this plan."""
    refs = {}
    for li, i in enumerate((0, 3, 6)):
        p = f"nocs_encoder.features.{i}."
        iw, ib = sd[p + "dcnv3.input_proj.weight"].double(), sd[p + "dcnv3.input_proj.bias"].double()
        cw, cb = sd[p + "conv.weight"].double().reshape(256, -1), sd[p + "conv.bias"].double()
        refs[f"enc{li}.fold_w"], refs[f"enc{li}.fold_b"] = iw @ cw, iw @ cb + ib
    if "enc0.xyz_m" in P.dst:
        refs["enc0.xyz_m"] = enc0_xyz_pack(sd, "nocs_encoder.features.0.", dtype=torch.float64)[0]
    return {k: v for k, v in refs.items() if k in P.dst}


BN_FOLD_KEYS = ("size.w1", "size.b1")


def _r32(x64):
    """One IEEE rounding of a float64 result to float32.  For +, -, x, / and sqrt of float32 operands, computing in float64 and rounding
    again is the correctly rounded float32 operation (53 >= 2 x 24 + 2 bits: the double rounding is innocuous)."""
    return x64.float().double()


def bn_fold_ieee(P, sd):
    """`_pack`'s BatchNorm fold -- sc = w / sqrt(var + 1e-5); w1 = conv_w sc; b1 = (conv_b - mean) sc + beta -- with every operation the
    correctly rounded float32 one: what `_pack` computes on a host whose torch rounds +, -, x, / and sqrt correctly, and what the
    device computes.  -> {packed key: fp32 tensor}."""
    (f,) = P.bnfolds
    d = lambda name: sd[name].double()
    eps = torch.tensor(f.eps, dtype=torch.float32).double()
    sc = _r32(d(f.bn_w) / _r32(torch.sqrt(_r32(d(f.var) + eps))))
    w1 = _r32(d(f.w).reshape(f.C, f.K) * sc[:, None])
    b1 = _r32(_r32(_r32(d(f.b) - d(f.mean)) * sc) + d(f.bn_b))
    return {"size.w1": w1.float(), "size.b1": b1.float()}


def host_exact_channels(P, sd):
    """The channels whose scale factor this host's torch computes as the correctly rounded one.  torch.sqrt on the CPU is not a correctly
    rounded operation: it misses by an ulp in a share of its inputs, and which inputs depends on the CPU, so `_pack`'s
    size.w1 / size.b1 are not one set of bits.  +, - and x are correctly rounded everywhere, which is asserted here."""
    (f,) = P.bnfolds
    var, w, b, mean, beta = sd[f.var], sd[f.bn_w], sd[f.b], sd[f.mean], sd[f.bn_b]
    eps = torch.tensor(f.eps, dtype=torch.float32)
    t = var + f.eps
    sc = w / torch.sqrt(t)
    dm = b - mean
    pr = dm * sc
    assert torch.equal(t, (var.double() + eps.double()).float()) and torch.equal(dm, (b.double() - mean.double()).float())
    assert torch.equal(pr, (dm.double() * sc.double()).float()) and torch.equal(pr + beta, (pr.double() + beta.double()).float())
    return sc == _r32(w.double() / _r32(torch.sqrt(t.double()))).float()


def fold_error(value, ref64):
    """max|value - ref64| / max|ref64| of a stored matrix fold."""
    return float((stored64(value).reshape(ref64.shape) - ref64).abs().max() / ref64.abs().max())


def check_against_host(P, got, host, sd, where=""):
    """`got` (device repack or interpreter) against `host` (`_pack`): key set, shapes, dtypes, bits for every key but the matrix folds,
    and the project's float64 rule for those: the error is at most 8 times `_pack`'s own, never held below 2^-24.  Returns the figures.
    The BatchNorm fold (size.w1 / size.b1) is held to the bits of the correctly rounded fp32 operations, and to `_pack`'s bits in every
    channel whose scale factor the host's torch computes as the correctly rounded one (`host_exact_channels`: torch.sqrt on the CPU is
    not correctly rounded, and which channels it misses depends on the CPU); the other channels' deviation is printed."""
    assert set(got) == set(host) == set(P.dst), (where, set(got) ^ set(host))
    refs = matrix_fold_refs(P, sd)
    ieee, exact = bn_fold_ieee(P, sd), host_exact_channels(P, sd)
    figures = {}
    for key in host:
        a, b = raw(got[key]).detach().cpu(), raw(host[key]).detach().cpu()
        assert isinstance(host[key], SplitW) == is_split(P, key), (where, key)
        assert torch.is_tensor(got[key]) or isinstance(got[key], SplitW) == is_split(P, key), (where, key)     # (the interpreter returns planes)
        assert a.shape == b.shape and a.dtype == b.dtype, (where, key, a.shape, b.shape, a.dtype, b.dtype)
        if key in repack.MATRIX_FOLD_KEYS:
            mine, theirs = fold_error(a, refs[key]), fold_error(b, refs[key])
            figures[key] = (mine, theirs)
            print(f"{where} {key}: device-form {mine:.3e}, _pack {theirs:.3e}, ratio {mine / max(theirs, 2.0 ** -24 / 8):.2f}")
            assert mine <= max(8 * theirs, 2.0 ** -24), (where, key, mine, theirs)
        else:
            bits = torch.int16 if a.dtype == torch.float16 else torch.int32
            if key in BN_FOLD_KEYS:
                # the correctly rounded fold on every host, and `_pack`'s bits in every channel whose scale factor this host's torch rounds correctly
                want = ieee[key].reshape(a.shape)
                assert torch.equal(a.view(bits), want.view(bits)), (where, key, "IEEE", int((a.view(bits) != want.view(bits)).sum()))
                assert torch.equal(a[exact].view(bits), b[exact].view(bits)), (where, key, int((a[exact].view(bits) != b[exact].view(bits)).sum()))
                if not bool(exact.all()):
                    d = (b.view(bits).long() - want.view(bits).long()).abs()
                    print(f"{where} {key}: torch.sqrt of this host misses the correctly rounded scale factor in {int((~exact).sum())} of {exact.numel()} "
                          f"channels; there _pack differs from the correctly rounded fold in {int((d > 0).sum())} elements by up to {int(d.max())} ulp")
                continue
            assert torch.equal(a.view(bits), b.view(bits)), (where, key, int((a.view(bits) != b.view(bits)).sum()))
    return figures
