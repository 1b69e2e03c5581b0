"""gp_convnext_mlp conformance (csrc/mlp.hip): every launch form of the fused ConvNeXt block MLP per element against the float64
reference and bound of tests/mlp_reference.py (put together from tests/gemm_reference.py; checked on the CPU by
tests/test_mlp_reference_cpu.py), and both W2 pack kernels bit for bit.

  A  dense operands with outlier rows / channels, M such that the grid is below, above and not a multiple of 8 workgroups (xcd_chunk)
  B  one-hot W2 (four selectors: every hidden unit read once): pins the W2 packing, the ring, the b1 index and the epilogue transpose
  C  every finite fp16 value through the form's own GELU call site (one-hot x and W2, so that out = fp16(GELU(W1 entry)))
  D  buffer discipline on the smallest dense case: sentinel rows behind M, repeat launch, out-of-place = in-place, operands unchanged
  E  gp_convnext_mlp_pack_w2 / _s32 against the index formulas of the kernel comments
  F  the refusal table (mlp_reference.REFUSALS): each row raises with its message fragment, and nothing else is refused

The three forms chosen by switches the library reads once per process (GP_GELU16=0: convnext_mlp_kernel<128,0> / <256,0>;
GP_MLP_WAVES=8: convnext_mlp_kernel<128,1,8>) run in a fresh child each, taken from the fork server conftest.py starts before any
GPU call; the child sets the switch before it imports givepose_amd and sends back (case, max err/bound, message) tuples.
"""
import multiprocessing as mp
import os
import time

import pytest
import torch

import mlp_reference as mr

pytestmark = pytest.mark.gpu

# Join limit of a child: a guard, not a measurement.  Families A - D of c128w4 + c256 (the forms that stand in, in this process, for
# what a child runs) took 0.9 s on the first MI355X run, references included; ten times that, rounded up to a minute.  (A child took
# 2.2 - 2.9 s from start() to its answer, 0.5 - 0.8 s of it in the cases: profiles/mlp_conformance.txt.)
CHILD_LIMIT_S = 60


# ---------------------------------------------------------------------------------------------------------------- launching
def _dev(op, form):
    """Device operands of a case, W2 packed by the library's own pack kernel of the form."""
    from givepose_amd import ops as o
    f = mr.FORMS[form]
    h = lambda t: t.to("cuda", torch.float16)
    d = dict(x=h(op.x), w1=h(op.w1), b1=op.b1.cuda(), b2=op.b2.cuda(), gamma=op.gamma.cuda(), res=h(op.res))
    d["w2p"] = o.convnext_mlp_pack_w2(h(op.w2), s32=f.s32)
    return d


def _launch(form, d, out, residual):
    from givepose_amd import ops as o
    return o.convnext_mlp(d["x"], d["w1"], d["b1"], d["w2p"], d["b2"], d["gamma"], residual, out, s32=mr.FORMS[form].s32)


def run_numeric(form, case):
    """(name, max err/bound, message or None, extra) of one A / B / C case: in place over the residual, as the network launches it."""
    f = mr.FORMS[form]
    op = mr.operands(f.C, case)
    d = _dev(op, form)
    out = d["res"].clone()
    _launch(form, d, out, out)
    torch.cuda.synchronize()
    ratio, msg = mr.check_case(form, case, out)
    extra = mr.gelu_summary(form, case, out) if case[0] == "C" else None
    return mr.case_name(form, case), ratio, msg, extra


def run_discipline(form):
    """Family D on the smallest dense case: list of problems (empty = fine)."""
    f = mr.FORMS[form]
    case = mr.cases(form, "A")[0]
    M = case[1]
    op = mr.operands(f.C, case)
    d = _dev(op, form)
    before = {k: v.clone() for k, v in d.items()}
    probs = []

    def buf(fill_from=None):
        b = torch.full((M + mr.SENT_ROWS, f.C), mr.SENT, dtype=torch.float16, device="cuda")
        if fill_from is not None:
            b[:M] = fill_from
        return b
    b1 = buf(d["res"])
    _launch(form, d, b1[:M], b1[:M])                         # in place
    b2 = buf(d["res"])
    _launch(form, d, b2[:M], b2[:M])                         # again
    b3 = buf()
    _launch(form, d, b3[:M], d["res"])                       # out of place
    torch.cuda.synchronize()
    ratio, msg = mr.check_case(form, case, b1[:M])
    if msg is not None:
        probs.append(msg)
    for name, b in (("in place", b1), ("second launch", b2), ("out of place", b3)):
        if not mr.sentinels_intact(b, M):
            probs.append(f"{form}: {name}: rows behind M = {M} were written")
    if not torch.equal(b1, b2):
        probs.append(f"{form}: the second launch differs in {int((b1 != b2).sum())} elements")
    if not torch.equal(b1, b3):
        probs.append(f"{form}: the out-of-place launch differs from the in-place one in {int((b1 != b3).sum())} elements")
    for k, v in before.items():
        if not torch.equal(v, d[k]):
            probs.append(f"{form}: operand {k} changed")
    return probs


def _raw_args(C, M, dt=torch.float16):
    HD = 4 * C
    z = lambda *s, t=dt: torch.zeros(*s, dtype=t, device="cuda")
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    return dict(x=z(M, C), w1=z(HD, C), b1=f(HD), w2p=z(C, HD), b2=f(C), gamma=f(C), residual=z(M, C), out=z(M, C))


def run_refusal(r):
    """None when row r of the refusal table raises the right error with its fragment, else what happened instead."""
    from givepose_amd import _lib, ops as o
    a = _raw_args(r.C, r.M)
    s32 = False
    C, M = r.C, r.M
    h = lambda *s: torch.zeros(*s, dtype=torch.float16, device="cuda")
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    w = r.what
    if w == "s32":
        s32 = True
    elif w == "offset8":
        a["x"] = h(M * C + 8)[4:4 + M * C].view(M, C)        # contiguous, 8 bytes past a 16-byte boundary
        assert a["x"].is_contiguous() and a["x"].data_ptr() % 16 == 8
    elif w == "out_is_x":
        a["out"] = a["x"]
    elif w == "fp32_x":
        a["x"] = f32(M, C)
    elif w == "fp32_out":
        a["out"] = f32(M, C)
    elif w == "fp16_b1":
        a["b1"] = h(4 * C)
    elif w == "fp16_gamma":
        a["gamma"] = h(C)
    elif w == "strided_out":
        a["out"] = h(M, 2 * C)[:, :C]
    elif w == "strided_w1":
        a["w1"] = h(C, 4 * C).t()
    elif w == "w1_shape":
        a["w1"] = h(C, 4 * C)
    elif w == "b1_shape":
        a["b1"] = f32(C)
    elif w == "w2p_shape":
        a["w2p"] = h(4 * C, C)
    elif w == "b2_shape":
        a["b2"] = f32(4 * C)
    elif w == "gamma_shape":
        a["gamma"] = f32(2 * C)
    elif w == "res_shape":
        a["residual"] = h(M // 2, C)
    elif w == "x_3d":
        a["x"] = h(2, M // 2, C)
    elif w == "cpu_x":
        a["x"] = torch.zeros(M, C, dtype=torch.float16)
    elif w not in (None, "fp32_raw"):
        return f"{r.name}: unknown departure {w}"
    want = _lib.GivePoseHipError if r.level == "lib" else (TypeError, RuntimeError)
    keep = a["out"].clone() if a["out"].is_cuda else None
    try:
        if w == "fp32_raw":       # fp32 storage announced to the library itself (the wrapper refuses fp32 tensors: row fp32-tensors)
            a = _raw_args(C, M, torch.float32)
            keep = a["out"].clone()
            p = o._ptr
            _lib.check(_lib.load().gp_convnext_mlp(p(a["x"]), p(a["w1"]), p(a["b1"]), p(a["w2p"]), p(a["b2"]), p(a["gamma"]), p(a["residual"]),
                                                   p(a["out"]), M, C, o.GP_F32, o._stream()), "gp_convnext_mlp")
        else:
            o.convnext_mlp(a["x"], a["w1"], a["b1"], a["w2p"], a["b2"], a["gamma"], a["residual"], a["out"], s32=s32)
    except Exception as e:      # noqa: BLE001 -- the kind of error is what is being checked
        torch.cuda.synchronize()
        if r.level == "lib" and not isinstance(e, _lib.GivePoseHipError):
            return f"{r.name}: raised {type(e).__name__} ({e}), expected the library's refusal"
        if r.level == "ops" and (isinstance(e, _lib.GivePoseHipError) or not isinstance(e, want)):
            return f"{r.name}: raised {type(e).__name__} ({e}), expected the wrapper's own refusal"
        if r.frag not in str(e):
            return f"{r.name}: refused with '{e}', expected a message containing '{r.frag}'"
        if keep is not None and keep.numel() and not torch.equal(keep, a["out"]):
            return f"{r.name}: refused, but the output was written"
        return None
    torch.cuda.synchronize()
    return f"{r.name}: ran, the table expects a refusal containing '{r.frag}'"


def _format(results):
    return "\n".join(f"{name}: max err/bound {ratio:.3g}" + (f"   GELU max |err| {extra[0]:.3g} for |v| <= 4.4, max |err|/|v| {extra[1]:.3g} beyond"
                                                            f" (against the exact GELU rounded to fp16)" if extra else "")
                     for name, ratio, msg, extra in results)


# ---------------------------------------------------------------------------------------------------------------- A, B, C, D in-process
@pytest.mark.parametrize("family", mr.FAMILIES)
@pytest.mark.parametrize("form", mr.DEFAULT_FORMS)
def test_mlp_conformance(form, family):
    res = [run_numeric(form, case) for case in mr.cases(form, family)]
    print("\n" + _format(res))
    bad = [msg for _, _, msg, _ in res if msg is not None]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("form", mr.DEFAULT_FORMS)
def test_mlp_buffer_discipline(form):
    probs = run_discipline(form)
    assert not probs, "\n".join(probs)


# ---------------------------------------------------------------------------------------------------------------- E: packing
@pytest.mark.parametrize("s32,C", [(False, 128), (False, 256), (False, 512), (True, 128), (True, 256)])
def test_pack_w2_bit_exact(s32, C):
    from givepose_amd import ops as o
    bits = mr.pack_probe(C)                                           # int16 bit patterns, (C, 4C)
    src = bits.cuda().view(torch.float16)
    keep = src.clone()
    got = o.convnext_mlp_pack_w2(src, s32=s32)
    torch.cuda.synchronize()
    want = mr.pack_w2(bits, mr.perm32() if s32 else mr.perm16())
    assert torch.equal(got.view(torch.int16).cpu(), want), int((got.view(torch.int16).cpu() != want).sum())
    assert torch.equal(src.view(torch.int16), keep.view(torch.int16))
    assert not torch.equal(want, bits)


def test_pack_w2_refusals():
    from givepose_amd import _lib, ops as o
    for s32, C, frag in ((False, 64, "C=64 must be 128, 256 or 512"), (False, 384, "C=384 must be 128, 256 or 512"),
                         (True, 512, "C=512 must be 128 or 256"), (True, 64, "C=64 must be 128 or 256")):
        with pytest.raises(_lib.GivePoseHipError) as e:
            o.convnext_mlp_pack_w2(torch.zeros(C, 4 * C, dtype=torch.float16, device="cuda"), s32=s32)
        assert frag in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------- F: refusals
@pytest.mark.parametrize("name", [r.name for r in mr.REFUSALS if r.env is None])
def test_mlp_refusal(name):
    problem = run_refusal(mr.REFUSAL_BY_NAME[name])
    assert problem is None, problem


def test_nothing_but_the_table_is_refused():
    """The converse of F: the smallest valid launch of every default form runs (the numeric tests run the rest)."""
    for form in mr.DEFAULT_FORMS:
        f = mr.FORMS[form]
        M = mr.dense_M(form)[0]
        assert mr.expected(f.C, M, f.s32) is None
        a = _raw_args(f.C, M)
        from givepose_amd import ops as o
        o.convnext_mlp(a["x"], a["w1"], a["b1"], a["w2p"], a["b2"], a["gamma"], a["residual"], a["out"], s32=f.s32)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the env-selected forms
def child_main(setting, q):
    """Runs in a fresh process: the switch is set before givepose_amd is imported (the library caches it at its first launch)."""
    var, val = setting
    os.environ[var] = val
    out = []
    try:
        import givepose_amd  # noqa: F401
        from givepose_amd import _lib
        _lib.load()
        t1 = time.time()
        for form in mr.ENV_SETTINGS[setting]:
            for fam in mr.FAMILIES:
                for case in mr.cases(form, fam):
                    name, ratio, msg, extra = run_numeric(form, case)
                    out.append((name, ratio, msg, extra))
            probs = run_discipline(form)
            out.append((f"{form}-D", 0.0, "\n".join(probs) if probs else None, None))
        for r in mr.REFUSALS:
            if r.env in (None, setting):
                p = run_refusal(r)
                out.append((f"refusal {r.name}", 0.0, p, None))
        out.append(("wall", time.time() - t1, None, None))
        q.put(("ok", out))
    except BaseException as e:      # noqa: BLE001 -- reported to the parent, which fails the test
        q.put(("error", out + [("child", float("inf"), f"{type(e).__name__}: {e}", None)]))


_CHILD_BROKEN = []        # a child that ended by a signal or at its limit: no further child is started


@pytest.mark.timeout(4 * CHILD_LIMIT_S)
@pytest.mark.parametrize("setting", sorted(mr.ENV_SETTINGS), ids=lambda s: f"{s[0]}={s[1]}")
def test_env_selected_forms_in_a_fresh_child(setting):
    assert not _CHILD_BROKEN, f"an earlier child ended badly ({_CHILD_BROKEN[0]}): no further process is started"
    ctx = mp.get_context("forkserver")        # server started in conftest.pytest_configure, before any GPU call
    q = ctx.Queue()
    p = ctx.Process(target=child_main, args=(setting, q))
    t0 = time.time()
    p.start()
    status, results = None, []
    while status is None and time.time() - t0 < CHILD_LIMIT_S:
        try:
            status, results = q.get(timeout=0.5)
        except Exception:       # noqa: BLE001 -- queue.Empty: not yet
            if not p.is_alive() and q.empty():
                break           # the child died without an answer: no point in waiting for the limit
    p.join(10 if status is not None else 0.1)
    if p.is_alive():
        p.kill()
        p.join(10)
        _CHILD_BROKEN.append(f"{setting[0]}={setting[1]}: no answer within {CHILD_LIMIT_S} s, killed")
    elif p.exitcode != 0:
        _CHILD_BROKEN.append(f"{setting[0]}={setting[1]}: exit code {p.exitcode}")
    assert not _CHILD_BROKEN, _CHILD_BROKEN[-1]
    assert status is not None, "the child ended without an answer"
    wall = [r for r in results if r[0] == "wall"]
    numeric = [r for r in results if r[0] != "wall" and not r[0].startswith("refusal") and not r[0].endswith("-D")]
    print(f"\n{setting[0]}={setting[1]}: child {time.time() - t0:.1f} s in all"
          + (f", {wall[0][1]:.1f} s of it in the cases" if wall else ""))
    print(_format(numeric))
    bad = [f"{name}: {msg}" for name, _, msg, _ in results if msg is not None]
    assert status == "ok" and not bad, "\n".join(bad)
    # every case the table lists for the setting came back
    want = {mr.case_name(form, case) for form in mr.ENV_SETTINGS[setting] for fam in mr.FAMILIES for case in mr.cases(form, fam)}
    assert {r[0] for r in numeric} == want
    assert {r[0] for r in results if r[0].endswith("-D")} == {f"{form}-D" for form in mr.ENV_SETTINGS[setting]}
    assert {r[0] for r in results if r[0].startswith("refusal")} == {f"refusal {r.name}" for r in mr.REFUSALS if r.env in (None, setting)}
