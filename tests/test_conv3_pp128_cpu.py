"""CPU: the weight-pack family (include/givepose_wpack.h, gpw_*) and the chunk-major copy of the 3x3 head weights
(gp_gemm_desc.W_cm): header == exported symbols == _lib.WPACK_PROTOTYPES, none of them in the other headers; the repack plan writes the
copy as a view of the conv weight that equals ops.conv3_pack_wcm of the packed weight; the kernel that reads it uses no scratch."""
import os
import re
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_prototypes_and_exports_agree():
    from givepose_amd import _lib, build
    hdr = _header("givepose_wpack.h")
    declared = set(re.findall(r"^int (gpw_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert declared == set(_lib.WPACK_PROTOTYPES) == {"gpw_conv3_pack_wcm", "gpw_gemm_desc_bytes"}
    tables = {n: getattr(_lib, n) for n in dir(_lib) if n.endswith("PROTOTYPES")}
    for n, other in tables.items():
        if n != "WPACK_PROTOTYPES":
            assert not any(k.startswith("gpw_") for k in other), n
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "givepose_wpack.h":
            assert "gpw_" not in _header(name), name
    build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert set(re.findall(r" T (gpw_[a-z0-9_]+)", out)) == declared
    assert "givepose_wpack.h" in open(os.path.join(ROOT, "givepose_amd", "build.py")).read()
    lib = _lib.load()
    for name, (argtypes, _) in _lib.WPACK_PROTOTYPES.items():
        assert getattr(lib, name).argtypes == argtypes
        decl = re.search(rf"^int {name}\s*\((.*?)\);", hdr, re.M | re.S).group(1)
        assert len([a for a in decl.split(",") if a.strip() != "void"]) == len(argtypes), name
    # the layout check that stands in for a new ABI number
    import ctypes
    assert lib.gpw_gemm_desc_bytes() == ctypes.sizeof(_lib.GemmDesc)
    # W_cm is the last field of the descriptor on both sides
    assert _lib.GemmDesc._fields_[-1][0] == "W_cm"
    body = re.search(r"typedef struct gp_gemm_desc \{(.*?)\} gp_gemm_desc;", _header("givepose_hip.h"), re.S).group(1)
    assert body.split(";")[-2].strip() == "const void* W_cm"


def test_host_pack_is_the_permutation():
    from givepose_amd import ops
    for cin in (32, 128, 256):
        w = torch.randn(256, 9 * cin).half()
        want = w.view(256, 9, cin // 32, 32).permute(0, 2, 1, 3).reshape(256, 9 * cin)
        assert torch.equal(ops.conv3_pack_wcm(w), want)


def test_repack_plan_writes_the_copy_as_a_view():
    """{head}.c{i}_wcm for the 32 x 32 and 64 x 64 layers of both heads, fp16 mode only: the entry's view of the fp32 conv weight
    (256, Cin, 3, 3), rounded, is conv3_pack_wcm of the packed c{i}_w."""
    from givepose_amd import PoseNetConfig, ops, repack
    cfg = PoseNetConfig()
    P = repack.plan(cfg, torch.float16, False)
    keys = [k for k in P.dst if k.endswith("_wcm")]
    assert keys == [f"{h}.c{i}_wcm" for h in ("xyz_nocs_head", "xyz_deform_head") for i in repack.CONV3_WCM_LAYERS]
    assert not any(k.endswith("_wcm") for k in repack.plan(cfg, torch.float32, False).dst)
    assert not any(k.endswith("_wcm") for k in repack.plan(cfg, torch.float32, True).dst)
    (e,) = [e for e in P.entries if e.dst == "xyz_nocs_head.c9_wcm"]
    cin = P.sources[e.src][1]
    w = torch.randn(256, cin, 3, 3)
    got = torch.as_strided(w.reshape(-1), e.dims, e.strides, e.offset).reshape(256, 9 * cin).half()
    packed = w.permute(0, 2, 3, 1).reshape(256, -1).half()
    assert torch.equal(got, ops.conv3_pack_wcm(packed)) and e.kind == repack.F16 and P.dst[e.dst] == ((256, 9 * cin), repack.F16)
