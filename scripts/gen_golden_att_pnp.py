#!/usr/bin/env python3
"""Generate tests/golden/att_pnp_*: the AttentionPnPNet pose head (pnp_head='att'), from the REFERENCE's own classes (build container
only; scripts/ref_shim.py stubs the third-party packages it imports, as for scripts/gen_golden_pnp_flags.py).

Run:  python scripts/gen_golden_att_pnp.py            (needs the reference checkout; never runs on the GPU box)

The reference defines AttentionPnPNet (network/attention_pnp_net.py:36-124) but never wires it: PoseNet.__init__ always builds
ConvPnPNet (network/PoseNet.py:162).  The end-to-end fixtures therefore replace `pnp_net` by a subclass of AttentionPnPNet(in_chans=5)
whose forward(coor_feat, mask_attention=None) calls the parent -- a subclass, so that the state-dict keys stay under `pnp_net.`.

Fixtures (weights are the seeded synthetic tensors of givepose_amd.synth, loaded by name; nothing large is stored):
  * att_pnp_module.npz          AttentionPnPNet(in_chans=5) on the input of pnp_flags_inputs (Philox seed 78, checked by CRC):
                                rot (2,6), t (2,3) and the flattened normalised tokens flat (2,12288)
  * att_pnp_e2e_<tag>.npz       network.PoseNet.forward at B = 4 (the batch of posenet_e2e_B4): rot, trans, size, pred_rot, pred_t
  * att_pnp_manifest.json       the non-backbone state-dict name -> shape of each e2e configuration
"""
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import ref_shim  # noqa: E402

FLAGS = ref_shim.install()
import torch  # noqa: E402

from givepose_amd.config import PoseNetConfig  # noqa: E402
from givepose_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)
SEED = 0
X_SEED = 78            # the module input of pnp_flags_inputs: Philox(key=[SEED, X_SEED]).uniform(-0.8, 0.8, (2, 5, 64, 64)) float32
# e2e configurations: tag -> PoseNetConfig fields (pnp_head is this build's switch; the others are the reference FLAGS of the same names)
E2E = {
    "att": dict(pnp_head="att"),
    "att_attenc": dict(pnp_head="att", nocsmap_encoder="att"),
    "att_ego_center": dict(pnp_head="att", r_type="ego_rot6d", t_type="center"),
}
FLAG_NAMES = ("flat_op", "mask_attention_type", "r_type", "t_type", "nocsmap_encoder", "use_dcn", "dataset")


def crc(a):
    return int(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def module_input():
    r = np.random.Generator(np.random.Philox(key=[SEED, X_SEED]))
    return r.uniform(-0.8, 0.8, (2, 5, 64, 64)).astype(np.float32)


def save(name, **arrs):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    size = os.path.getsize(path)
    print(f"  wrote {name}.npz ({size / 1024:.0f} KB)")
    assert size < 200 * 1024


def load_synth_into(module, prefix, rename=None):
    sd = module.state_dict()
    new = {}
    for k, v in sd.items():
        canon = rename(k) if rename else k
        new[k] = v if canon is None else torch.from_numpy(synth.synth_tensor(prefix + canon, tuple(v.shape), SEED)).to(v.dtype)
    module.load_state_dict(new, strict=True)
    return module


def set_flags(**kw):
    base = {f: getattr(PoseNetConfig(), f) for f in FLAG_NAMES}
    base.update({k: v for k, v in kw.items() if k in FLAG_NAMES})
    for k, v in base.items():
        setattr(FLAGS, k, v)


def att_pnp_class():
    from network.attention_pnp_net import AttentionPnPNet

    class AttPnPHead(AttentionPnPNet):
        """AttentionPnPNet in ConvPnPNet's seat: PoseNet.forward passes mask_attention=, which AttentionPnPNet.forward does not take."""

        def forward(self, coor_feat, mask_attention=None):
            return super().forward(coor_feat)

    return AttPnPHead


def gen_module():
    print("AttentionPnPNet(in_chans=5) module")
    x = module_input()
    z = np.load(os.path.join(GOLD, "pnp_flags_inputs.npz"))
    assert crc(x) == int(z["x_crc"]) and int(z["x_seed"]) == X_SEED
    m = load_synth_into(att_pnp_class()(in_chans=5).eval(), "pnp_net.")
    ours = synth.param_manifest(PoseNetConfig(pnp_head="att"))
    assert [k for k in ours if k.startswith("pnp_net.")] == ["pnp_net." + k for k in m.state_dict()], "module key order"
    assert all(tuple(v.shape) == tuple(ours["pnp_net." + k]) for k, v in m.state_dict().items())
    rot, t, flat = m(torch.from_numpy(x))
    assert tuple(flat.shape) == (2, 12288)
    print(f"  rot[0] {rot[0].numpy().round(3)} t[0] {t[0].numpy().round(3)}")
    save("att_pnp_module", x_seed=X_SEED, x_crc=crc(x), rot=rot, t=t, flat=flat)


def gen_e2e():
    from network.PoseNet import PoseNet
    print("PoseNet e2e with AttentionPnPNet, B = 4")

    def rename(k):
        if k.startswith("backbone."):
            t = synth.hf_to_timm(k[len("backbone."):])
            return None if t is None else "backbone." + t
        return k

    manifests = {}
    B = 4
    npb = synth.synth_batch(B, seed=100 + B)        # the batch of posenet_e2e_B4
    data = {k: torch.from_numpy(v) for k, v in npb.items()}
    head = att_pnp_class()
    for tag, kw in E2E.items():
        set_flags(**kw)
        cfg = PoseNetConfig(**kw)
        net = PoseNet()
        net.pnp_net = head(img_size=64, patch_size=8, in_chans=5, embed_dim=192, depth=3, num_heads=8, flat_op="flatten")
        net = load_synth_into(net.eval(), "", rename=rename)
        manifest = {k: list(v.shape) for k, v in net.state_dict().items() if not k.startswith("backbone.")}
        ours = synth.param_manifest(cfg)
        assert [k for k in ours if not k.startswith("backbone.")] == list(manifest), (tag, "manifest order/name mismatch")
        assert all(tuple(manifest[k]) == tuple(ours[k]) for k in manifest), tag
        manifests[tag] = {"config": kw, "non_backbone": manifest}
        mid = {}
        net.pnp_net.register_forward_hook(lambda mod, a, o: mid.update(pred_rot=o[0], pred_t=o[1]))
        out = net(data, "cpu", do_loss=False)
        print(f"  {tag:16s} pred_rot[0] {mid['pred_rot'][0].numpy().round(3)} t[0] {out['trans'][0].numpy().round(3)}")
        save(f"att_pnp_e2e_{tag}", batch_seed=100 + B, roi_img_crc=crc(npb["roi_img"]), rot=out["rot"], trans=out["trans"],
             size=out["size"], pred_rot=mid["pred_rot"], pred_t=mid["pred_t"])
    set_flags()
    with open(os.path.join(GOLD, "att_pnp_manifest.json"), "w") as f:
        json.dump(manifests, f, indent=0)
    print("  wrote att_pnp_manifest.json")


if __name__ == "__main__":
    which = sys.argv[1:] or ["module", "e2e"]
    if "module" in which:
        gen_module()
    if "e2e" in which:
        gen_e2e()
    print("done")
