"""CPU: the AttentionPnPNet pose head (PoseNetConfig.pnp_head='att') in the config, the parameter manifest and the checkpoint
interface, and tests/att_pnp_ref.py against the goldens scripts/gen_golden_att_pnp.py captured from the reference's own classes."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

from givepose_amd import PoseNet, PoseNetConfig, checkpoint, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E2E = {
    "att": dict(pnp_head="att"),
    "att_attenc": dict(pnp_head="att", nocsmap_encoder="att"),
    "att_ego_center": dict(pnp_head="att", r_type="ego_rot6d", t_type="center"),
}


def _manifests():
    with open(os.path.join(GOLDEN, "att_pnp_manifest.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("tag", list(E2E))
def test_manifest_matches_reference(tag):
    ref = _manifests()[tag]
    assert ref["config"] == E2E[tag]
    ours = synth.param_manifest(PoseNetConfig(**ref["config"]))
    got = [(k, list(v)) for k, v in ours.items() if not k.startswith("backbone.")]
    assert got == list(ref["non_backbone"].items())


def test_manifest_att_head_shapes():
    m = synth.param_manifest(PoseNetConfig(pnp_head="att"))
    assert not [k for k in m if k.startswith("pnp_net.features.")]
    assert m["pnp_net.pos_embed"] == (1, 64, 192) and m["pnp_net.patch_embed.proj.weight"] == (192, 5, 8, 8)
    assert m["pnp_net.block.2.attn.qkv.weight"] == (576, 192) and "pnp_net.block.0.attn.qkv.bias" not in m
    assert m["pnp_net.block.1.mlp.fc1.weight"] == (768, 192) and m["pnp_net.block.1.mlp.fc2.weight"] == (192, 768)
    assert m["pnp_net.fc1.weight"] == (1024, 12288) and m["pnp_net.fc1_z.weight"] == (1024, 12288)
    assert m["pnp_net.fc_r.weight"] == (6, 256)
    assert PoseNetConfig(pnp_head="att").fc_in_dim == 12288 and PoseNetConfig().fc_in_dim == 8192


def test_default_head_unchanged():
    assert PoseNetConfig().pnp_head == "conv"
    assert synth.param_manifest(PoseNetConfig()) == synth.param_manifest(PoseNetConfig(pnp_head="conv"))


@pytest.mark.parametrize("kw,why", [
    (dict(flat_op="avg"), "reduces over the channel axis"),
    (dict(flat_op="avg-max-min"), "reduces over the channel axis"),
    (dict(mask_attention_type="mul"), "takes no mask"),
    (dict(r_type="allo_quat"), "Linear\\(256, 6\\)"),
    (dict(r_type="ego_quat"), "Linear\\(256, 6\\)"),
])
def test_refusals_say_why(kw, why):
    with pytest.raises(NotImplementedError, match=why):
        PoseNet(PoseNetConfig(pnp_head="att", **kw), dtype=torch.float32)


@pytest.mark.parametrize("head", ["mlp", "ATT", "", "cross"])
def test_unknown_pnp_head(head):
    with pytest.raises(ValueError, match="pnp_head"):
        PoseNet(PoseNetConfig(pnp_head=head), dtype=torch.float32)


@pytest.mark.parametrize("kw", [dict(), dict(r_type="euler"), dict(r_type="allo_rot6d_z"), dict(r_type="ego_rot6d", t_type="center"),
                                dict(dataset="wild6d"), dict(nocsmap_encoder="att"), dict(use_dcn=""), dict(use_dcn="", nocsmap_encoder="att"),
                                dict(main_backbone="resnet34")])
def test_accepted_combinations_load_strict(kw):
    cfg = PoseNetConfig(pnp_head="att", **kw)
    net = PoseNet(cfg, dtype=torch.float32)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(cfg, 0).items()}
    net.load_state_dict(sd, strict=True)
    got = net.state_dict()
    assert list(got) == list(sd)
    assert np.array_equal(got["pnp_net.block.1.attn.qkv.weight"].numpy(), sd["pnp_net.block.1.attn.qkv.weight"].numpy())


def test_expected_keys_follow_flag():
    keys = dict(checkpoint.expected_keys(PoseNetConfig(pnp_head="att")))
    assert keys["pnp_net.fc1.weight"] == (1024, 12288) and keys["pnp_net.pos_embed"] == (1, 64, 192)
    assert not [k for k in keys if k.startswith("pnp_net.features.")]
    ref = _manifests()["att_attenc"]["non_backbone"]
    keys = dict(checkpoint.expected_keys(PoseNetConfig(pnp_head="att", nocsmap_encoder="att")))
    assert {k: list(v) for k, v in keys.items() if not k.startswith("backbone.")} == ref
    conv = dict(checkpoint.expected_keys(PoseNetConfig()))
    assert "pnp_net.features.0.weight" in conv and "pnp_net.pos_embed" not in conv


# ------------------------------------------------------------------------------------------------ the CPU restatement
@functools.lru_cache(maxsize=1)
def _base_sd():
    return {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(PoseNetConfig(), 0).items()}


def _params(cfg):
    """Seed-0 synthetic weights of cfg, reusing the default configuration's tensors (same names: same values)."""
    base = _base_sd()
    return {k: base[k] if k in base and tuple(base[k].shape) == tuple(s) else torch.from_numpy(synth.synth_tensor(k, s, 0))
            for k, s in synth.param_manifest(cfg).items()}


def test_ref_module_matches_golden():
    import att_pnp_ref
    z = np.load(os.path.join(GOLDEN, "att_pnp_module.npz"))
    r = np.random.Generator(np.random.Philox(key=[0, int(z["x_seed"])]))
    x = r.uniform(-0.8, 0.8, (2, 5, 64, 64)).astype(np.float32)
    assert zlib.crc32(x.tobytes()) == int(z["x_crc"])
    P = {k: v for k, v in _params(PoseNetConfig(pnp_head="att")).items() if k.startswith("pnp_net.")}
    rot, t, flat = att_pnp_ref.att_pnp_ref(P, torch.from_numpy(x))
    for name, got in (("rot", rot), ("t", t), ("flat", flat)):
        err = float(np.abs(got.numpy() - z[name]).max())
        print(f"att_pnp_ref {name}: max abs err {err:.2e}")
        assert err < 2e-5, (name, err)


@pytest.mark.parametrize("tag", list(E2E))
def test_ref_e2e_matches_golden(tag):
    import att_pnp_ref
    z = np.load(os.path.join(GOLDEN, f"att_pnp_e2e_{tag}.npz"))
    npb = synth.synth_batch(4, seed=int(z["batch_seed"]))
    assert zlib.crc32(np.ascontiguousarray(npb["roi_img"]).tobytes()) == int(z["roi_img_crc"])
    cfg = PoseNetConfig(**E2E[tag])
    out = att_pnp_ref.posenet_att_forward_ref(_params(cfg), {k: torch.from_numpy(v) for k, v in npb.items()}, cfg)
    for k in ("rot", "trans", "size", "pred_rot", "pred_t"):
        err = float(np.abs(out[k].detach().float().numpy() - z[k]).max())
        print(f"{tag} {k}: max abs err {err:.2e}")
        assert err < 2e-5, (k, err)
