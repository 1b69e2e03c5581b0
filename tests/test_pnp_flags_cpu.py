"""CPU: ConvPnPNet's flat_op / mask_attention_type and the rotation type (r_type) in the config, the parameter manifest and the
checkpoint interface -- every pose-head flag either works (the shapes the reference registers for it) or refuses."""
import json
import os

import numpy as np
import pytest
import torch

from givepose_amd import PoseNet, PoseNetConfig, checkpoint, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _manifests():
    with open(os.path.join(GOLDEN, "pnp_flags_manifest.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("tag", ["avgmaxmin", "mul", "ego_rot6d", "allo_quat", "euler", "avg_mul_ego_quat"])
def test_manifest_matches_reference(tag):
    ref = _manifests()[tag]
    ours = synth.param_manifest(PoseNetConfig(**ref["config"]))
    got = [(k, list(v)) for k, v in ours.items() if not k.startswith("backbone.")]
    assert got == list(ref["non_backbone"].items())


@pytest.mark.parametrize("flat_op,fin", [("flatten", 8192), ("avg", 128), ("avg-max", 256), ("avg-max-min", 384)])
@pytest.mark.parametrize("r_type,rot_dim", [("allo_rot6d", 6), ("ego_quat", 4), ("euler", 6)])
def test_manifest_pnp_shapes(flat_op, fin, r_type, rot_dim):
    m = synth.param_manifest(PoseNetConfig(flat_op=flat_op, r_type=r_type))
    assert m["pnp_net.fc1.weight"] == (1024, fin) and m["pnp_net.fc1_z.weight"] == (1024, fin)
    assert m["pnp_net.fc_r.weight"] == (rot_dim, 256) and m["pnp_net.fc_r.bias"] == (rot_dim,)


def test_expected_keys_follow_flags():
    keys = dict(checkpoint.expected_keys(PoseNetConfig(flat_op="avg-max", r_type="allo_quat")))
    assert keys["pnp_net.fc1.weight"] == (1024, 256) and keys["pnp_net.fc1_z.weight"] == (1024, 256)
    assert keys["pnp_net.fc_r.weight"] == (4, 256) and keys["pnp_net.fc_r.bias"] == (4,)
    ref = _manifests()["avg_mul_ego_quat"]["non_backbone"]
    keys = dict(checkpoint.expected_keys(PoseNetConfig(flat_op="avg", mask_attention_type="mul", r_type="ego_quat")))
    assert {k: list(v) for k, v in keys.items() if not k.startswith("backbone.")} == ref


def test_avg_state_dict_loads_strict():
    cfg = PoseNetConfig(flat_op="avg")
    net = PoseNet(cfg, dtype=torch.float32)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(cfg, 0).items()}
    net.load_state_dict(sd, strict=True)
    assert tuple(net.state_dict()["pnp_net.fc1.weight"].shape) == (1024, 128)
    assert np.array_equal(net.state_dict()["pnp_net.fc1_z.weight"].numpy(), sd["pnp_net.fc1_z.weight"].numpy())


@pytest.mark.parametrize("kw", [dict(flat_op="avg-max-min"), dict(mask_attention_type="mul"), dict(r_type="ego_rot6d"),
                                dict(r_type="allo_rot6d_z"), dict(r_type="allo_quat"), dict(r_type="euler"), dict(t_type="center"),
                                dict(use_dcn="", nocsmap_encoder="att"), dict(main_backbone="resnet34")])
def test_accepted_values_build(kw):
    PoseNet(PoseNetConfig(**kw), dtype=torch.float32)


@pytest.mark.parametrize("kw", [dict(mask_attention_type="concat"), dict(size_head_out_dim=1), dict(out_res=32), dict(img_size=224)])
def test_refused_not_implemented(kw):
    with pytest.raises(NotImplementedError):
        PoseNet(PoseNetConfig(**kw), dtype=torch.float32)


def test_concat_refusal_says_why():
    with pytest.raises(NotImplementedError, match="6 channels"):
        PoseNet(PoseNetConfig(mask_attention_type="concat"), dtype=torch.float32)


@pytest.mark.parametrize("kw", [dict(flat_op="max"), dict(mask_attention_type="add"), dict(r_type="allo_rot9d"), dict(r_type="quat"),
                                dict(nocsmap_encoder="mlp"), dict(use_dcn="dcnv2"), dict(t_type="abs")])
def test_refused_unknown_value(kw):
    with pytest.raises(ValueError):
        PoseNet(PoseNetConfig(**kw), dtype=torch.float32)
