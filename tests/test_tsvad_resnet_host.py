"""TS-VAD with the ResNet34 speech encoder (resnet34_wespeaker): configuration, key layout, the torch-functional
restatement against the reference goldens, and the transposed conv's phase-conv repacking.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from speaker_diarization_amd.weights import (TSVADConfig, resnet34_layout, to_torch, tsvad_layout,  # noqa: E402
                                             tsvad_state_dict)
import tsvad_resnet_ref as rn  # noqa: E402
from make_golden_resnet import rn34_case_inputs  # noqa: E402

GOLD = os.path.join(HERE, "golden")
CFG = TSVADConfig(speech_encoder_type="resnet34_wespeaker")


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def test_config_variant():
    assert CFG.variant == 2
    assert TSVADConfig().variant == 0
    assert TSVADConfig.ots_vad_v1().variant == 1


def test_v1_style_with_resnet_raises():
    with pytest.raises(ValueError, match="ots_vad_style v1 is built for CAM\\+\\+_ots_vad"):
        TSVADConfig(speech_encoder_type="resnet34_wespeaker", single_backend_type="conformer_ots_vad",
                    multi_backend_type="lstm_ots_vad", ots_vad_style="v1").variant
    with pytest.raises(ValueError):
        TSVADConfig(speech_encoder_type="resnet34_wespeaker", ots_vad_style="v1").variant
    with pytest.raises(ValueError, match="unsupported TS-VAD configuration"):
        TSVADConfig(speech_encoder_type="resnet34_wespeaker", multi_backend_type="lstm_ots_vad").variant


def test_layout_matches_reference_keys():
    g = gold("tsvad_rn34_keys")
    ref = {str(n): tuple(int(d) for d in str(s).split(",") if d) for n, s in zip(g["names"], g["shapes"])}
    ours = {n: tuple(s) for n, s, _ in tsvad_layout(CFG)}
    assert len(ours) == len(tsvad_layout(CFG)), "duplicate key in the layout"
    assert set(ours) == set(ref), (sorted(set(ours) - set(ref))[:5], sorted(set(ref) - set(ours))[:5])
    assert ours == ref


def test_encoder_layout_has_no_pool_or_embedding_head():
    names = [n for n, _, _ in resnet34_layout()]
    assert not [n for n in names if "pool" in n or "seg_" in n]
    assert sum(n.endswith("conv1.weight") or n.endswith("conv2.weight") for n in names) == 33
    assert sum(n.endswith("shortcut.0.weight") for n in names) == 3


@pytest.mark.parametrize("name", ["tsvad_rn34_rs4", "tsvad_rn34_rs4_short", "tsvad_rn34_tiny"])
def test_restatement_matches_reference(name):
    g = gold(name)
    (_, _, n_lab, _, wseed, _), ref_speech, ts = rn34_case_inputs(name)
    sd = to_torch(tsvad_state_dict(CFG, seed=wseed))
    with torch.no_grad():
        trunk = rn.resnet34_time_out(sd, torch.from_numpy(ref_speech))
        enc = rn.upsample(sd, trunk)
    assert enc.shape == g["speech_enc"].shape
    err = float(np.abs(enc.numpy() - g["speech_enc"]).max())
    print(name, "speech_enc max err", err)
    assert err < 1e-5
    if "trunk" in g:
        terr = float(np.abs(trunk.numpy() - g["trunk"]).max())
        print(name, "trunk max err", terr)
        assert terr < 1e-5
    logits = rn.tsvad_forward(sd, CFG, torch.from_numpy(ref_speech), torch.from_numpy(ts), n_lab).numpy()
    assert np.abs(logits - g["logits"]).max() < 1e-4


def test_seeded_model_is_alive():
    g = gold("tsvad_rn34_rs4")
    assert 0.5 <= np.abs(g["logits"]).max() <= 20.0
    assert g["logits"].std(-1).mean() > 0.05
    assert (g["speech_enc"] != 0).mean() > 0.30


def test_nan_golden_shape():
    g, s = gold("tsvad_rn34_nan"), gold("tsvad_rn34_rs4_short")
    assert np.isnan(g["logits"][2]).all() and np.isfinite(g["logits"][:2]).all()
    assert np.abs(g["logits"][:2] - s["logits"][:2]).max() > 1e-3   # the batch's BatchNorm1D was bypassed


@pytest.mark.parametrize("T", [1, 2, 5, 25])
def test_phase_convs_equal_conv_transpose(T):
    rng = np.random.default_rng(100 + T)
    cin, cout, B = 24, 7, 2
    x = rng.standard_normal((B, cin, T)).astype(np.float32)
    w = rng.standard_normal((cin, cout, 5)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    ref = F.conv_transpose1d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=2, padding=2,
                             output_padding=1).numpy()
    got = rn.phase_upsample(x, w, b)
    assert got.shape == ref.shape == (B, cout, 2 * T)
    assert np.abs(got - ref).max() < 1e-5
