"""TS-VAD with the w2v-BERT 2.0 speech encoder (speech_encoder_type "w2v-bert2", variant 7), host side: the torch
restatement (tests/w2vbert_ref.py) against every reference golden of tests/golden/make_golden_w2vbert.py at the fp32
bar, the configuration rules, the state_dict layout against the reference's stored key list, the label-length rule
against the reference's accept / raise cases and the odd-T refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import w2vbert_ref as ref  # noqa: E402
from w2vbert_cases import NAN, RAISES, TSVAD, tsvad_cfg, tsvad_inputs  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ssl.w2vbert import W2vBertConfig  # noqa: E402
from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_layout, tsvad_state_dict  # noqa: E402

GOLD = os.path.join(HERE, "golden")
FP32_RTOL = 1e-3


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(TSVAD) + list(NAN))
def test_restatement_vs_reference_golden(name):
    (B, T, nl, wseed), x, ts = tsvad_inputs(name)
    cfg = tsvad_cfg(name)
    g = gold(name)["logits"]
    out = ref.tsvad_forward(to_torch(tsvad_state_dict(cfg, seed=wseed)), cfg, torch.from_numpy(x), torch.from_numpy(ts),
                            nl).numpy()
    keep = np.isfinite(g)
    assert (np.isfinite(out) == keep).all()
    err = float(np.abs(out[keep] - g[keep]).max())
    print(f"{name}: max|logit diff| = {err:.3e}")
    assert err <= FP32_RTOL * max(1.0, float(np.abs(g[keep]).max()))


def test_label_rule_matches_the_reference():
    """T = 22 gives 11 encoder frames and 6 mix frames: the reference accepted 5 and 6 labels and raised on 2 and 10."""
    keys = gold("tsvad_w2vbert_keys")
    assert sorted(map(tuple, keys["label_rule.accept"])) == [(22, 5), (22, 6)]
    assert sorted(map(tuple, keys["label_rule.raise"])) == sorted((TSVAD[b][1], nl) for b, nl in RAISES)
    assert ref.mix_frames(22) == 6 and ref.mix_frames(400) == 100 and ref.mix_frames(2) == 1
    for base, nl in RAISES:
        (B, T, _, wseed), x, ts = tsvad_inputs(base)
        cfg = tsvad_cfg(base)
        with pytest.raises(AssertionError, match=r"label and ref_speech\(mix speech\) diff"):
            ref.tsvad_forward(to_torch(tsvad_state_dict(cfg, seed=wseed)), cfg, torch.from_numpy(x), torch.from_numpy(ts), nl)


def test_odd_frame_count_is_refused_as_the_reference_raises():
    keys = gold("tsvad_w2vbert_keys")
    assert "is invalid for input of size" in str(keys["odd_T_raises"])      # the reference's own error text
    with pytest.raises(ValueError, match="even number of fbank frames"):
        ref.pair_frames(torch.zeros(2, 21, 80))


def test_variant_rules():
    c = TSVADConfig(speech_encoder_type="w2v-bert2")
    assert c.variant == 7 and c.backend == 0 and c.n_mels == 80 and not c.waveform_input
    assert c.w2vbert_cfg is None and c.effective_w2vbert_cfg().num_hidden_layers == 6      # the published geometry
    deep = W2vBertConfig(num_hidden_layers=24)
    c2 = TSVADConfig(speech_encoder_type="w2v-bert2", w2vbert_cfg=deep, select_encoder_layer_nums=2)
    assert c2.variant == 7 and c2.effective_w2vbert_cfg().num_hidden_layers == 2 and deep.num_hidden_layers == 24
    for kw in (dict(single_backend_type="mamba2"), dict(single_backend_type="mamba2", multi_backend_type="mamba2"),
               dict(single_backend_type="conformer_ots_vad", multi_backend_type="lstm_ots_vad"),
               dict(ots_vad_style="v1")):
        with pytest.raises(ValueError, match="transformer single and multi back ends only"):
            TSVADConfig(speech_encoder_type="w2v-bert2", **kw).variant
    for field, bad in (("hidden_size", 768), ("num_attention_heads", 8), ("intermediate_size", 3072),
                       ("conv_depthwise_kernel_size", 15), ("left_max_position_embeddings", 32),
                       ("right_max_position_embeddings", 0), ("feature_projection_input_dim", 80),
                       ("position_embeddings_type", "rotary"), ("add_adapter", True), ("hidden_act", "gelu")):
        with pytest.raises(ValueError, match=field):
            TSVADConfig(speech_encoder_type="w2v-bert2", w2vbert_cfg=W2vBertConfig(**{field: bad})).variant
    with pytest.raises(ValueError, match="num_hidden_layers must be 1..24"):      # after the override
        TSVADConfig(speech_encoder_type="w2v-bert2", select_encoder_layer_nums=0).variant
    with pytest.raises(ValueError, match="unsupported TS-VAD configuration.*w2v-bert2 with transformer"):
        TSVADConfig(speech_encoder_type="hubert").variant
    assert TSVADConfig().variant == 0


def test_layout_matches_reference_keys():
    keys = gold("tsvad_w2vbert_keys")
    assert (keys["perturbation.fp32_bars"] >= 10).all() and len(keys["perturbation.names"]) == 9
    for tag, name in (("se192_d2_l2", "tsvad_w2vbert_t100"), ("se256_d2_l2", "tsvad_w2vbert_se256"),
                      ("se192_d4_l2", "tsvad_w2vbert_cut")):
        want = {n: tuple(int(d) for d in s.split(",") if d) for n, s in zip(keys[tag + ".names"], keys[tag + ".shapes"])}
        cfg = tsvad_cfg(name)
        lay = [(n, tuple(s)) for n, s, _ in tsvad_layout(cfg)]
        assert dict(lay) == want, (set(dict(lay)) ^ set(want))
        assert "speech_encoder.masked_spec_embed" in want
        sd = tsvad_state_dict(cfg, seed=3)
        assert {k: tuple(v.shape) for k, v in sd.items()} == want


def test_tsvad_create_variant_7_rules():
    """sd_tsvad_create: variant 7 takes backend 0 and precision 0 / 1 only, a depth of 1..24 and proj_layer sizes."""
    good = dict(variant=7, max_num_speaker=4, rs_len=4, max_batch=1, max_fbank_frames=398, precision=0,
                num_transformer_layer=2, num_attention_head=4, transformer_embed_dim=384,
                transformer_ffn_embed_dim=1536, speaker_embed_dim=192, w2vbert_layers=2)
    for bad, msg in ((dict(precision=2), "bf16x3"), (dict(backend=1, d_state=64, expand=4), "variant 0"),
                     (dict(w2vbert_layers=0), "w2vbert_layers must be 1..24"),
                     (dict(w2vbert_layers=25), "w2vbert_layers must be 1..24"),
                     (dict(speaker_embed_dim=200), "multiple of 32")):
        h = ctypes.c_void_p()
        with pytest.raises(ValueError, match=msg):
            _lib.call("sd_tsvad_create", ctypes.byref(_lib.TsvadConfig(**dict(good, **bad))), ctypes.byref(h))
        assert h.value is None
    # the depth field is the struct's last: a config that ends before it, zero-extended, is an older model
    assert _lib.TsvadConfig._fields_[-1][0] == "w2vbert_layers"
