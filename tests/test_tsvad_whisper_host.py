"""TS-VAD with the Whisper-PMFA speech encoder (speech_encoder_type "whisper", variant 8), host side: the torch
restatement (tests/whisper_ref.py) against every reference golden of tests/golden/make_golden_tsvad_whisper.py at the
fp32 bar, the configuration rules, the state_dict layout against the reference's stored key lists, the label-length
rule, and the C ABI: sd_tsvad_create refuses variant 8, sd_tsvad_create_whisper's argument rules, and sd_tsvad_config
keeps its fields."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import whisper_ref as ref  # noqa: E402
from whisper_cases import NAN, PUBLISHED, RAISES, TSVAD, config, tsvad_cfg, tsvad_inputs  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ssl.whisper import WhisperConfig  # noqa: E402
from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_layout, tsvad_state_dict  # noqa: E402

GOLD = os.path.join(HERE, "golden")


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(TSVAD) + list(NAN))
def test_restatement_vs_reference_golden(name):
    (B, n, nl, wseed), wav, ts = tsvad_inputs(name)
    cfg = tsvad_cfg(name)
    g = gold(name)["logits"]
    out = ref.tsvad_forward(to_torch(tsvad_state_dict(cfg, seed=wseed)), cfg, torch.from_numpy(wav),
                            torch.from_numpy(ts), nl).numpy()
    keep = np.isfinite(g)
    assert (np.isfinite(out) == keep).all()
    err = float(np.abs(out[keep] - g[keep]).max())
    print(f"{name}: max|logit diff| = {err:.3e}")
    assert err <= ref.fp32_bar(g[keep])


def test_label_rule_matches_the_reference():
    """3280 samples give 20 mel frames, 10 encoder frames and 5 mix frames: the reference accepted 2, 7 and 8 labels
    (goldens) and raised on 1 and 9."""
    assert ref.mix_frames(3280) == 5 and ref.mix_frames(64000) == 100 and ref.mix_frames(640) == 1
    assert ref.mix_frames(16160) == 26
    for base, nl in RAISES:
        (B, n, _, wseed), wav, ts = tsvad_inputs(base)
        cfg = tsvad_cfg(base)
        with pytest.raises(AssertionError, match=r"label and ref_speech\(mix speech\) diff"):
            ref.tsvad_forward(to_torch(tsvad_state_dict(cfg, seed=wseed)), cfg, torch.from_numpy(wav),
                              torch.from_numpy(ts), nl)


def test_variant_rules():
    c = TSVADConfig(speech_encoder_type="whisper")
    assert c.variant == 8 and c.backend == 0 and c.waveform_input
    w = c.effective_whisper_cfg()      # None: the published ModelDimensions()
    assert c.whisper_cfg is None and (w.n_mels, w.n_audio_state, w.n_audio_layer, w.layer_st, w.layer_ed) == \
        (80, 1280, 24, 16, 23)
    c128 = TSVADConfig(speech_encoder_type="whisper", whisper_n_mels=128)
    assert c128.variant == 8 and c128.effective_whisper_cfg().n_mels == 128
    for kw in (dict(single_backend_type="mamba2"), dict(single_backend_type="mamba2", multi_backend_type="mamba2"),
               dict(single_backend_type="conformer_ots_vad", multi_backend_type="lstm_ots_vad"),
               dict(multi_backend_type="lstm"), dict(single_backend_type="conformer"), dict(ots_vad_style="v1")):
        with pytest.raises(ValueError, match="transformer single and multi back ends only"):
            TSVADConfig(speech_encoder_type="whisper", **kw).variant
    with pytest.raises(ValueError, match="n_mels must be 80 or 128"):
        TSVADConfig(speech_encoder_type="whisper", whisper_n_mels=64).variant
    with pytest.raises(ValueError, match="differs from whisper_n_mels"):
        TSVADConfig(speech_encoder_type="whisper", whisper_n_mels=128, whisper_cfg=WhisperConfig()).variant
    with pytest.raises(ValueError, match="n_audio_state must be 64"):
        TSVADConfig(speech_encoder_type="whisper", whisper_cfg=WhisperConfig(n_audio_head=16)).variant
    with pytest.raises(ValueError, match="at most 16384"):
        TSVADConfig(speech_encoder_type="whisper",
                    whisper_cfg=WhisperConfig(n_audio_layer=32, layer_st=0, layer_ed=31)).variant
    with pytest.raises(ValueError, match="unsupported TS-VAD configuration.*w2v-bert2 with transformer"):
        TSVADConfig(speech_encoder_type="hubert").variant
    # the earlier variants keep their numbers
    assert TSVADConfig().variant == 0 and TSVADConfig(speech_encoder_type="w2v-bert2").variant == 7


def test_layout_matches_reference_keys():
    keys = gold("tsvad_whisper_keys")
    assert (keys["perturbation.fp32_bars"] >= 10).all() and len(keys["perturbation.names"]) == 9
    assert any("clamp removed" in str(n) for n in keys["perturbation.names"])
    pub = TSVADConfig(speech_encoder_type="whisper", whisper_cfg=config(PUBLISHED))
    for tag, cfg in (("s_m80_se192", tsvad_cfg("tsvad_whisper_s")), ("s_m128_se192", tsvad_cfg("tsvad_whisper_m128")),
                     ("wd_m80_se192", tsvad_cfg("tsvad_whisper_wide")), ("s_m80_se256", tsvad_cfg("tsvad_whisper_se256")),
                     ("published", pub)):
        want = {n: tuple(int(d) for d in s.split(",") if d) for n, s in zip(keys[tag + ".names"], keys[tag + ".shapes"])}
        lay = [(n, tuple(s)) for n, s, _ in tsvad_layout(cfg)]
        assert dict(lay) == want, (set(dict(lay)) ^ set(want))
        assert "speech_encoder.positional_embedding" in want and "speech_encoder.mel_filters" not in want
        assert not any(n.endswith("attn.key.bias") for n in want)
    assert dict(zip(keys["published.names"], keys["published.shapes"]))["speech_down_or_up.0.weight"] == "192,10240,5"
    sd = tsvad_state_dict(tsvad_cfg("tsvad_whisper_se256"), seed=3)
    want = {n: tuple(int(d) for d in s.split(",") if d)
            for n, s in zip(keys["s_m80_se256.names"], keys["s_m80_se256.shapes"])}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want and "proj_layer.weight" in want


GOOD = dict(variant=8, max_num_speaker=4, rs_len=4, max_batch=1, max_fbank_frames=398, precision=0,
            num_transformer_layer=2, num_attention_head=4, transformer_embed_dim=384, transformer_ffn_embed_dim=1536,
            speaker_embed_dim=192, max_samples=64000)
WGOOD = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=256, n_audio_head=4, n_audio_layer=4, layer_st=1, layer_ed=3)


def test_tsvad_create_refuses_variant_8_and_points_to_the_call():
    h = ctypes.c_void_p()
    with pytest.raises(ValueError, match="sd_tsvad_create_whisper"):
        _lib.call("sd_tsvad_create", ctypes.byref(_lib.TsvadConfig(**GOOD)), ctypes.byref(h))
    assert h.value is None
    with pytest.raises(ValueError, match="unknown TS-VAD variant"):
        _lib.call("sd_tsvad_create", ctypes.byref(_lib.TsvadConfig(**dict(GOOD, variant=9))), ctypes.byref(h))


def test_tsvad_create_whisper_argument_rules():
    lib = _lib.load()
    h = ctypes.c_void_p()
    conf, wconf = _lib.TsvadConfig(**GOOD), _lib.WhisperConfig(**WGOOD)
    assert lib.sd_tsvad_create_whisper(ctypes.byref(conf), None, ctypes.byref(h)) == _lib.SD_ERR_INVALID
    assert lib.sd_tsvad_create_whisper(None, ctypes.byref(wconf), ctypes.byref(h)) == _lib.SD_ERR_INVALID
    assert lib.sd_tsvad_create_whisper(ctypes.byref(conf), ctypes.byref(wconf), None) == _lib.SD_ERR_INVALID
    for bad, wbad, msg in ((dict(precision=2), {}, "bf16x3"), (dict(backend=1, d_state=64, expand=4), {}, "variant 0"),
                           (dict(variant=5), {}, "variant 8 only"), (dict(speaker_embed_dim=200), {}, "multiple of 32"),
                           (dict(max_samples=0), {}, "max_samples"), ({}, dict(n_mels=64), "n_mels"),
                           ({}, dict(n_audio_head=5), "n_audio_state must be 64"),
                           ({}, dict(layer_ed=4), "layer_ed"), ({}, dict(n_audio_layer=33), "n_audio_layer")):
        with pytest.raises(ValueError, match=msg):
            _lib.call("sd_tsvad_create_whisper", ctypes.byref(_lib.TsvadConfig(**dict(GOOD, **bad))),
                      ctypes.byref(_lib.WhisperConfig(**dict(WGOOD, **wbad))), ctypes.byref(h))
        assert h.value is None
    # (a good pair allocates the handle's pinned flags on the device: tests/test_gpu_tsvad_whisper.py creates those)


def test_tsvad_config_keeps_its_fields():
    """The trunk's geometry travels in sd_whisper_config: sd_tsvad_config gained nothing."""
    assert _lib.TsvadConfig._fields_[-1][0] == "w2vbert_layers"
    assert not any("whisper" in n for n, _ in _lib.TsvadConfig._fields_)
    assert [n for n, _ in _lib.WhisperConfig._fields_] == [
        "n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer", "layer_st", "layer_ed", "precision",
        "max_batch", "max_samples"]
