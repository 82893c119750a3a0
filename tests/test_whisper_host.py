"""Whisper-PMFA encoder, host side: the CPU restatement (tests/whisper_ref.py) against the reference module's goldens,
the state_dict layout against the reference's, the mel matrix against transformers', the configuration rules and the
C ABI's refusals.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import whisper_ref as ref  # noqa: E402
from whisper_cases import PUBLISHED, S, TRUNK, WD, config, trunk_input  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.feature import whisper_mel_filters  # noqa: E402
from speaker_diarization_amd.ssl.whisper import WhisperConfig, WhisperEncoder, check_config, check_samples, frames  # noqa: E402
from speaker_diarization_amd.weights import to_torch, whisper_layout, whisper_sinusoids, whisper_state_dict  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(TRUNK))
def test_restatement_matches_the_reference_golden(name):
    geom, n_mels, B, n, _, wseed = TRUNK[name]
    cfg = config(geom, n_mels)
    g = gold(name)
    got = ref.encoder(to_torch(whisper_state_dict(cfg, wseed)), cfg, torch.from_numpy(trunk_input(name))).numpy()
    assert got.shape == g["x"].shape == (B, frames(n), cfg.out_dim)
    err = float(np.abs(got - g["x"]).max())
    print(f"{name}: restatement vs reference {err:.3e}")
    assert err <= ref.fp32_bar(g["x"])
    # every wrong implementation the generator tried moved the output by ten bars or more
    assert len(g["perturbation_names"]) >= 4 and g["perturbation_fp32_bars"].min() >= 10


@pytest.mark.parametrize("tag,geom,n_mels", [("s", S, 80), ("s128", S, 128), ("wd", WD, 80), ("published", PUBLISHED, 80)])
def test_layout_is_the_reference_modules(tag, geom, n_mels):
    k = gold("whisper_keys")
    lay = whisper_layout(config(geom, n_mels))
    assert [n for n, _, _ in lay] == list(k[tag + ".names"])
    assert [",".join(str(d) for d in s) for _, s, _ in lay] == list(k[tag + ".shapes"])
    assert not any(n.endswith("attn.key.bias") for n, _, _ in lay)


def test_state_dict_follows_the_layout_and_perturbs_the_positions():
    cfg = config(S)
    sd = whisper_state_dict(cfg, 5)
    assert [(n, s) for n, s, _ in whisper_layout(cfg)] == [(n, v.shape) for n, v in sd.items()]
    assert all(v.dtype == np.float32 for v in sd.values())
    # the loaded table is not the sinusoid: a model that recomputes it misses the goldens
    assert np.abs(sd["positional_embedding"] - whisper_sinusoids(cfg.n_audio_ctx, cfg.n_audio_state)).max() > 0.1
    assert [n for n, _, _ in whisper_layout(cfg, "speech_encoder.")][0] == "speech_encoder.positional_embedding"


@pytest.mark.parametrize("n_mels", [80, 128])
def test_mel_matrix_is_transformers(n_mels):
    from transformers import WhisperFeatureExtractor
    want = WhisperFeatureExtractor(feature_size=n_mels).mel_filters.T
    got = whisper_mel_filters(n_mels)
    assert got.shape == (n_mels, 201) and got.dtype == np.float32
    assert np.abs(got - want).max() <= 1e-7
    with pytest.raises(ValueError, match="n_mels must be 80 or 128"):
        whisper_mel_filters(64)


def test_restated_log_mel_fp32_against_float64():
    wav = torch.from_numpy(trunk_input("whisper_s_t50"))
    a = ref.log_mel_batch(wav, 80).numpy()
    b = ref.log_mel_batch(wav, 80, torch.float64).numpy()
    assert a.shape == (2, 80, 100) and np.abs(a - b).max() <= 1.5e-5
    # a NaN sample: torch's max / maximum make the whole window NaN
    w = wav[0].clone()
    w[777] = float("nan")
    assert torch.isnan(ref.log_mel(w, 80)).all()


def test_defaults_are_the_references():
    c = WhisperConfig()
    assert (c.n_mels, c.n_audio_ctx, c.n_audio_state, c.n_audio_head, c.n_audio_layer, c.layer_st, c.layer_ed) == \
        (80, 1500, 1280, 20, 24, 16, 23)
    assert c.out_dim == 10240 and c.n_cat == 8
    check_config(c)
    assert frames(16000) == 50 and frames(16160) == 51 and frames(400) == 1 and frames(640) == 2


@pytest.mark.parametrize("kw,field", [
    (dict(n_mels=64), "n_mels"),
    (dict(n_audio_state=1280, n_audio_head=16), "n_audio_state must be 64"),
    (dict(n_audio_state=96, n_audio_head=2), "n_audio_state must be 64"),
    (dict(n_audio_layer=0), "n_audio_layer"),
    (dict(n_audio_layer=33), "n_audio_layer"),
    (dict(layer_st=17, layer_ed=16), "layer_st"),
    (dict(layer_st=-1), "layer_st"),
    (dict(layer_ed=24), "layer_ed"),
    (dict(n_audio_layer=32, layer_st=0, layer_ed=31), "at most 16384"),
    (dict(n_audio_ctx=0), "n_audio_ctx"),
])
def test_config_refusals_name_the_field(kw, field):
    with pytest.raises(ValueError, match=field):
        check_config(WhisperConfig(**kw))


def test_sample_rules():
    c = config(S)
    with pytest.raises(ValueError, match="at least 400"):
        check_samples(c, 399)
    check_samples(c, 400)
    small = WhisperConfig(n_audio_ctx=10, n_audio_state=256, n_audio_head=4, n_audio_layer=2, layer_st=0, layer_ed=1)
    check_samples(small, 3200)          # 20 mel frames -> 10
    with pytest.raises(ValueError, match="truncates.*label-length assertion"):
        check_samples(small, 3520)      # 22 mel frames -> 11


def test_wrapper_refuses_before_touching_the_device():
    with pytest.raises(ValueError, match="bf16x3"):
        WhisperEncoder(config(S), precision="bf16x3")
    with pytest.raises(ValueError, match="n_mels"):
        WhisperEncoder(WhisperConfig(n_mels=40))


def _create(**kw):
    base = dict(n_mels=80, n_audio_ctx=1500, n_audio_state=256, n_audio_head=4, n_audio_layer=4, layer_st=1, layer_ed=3,
                precision=0, max_batch=2, max_samples=16000)
    base.update(kw)
    h = ctypes.c_void_p()
    rc = _lib.load().sd_whisper_create(ctypes.byref(_lib.WhisperConfig(**base)), ctypes.byref(h))
    return rc, h, _lib.load().sd_last_error().decode()


@pytest.mark.parametrize("kw,field", [
    (dict(precision=2), "bf16x3"),
    (dict(n_mels=64), "n_mels"),
    (dict(n_audio_head=5), "n_audio_state must be 64"),
    (dict(n_audio_layer=33), "n_audio_layer"),
    (dict(layer_st=4, layer_ed=3), "layer_st"),
    (dict(layer_ed=4), "layer_ed"),
    (dict(n_audio_state=2048, n_audio_head=32, n_audio_layer=9, layer_st=0, layer_ed=8), "16384"),
    (dict(max_batch=0), "max_batch"),
    (dict(max_samples=399), "max_samples"),
])
def test_abi_create_refusals(kw, field):
    rc, h, msg = _create(**kw)
    assert rc == _lib.SD_ERR_INVALID and not h.value
    assert field in msg


def test_abi_lifecycle_without_weights():
    """create and destroy need no device; forward before finalize is a state error, null arguments are invalid."""
    lib = _lib.load()
    rc, h, _ = _create()
    assert rc == _lib.SD_OK and h.value
    assert lib.sd_whisper_device_bytes(h) == 0
    assert lib.sd_whisper_forward(h, None, 1, 400, None, None) == _lib.SD_ERR_INVALID
    assert lib.sd_whisper_destroy(h) == _lib.SD_OK
    assert lib.sd_whisper_create(None, None) == _lib.SD_ERR_INVALID
    assert lib.sd_whisper_frames(399) == 0 and lib.sd_whisper_frames(400) == 1 and lib.sd_whisper_frames(64000) == 200
    assert "whisper" in _lib.KINDS and "sd_whisper_forward" in _lib.EXPORTED
