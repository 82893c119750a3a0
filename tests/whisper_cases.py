"""The cases of the Whisper-PMFA goldens (tests/golden/make_golden_whisper.py, make_golden_tsvad_whisper.py), shared by
the generators and the tests: geometries, seeds, shapes and the seeded inputs.  No reference import."""
from __future__ import annotations

import numpy as np

# ModelDimensions fields: (n_audio_state, n_audio_head, n_audio_layer, layer_st, layer_ed)
S = (256, 4, 4, 1, 3)
WD = (1280, 20, 3, 1, 2)          # the published width and head count, two concatenated layers
PUBLISHED = (1280, 20, 24, 16, 23)
N_CTX = 1500

# stand-alone encoder: name -> (geometry, n_mels, B, n_samples, input seed, weight seed)
TRUNK = {
    "whisper_s_t50": (S, 80, 2, 16000, 401, 4001),
    "whisper_s_t1": (S, 80, 1, 400, 402, 4002),
    "whisper_wd_t10": (WD, 80, 1, 3200, 403, 4003),
}

# TS-VAD: name -> (geometry, n_mels, B, n_samples, n_label, speaker_embed_dim, input seed, weight seed)
TSVAD = {
    "tsvad_whisper_s": (S, 80, 2, 16000, 25, 192, 411, 4011),
    "tsvad_whisper_rs4": (S, 80, 1, 64000, 100, 192, 412, 4012),
    "tsvad_whisper_pad2": (S, 80, 2, 3280, 7, 192, 413, 4013),
    "tsvad_whisper_pad3": (S, 80, 2, 3280, 8, 192, 413, 4013),
    "tsvad_whisper_cut3": (S, 80, 2, 3280, 2, 192, 413, 4013),
    "tsvad_whisper_t1": (S, 80, 1, 640, 1, 192, 414, 4014),
    "tsvad_whisper_odd": (S, 80, 2, 16160, 25, 192, 415, 4015),
    "tsvad_whisper_tail": (S, 80, 2, 16000, 25, 192, 416, 4016),
    "tsvad_whisper_m128": (S, 128, 2, 16000, 25, 192, 417, 4017),
    "tsvad_whisper_wide": (WD, 80, 1, 16000, 25, 192, 418, 4018),
    "tsvad_whisper_se256": (S, 80, 2, 16000, 25, 256, 419, 4019),
}
NAN = {"tsvad_whisper_nan": ("tsvad_whisper_s", 1, 777)}   # base case, window, sample of the NaN
RAISES = (("tsvad_whisper_pad3", 9), ("tsvad_whisper_pad3", 1))   # label lengths the reference asserts on (5 mix frames)
TAIL_FROM = 8000        # tsvad_whisper_tail: window 1 is zero from this sample on (the collater's padding)
PERTURB_CASE = "tsvad_whisper_s"


def config(geom, n_mels=80):
    from speaker_diarization_amd.ssl.whisper import WhisperConfig
    D, H, L, st, ed = geom
    return WhisperConfig(n_mels=n_mels, n_audio_ctx=N_CTX, n_audio_state=D, n_audio_head=H, n_audio_layer=L,
                         layer_st=st, layer_ed=ed)


def wave(B, n, seed):
    """0.5 N(0, 1)."""
    return (np.random.default_rng(seed).standard_normal((B, n)) * 0.5).astype(np.float32)


def trunk_input(name):
    _, _, B, n, iseed, _ = TRUNK[name]
    return wave(B, n, iseed)


def tsvad_cfg(name):
    from speaker_diarization_amd.weights import TSVADConfig
    geom, n_mels, _, _, _, se, _, _ = TSVAD[NAN[name][0] if name in NAN else name]
    return TSVADConfig(speech_encoder_type="whisper", whisper_n_mels=n_mels, whisper_cfg=config(geom, n_mels),
                       speaker_embed_dim=se)


def tsvad_inputs(name):
    base, nan_at = (NAN[name][0], NAN[name][1:]) if name in NAN else (name, None)
    _, _, B, n, n_lab, se, iseed, wseed = TSVAD[base]
    rng = np.random.default_rng(iseed)
    wav = (rng.standard_normal((B, n)) * 0.5).astype(np.float32)
    ts = rng.standard_normal((B, 4, se)).astype(np.float32)
    if base == "tsvad_whisper_tail":
        wav[1, TAIL_FROM:] = 0.0
    if nan_at is not None:
        wav[nan_at] = np.nan
    return (B, n, n_lab, wseed), wav, ts
