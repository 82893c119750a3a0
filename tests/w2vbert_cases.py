"""The cases of the w2v-BERT 2.0 goldens (tests/golden/make_golden_w2vbert.py), shared by the generator and the tests:
seeds, shapes and the seeded inputs.  No reference and no `transformers` import."""
from __future__ import annotations

import numpy as np

# trunk: name -> (layers, B, T2, input seed, weight seed, store every layer)
TRUNK = {
    "w2vbert_t1": (2, 1, 1, 301, 3001, False),
    "w2vbert_t11": (2, 2, 11, 302, 3002, True),
    "w2vbert_t66": (2, 1, 66, 303, 3003, False),
    "w2vbert_t200": (2, 1, 200, 304, 3004, False),
}
# TS-VAD: name -> (B, T, n_label, speaker_embed_dim, config depth, select_encoder_layer_nums, input seed, weight seed)
TSVAD = {
    "tsvad_w2vbert_t100": (2, 100, 25, 192, 2, 2, 311, 3011),
    "tsvad_w2vbert_rs4": (1, 400, 100, 192, 2, 2, 312, 3012),
    "tsvad_w2vbert_t22_l5": (2, 22, 5, 192, 2, 2, 313, 3013),
    "tsvad_w2vbert_t22_l6": (2, 22, 6, 192, 2, 2, 313, 3013),
    "tsvad_w2vbert_t2": (1, 2, 1, 192, 2, 2, 314, 3014),
    "tsvad_w2vbert_se256": (2, 100, 25, 256, 2, 2, 315, 3015),
    "tsvad_w2vbert_cut": (2, 100, 25, 192, 4, 2, 316, 3016),
}
NAN = {"tsvad_w2vbert_nan": ("tsvad_w2vbert_t100", 1, 33, 7)}   # base case, window, frame, bin of the NaN
RAISES = (("tsvad_w2vbert_t22_l5", 2), ("tsvad_w2vbert_t22_l5", 10))   # label lengths the reference asserts on (6 mix frames)
PERTURB_CASE = "tsvad_w2vbert_rs4"


def keep_frames(T: int):
    """Frames of a trunk output that are stored: both ends, the clamp edges and the tile edges."""
    want = {0, 1, 8, 9, 10, 15, 16, 17, 30, 31, 63, 64, 65, T // 2, T - 2, T - 1}
    return sorted(t for t in want if 0 <= t < T)


def trunk_config(layers):
    from speaker_diarization_amd.ssl.w2vbert import W2vBertConfig
    return W2vBertConfig(num_hidden_layers=layers)


def trunk_input(name):
    _, B, T2, iseed, _, _ = TRUNK[name]
    return np.random.default_rng(iseed).standard_normal((B, T2, 160)).astype(np.float32)


def tsvad_cfg(name):
    from speaker_diarization_amd.weights import TSVADConfig
    _, _, _, se, depth, select, _, _ = TSVAD[NAN[name][0] if name in NAN else name]
    return TSVADConfig(speech_encoder_type="w2v-bert2", w2vbert_cfg=trunk_config(depth),
                       select_encoder_layer_nums=select, speaker_embed_dim=se)


def tsvad_inputs(name):
    base, nan_at = (NAN[name][0], NAN[name][1:]) if name in NAN else (name, None)
    B, T, n_lab, se, _, _, iseed, wseed = TSVAD[base]
    rng = np.random.default_rng(iseed)
    ref = rng.standard_normal((B, T, 80)).astype(np.float32)
    ts = rng.standard_normal((B, 4, se)).astype(np.float32)
    if nan_at is not None:
        ref[nan_at] = np.nan
    return (B, T, n_lab, wseed), ref, ts
