"""Torch restatement of TS-VAD with the WavLM speech encoders (speech_encoder_type "WavLM" / "WavLM_weight_sum" with
wavlm_fuse_feat_post_norm; variants 5 / 6) on top of tests/wavlm_ref.py and the back end pieces of oracle/tsvad_ref.py.

    ref_speech (B, n_samples) -> WavLM -> [weights -> wavlmproj -> wavlmlnorm] -> Conv1d(k5, stride 2, pad 2) ->
    BatchNorm1D (NaN bypass) -> ReLU -> the MagicData length rule -> variant 0's transformer back end
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import wavlm_ref  # noqa: E402
from oracle.tsvad_ref import _bn1d_nan_bypass, positional_encoding, transformer_layer  # noqa: E402

PRE = "speech_encoder."


def wavlm_frames(n_samples: int) -> int:
    return (n_samples - 400) // 320 + 1


def mix_frames(n_samples: int) -> int:
    return (wavlm_frames(n_samples) - 1) // 2 + 1


def encoder_map(sd, cfg, wav):
    """(B, T, C): the map speech_down_or_up's conv reads, C = the WavLM width (variant 5) or speaker_embed_dim (6)."""
    w = cfg.effective_wavlm_cfg()
    enc = {k[len(PRE):]: v for k, v in sd.items() if k.startswith(PRE)}
    if cfg.variant == 5:
        return wavlm_ref.extract_features(enc, w, wav)["x"]
    layers = wavlm_ref.extract_features(enc, w, wav, output_layer=w.encoder_layers)["layers"]
    x = (torch.stack(layers[1:], -1) * sd["weights.weight"][0]).sum(-1)      # the input to layer 0 is dropped
    x = F.linear(x, sd["wavlmproj.weight"], sd["wavlmproj.bias"])
    return F.layer_norm(x, (x.shape[-1],), sd["wavlmlnorm.weight"], sd["wavlmlnorm.bias"])


def speech_encoder_out(sd, cfg, wav):
    """(B, speaker_embed_dim, T3): speech_down_or_up's output."""
    x = encoder_map(sd, cfg, wav).transpose(1, 2)
    x = F.conv1d(x, sd["speech_down_or_up.0.weight"], sd["speech_down_or_up.0.bias"], stride=2, padding=2)
    return F.relu(_bn1d_nan_bypass(x, sd, "speech_down_or_up.1.bn"))


def tsvad_forward(sd, cfg, ref_speech, target_speech, max_len):
    """ref_speech (B, n_samples), target_speech (B, NS, D) -> logits (B, NS, max_len)."""
    x = speech_encoder_out(sd, cfg, ref_speech)
    gap = x.size(-1) - max_len
    assert abs(gap) <= 3, f"label and ref_speech(mix speech) diff: {gap}, label len: {max_len}, ref_speech len: {x.size(-1)}"
    if gap < 0:
        x = F.pad(x, (0, -gap))
    mix = x[:, :, :max_len].transpose(1, 2)
    B, T, _ = mix.shape
    nh = cfg.num_attention_head
    outs = []
    for i in range(cfg.max_num_speaker):
        cat = torch.cat((target_speech[:, i, None, :].expand(B, T, -1), mix), 2)
        if "proj_layer.weight" in sd:
            cat = F.linear(cat, sd["proj_layer.weight"], sd["proj_layer.bias"])
        cat = positional_encoding(cat.transpose(0, 1), sd)
        for l in range(cfg.num_transformer_layer):
            cat = transformer_layer(cat, sd, f"single_backend.layers.{l}.", nh)
        outs.append(cat.transpose(0, 1))
    cat = torch.stack(outs).permute(1, 0, 3, 2).reshape(B, -1, T)
    cat = F.relu(_bn1d_nan_bypass(F.conv1d(cat, sd["backend_down.0.weight"], sd["backend_down.0.bias"], padding=2),
                                  sd, "backend_down.1.bn"))
    cat = positional_encoding(cat.permute(2, 0, 1), sd)
    for l in range(cfg.num_transformer_layer):
        cat = transformer_layer(cat, sd, f"multi_backend.layers.{l}.", nh)
    return F.linear(cat.transpose(0, 1), sd["fc.weight"], sd["fc.bias"]).transpose(1, 2)
