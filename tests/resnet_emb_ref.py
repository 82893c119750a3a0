"""The WeSpeaker ResNet34 embedding extractor and TS-VAD with proj_layer restated with torch.nn.functional on CPU.

Written from the architecture: the ResNet34 trunk of tsvad_resnet_ref.py (prefix ""), temporal statistics pooling
(mean and sqrt(unbiased variance + 1e-7) over time of the (B, 2560, T') map), seg_1 Linear(5120 -> E)
[-> ReLU -> BatchNorm1d(affine=False) -> seg_2 Linear(E -> E)]; the extractor's chunk loop (6 s every 1 s, or the
whole file); and the TS-VAD forward whose per-speaker input goes through proj_layer = Linear(2 SE, E) when
2 SE != E.  `sd` is a flat state_dict of torch tensors under the reference key names.  Pinned against
tests/golden/resnet_emb*.npz and tsvad_proj_*.npz (reference outputs) by tests/test_resnet_emb_host.py.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tsvad_ref
from oracle.tsvad_ref import _bn, _bn1d_nan_bypass, positional_encoding, transformer_layer

import tsvad_resnet_ref as rn


def tstp(x):
    """(B, C, T) -> (B, 2C): [mean | sqrt(var_unbiased + 1e-7)] over time."""
    return torch.cat((x.mean(dim=-1), torch.sqrt(torch.var(x, dim=-1) + 1e-7)), 1)


@torch.no_grad()
def resnet34_embedding(sd, fbank, two_emb_layer=False):
    """fbank (B, T, 80) -> dict(time_out (B, 2560, T'), stats (B, 5120), embed_a, embed_b or None)."""
    tout = rn.resnet34_time_out(sd, fbank, pre="")
    stats = tstp(tout)
    a = F.linear(stats, sd["seg_1.weight"], sd["seg_1.bias"])
    b = None
    if two_emb_layer:
        b = F.linear(_bn(F.relu(a), sd, "seg_bn_1"), sd["seg_2.weight"], sd["seg_2.bias"])
    return dict(time_out=tout, stats=stats, embed_a=a, embed_b=b)


def extract_embed(sd, wav, length_embedding=6.0, step_embedding=1.0, batch_size=96):
    """The extractor's chunk loop with FBank(80, mean_nor=True): wav float64 in [-1, 1) -> (n_chunks, E) float32."""
    from oracle.fbank_ref import embed_fbank
    chunks = tsvad_ref.embedding_chunks(len(wav), length_embedding, step_embedding)
    feats = [embed_fbank(wav[a:b]) for a, b in chunks]
    out = []
    for i in range(0, len(feats), batch_size):
        out.append(resnet34_embedding(sd, torch.from_numpy(np.stack(feats[i:i + batch_size])))["embed_a"])
    return torch.cat(out)


def proj_split(w, se):
    """proj_layer.weight (E, 2 SE) -> (W_ts, W_mix): Linear(cat(ts, mix)) = W_ts ts + W_mix mix + b."""
    return w[:, :se], w[:, se:]


@torch.no_grad()
def tsvad_forward(sd, cfg, ref_speech, target_speech, max_len):
    """TS-VAD (CAM++ or ResNet34 speech encoder, transformer back ends) with proj_layer when the state_dict has
    one: ref_speech (B, T_fb, 80), target_speech (B, NS, SE) -> logits (B, NS, max_len)."""
    x = rn.speech_encoder_out(sd, ref_speech) if cfg.variant == 2 else tsvad_ref.speech_encoder_out(sd, ref_speech)
    gap = x.size(-1) - max_len
    assert -1 <= gap <= 2, f"label and ref_speech(mix speech) diff: {gap}"
    assert gap != -1 or cfg.variant != 2, "the reference raises here (its pad call is misspelt)"
    if gap == -1:
        x = F.pad(x, (0, 1))
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
