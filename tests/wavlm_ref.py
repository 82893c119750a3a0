"""Functional CPU restatement of WavLM.extract_features over a state dict, written from the published architecture
(WavLM: Chen et al. 2022; the fairseq-style wav2vec 2.0 trunk with a gated relative-position bias).  It is the op-level
oracle of tests/test_gpu_wavlm_ops.py and the one model reference that runs where the reference repository is absent;
tests/test_wavlm_host.py holds it to the goldens the reference module produced.

cfg: any object with encoder_embed_dim, encoder_attention_heads, encoder_layers, extractor_mode, layer_norm_first.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

CONV_LAYERS = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2
NUM_BUCKETS = 320
MAX_DISTANCE = 800


def frames(n_samples: int) -> int:
    n = n_samples
    for _, k, s in CONV_LAYERS:
        n = (n - k) // s + 1
    return n


def conv_layer0(sd, wav, mode: str):
    """wav (B, n) -> (B, 512, T0): conv k10 s5 + (GroupNorm(512, 512) | LayerNorm over channels) + GELU."""
    p = "feature_extractor.conv_layers.0."
    x = F.conv1d(wav.unsqueeze(1), sd[p + "0.weight"], stride=5)
    if mode == "layer_norm":
        x = F.layer_norm(x.transpose(1, 2), (512,), sd[p + "2.1.weight"], sd[p + "2.1.bias"]).transpose(1, 2)
    else:
        x = F.group_norm(x, 512, sd[p + "2.weight"], sd[p + "2.bias"])
    return F.gelu(x)


def conv_layer(sd, x, i: int, mode: str):
    """x (B, 512, T) -> (B, 512, (T - k) // 2 + 1): conv + (LayerNorm in layer_norm mode) + GELU, layers 1..6."""
    p = f"feature_extractor.conv_layers.{i}."
    x = F.conv1d(x, sd[p + "0.weight"], stride=CONV_LAYERS[i][2])
    if mode == "layer_norm":
        x = F.layer_norm(x.transpose(1, 2), (512,), sd[p + "2.1.weight"], sd[p + "2.1.bias"]).transpose(1, 2)
    return F.gelu(x)


def pos_conv_weight(sd):
    """The weight-normalised (dim 2) positional conv weight g v / |v|, from either key spelling."""
    p = "encoder.pos_conv.0."
    if p + "weight_g" in sd:
        g, v = sd[p + "weight_g"], sd[p + "weight_v"]
    else:
        g, v = sd[p + "parametrizations.weight.original0"], sd[p + "parametrizations.weight.original1"]
    return g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()


def pos_conv(sd, x):
    """x (B, T, D) -> x + GELU(pos_conv(x)): 128 taps, padding 64, 16 groups, the last output frame dropped."""
    y = F.conv1d(x.transpose(1, 2), pos_conv_weight(sd), sd["encoder.pos_conv.0.bias"], padding=64, groups=16)
    return x + F.gelu(y[:, :, :-1]).transpose(1, 2)


def buckets(rel):
    """Bucket of each relative position (key - query), bidirectional: 160 per sign, exact below 80, logarithmic up to
    800 (float32 log, as torch evaluates it)."""
    nb = NUM_BUCKETS // 2
    out = (rel > 0).long() * nb
    a = rel.abs()
    exact = nb // 2
    large = exact + (torch.log(a.float() / exact) / math.log(MAX_DISTANCE / exact) * (nb - exact)).long()
    large = torch.clamp(large, max=nb - 1)
    return out + torch.where(a < exact, a, large)


def bias_table(sd, T: int):
    """(H, 2 T - 1): the bias of relative position r = key - query at column r + T - 1."""
    rel = torch.arange(-(T - 1), T)
    return sd["encoder.layers.0.self_attn.relative_attention_bias.weight"][buckets(rel)].t().contiguous()


def gates(sd, i: int, x, H: int):
    """x (B, T, D), the layer's input -> gate (B, H, T)."""
    p = f"encoder.layers.{i}.self_attn."
    B, T, D = x.shape
    q = x.view(B, T, H, D // H).permute(0, 2, 1, 3)
    g = F.linear(q, sd[p + "grep_linear.weight"], sd[p + "grep_linear.bias"]).view(B, H, T, 2, 4).sum(-1)
    ga, gb = torch.sigmoid(g).unbind(-1)
    return ga * (gb * sd[p + "grep_a"].view(1, H, 1) - 1.0) + 2.0


def gated_attention(q, k, v, gate, table):
    """q / k / v (B, H, T, 64), gate (B, H, T), table (H, 2 T - 1) -> softmax(q k^T / 8 + gate * bias) v."""
    T = q.shape[2]
    idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1     # [query, key]
    bias = table[:, idx]                                                   # (H, T, T)
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1]) + gate.unsqueeze(-1) * bias.unsqueeze(0)
    return torch.softmax(s, dim=-1) @ v


def self_attn(sd, i: int, x, H: int, table):
    p = f"encoder.layers.{i}.self_attn."
    B, T, D = x.shape

    def heads(t):
        return t.view(B, T, H, D // H).permute(0, 2, 1, 3)

    q = heads(F.linear(x, sd[p + "q_proj.weight"], sd[p + "q_proj.bias"]))
    k = heads(F.linear(x, sd[p + "k_proj.weight"], sd[p + "k_proj.bias"]))
    v = heads(F.linear(x, sd[p + "v_proj.weight"], sd[p + "v_proj.bias"]))
    o = gated_attention(q, k, v, gates(sd, i, x, H), table)
    return F.linear(o.permute(0, 2, 1, 3).reshape(B, T, D), sd[p + "out_proj.weight"], sd[p + "out_proj.bias"])


def encoder_layer(sd, i: int, x, H: int, table, pre_ln: bool):
    p = f"encoder.layers.{i}."
    D = x.shape[-1]

    def ln(t, name):
        return F.layer_norm(t, (D,), sd[p + name + ".weight"], sd[p + name + ".bias"])

    def ffn(t):
        return F.linear(F.gelu(F.linear(t, sd[p + "fc1.weight"], sd[p + "fc1.bias"])), sd[p + "fc2.weight"],
                        sd[p + "fc2.bias"])

    if pre_ln:
        x = x + self_attn(sd, i, ln(x, "self_attn_layer_norm"), H, table)
        return x + ffn(ln(x, "final_layer_norm"))
    x = ln(x + self_attn(sd, i, x, H, table), "self_attn_layer_norm")
    return ln(x + ffn(x), "final_layer_norm")


def extract_features(sd, cfg, wav, output_layer=None):
    """wav (B, n) -> dict(x (B, T, D), features (B, T, D), layers: list of (B, T, D), empty without output_layer)."""
    mode, pre_ln = cfg.extractor_mode, bool(cfg.layer_norm_first)
    D, H, L = cfg.encoder_embed_dim, cfg.encoder_attention_heads, cfg.encoder_layers
    x = conv_layer0(sd, wav, mode)
    for i in range(1, 7):
        x = conv_layer(sd, x, i, mode)
    x = F.layer_norm(x.transpose(1, 2), (512,), sd["layer_norm.weight"], sd["layer_norm.bias"])
    features = F.linear(x, sd["post_extract_proj.weight"], sd["post_extract_proj.bias"])
    x = pos_conv(sd, features)
    if not pre_ln:
        x = F.layer_norm(x, (D,), sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"])
    table = bias_table(sd, x.shape[1])
    layers = [x] if output_layer is not None else []
    for i in range(L if output_layer is None else output_layer):
        x = encoder_layer(sd, i, x, H, table, pre_ln)
        if output_layer is not None:
            layers.append(x)
    if pre_ln and output_layer is None:
        x = F.layer_norm(x, (D,), sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"])
    return dict(x=x, features=features, layers=layers)
