"""Plain-torch restatement of the w2v-BERT 2.0 trunk (transformers' Wav2Vec2BertModel in eval mode with relative_key
position embeddings, hidden_act "swish", no adapter) and of TS-VAD with it as the speech encoder (speech_encoder_type
"w2v-bert2", variant 7), on state dicts under the HF / reference key names.

    ref_speech (B, T, 80) -> reshape (B, T / 2, 160) -> LayerNorm -> Linear(160 -> 1024)
      -> layers: x += 0.5 ffn1(LN x); x += attn(LN x); x += conv(x); x += 0.5 ffn2(LN x); x = final_layer_norm(x)
      -> hidden_states[-1] -> Conv1d(1024 -> SE, k5, stride 2, pad 2) -> BatchNorm1D (NaN bypass) -> ReLU
      -> the MagicData length rule -> variant 0's transformer back end (oracle/tsvad_ref.py)

emulate_bf16: every GEMM / attention operand is rounded to bf16 as the engine's bf16 mode rounds it (activations and
weights of every projection, q / k / v, the distance embedding, the softmax weights for P V, pointwise_conv1's stored
output, the back end's stored sub-block outputs), with fp32 accumulation, LayerNorms, softmax, depthwise conv and
residual stream: the CPU model of the bf16 mode's error that the GPU tests' bound is derived from.  With it the back
end is restated here too (post-LN transformer layers), since the oracle's runs in fp32 only.
"""
from __future__ import annotations

import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle.tsvad_ref import _bn1d_nan_bypass, positional_encoding, transformer_layer  # noqa: E402

PRE = "speech_encoder."
HEADS, LEFT, RIGHT, KERNEL = 16, 64, 8, 31


def rb(x):
    """fp32 values rounded to bf16 (round to nearest even)."""
    return x.to(torch.bfloat16).float()


def _r(x, emu):
    return rb(x) if emu else x


def linear(x, w, b=None, emu=False):
    return F.linear(_r(x, emu), _r(w, emu), b)


def ln(sd, p, x):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def distance_index(T, device=None):
    pos = torch.arange(T, device=device)
    return torch.clamp(pos[None, :] - pos[:, None], -LEFT, RIGHT) + LEFT     # [query l, key r]


def relative_key_attention(q, k, v, E, emu=False):
    """q, k, v (B, H, T, 64), E (73, 64) -> (B, H, T, 64): softmax((q k^T + q E[clamp(r - l)]^T) / 8) v."""
    q, k, v, E = _r(q, emu), _r(k, emu), _r(v, emu), _r(E, emu)
    T = q.shape[2]
    scores = q @ k.transpose(-1, -2)
    rel = (q @ E.t()).gather(-1, distance_index(T, q.device).expand(q.shape[0], q.shape[1], T, T))
    p = torch.softmax((scores + rel) / math.sqrt(q.shape[-1]), -1)
    if emu:   # P is rounded for P V; the row sum keeps the unrounded values
        m = ((scores + rel) / 8.0).amax(-1, keepdim=True)
        e = torch.exp((scores + rel) / 8.0 - m)
        return (rb(e) @ v) / e.sum(-1, keepdim=True)
    return p @ v


def conv_mix(x, w, g, beta):
    """x (B, T, 2048) pointwise_conv1's output -> (B, T, 1024): GLU, left pad 30 + depthwise k31, LayerNorm, swish."""
    y = F.glu(x.transpose(1, 2), dim=1)
    y = F.conv1d(F.pad(y, (KERNEL - 1, 0)), w, groups=w.shape[0])
    y = F.layer_norm(y.transpose(1, 2), (w.shape[0],), g, beta, 1e-5)
    return F.silu(y)


def encoder_layer(sd, p, x, emu=False):
    def ffn(q, y):
        h = F.silu(linear(y, sd[q + ".intermediate_dense.weight"], sd[q + ".intermediate_dense.bias"], emu))
        return linear(h, sd[q + ".output_dense.weight"], sd[q + ".output_dense.bias"], emu)

    B, T, D = x.shape
    x = x + 0.5 * ffn(p + "ffn1", ln(sd, p + "ffn1_layer_norm", x))
    y = ln(sd, p + "self_attn_layer_norm", x)
    a = p + "self_attn."
    q, k, v = (linear(y, sd[a + n + ".weight"], sd[a + n + ".bias"], emu).view(B, T, HEADS, -1).transpose(1, 2)
               for n in ("linear_q", "linear_k", "linear_v"))
    o = relative_key_attention(q, k, v, sd[a + "distance_embedding.weight"], emu)
    x = x + linear(o.transpose(1, 2).reshape(B, T, D), sd[a + "linear_out.weight"], sd[a + "linear_out.bias"], emu)
    c = p + "conv_module."
    h = linear(ln(sd, c + "layer_norm", x), sd[c + "pointwise_conv1.weight"][:, :, 0], None, emu)
    h = conv_mix(_r(h, emu), sd[c + "depthwise_conv.weight"], sd[c + "depthwise_layer_norm.weight"],
                 sd[c + "depthwise_layer_norm.bias"])
    x = x + linear(h, sd[c + "pointwise_conv2.weight"][:, :, 0], None, emu)
    x = x + 0.5 * ffn(p + "ffn2", ln(sd, p + "ffn2_layer_norm", x))
    return ln(sd, p + "final_layer_norm", x)


@torch.no_grad()
def trunk(sd, layers, x, emulate_bf16=False):
    """input_features (B, T2, 160) -> hidden_states: [input to layer 0, each layer's output] of (B, T2, 1024)."""
    x = linear(ln(sd, "feature_projection.layer_norm", x), sd["feature_projection.projection.weight"],
               sd["feature_projection.projection.bias"], emulate_bf16)
    hs = [x]
    for i in range(layers):
        x = encoder_layer(sd, f"encoder.layers.{i}.", x, emulate_bf16)
        hs.append(x)
    return hs


def pair_frames(ref_speech):
    B, T, C = ref_speech.shape
    if T % 2:
        raise ValueError(f"w2v-bert2 needs an even number of fbank frames, got {T}")
    return ref_speech.reshape(B, T // 2, 2 * C)


def mix_frames(T):
    return (T // 2 - 1) // 2 + 1


def speech_encoder_out(sd, cfg, ref_speech, emu=False):
    """(B, speaker_embed_dim, T3): speech_down_or_up's output."""
    enc = {k[len(PRE):]: v for k, v in sd.items() if k.startswith(PRE)}
    x = trunk(enc, cfg.select_encoder_layer_nums, pair_frames(ref_speech), emu)[-1].transpose(1, 2)
    x = F.conv1d(_r(x, emu), _r(sd["speech_down_or_up.0.weight"], emu), sd["speech_down_or_up.0.bias"], stride=2,
                 padding=2)
    return F.relu(_bn1d_nan_bypass(x, sd, "speech_down_or_up.1.bn"))


def _transformer_layer_bf16(x, sd, p, nh):
    """nn.TransformerEncoderLayer (post-LN, ReLU) on (T, B, E) with the engine's bf16 roundings."""
    T, B, E = x.shape
    a = p + "self_attn."
    qkv = rb(linear(x, sd[a + "in_proj_weight"], sd[a + "in_proj_bias"], True))
    q, k, v = (t.reshape(T, B, nh, E // nh).permute(1, 2, 0, 3) for t in qkv.split(E, -1))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(E // nh)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    o = (rb(e) @ v) / e.sum(-1, keepdim=True)
    o = rb(linear(o.permute(2, 0, 1, 3).reshape(T, B, E), sd[a + "out_proj.weight"], sd[a + "out_proj.bias"], True))
    x = F.layer_norm(x + o, (E,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-5)
    h = F.relu(linear(x, sd[p + "linear1.weight"], sd[p + "linear1.bias"], True))
    h = rb(linear(h, sd[p + "linear2.weight"], sd[p + "linear2.bias"], True))
    return F.layer_norm(x + h, (E,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-5)


@torch.no_grad()
def tsvad_forward(sd, cfg, ref_speech, target_speech, max_len, emulate_bf16=False):
    """ref_speech (B, T, 80), target_speech (B, NS, D) -> logits (B, NS, max_len)."""
    emu = emulate_bf16
    layer = _transformer_layer_bf16 if emu else transformer_layer
    x = speech_encoder_out(sd, cfg, ref_speech, emu)
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
            cat = linear(cat, sd["proj_layer.weight"], sd["proj_layer.bias"], emu)
        cat = positional_encoding(cat.transpose(0, 1), sd)
        for l in range(cfg.num_transformer_layer):
            cat = layer(cat, sd, f"single_backend.layers.{l}.", nh)
        outs.append(cat.transpose(0, 1))
    cat = torch.stack(outs).permute(1, 0, 3, 2).reshape(B, -1, T)
    cat = F.conv1d(_r(cat, emu), _r(sd["backend_down.0.weight"], emu), sd["backend_down.0.bias"], padding=2)
    cat = F.relu(_bn1d_nan_bypass(cat, sd, "backend_down.1.bn"))
    cat = positional_encoding(cat.permute(2, 0, 1), sd)
    for l in range(cfg.num_transformer_layer):
        cat = layer(cat, sd, f"multi_backend.layers.{l}.", nh)
    return linear(cat.transpose(0, 1), sd["fc.weight"], sd["fc.bias"], emu).transpose(1, 2)
