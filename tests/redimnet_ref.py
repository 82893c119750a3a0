"""ReDimNetB2 (trunk, 192-d extractor, TS-VAD with it as the speech encoder) restated with torch.nn.functional on CPU
(fp32).

Written from the architecture.  C = 16 channels on F = 72 mel bins; every map has C * F = 1152 values per frame, seen
either as 1-D (B, 1152, T) with channel f * c + ch or as 2-D (B, c, f, T).  Stem: Conv2d(1 -> 16, 3x3, same) and a
LayerNorm over the 16 channels.  Six stages (stride, blocks, reduction) = REDIM_STAGES; each takes a softmax-weighted
sum (per channel) of ALL earlier 1-D outputs, views it 2-D, applies a Conv2d with kernel and stride (stride, 1) that
folds `stride` frequency rows into stride x the channels, then `blocks` ConvNeXt-like blocks
x + pw(gelu(bn(grouped3x3(x)))) with 4 channels per group, views the result 1-D and applies the time-context block:
x + exp(tcm(LN(red(x)))) where red / exp are 1x1 convs to / from hC = 1152 / reduction and tcm is four 1-D ConvNeXt-like
blocks (depthwise k = 7, 19, 31, 59) and one post-LN transformer layer (4 heads, FFN width hC, tanh GELU, eps 1e-6).
The frame-level map is the weighted sum over all seven outputs; the extractor adds attentive statistics pooling with
the global context and a linear layer.  TS-VAD (speech_encoder_type "ReDimNetB2") applies Conv1d(1152 -> D, k5, stride
4, pad 2) + BatchNorm1D (NaN bypass) + ReLU to the frame-level map, brings it to the label length (within 3 frames:
zero-padded when short, cut when long, an assertion beyond) and runs the CAM++ / transformer model's back end.  `sd` is
a flat state_dict of torch tensors under the reference key names.  Pinned against tests/golden/redimnet_*.npz and
tsvad_redimnet_*.npz (reference outputs) by tests/test_redimnet_host.py.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ecapa_ref import astp
from oracle.tsvad_ref import _bn, _bn1d_nan_bypass, positional_encoding, transformer_layer
from speaker_diarization_amd.weights import REDIM_CF, REDIM_KERNELS, REDIM_STAGES

C0, F0, HEADS, LN_EPS = 16, 72, 4, 1e-6


def ln_channels(x, w, b):
    """LayerNorm over dim 1 of (B, C, ...) with the biased variance."""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    x = (x - u) / torch.sqrt(s + LN_EPS)
    shape = (1, -1) + (1,) * (x.dim() - 2)
    return w.view(shape) * x + b.view(shape)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def to1d(x):
    B, c, f, T = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, c * f, T)


def to2d(x, c, f):
    B, _, T = x.shape
    return x.reshape(B, f, c, T).permute(0, 2, 1, 3)


def block2d(sd, p, x):
    """ConvNeXt-like 2-D block at prefix `p` (…conv_block.): x (B, c, f, T)."""
    c = x.shape[1]
    y = F.conv2d(x, sd[p + "dwconvs.0.weight"], sd[p + "dwconvs.0.bias"], padding=1, groups=c // 4)
    y = F.gelu(_bn(y, sd, p + "norm"))
    return x + F.conv2d(y, sd[p + "pwconv1.weight"], sd[p + "pwconv1.bias"])


def block1d(sd, p, x, k):
    y = F.conv1d(x, sd[p + "dwconvs.0.weight"], sd[p + "dwconvs.0.bias"], padding=k // 2, groups=x.shape[1])
    y = F.gelu(_bn(y, sd, p + "norm"))
    return x + F.conv1d(y, sd[p + "pwconv1.weight"], sd[p + "pwconv1.bias"])


def pad_heads(sd, p, hd, hdp):
    """The attention projections at prefix `p` with every head zero-padded from hd to hdp values: q / k / v gain zero
    rows (and zero bias), out_proj zero columns.  Returns (wq, bq, wk, bk, wv, bv, wo)."""
    out = []
    for n in ("q_proj", "k_proj", "v_proj"):
        w, b = sd[p + n + ".weight"], sd[p + n + ".bias"]
        hc = w.shape[1]
        wp = torch.zeros(HEADS, hdp, hc, dtype=w.dtype)
        wp[:, :hd] = w.view(HEADS, hd, hc)
        bp = torch.zeros(HEADS, hdp, dtype=b.dtype)
        bp[:, :hd] = b.view(HEADS, hd)
        out += [wp.reshape(HEADS * hdp, hc), bp.reshape(-1)]
    wo = sd[p + "out_proj.weight"]
    wop = torch.zeros(wo.shape[0], HEADS, hdp, dtype=wo.dtype)
    wop[:, :, :hd] = wo.view(wo.shape[0], HEADS, hd)
    out.append(wop.reshape(wo.shape[0], HEADS * hdp))
    return out


def mha(sd, p, x, pad_to=None):
    """x (B, T, hC) -> (B, T, hC): q scaled by head_dim^-0.5 of the TRUE head width, softmax over the keys."""
    B, T, hc = x.shape
    hd = hc // HEADS
    if pad_to is None:
        wq, bq, wk, bk, wv, bv = (sd[p + n] for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias",
                                                       "v_proj.weight", "v_proj.bias"))
        wo, w = sd[p + "out_proj.weight"], hd
    else:
        wq, bq, wk, bk, wv, bv, wo = pad_heads(sd, p, hd, pad_to)
        w = pad_to
    split = lambda t: t.view(B, T, HEADS, w).transpose(1, 2)   # noqa: E731
    q = split(F.linear(x, wq, bq) * hd ** -0.5)
    k, v = split(F.linear(x, wk, bk)), split(F.linear(x, wv, bv))
    a = torch.softmax(q @ k.transpose(2, 3), -1) @ v
    return F.linear(a.transpose(1, 2).reshape(B, T, HEADS * w), wo, sd[p + "out_proj.bias"])


def transformer(sd, p, x, pad_to=None):
    """Post-LN layer on x (B, hC, T)."""
    h = x.transpose(1, 2)
    hc = h.shape[-1]
    h = F.layer_norm(h + mha(sd, p + "attention.", h, pad_to), (hc,), sd[p + "layer_norm.weight"],
                     sd[p + "layer_norm.bias"], LN_EPS)
    ff = F.linear(gelu_tanh(F.linear(h, sd[p + "feed_forward.intermediate_dense.weight"],
                                     sd[p + "feed_forward.intermediate_dense.bias"])),
                  sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"])
    h = F.layer_norm(h + ff, (hc,), sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], LN_EPS)
    return h.transpose(1, 2)


def time_context(sd, p, x, pad_to=None):
    """TimeContextBlock1d at prefix `p` on x (B, 1152, T)."""
    y = F.conv1d(x, sd[p + "red_dim_conv.0.weight"], sd[p + "red_dim_conv.0.bias"])
    y = ln_channels(y, sd[p + "red_dim_conv.1.weight"], sd[p + "red_dim_conv.1.bias"])
    for j, k in enumerate(REDIM_KERNELS):
        y = block1d(sd, f"{p}tcm.{j}.", y, k)
    y = transformer(sd, p + "tcm.4.", y, pad_to)
    return x + F.conv1d(y, sd[p + "exp_dim_conv.weight"], sd[p + "exp_dim_conv.bias"])


def mix(sd, bb, outs, i):
    w = torch.softmax(sd[f"{bb}inputs_weights.{i}"], 1)           # (1, n, 1152, 1) or (1, 1, 1, 1)
    return (w * torch.stack(outs, 1)).sum(1)


def padded_width(hd):
    return 32 if hd <= 32 else 48 if hd <= 48 else 64 if hd <= 64 else 96


@torch.no_grad()
def frame_level(sd, fbank, pre="", padded=False):
    """fbank (B, T, 72) -> the frame-level map (B, 1152, T).  padded: the attention heads zero-padded as the engine
    uploads them (exact)."""
    bb = pre + "backbone."
    x = fbank.permute(0, 2, 1).unsqueeze(1)                        # (B, 1, F, T)
    x = F.conv2d(x, sd[bb + "stem.0.weight"], sd[bb + "stem.0.bias"], padding=1)
    x = ln_channels(x, sd[bb + "stem.1.weight"], sd[bb + "stem.1.bias"])
    outs = [to1d(x)]
    c, f = C0, F0
    for i, (stride, blocks, red) in enumerate(REDIM_STAGES):
        sp = f"{bb}stage{i}."
        x = to2d(mix(sd, bb, outs, i), c, f)
        x = F.conv2d(x, sd[sp + "0.weight"], sd[sp + "0.bias"], stride=(stride, 1))
        c, f = c * stride, f // stride
        for b in range(1, blocks + 1):
            x = block2d(sd, f"{sp}{b}.conv_block.", x)
        hd = REDIM_CF // red // HEADS
        outs.append(time_context(sd, f"{sp}{blocks + 2}.", to1d(x), padded_width(hd) if padded else None))
    return mix(sd, bb, outs, len(REDIM_STAGES))


@torch.no_grad()
def embed(sd, fbank, padded=False):
    """The extractor: fbank (B, T, 72) -> (embedding (B, E), frame-level map (B, 1152, T))."""
    t = frame_level(sd, fbank, "", padded)
    return F.linear(astp(sd, t), sd["seg_1.weight"], sd["seg_1.bias"]), t


def speech_encoder_out(sd, ref_speech, padded=False):
    """ref_speech (B, T_fb, 72) -> (B, D, (T_fb - 1) // 4 + 1): speech_down_or_up of the frame-level map."""
    x = F.conv1d(frame_level(sd, ref_speech, "speech_encoder.", padded), sd["speech_down_or_up.0.weight"],
                 sd["speech_down_or_up.0.bias"], stride=4, padding=2)
    return F.relu(_bn1d_nan_bypass(x, sd, "speech_down_or_up.1.bn"))


@torch.no_grad()
def tsvad_forward(sd, cfg, ref_speech, target_speech, max_len):
    """ref_speech (B, T_fb, 72), target_speech (B, NS, D) -> logits (B, NS, max_len)."""
    x = speech_encoder_out(sd, ref_speech)
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
