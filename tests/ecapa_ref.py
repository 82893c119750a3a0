"""ECAPA-TDNN (c1024, global-context ASTP) and TS-VAD with it as the speech encoder, restated with
torch.nn.functional on CPU (fp32).

Written from the architecture: layer1 = conv(80 -> 1024, k5, pad 2) -> ReLU -> BatchNorm (in that order: the norm
follows the rectifier everywhere in this trunk); three SE-Res2 blocks at dilation 2, 3, 4, each
x + SE(conv1x1(Res2(conv1x1(x)))) with the Res2 chain over 8 groups of 128 channels (stage i convolves the previous
stage's output plus group i, group 7 passes through) and SE = sigmoid(W2 relu(W1 mean_t)); the three block outputs
concatenated and a 1x1 conv 3072 -> 1536 + ReLU.  TS-VAD then applies Conv1d(1536 -> D, k5, stride 4, pad 2) +
BatchNorm1D (NaN bypass) + ReLU and the CAM++/transformer model's back end; the extractor applies attentive statistics
pooling with the global context, BatchNorm and a linear layer.  `sd` is a flat state_dict of torch tensors under the
reference key names.  Pinned against tests/golden/tsvad_ecapa_*.npz and ecapa_emb*.npz (reference outputs) by
tests/test_ecapa_host.py.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.tsvad_ref import _bn, _bn1d_nan_bypass, positional_encoding, transformer_layer

DILATIONS = {2: 2, 3: 3, 4: 4}
WIDTH, STAGES = 128, 7


def _conv_relu_bn(sd, p, x, padding=0, dilation=1):
    y = F.conv1d(x, sd[p + "conv.weight"], sd[p + "conv.bias"], padding=padding, dilation=dilation)
    return _bn(F.relu(y), sd, p + "bn")


def res2_chain(sd, p, x, dilation):
    """x (B, 1024, T) -> (B, 1024, T): `p` is the Res2Conv1dReluBn prefix (convs.i / bns.i)."""
    groups = torch.split(x, WIDTH, 1)
    out, sp = [], None
    for i in range(STAGES):
        sp = groups[i] if i == 0 else sp + groups[i]
        sp = F.conv1d(sp, sd[f"{p}convs.{i}.weight"], sd[f"{p}convs.{i}.bias"], padding=dilation, dilation=dilation)
        sp = _bn(F.relu(sp), sd, f"{p}bns.{i}")
        out.append(sp)
    out.append(groups[STAGES])
    return torch.cat(out, 1)


def se_gate(sd, p, y):
    """y (B, 1024, T) -> the per-(window, channel) gate (B, 1024): the mean runs over every frame of the call."""
    g = F.relu(F.linear(y.mean(2), sd[p + "linear1.weight"], sd[p + "linear1.bias"]))
    return torch.sigmoid(F.linear(g, sd[p + "linear2.weight"], sd[p + "linear2.bias"]))


def se_res2_block(sd, p, x, dilation, gates=None):
    q = p + "se_res2block."
    y = _conv_relu_bn(sd, q + "0.", x)
    y = res2_chain(sd, q + "1.", y, dilation)
    y = _conv_relu_bn(sd, q + "2.", y)
    g = se_gate(sd, q + "3.", y)
    if gates is not None:
        gates.append(g)
    return x + y * g.unsqueeze(2)


def ecapa_time_out(sd, fbank, pre="speech_encoder.", gates=None):
    """fbank (B, T, 80) -> (B, 1536, T), the time axis never subsampled."""
    out = _conv_relu_bn(sd, pre + "layer1.", fbank.permute(0, 2, 1), padding=2)
    outs = []
    for layer, dil in DILATIONS.items():
        out = se_res2_block(sd, f"{pre}layer{layer}.", out, dil, gates)
        outs.append(out)
    return F.relu(F.conv1d(torch.cat(outs, 1), sd[pre + "conv.weight"], sd[pre + "conv.bias"]))


def astp(sd, x, p="pool.", alpha_out=None):
    """Attentive statistics pooling with the global context: x (B, C, T) -> (B, 2 C) [mean | std]."""
    T = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    std = torch.sqrt(x.var(-1, keepdim=True) + 1e-7)   # unbiased: NaN at T == 1
    x_in = torch.cat((x, mean.expand(-1, -1, T), std.expand(-1, -1, T)), 1)
    a = torch.tanh(F.conv1d(x_in, sd[p + "linear1.weight"], sd[p + "linear1.bias"]))
    a = torch.softmax(F.conv1d(a, sd[p + "linear2.weight"], sd[p + "linear2.bias"]), 2)
    if alpha_out is not None:
        alpha_out.append(a)
    m = (a * x).sum(2)
    var = (a * x * x).sum(2) - m * m
    return torch.cat((m, torch.sqrt(var.clamp(min=1e-7))), 1)


@torch.no_grad()
def ecapa_embed(sd, fbank):
    """The extractor: fbank (B, T, 80) -> (embedding (B, E), pre-bn ASTP statistics (B, 3072), time output)."""
    t = ecapa_time_out(sd, fbank, "")
    stats = astp(sd, t)
    z = _bn(stats.unsqueeze(2), sd, "bn").squeeze(2)
    return F.linear(z, sd["linear.weight"], sd["linear.bias"]), stats, t


def speech_encoder_out(sd, ref_speech):
    x = F.conv1d(ecapa_time_out(sd, ref_speech), sd["speech_down_or_up.0.weight"], sd["speech_down_or_up.0.bias"],
                 stride=4, padding=2)
    return F.relu(_bn1d_nan_bypass(x, sd, "speech_down_or_up.1.bn"))


@torch.no_grad()
def tsvad_forward(sd, cfg, ref_speech, target_speech, max_len):
    """ref_speech (B, T_fb, 80), target_speech (B, NS, D) -> logits (B, NS, max_len)."""
    x = speech_encoder_out(sd, ref_speech)
    gap = x.size(-1) - max_len
    assert -1 <= gap <= 2, f"label and ref_speech(mix speech) diff: {gap}"
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
