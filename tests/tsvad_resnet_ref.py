"""TS-VAD with the WeSpeaker ResNet34 speech encoder restated with torch.nn.functional on CPU (fp32).

Written from the architecture (ResNet34 of BasicBlocks [3, 4, 6, 3] at 32/64/128/256 channels over the
(80, T) fbank map, stages 2-4 opening with stride 2 in both axes and a 1x1 stride-2 shortcut; then
ConvTranspose1d(2560 -> D, k5, stride 2, pad 2, output_padding 1) + BatchNorm1D (NaN bypass) + ReLU; then the
CAM++/transformer model's back end).  `sd` is a flat state_dict of torch tensors under the reference key names.
Pinned against tests/golden/tsvad_rn34_*.npz (reference outputs) by tests/test_tsvad_resnet_host.py.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.tsvad_ref import _bn, _bn1d_nan_bypass, positional_encoding, transformer_layer

STAGES = ((32, 3), (64, 4), (128, 6), (256, 3))


def resnet34_time_out(sd, fbank, pre="speech_encoder."):
    """fbank (B, T, 80) -> (B, 2560, T') with channel c * 10 + f (out.reshape(B, C * F, T))."""
    x = fbank.permute(0, 2, 1).unsqueeze(1)
    out = F.relu(_bn(F.conv2d(x, sd[pre + "conv1.weight"], padding=1), sd, pre + "bn1"))
    for layer, (_, n) in enumerate(STAGES, start=1):
        for blk in range(n):
            q = f"{pre}layer{layer}.{blk}."
            stride = 2 if (blk == 0 and layer > 1) else 1
            y = F.relu(_bn(F.conv2d(out, sd[q + "conv1.weight"], stride=stride, padding=1), sd, q + "bn1"))
            y = _bn(F.conv2d(y, sd[q + "conv2.weight"], padding=1), sd, q + "bn2")
            if q + "shortcut.0.weight" in sd:
                sc = _bn(F.conv2d(out, sd[q + "shortcut.0.weight"], stride=stride), sd, q + "shortcut.1")
            else:
                sc = out
            out = F.relu(y + sc)
    b, c, f, t = out.shape
    return out.reshape(b, c * f, t)


def upsample(sd, x):
    """SpeechFeatUpsample2: (B, 2560, T') -> (B, D, 2 T')."""
    x = F.conv_transpose1d(x, sd["speech_down_or_up.up.weight"], sd["speech_down_or_up.up.bias"], stride=2,
                           padding=2, output_padding=1)
    return F.relu(_bn1d_nan_bypass(x, sd, "speech_down_or_up.batchnorm.bn"))


def speech_encoder_out(sd, ref_speech):
    return upsample(sd, resnet34_time_out(sd, ref_speech))


@torch.no_grad()
def tsvad_forward(sd, cfg, ref_speech, target_speech, max_len):
    """ref_speech (B, T_fb, 80), target_speech (B, NS, D) -> logits (B, NS, max_len)."""
    x = speech_encoder_out(sd, ref_speech)
    gap = x.size(-1) - max_len
    assert -1 <= gap <= 2, f"label and ref_speech(mix speech) diff: {gap}"
    assert gap != -1, "the reference raises here (its pad call is misspelt)"
    mix = x[:, :, :max_len].transpose(1, 2)
    B, T, _ = mix.shape
    nh = cfg.num_attention_head
    outs = []
    for i in range(cfg.max_num_speaker):
        cat = torch.cat((target_speech[:, i, None, :].expand(B, T, -1), mix), 2).transpose(0, 1)
        cat = positional_encoding(cat, sd)
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


def phase_convs(w):
    """ConvTranspose1d weight (Cin, Cout, 5) [stride 2, pad 2, output_padding 1] as two ordinary convolutions over
    the same input x (zero padded by one frame at both ends): numpy (Cout, Cin, taps) weights whose tap t reads
    x[j - 1 + t].  even: y[2j] = w4 x[j-1] + w2 x[j] + w0 x[j+1];  odd: y[2j+1] = w3 x[j] + w1 x[j+1] (tap 0 zero)."""
    w = np.asarray(w)
    even = np.stack([w[:, :, 4], w[:, :, 2], w[:, :, 0]], axis=-1).transpose(1, 0, 2)
    odd = np.stack([np.zeros_like(w[:, :, 3]), w[:, :, 3], w[:, :, 1]], axis=-1).transpose(1, 0, 2)
    return even, odd


def phase_upsample(x, w, bias):
    """numpy: x (B, Cin, T') -> (B, Cout, 2 T') through the two phase convolutions."""
    even, odd = phase_convs(w)
    B, _, T = x.shape
    xp = np.pad(np.asarray(x), ((0, 0), (0, 0), (1, 1)))
    y = np.zeros((B, even.shape[0], 2 * T), np.float64)
    for t in range(3):
        seg = xp[:, :, t:t + T]
        y[:, :, 0::2] += np.einsum("oc,bct->bot", even[:, :, t], seg)
        y[:, :, 1::2] += np.einsum("oc,bct->bot", odd[:, :, t], seg)
    return y + np.asarray(bias)[None, :, None]
