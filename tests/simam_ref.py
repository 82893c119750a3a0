"""The WeSpeaker SimAM-ResNet34 embedding extractor restated with torch.nn.functional on CPU (fp32).

Written from the architecture: a ResNet34 of BasicBlocks [3, 4, 6, 3] at 64/128/256/512 channels over the (80, T)
fbank map, stages 2-4 opening with stride 2 in both axes and a 1x1 stride-2 `downsample` pair; every block gates
bn2(conv2(.)) with SimAM (per channel over the map: d = (Y - mean)^2, v = sum d / (H W - 1), Y * sigmoid(d / (4 (v +
1e-4)) + 0.5)) before the residual sum and the ReLU.  Then attentive statistics pooling over time of the (B, 5120, T')
map (attention = Conv1d(5120, 128, 1), ReLU, BatchNorm1d, Conv1d(128, 5120, 1), softmax over time; [mu | sqrt(clamp(
sum w x^2 - mu^2, 1e-5))]) and bottleneck = Linear(10240, E); and the extractor's chunk loop.  `sd` is a flat
state_dict of torch tensors under the reference key names.  Pinned against tests/golden/simam_emb*.npz (reference
outputs) by tests/test_simam_host.py.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tsvad_ref
from oracle.tsvad_ref import _bn

STAGES = ((64, 3), (128, 4), (256, 6), (512, 3))


def simam(y, lambda_p=1e-4):
    """(B, C, H, W) -> the gated map; gates(y) = the sigmoid factor alone."""
    return y * gates(y, lambda_p)


def gates(y, lambda_p=1e-4):
    n = y.shape[2] * y.shape[3] - 1
    d = (y - y.mean(dim=[2, 3], keepdim=True)).pow(2)
    v = d.sum(dim=[2, 3], keepdim=True) / n
    return torch.sigmoid(d / (4 * (v + lambda_p)) + 0.5)


def front(sd, fbank, pre="front.", last_gates=None):
    """fbank (B, T, 80) -> (B, 5120, T') with channel c * 10 + f (x.reshape(B, -1, T)).  last_gates: a list that
    receives the SimAM gates of the last block."""
    x = fbank.permute(0, 2, 1).unsqueeze(1)
    out = F.relu(_bn(F.conv2d(x, sd[pre + "conv1.weight"], padding=1), sd, pre + "bn1"))
    for layer, (_, n) in enumerate(STAGES, start=1):
        for blk in range(n):
            q = f"{pre}layer{layer}.{blk}."
            stride = 2 if (blk == 0 and layer > 1) else 1
            y = F.relu(_bn(F.conv2d(out, sd[q + "conv1.weight"], stride=stride, padding=1), sd, q + "bn1"))
            y = _bn(F.conv2d(y, sd[q + "conv2.weight"], padding=1), sd, q + "bn2")
            if last_gates is not None and layer == 4 and blk == n - 1:
                last_gates.append(gates(y))
            if q + "downsample.0.weight" in sd:
                sc = _bn(F.conv2d(out, sd[q + "downsample.0.weight"], stride=stride), sd, q + "downsample.1")
            else:
                sc = out
            out = F.relu(simam(y) + sc)
    b, c, f, t = out.shape
    return out.reshape(b, c * f, t)


def attention(sd, x):
    """(B, 5120, T') -> the softmax weights over time."""
    h = F.relu(F.conv1d(x, sd["pooling.attention.0.weight"], sd["pooling.attention.0.bias"]))
    h = _bn(h, sd, "pooling.attention.2")
    return torch.softmax(F.conv1d(h, sd["pooling.attention.3.weight"], sd["pooling.attention.3.bias"]), dim=2)


def asp(sd, x):
    """(B, 5120, T') -> (B, 10240) [mu | sg]."""
    w = attention(sd, x)
    mu = torch.sum(x * w, dim=2)
    sg = torch.sqrt((torch.sum((x ** 2) * w, dim=2) - mu ** 2).clamp(min=1e-5))
    return torch.cat((mu, sg), 1)


@torch.no_grad()
def simam_resnet34_embedding(sd, fbank):
    """fbank (B, T, 80) -> dict(front (B, 5120, T'), stats (B, 10240), emb (B, E))."""
    x = front(sd, fbank)
    stats = asp(sd, x)
    return dict(front=x, stats=stats, emb=F.linear(stats, sd["bottleneck.weight"], sd["bottleneck.bias"]))


def extract_embed(sd, wav, length_embedding=6.0, step_embedding=1.0, batch_size=96):
    """The extractor's chunk loop with FBank(80, mean_nor=True): wav float64 in [-1, 1) -> (n_chunks, E) float32."""
    from oracle.fbank_ref import embed_fbank
    chunks = tsvad_ref.embedding_chunks(len(wav), length_embedding, step_embedding)
    feats = [embed_fbank(wav[a:b]) for a, b in chunks]
    out = []
    for i in range(0, len(feats), batch_size):
        out.append(simam_resnet34_embedding(sd, torch.from_numpy(np.stack(feats[i:i + batch_size])))["emb"])
    return torch.cat(out)
