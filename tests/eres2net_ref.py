"""The 3D-Speaker ERes2NetV2 embedding extractor restated with torch.nn.functional on CPU (fp32).

Written from the architecture: stem conv 1 -> 64 (3x3) + BN + ReLU on the (80, T) fbank map, then Res2Net blocks [3, 4,
6, 3] at planes 64 / 128 / 256 / 512, stages 2-4 opening with stride 2 carried by the block's 1x1 conv1 and 1x1 shortcut.
A block: conv1 1x1 to width * scale channels (width = floor(planes * baseWidth / 64)), BN, clamp to [0, 20]; the result
split into `scale` slices; slice i enters a 3x3 conv (+ BN + clamp) as itself (i = 0), as previous output + slice
(stages 1-2) or as AFF(previous output, slice) (stages 3-4); the outputs are concatenated; conv3 1x1 to planes *
expansion, BN, + shortcut, clamp.  AFF(x, y): att = BN(W2 SiLU(BN(W1 cat(x, y) + b1)) + b2), x_att = 1 + tanh(att), out
= x x_att + y (2 - x_att).  Head: layer3_ds (3x3 stride 2, no BN) of out3, fuse34 = AFF(out4, layer3_ds(out3)), TSTP
over time ([mean | sqrt(unbiased var + 1e-8)], flattened c * 10 + f), seg_1.  The two frame-level outputs order the
channels f * C + c (the map transposed to (B, T, F, C), then flattened).  `sd` is a flat state_dict of torch tensors
under the reference key names.  Pinned against tests/golden/eres2net_*.npz (reference outputs) by
tests/test_eres2net_host.py.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import tsvad_ref
from oracle.tsvad_ref import _bn

STAGES = ((64, 3), (128, 4), (256, 6), (512, 3))


def clamp20(x):
    """nn.Hardtanh(0, 20): NaN stays, +inf -> 20."""
    return torch.clamp(x, 0.0, 20.0)


def aff_att(sd, p, x, y):
    """tanh(local_att(cat(x, y))) of the AFF at `p` (keys p + local_att.{0,1,3,4})."""
    a = p + "local_att."
    h = F.silu(_bn(F.conv2d(torch.cat((x, y), 1), sd[a + "0.weight"], sd[a + "0.bias"]), sd, a + "1"))
    return torch.tanh(_bn(F.conv2d(h, sd[a + "3.weight"], sd[a + "3.bias"]), sd, a + "4"))


def aff(sd, p, x, y, taps=None):
    t = aff_att(sd, p, x, y)
    if taps is not None:
        taps.append(t)
    return x * (1.0 + t) + y * (1.0 - t)


def block(sd, q, x, stride, width, scale, fuse, taps=None):
    out = clamp20(_bn(F.conv2d(x, sd[q + "conv1.weight"], stride=stride), sd, q + "bn1"))
    spx = torch.split(out, width, 1)
    outs = []
    sp = None
    for i in range(scale):
        if i == 0:
            sp = spx[0]
        elif fuse:
            sp = aff(sd, f"{q}fuse_models.{i - 1}.", sp, spx[i], taps)
        else:
            sp = sp + spx[i]
        sp = clamp20(_bn(F.conv2d(sp, sd[f"{q}convs.{i}.weight"], padding=1), sd, f"{q}bns.{i}"))
        outs.append(sp)
    out = _bn(F.conv2d(torch.cat(outs, 1), sd[q + "conv3.weight"]), sd, q + "bn3")
    if q + "shortcut.0.weight" in sd:
        res = _bn(F.conv2d(x, sd[q + "shortcut.0.weight"], stride=stride), sd, q + "shortcut.1")
    else:
        res = x
    return clamp20(out + res)


def trunk(sd, fbank, base_width, scale, taps=None):
    """fbank (B, T, 80) -> (out3 (B, 256 e, 20, T3), out4 (B, 512 e, 10, T'))."""
    x = fbank.permute(0, 2, 1).unsqueeze(1)
    out = F.relu(_bn(F.conv2d(x, sd["conv1.weight"], padding=1), sd, "bn1"))
    out3 = None
    for layer, (planes, n) in enumerate(STAGES, start=1):
        width = planes * base_width // 64
        for blk in range(n):
            stride = 2 if (blk == 0 and layer > 1) else 1
            out = block(sd, f"layer{layer}.{blk}.", out, stride, width, scale, layer >= 3, taps)
        if layer == 3:
            out3 = out
    return out3, out


def fuse34(sd, fbank, base_width, scale, taps=None):
    """fbank -> (out3, the fuse34 map (B, 512 e, 10, T'))."""
    out3, out4 = trunk(sd, fbank, base_width, scale, taps)
    ds = F.conv2d(out3, sd["layer3_ds.weight"], stride=2, padding=1)
    return out3, aff(sd, "fuse34.", out4, ds, taps)


def tstp(x):
    """(B, C, F, T) -> (B, 2 C F): [mean | sqrt(unbiased var + 1e-8)] over time, flattened c * F + f."""
    return torch.cat((x.mean(-1).flatten(1), torch.sqrt(x.var(-1) + 1e-8).flatten(1)), 1)


def frames(x):
    """(B, C, F, T) -> (B, F C, T), channel f * C + c."""
    return x.transpose(1, 3).flatten(2).permute(0, 2, 1)


@torch.no_grad()
def forward(sd, fbank, base_width=26, scale=2):
    """fbank (B, T, 80) -> dict(emb (B, E), stats, frame (B, 5120 e, T'), frame25 (B, 5120 e, T3))."""
    out3, fu = fuse34(sd, fbank, base_width, scale)
    stats = tstp(fu)
    return {"emb": F.linear(stats, sd["seg_1.weight"], sd["seg_1.bias"]), "stats": stats, "frame": frames(fu),
            "frame25": frames(out3)}


def extract_embed(sd, wav, base_width=26, scale=2, length_embedding=6.0, step_embedding=1.0, batch_size=96):
    """The extractor's chunk loop with FBank(80, mean_nor=True): wav float64 in [-1, 1) -> (n_chunks, E) float32."""
    from oracle.fbank_ref import embed_fbank
    chunks = tsvad_ref.embedding_chunks(len(wav), length_embedding, step_embedding)
    feats = [embed_fbank(wav[a:b]) for a, b in chunks]
    out = []
    for i in range(0, len(feats), batch_size):
        out.append(forward(sd, torch.from_numpy(np.stack(feats[i:i + batch_size])), base_width, scale)["emb"])
    return torch.cat(out)
