"""CPU restatement of TS-VAD with the conformer back ends (plain torch): single_backend_type "conformer" with
multi_backend_type "transformer" or "conformer" behind CAM++ (egs/magicdata-ramc/ts_vad2/model.py:290-313, 451-463,
1330-1400).

Built from oracle.tsvad_ref: the CAM++ speech encoder, the positional encoding, the BatchNorm1D NaN bypass, the
transformer layer and conformer(..., group_norm=False), the BatchNorm form of torchaudio.models.Conformer.  Everything
around the conformer is pinned by reference runs (tests/golden/tsvad_conf_*.npz, written by
tests/golden/make_golden_tsvad_conformer.py with oracle.torchaudio_conformer.Conformer standing in for torchaudio's
class); the conformer arithmetic itself is restated from the published torchaudio 2.5.1 algorithm (parity unpinned:
torchaudio is not installed where this was written), as for ots_vad_style v1.

Unlike the Mamba2 back ends the sequence axis here is time: each (window, speaker) is one batch-first sequence of T
frames, `lengths` are all T (no padding mask), and windows influence each other only through BatchNorm1D's NaN bypass.
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import tsvad_ref as tr  # noqa: E402


def to_double(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def drop_bn_fold(sd):
    """sd with every conformer conv module's BatchNorm1d made the identity (a runtime that forgot to fold it)."""
    out = dict(sd)
    for k, v in sd.items():
        if ".conv_module.sequential.3." not in k:
            continue
        if k.endswith(("running_mean", ".bias")):
            out[k] = torch.zeros_like(v)
        elif k.endswith("running_var"):
            out[k] = torch.ones_like(v) - 1e-5   # (x - 0) / sqrt(var + eps) = x
        elif k.endswith(".weight"):
            out[k] = torch.ones_like(v)
    return out


@torch.no_grad()
def tsvad_forward(sd, cfg, ref_speech, target_speech, max_len, fp64=False, nh=None):
    """TSVADModel.forward in eval with single_backend_type "conformer" (ONE reference forward call over the B windows
    given): ref_speech (B, T_fb, 80), target_speech (B, NS, SE) -> logits (B, NS, max_len) fp32.  fp64: the back end in
    float64 (the speech encoder stays fp32, as in tests/mamba2_ref.py).  nh: the conformers' head count, default
    cfg.num_attention_head (the perturbation check passes another)."""
    assert cfg.single_backend_type == "conformer" and cfg.multi_backend_type in ("transformer", "conformer")
    ns, heads, nl = cfg.max_num_speaker, cfg.num_attention_head, cfg.num_transformer_layer
    cnh = heads if nh is None else nh
    x = tr.speech_encoder_out(sd, ref_speech)
    gap = x.size(-1) - max_len
    assert abs(gap) <= 3, f"label and ref_speech(mix speech) diff: {gap}"      # magicdata model.py:1296-1309
    if gap < 0:
        x = F.pad(x, (0, -gap))
    mix = x[:, :, :max_len].transpose(1, 2)
    ts = target_speech
    if fp64:
        mix, ts, sd = mix.double(), ts.double(), to_double(sd)
    B, T, _ = mix.shape
    lengths = torch.full((B,), T)
    outs = []
    for i in range(ns):
        cat = torch.cat((ts[:, i, None, :].expand(B, T, -1), mix), 2)
        if "proj_layer.weight" in sd:
            cat = F.linear(cat, sd["proj_layer.weight"], sd["proj_layer.bias"])
        cat = tr.positional_encoding(cat.transpose(0, 1), sd).transpose(0, 1)      # (B, T, E), batch first (:1340-1351)
        outs.append(tr.conformer(cat, lengths, sd, "single_backend.", num_layers=nl, nh=cnh, group_norm=False))
    cat = torch.stack(outs).permute(1, 0, 3, 2).reshape(B, -1, T)
    cat = F.relu(tr._bn1d_nan_bypass(F.conv1d(cat, sd["backend_down.0.weight"], sd["backend_down.0.bias"], padding=2),
                                     sd, "backend_down.1.bn"))
    cat = tr.positional_encoding(cat.permute(2, 0, 1), sd)                         # (T, B, E)
    if cfg.multi_backend_type == "conformer":
        cat = tr.conformer(cat.transpose(0, 1), lengths, sd, "multi_backend.", num_layers=nl, nh=cnh, group_norm=False)
    else:
        for l in range(nl):
            cat = tr.transformer_layer(cat, sd, f"multi_backend.layers.{l}.", heads)
        cat = cat.transpose(0, 1)
    return F.linear(cat, sd["fc.weight"], sd["fc.bias"]).transpose(1, 2).float()


def tsvad_forward_grouped(sd, cfg, ref_speech, target_speech, max_len, forward_batch=0, fp64=False):
    """The reference loop over forward calls of `forward_batch` consecutive windows (0: one call): the scope of the
    BatchNorm1D bypass."""
    B = ref_speech.shape[0]
    G = forward_batch if forward_batch > 0 else B
    return torch.cat([tsvad_forward(sd, cfg, ref_speech[g:g + G], target_speech[g:g + G], max_len, fp64=fp64)
                      for g in range(0, B, G)])
