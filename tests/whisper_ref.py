"""CPU restatement of the Whisper-PMFA speech encoder (egs/magicdata-ramc/ts_vad2/whisper_encoder.py:150-244) and of its
log-mel front end, for the tests.  Functional: it reads a state_dict under the reference class's key names.

`log_mel` restates the published formula of whisper.log_mel_spectrogram (whisper/audio.py) with torch.stft, per
window and without the 30-s padding; the `whisper` package is not a dependency.  In float32 it is the form the golden
generators hand the reference module; in float64 it is the yardstick of the GPU front end's test.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from speaker_diarization_amd.feature import whisper_mel_filters

N_FFT, HOP = 400, 160


def log_mel(wav: torch.Tensor, n_mels: int = 80, dtype=torch.float32, clamp: bool = True) -> torch.Tensor:
    """One window (n,) -> (n_mels, n // 160).  clamp False: without the `max - 8` dynamic-range clamp."""
    wav = wav.to(dtype)
    window = torch.hann_window(N_FFT, dtype=dtype, device=wav.device)
    stft = torch.stft(wav, N_FFT, HOP, window=window, return_complex=True)
    magnitudes = stft[..., :-1].abs() ** 2
    filters = torch.from_numpy(whisper_mel_filters(n_mels)).to(wav.device, dtype)
    mel_spec = filters @ magnitudes
    log_spec = torch.clamp(mel_spec, min=1e-10).log10()
    if clamp:
        log_spec = torch.maximum(log_spec, log_spec.max() - 8.0)
    return (log_spec + 4.0) / 4.0


def log_mel_batch(wavs: torch.Tensor, n_mels: int = 80, dtype=torch.float32) -> torch.Tensor:
    """(B, n) -> (B, n_mels, F), window by window as WhisperEncoder.forward does (:199-207)."""
    return torch.stack([log_mel(w, n_mels, dtype) for w in wavs])


def stem(sd, x, prefix=""):
    """(B, n_mels, F) -> (B, T', D): conv1 + GELU, conv2 + GELU, + positional_embedding[:T'] (:216-231)."""
    x = F.gelu(F.conv1d(x, sd[prefix + "conv1.weight"], sd[prefix + "conv1.bias"], padding=1))
    x = F.gelu(F.conv1d(x, sd[prefix + "conv2.weight"], sd[prefix + "conv2.bias"], stride=2, padding=1))
    x = x.permute(0, 2, 1)
    pe = sd[prefix + "positional_embedding"]
    assert x.shape[1] <= pe.shape[0], "more frames than n_audio_ctx"
    return x + pe[:x.shape[1]]


def block(sd, p, x, n_head):
    """ResidualAttentionBlock.forward (:135-147) without cross attention."""
    B, T, D = x.shape

    def attn(y):
        q = F.linear(y, sd[p + "attn.query.weight"], sd[p + "attn.query.bias"])
        k = F.linear(y, sd[p + "attn.key.weight"])
        v = F.linear(y, sd[p + "attn.value.weight"], sd[p + "attn.value.bias"])
        scale = (D // n_head) ** -0.25
        q = q.view(B, T, n_head, -1).permute(0, 2, 1, 3) * scale
        k = k.view(B, T, n_head, -1).permute(0, 2, 3, 1) * scale
        v = v.view(B, T, n_head, -1).permute(0, 2, 1, 3)
        w = F.softmax((q @ k).float(), dim=-1).to(q.dtype)
        o = (w @ v).permute(0, 2, 1, 3).flatten(start_dim=2)
        return F.linear(o, sd[p + "attn.out.weight"], sd[p + "attn.out.bias"])

    x = x + attn(F.layer_norm(x, (D,), sd[p + "attn_ln.weight"], sd[p + "attn_ln.bias"]))
    h = F.layer_norm(x, (D,), sd[p + "mlp_ln.weight"], sd[p + "mlp_ln.bias"])
    h = F.linear(F.gelu(F.linear(h, sd[p + "mlp.0.weight"], sd[p + "mlp.0.bias"])), sd[p + "mlp.2.weight"],
                 sd[p + "mlp.2.bias"])
    return x + h


def encoder(sd, cfg, wavs: torch.Tensor, prefix: str = "") -> torch.Tensor:
    """WhisperEncoder.forward: wavs (B, n) -> (B, T', n_audio_state * n_cat)."""
    with torch.no_grad():
        x = stem(sd, log_mel_batch(wavs, cfg.n_mels), prefix)
        out = []
        for i in range(cfg.n_audio_layer):
            x = block(sd, f"{prefix}layers.{i}.", x, cfg.n_audio_head)
            if cfg.layer_st <= i <= cfg.layer_ed:
                out.append(x)
        xs = torch.cat(out, dim=-1)
        return F.layer_norm(xs, (xs.shape[-1],), sd[prefix + "ln_post2.weight"], sd[prefix + "ln_post2.bias"])


PRE = "speech_encoder."


def mix_frames(n_samples: int) -> int:
    return ((n_samples // HOP - 1) // 2 + 1 - 1) // 2 + 1


def tsvad_forward(sd, cfg, ref_speech, target_speech, max_len):
    """TS-VAD with speech_encoder_type "whisper" (egs/magicdata-ramc/ts_vad2/model.py:928-955, 1216-1223, 1296-1309 and
    variant 0's transformer back end): ref_speech (B, n_samples), target_speech (B, NS, D) -> logits (B, NS, max_len)."""
    from oracle.tsvad_ref import _bn1d_nan_bypass, positional_encoding, transformer_layer
    with torch.no_grad():
        x = encoder(sd, cfg.effective_whisper_cfg(), ref_speech, PRE).transpose(1, 2)
        x = F.conv1d(x, sd["speech_down_or_up.0.weight"], sd["speech_down_or_up.0.bias"], stride=2, padding=2)
        x = F.relu(_bn1d_nan_bypass(x, sd, "speech_down_or_up.1.bn"))
        gap = x.size(-1) - max_len
        assert abs(gap) <= 3, \
            f"label and ref_speech(mix speech) diff: {gap}, label len: {max_len}, ref_speech len: {x.size(-1)}"
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


def fp32_bar(g, rtol: float = 1e-3) -> float:
    return rtol * max(1.0, float(np.abs(g).max()))
