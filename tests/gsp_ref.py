"""CPU restatement of the TS-VAD speech encoder "CAM++_frame_level_gsp_fc" (egs/magicdata-ramc/ts_vad2/model.py:543-563,
1275-1287), in the reference's UNFOLDED order: CAM++ time output (B, 512, T') -> per-frame mean and unbiased std over
the channels -> gsp_fc = Linear(2, 256) -> Conv1d(256 -> SE, k5, stride 2, pad 2) -> BatchNorm1D (NaN bypass) -> ReLU.

oracle.tsvad_ref.tsvad_forward, tests/mamba2_ref.py and tests/tsvad_conformer_ref.py all reach the speech encoder
through oracle.tsvad_ref.speech_encoder_out, so `swapped()` turns each of them into the whole-model restatement of this
encoder with back ends 0, 1 / 2 and 4 / 5; nothing is copied.

Also the float64 numpy forms the kernel tests compare against: the unfolded stage on a raw trunk map (`stage_f64`), the
host fold (`fold_f64`) and the folded evaluation (`folded_f64`) as the runtime computes it.
"""
from __future__ import annotations

import os
import sys
from unittest import mock

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import tsvad_ref as tr  # noqa: E402


def gsp_fc_conv(sd, x):
    """x (B, 512, T') the CAM++ time output -> speech_down_or_up.0's output (B, SE, T3) (model.py:1279-1287)."""
    mean = x.mean(dim=1, keepdim=True)
    std = x.std(dim=1, keepdim=True)
    stats = torch.cat([mean, std], dim=1).permute(0, 2, 1)
    y = F.linear(stats, sd["gsp_fc.weight"], sd["gsp_fc.bias"]).permute(0, 2, 1)
    return F.conv1d(y, sd["speech_down_or_up.0.weight"], sd["speech_down_or_up.0.bias"], stride=2, padding=2)


def speech_encoder_out(sd, ref_speech):
    """ref_speech (B, T, 80) -> (B, SE, T3): what oracle.tsvad_ref.speech_encoder_out is for "CAM++"."""
    x = gsp_fc_conv(sd, tr.campplus_time_out(sd, ref_speech))
    return F.relu(tr._bn1d_nan_bypass(x, sd, "speech_down_or_up.1.bn"))


def swapped():
    """Context manager: every restatement built on oracle.tsvad_ref.speech_encoder_out runs this encoder."""
    return mock.patch.object(tr, "speech_encoder_out", speech_encoder_out)


# ----------------------------------------------------------------------------- float64 forms for the kernel tests
def frame_stats_f64(x, s, h):
    """x (B, T2, 512) the trunk map before out_nonlinear, s / h (512) its folded BatchNorm -> mean, std (B, T2) of
    relu(s x + h) over the channels (std unbiased), float64."""
    v = np.maximum(np.asarray(x, np.float64) * np.asarray(s, np.float64) + np.asarray(h, np.float64), 0.0)
    return v.mean(-1), v.std(-1, ddof=1)


def unfolded_f64(mean, std, gw, gb, w, cb):
    """gsp_fc then the k5 stride-2 pad-2 conv over its ZERO-PADDED output, float64: (B, T2) x 2 -> (B, T3, SE)."""
    gw, gb, w, cb = (np.asarray(a, np.float64) for a in (gw, gb, w, cb))
    B, T2 = mean.shape
    z = mean[..., None] * gw[:, 0] + std[..., None] * gw[:, 1] + gb          # (B, T2, 256)
    zp = np.zeros((B, T2 + 4, z.shape[-1]))
    zp[:, 2:T2 + 2] = z
    T3 = (T2 - 1) // 2 + 1
    y = np.empty((B, T3, w.shape[0]))
    for j in range(T3):
        y[:, j] = np.einsum("bkc,ock->bo", zp[:, 2 * j:2 * j + 5], w) + cb
    return y


def stage_f64(x, s, h, gw, gb, w, cb):
    mean, std = frame_stats_f64(x, s, h)
    return unfolded_f64(mean, std, gw, gb, w, cb)


def fold_f64(gw, gb, w):
    """A[o,k] = sum_c W[o,c,k] gw[c,0], S[o,k] = sum_c W[o,c,k] gw[c,1], C[o,k] = sum_c W[o,c,k] gb[c]: each (SE, 5)."""
    gw, gb, w = (np.asarray(a, np.float64) for a in (gw, gb, w))
    return np.einsum("ock,c->ok", w, gw[:, 0]), np.einsum("ock,c->ok", w, gw[:, 1]), np.einsum("ock,c->ok", w, gb)


def folded_f64(mean, std, A, S, C, cb):
    """y[j,o] = cb[o] + sum over k with 0 <= 2j+k-2 < T2 of (A[o,k] mean + S[o,k] std + C[o,k]): a padded tap drops
    its C term too."""
    B, T2 = mean.shape
    T3 = (T2 - 1) // 2 + 1
    y = np.tile(np.asarray(cb, np.float64), (B, T3, 1))
    for j in range(T3):
        for k in range(5):
            t = 2 * j + k - 2
            if 0 <= t < T2:
                y[:, j] += mean[:, t, None] * A[:, k] + std[:, t, None] * S[:, k] + C[:, k]
    return y


def stage_f32_torch(x, s, h, gw, gb, w, cb):
    """The unfolded stage as torch computes it on the CPU in float32 (the reference's own arithmetic): the yardstick
    e32 of the kernel test's tolerance.  Same arguments as stage_f64 (numpy float32)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    v = F.relu(t(x) * t(s) + t(h)).permute(0, 2, 1)                               # (B, 512, T2)
    sd = {"gsp_fc.weight": t(gw), "gsp_fc.bias": t(gb), "speech_down_or_up.0.weight": t(w),
          "speech_down_or_up.0.bias": t(cb)}
    return gsp_fc_conv(sd, v).permute(0, 2, 1).numpy()
