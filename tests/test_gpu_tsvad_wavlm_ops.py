"""The kernels TS-VAD's WavLM speech encoders add (csrc/wavlm.hip), through their test ops, against the torch formula.

Tolerances, as in tests/test_gpu_wavlm_ops.py.  fp32 arms: the project's fp32 bar, max |got - ref| <= 1e-3 max(1, max |ref|).
wavlm_mix_proj_ln's bf16 arm: the reference is computed in fp32 on acc and W rounded to bf16 as the kernel rounds them
(fp32 accumulation and LayerNorm in both), and the kernel stores a bf16 map, one more rounding of at most 2^-8 of the
value: fp32 bar + 2^-8 max |ref|.  The rows have a standard deviation of at least 0.5 before the LayerNorm (asserted), so
its division amplifies an error by at most 2.  window_wave only moves values: compared exactly.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.frontend import window_wave  # noqa: E402

pytestmark = pytest.mark.gpu


def fp32_bar(ref):
    return 1e-3 * max(1.0, float(ref.abs().max()))


def rb(x):
    return x.to(torch.bfloat16).float()


def check(got, ref, bound, what):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    e = float((got - ref).abs().max())
    print(f"{what}: max|got - ref| {e:.3e}  bound {bound:.3e}  max|ref| {float(ref.abs().max()):.3f}")
    assert e <= bound, (what, e, bound)


@pytest.mark.parametrize("D", [768, 1024])
@pytest.mark.parametrize("rows", [1, 98])
@pytest.mark.parametrize("L", [1, 3])
def test_layer_mix(gpu, L, rows, D):
    rng = np.random.default_rng(31 + L + rows + D)
    x = torch.from_numpy(rng.standard_normal((L, rows, D)).astype(np.float32) * 2)
    w = (rng.permutation(np.linspace(-0.9, 1.3, L)) + 0.01).astype(np.float32)
    ref = (x.double() * torch.from_numpy(w).double()[:, None, None]).sum(0).float()
    xd = x.to(gpu).contiguous()
    acc = torch.full((rows, D), float("nan"), device=gpu)     # the first layer writes, it does not accumulate
    _lib.call("sd_op_wavlm_layer_mix", _lib.ptr(xd), L, rows * D, w.ctypes.data_as(ctypes.c_void_p), _lib.ptr(acc),
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    check(acc.cpu(), ref, fp32_bar(ref), f"layer_mix L={L} rows={rows} D={D}")


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("D", [768, 1024])
@pytest.mark.parametrize("SE", [192, 256])
@pytest.mark.parametrize("rows", [1, 98, 37])     # 98 = 6 row tiles + 2; 37: another remainder of the 16-row tile
def test_mix_proj_ln(gpu, rows, SE, D, precision):
    rng = np.random.default_rng(47 + rows + SE + D)
    acc = torch.from_numpy(rng.standard_normal((rows, D)).astype(np.float32) * 2)
    w = torch.from_numpy((rng.standard_normal((SE, D)) / np.sqrt(D)).astype(np.float32))
    bias = torch.from_numpy((0.2 * rng.standard_normal(SE)).astype(np.float32))
    g = torch.from_numpy(rng.uniform(0.7, 1.3, SE).astype(np.float32))
    beta = torch.from_numpy((0.1 * rng.standard_normal(SE)).astype(np.float32))
    a, wq = (rb(acc), rb(w)) if precision else (acc, w)
    pre = F.linear(a.double(), wq.double(), bias.double())
    assert float(pre.std(1).min()) >= 0.5
    ref = F.layer_norm(pre, (SE,), g.double(), beta.double(), 1e-5).float()
    d = [t.to(gpu).contiguous() for t in (acc, w, bias, g, beta)]
    out = torch.full((rows, SE), float("nan"), device=gpu)
    _lib.call("sd_op_wavlm_mix_proj_ln", _lib.ptr(d[0]), rows, D, _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]),
              _lib.ptr(d[4]), SE, _lib.ptr(out), precision, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    bound = fp32_bar(ref) + (2.0 ** -8 * float(ref.abs().max()) if precision else 0.0)
    check(out.cpu(), ref, bound, f"mix_proj_ln rows={rows} SE={SE} D={D} precision={precision}")


def test_window_wave(gpu):
    """A full window, a short one (zero tail), an empty one, and one that runs past the end of the waveform."""
    n, n_out = 5000, 1280
    wav = torch.from_numpy(np.random.default_rng(5).standard_normal(n).astype(np.float32))
    start = np.array([0, 640, 1920, 4360], np.int32)
    cnt = np.array([1280, 640, 0, 1280], np.int32)
    ref = torch.zeros(4, n_out)
    for i, (s, c) in enumerate(zip(start, cnt)):
        m = min(int(c), n - int(s))
        ref[i, :m] = wav[s:s + m]
    out = window_wave(wav.to(gpu), torch.from_numpy(start).to(gpu), torch.from_numpy(cnt).to(gpu), n_out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)
