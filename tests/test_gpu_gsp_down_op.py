"""sd_op_gsp_down, the "CAM++_frame_level_gsp_fc" stage between the CAM++ trunk and the mix embeddings (out_nonlinear's
BatchNorm + ReLU, per-frame mean / unbiased std over 512 channels, gsp_fc folded into the k5 stride-2 conv), against a
float64 numpy evaluation of the UNFOLDED formula (tests/gsp_ref.py) on the same inputs.

Tolerance: e32 = max|float32 torch-CPU unfolded reference - float64| on the case's own inputs (the reference's own
rounding), and the kernel must be within 4 e32: the fold reassociates the 256-channel sum and the channel reduction runs
as a wave tree, so its rounding differs from torch's by a small factor, not by an order.  Measured on MI355X (printed by
each test), |y| up to about 9:
    case (B x T2 x SE)   fp32 map: e32   kernel error   bf16 map: e32   kernel error
    1x1x192              5.16e-07        2.12e-07       7.98e-07        3.05e-07
    1x2x192              9.40e-07        2.82e-07       8.66e-07        2.58e-07
    2x5x192              2.00e-06        7.23e-07       1.39e-06        7.99e-07
    3x19x192             1.94e-06        1.05e-06       2.29e-06        9.69e-07
    2x20x256             2.24e-06        1.09e-06       2.05e-06        9.71e-07
    1x3x32               4.61e-06        3.18e-07       3.54e-06        4.12e-07
    1x35x192             5.93e-06        1.00e-06       6.96e-06        8.57e-07
    constant channels    9.51e-06        3.52e-06       9.51e-06        3.52e-06
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gsp_ref  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 32   # input frames per workgroup tile (sd_gsp_down_frame_tile; 16 output frames), a 2-frame halo on each side
# (B, T2, SE): one frame (every tap but the centre out of range), two, odd / even lengths, the smallest width, and
# T2 = TILE + 3 so that a halo crosses the tile boundary
SHAPES = [(1, 1, 192), (1, 2, 192), (2, 5, 192), (3, 19, 192), (2, 20, 256), (1, 3, 32), (1, TILE + 3, 192)]
C, F = 512, 256
_cases = {}


def bf16_round(a):
    return torch.from_numpy(a).bfloat16().float().numpy()


def case(shape, bf):
    """Inputs and the float64 / float32 references of one shape, computed once.  bf: the map rounded to bf16 first, so
    only the kernel's fp32 arithmetic is judged."""
    if (shape, bf) not in _cases:
        B, T2, SE = shape
        rng = np.random.default_rng(7000 + 100 * T2 + SE)
        d = dict(x=rng.standard_normal((B, T2, C)).astype(np.float32),
                 s=rng.uniform(0.5, 1.5, C).astype(np.float32), h=(0.3 * rng.standard_normal(C)).astype(np.float32),
                 gw=rng.standard_normal((F, 2)).astype(np.float32), gb=rng.standard_normal(F).astype(np.float32),
                 w=(rng.standard_normal((SE, F, 5)) / np.sqrt(5 * F / 4)).astype(np.float32),
                 cb=rng.standard_normal(SE).astype(np.float32))
        if bf:
            d["x"] = bf16_round(d["x"])
        finish(d)
        _cases[shape, bf] = d
    return _cases[shape, bf]


def finish(d):
    args = [d[k] for k in ("x", "s", "h", "gw", "gb", "w", "cb")]
    d["want"] = gsp_ref.stage_f64(*args)
    d["e32"] = float(np.abs(gsp_ref.stage_f32_torch(*args) - d["want"]).max())
    return d


def run(d, gpu, bf):
    B, T2, _ = d["x"].shape
    SE = d["cb"].shape[0]
    dev = {k: torch.from_numpy(d[k]).to(gpu) for k in ("s", "h", "gw", "gb", "w", "cb")}
    x = torch.from_numpy(d["x"]).to(gpu)
    if bf:
        x = x.bfloat16()
        assert torch.equal(x.float().cpu(), torch.from_numpy(d["x"]))   # the rounding happened on the host already
    y = torch.full((B, (T2 - 1) // 2 + 1, SE), float("nan"), device=gpu)
    _lib.call("sd_op_gsp_down", _lib.ptr(x), int(bf), _lib.ptr(dev["s"]), _lib.ptr(dev["h"]), _lib.ptr(dev["gw"]),
              _lib.ptr(dev["gb"]), _lib.ptr(dev["w"]), _lib.ptr(dev["cb"]), B, T2, SE, _lib.ptr(y),
              _lib.stream_ptr(gpu))
    return y.cpu().numpy()


def test_tile_constant():
    assert _lib.load().sd_gsp_down_frame_tile() == TILE


@pytest.mark.parametrize("bf", [False, True], ids=["f32map", "bf16map"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vs_float64_unfolded(gpu, shape, bf):
    d = case(shape, bf)
    got = run(d, gpu, bf)
    err = float(np.abs(got - d["want"]).max())
    print(f"gsp_down {shape} {'bf16' if bf else 'fp32'} map: e32 = {d['e32']:.3e}, kernel error = {err:.3e}, "
          f"|y| max {float(np.abs(d['want']).max()):.2f}")
    assert np.isfinite(got).all()
    assert err <= 4 * d["e32"]
    assert np.array_equal(got.view(np.uint32), run(d, gpu, bf).view(np.uint32))   # two runs: the same bits


def fold_sequential(gb, w):
    """C[o,k] in the runtime's own order (float64, features ascending), rounded to float32 as it is uploaded."""
    c = np.zeros((w.shape[0], 5))
    for f in range(F):
        c = c + w[:, f, :].astype(np.float64) * np.float64(gb[f])
    return c.astype(np.float32)


@pytest.mark.parametrize("bf", [False, True], ids=["f32map", "bf16map"])
@pytest.mark.parametrize("T2", [1, 6, 7, TILE + 3])
def test_all_zero_activations_leave_bias_and_in_range_c_terms_exactly(gpu, T2, bf):
    """relu(s x + h) = 0 everywhere (s = 0, h < 0): mean = std = 0, so y = cb + the C terms of the taps inside
    [0, T2), in the kernel's tap order, exactly; a kernel that adds all five C terms is wrong at the two ends."""
    d = dict(case((2, 5, 192), bf))   # its weights; the map below is two windows of T2 frames
    rng = np.random.default_rng(7500 + T2)
    d["x"] = bf16_round(rng.standard_normal((2, T2, C)).astype(np.float32))
    d["s"], d["h"] = np.zeros(C, np.float32), np.full(C, -1.0, np.float32)
    got = run(d, gpu, bf)
    c32 = fold_sequential(d["gb"], d["w"])
    T3 = (T2 - 1) // 2 + 1
    want = np.empty((T3, 192), np.float32)
    for j in range(T3):
        acc = d["cb"].copy()
        for k in range(5):
            if 0 <= 2 * j + k - 2 < T2:
                acc = acc + c32[:, k]          # float32, ascending taps
        want[j] = acc
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    # the boundary frames on their own: frame 0 has no taps 0 and 1, the last frame none past T2 - 1
    all_taps = d["cb"] + c32.sum(1)
    assert np.abs(got[0, 0] - all_taps).max() > 1e-3 and np.abs(got[0, -1] - all_taps).max() > 1e-3
    f64 = gsp_ref.stage_f64(*[d[k] for k in ("x", "s", "h", "gw", "gb", "w", "cb")])
    assert np.abs(got - f64).max() < 1e-5


@pytest.mark.parametrize("bf", [False, True], ids=["f32map", "bf16map"])
def test_constant_over_channels_has_zero_std(gpu, bf):
    """Every channel of a frame equal (s = 1, h = 0, a positive value per frame): std = 0 and only the mean term and the
    C terms remain, boundary frames included."""
    base = case((3, 19, 192), bf)
    rng = np.random.default_rng(7600)
    d = dict(base)
    d["x"] = np.repeat((rng.integers(1, 64, (3, 19, 1)) / 8.0).astype(np.float32), C, axis=2)   # exact in bf16 too
    d["s"], d["h"] = np.ones(C, np.float32), np.zeros(C, np.float32)
    finish(d)
    mean, std = gsp_ref.frame_stats_f64(d["x"], d["s"], d["h"])
    assert np.abs(std).max() == 0.0 and mean.min() > 0
    got = run(d, gpu, bf)
    err = np.abs(got - d["want"]).max(axis=(0, 2))
    print(f"constant over channels {'bf16' if bf else 'fp32'} map: e32 = {d['e32']:.3e}, kernel error = {err.max():.3e} "
          f"(first frame {err[0]:.3e}, last {err[-1]:.3e})")
    assert err.max() <= 4 * d["e32"] and err[0] <= 4 * d["e32"] and err[-1] <= 4 * d["e32"]
    # the S coefficients took no part: the same outputs with gsp_fc's std column zeroed
    d2 = dict(d)
    d2["gw"] = d["gw"].copy()
    d2["gw"][:, 1] = 0
    assert np.array_equal(run(d2, gpu, bf), got)


def test_refuses_bad_shapes(gpu):
    d = case((1, 3, 32), False)
    z = torch.zeros(4096, device=gpu)
    for B, T2, SE, msg in ((1, 3, 48, "multiple of 32"), (1, 3, 0, "multiple of 32"), (1, 0, 32, "at least 1"),
                           (0, 3, 32, "at least 1")):
        with pytest.raises(ValueError, match=msg):
            _lib.call("sd_op_gsp_down", _lib.ptr(z), 0, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z),
                      _lib.ptr(z), B, T2, SE, _lib.ptr(z), _lib.stream_ptr(gpu))
    assert d["e32"] > 0
