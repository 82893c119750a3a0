"""The fused CAM++ FCM stem + layer1.0 kernel (fcm_conv.hip fcm_stem_block_kernel, sd_op_fcm_stem_block fused = 1)
against the trunk's two launches (fused = 0: conv1 with the stem computed in LDS and the shortcut as a second output,
then conv2 + residual), value for value, and against a torch-CPU restatement of the stem + BasicResBlock
(cam_pplus_wespeaker.py:240-308) that rounds where the kernels round.

"Value-identical" is tests/test_gpu_fcm_block.py's `_same`: equal, or NaN in the same places.  The BN shifts are nonzero
and mostly positive, so a stem or intermediate pixel outside the map that was left at relu(shift) instead of the next
conv's zero padding changes the output.  Shapes: a band is R = 8 output rows (16 fbank bins) x 62 frames; F covers one
row, the stride-2 parity and the rows around one band, W the narrowest supported width (113), two 62-frame tiles
(123 - 125), the pair kernel's own tile boundary (304 / 305) and the production widths."""
import math

import pytest
import torch
import torch.nn.functional as F

from speaker_diarization_amd import _lib

pytestmark = pytest.mark.gpu

R, TW = 8, 62   # fcm_conv.hip SbGeom::R, kFbTW
KEYS = ("stem_w", "stem_a", "stem_b", "w1", "a1", "b1", "w2", "a2", "b2", "wsc", "asc", "bsc")


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _same(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(stem_w=r(32, 1, 3, 3) / 3, stem_a=1 + 0.2 * r(32), stem_b=0.3 + 0.2 * r(32),
                w1=r(32, 32, 3, 3) / math.sqrt(288), a1=1 + 0.2 * r(32), b1=0.3 + 0.2 * r(32),
                w2=r(32, 32, 3, 3) / math.sqrt(288), a2=1 + 0.2 * r(32), b2=0.2 + 0.2 * r(32),
                wsc=r(32, 32, 1, 1) / math.sqrt(32), asc=1 + 0.2 * r(32), bsc=0.1 * r(32))


def _fbank(B, W, nF, seed):
    return 2.0 * torch.randn(B, W, nF, generator=torch.Generator().manual_seed(seed))


def _run(gpu, fb, p, fused):
    B, W, nF = fb.shape
    fd = fb.to(gpu).contiguous()
    dp = {k: v.float().to(gpu).contiguous() for k, v in p.items()}
    out = torch.full((B, (nF - 1) // 2 + 1, W, 32), 7.0, dtype=torch.bfloat16, device=gpu)   # sentinel
    _lib.call("sd_op_fcm_stem_block", _lib.ptr(fd), B, W, nF, *(_lib.ptr(dp[k]) for k in KEYS), _lib.ptr(out), fused,
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert _same(fd.cpu(), fb)   # the fbank is left alone
    return out.cpu().float()


def _reference(fb, p):
    """fp32 convs on operands rounded as the kernels round them: fbank taps and alpha * w of the stem to bf16 (its shift
    as a bf16 hi + lo pair), the block's weights to bf16, and the stem, intermediate, shortcut and output maps to bf16."""
    ch = lambda v: v.view(1, 32, 1, 1)
    x = _bf(fb).permute(0, 2, 1).unsqueeze(1)   # (B, 1, F, W)
    b_hi = _bf(p["stem_b"])
    shift = b_hi + _bf(p["stem_b"] - b_hi)
    s = _bf(F.relu(F.conv2d(x, _bf(p["stem_w"] * ch(p["stem_a"]).view(32, 1, 1, 1)), padding=1) + ch(shift)))
    t = F.conv2d(s, _bf(p["w1"]), stride=(2, 1), padding=1)
    t = _bf(F.relu(t * ch(p["a1"]) + ch(p["b1"])))
    y = F.conv2d(t, _bf(p["w2"]), padding=1) * ch(p["a2"]) + ch(p["b2"])
    res = _bf(F.conv2d(s, _bf(p["wsc"]), stride=(2, 1)) * ch(p["asc"]) + ch(p["bsc"]))
    return _bf(F.relu(y + res)).permute(0, 2, 3, 1)


FS = [1, 2, 7, 8, 2 * R - 1, 2 * R, 2 * R + 1, 80]
WS = [113, 123, 124, 125, 187, 304, 305, 398, 598]


@pytest.mark.parametrize("nF", FS)
@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("B", [1, 3])
def test_fused_equals_two_launches(gpu, B, W, nF):
    fb = _fbank(B, W, nF, 1000 * nF + W + B)
    p = _params(nF + W)
    assert _same(_run(gpu, fb, p, 1), _run(gpu, fb, p, 0))


def _bands(B, nF, W):
    """Bands of the fused kernel's launch: images x row bands of R output rows x tiles of TW frames."""
    Ho = (nF - 1) // 2 + 1
    return B * ((Ho + R - 1) // R) * ((W + TW - 1) // TW)


def test_fused_equals_two_launches_wrapping_walk(gpu):
    """The grid is one workgroup per CU at most; with more than 3 bands per CU every workgroup walks at least 4
    bands, so both fbank tiles, the stem image and the intermediate image are rewritten right after an earlier band's
    reads of them (what the three barriers and the tile wait order).  F 80, W 598; B from the device's CU count (B 16,
    800 bands, 3 MB in, 25 MB out on 256 CUs)."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    nF, W = 80, 598
    B = (3 * cus) // _bands(1, nF, W) + 1
    assert _bands(B, nF, W) > 3 * cus
    fb = _fbank(B, W, nF, 31)
    p = _params(41)
    assert _same(_run(gpu, fb, p, 1), _run(gpu, fb, p, 0))


def test_fused_equals_two_launches_nan_inf(gpu):
    """A NaN on a band-edge bin (the last fbank bin of the first band's output rows) and +Inf on tile-edge frames:
    both reach the neighbouring bands / tiles through the stem and conv halos.  (The kernels' ReLU is fmaxf(v, 0),
    which turns a NaN into 0, so the outputs need not hold a NaN themselves; where they do, the positions must
    agree.)"""
    nF, W = 4 * R + 5, 2 * TW + 5
    fb = _fbank(2, W, nF, 21)
    fb[0, 20, 2 * R - 1] = float("nan")
    fb[1, TW - 1, 2 * R] = float("inf")
    fb[1, TW, 2] = float("inf")
    p = _params(22)
    assert _same(_run(gpu, fb, p, 1), _run(gpu, fb, p, 0))


@pytest.mark.parametrize("B,W,nF", [(3, 2 * TW + 3, 2 * R + 1), (1, 187, 80), (2, 305, 7)])
def test_fused_matches_reference(gpu, B, W, nF):
    fb = _fbank(B, W, nF, 1000 * nF + W + B)
    p = _params(nF + W)
    got, ref = _run(gpu, fb, p, 1), _reference(fb, p)
    rel = float((got - ref).abs().max() / (ref.abs().max() + 1e-12))   # test_gpu_ops._rel_err
    print(f"B {B} W {W} F {nF}: relative error {rel:.3e}")
    assert rel < 1e-2   # tests/test_gpu_ops.py::test_conv2d's bf16 bound


def test_fused_rejects_narrow_maps_and_a_missing_shortcut(gpu):
    p = {k: v.float().to(gpu) for k, v in _params(1).items()}
    st = _lib.stream_ptr(gpu)
    out = torch.zeros(1, 4, 113, 32, dtype=torch.bfloat16, device=gpu)
    fb = torch.zeros(1, 113, 8, device=gpu)
    args = [_lib.ptr(p[k]) for k in KEYS]
    with pytest.raises(ValueError):      # W 112: the pair runs its fp32 stem there, whose values differ
        _lib.call("sd_op_fcm_stem_block", _lib.ptr(fb), 1, 112, 8, *args, _lib.ptr(out), 1, st)
    with pytest.raises(ValueError):      # layer1.0 has a shortcut
        _lib.call("sd_op_fcm_stem_block", _lib.ptr(fb), 1, 113, 8, *args[:9], None, None, None, _lib.ptr(out), 1, st)
    _lib.call("sd_op_fcm_stem_block", _lib.ptr(fb), 1, 113, 8, *args, _lib.ptr(out), 1, st)   # the same call, complete
    torch.cuda.synchronize()
