"""The fused CAM++ FCM residual block (fcm_conv.hip fcm_block_kernel, sd_op_fcm_block fused = 1) against the
trunk's two launches (fused = 0), value for value, and against a torch-CPU restatement of BasicResBlock
(cam_pplus_wespeaker.py:240-268) that rounds the intermediate and the output to bf16 as the kernels do.

"Value-identical" is ((a == b) | (isnan(a) & isnan(b))).all() on the bf16 outputs read as float: -0 equals +0 and
the NaN positions must agree.  The BN shifts are nonzero and mostly positive, so an intermediate pixel outside the
map that was left at relu(shift) instead of conv2's zero padding changes the output.  Shapes sit around the
kernel's band (R output rows x TW frames; the stride-2 form has R = 4): one row, R - 1, R, R + 1 rows, widths
around 16-frame blocks and around one and two tiles, and for each stride one map with more than three bands per CU
(the band count is worked out from the geometry and the device), so every workgroup reuses both ring slots and the
persistent walk wraps."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from speaker_diarization_amd import _lib

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

R1, R2, TW = 8, 4, 62   # fcm_conv.hip FbGeom<1>::R, FbGeom<2>::R, kFbTW


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _params(stride, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    p = dict(w1=r(32, 32, 3, 3) / math.sqrt(288), a1=1 + 0.2 * r(32), b1=0.3 + 0.2 * r(32),
             w2=r(32, 32, 3, 3) / math.sqrt(288), a2=1 + 0.2 * r(32), b2=0.2 + 0.2 * r(32))
    if stride == 2:
        p.update(wsc=r(32, 32, 1, 1) / math.sqrt(32), asc=1 + 0.2 * r(32), bsc=0.1 * r(32))
    return p


def _input(B, H, W, seed):
    return _bf(torch.randn(B, H, W, 32, generator=torch.Generator().manual_seed(seed)))


def _run(gpu, x, stride, p, fused):
    B, H, W, _ = x.shape
    xd = x.to(torch.bfloat16).to(gpu).contiguous()
    dp = {k: v.float().to(gpu).contiguous() for k, v in p.items()}
    out = torch.full((B, (H - 1) // stride + 1, W, 32), 7.0, dtype=torch.bfloat16, device=gpu)
    sc = [_lib.ptr(dp[k]) if stride == 2 else None for k in ("wsc", "asc", "bsc")]
    _lib.call("sd_op_fcm_block", _lib.ptr(xd), B, H, W, stride, *(_lib.ptr(dp[k]) for k in ("w1", "a1", "b1", "w2", "a2", "b2")),
              *sc, _lib.ptr(out), fused, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert _same(xd.cpu().float(), x)   # the input map is left alone
    return out.cpu().float()


def _same(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _reference(x, stride, p):
    """fp32 conv / BN / ReLU on the bf16 input and bf16-rounded weights; intermediate, shortcut and output rounded
    to bf16 where the kernels store (or would store) them."""
    xc = x.permute(0, 3, 1, 2)
    ch = lambda v: v.view(1, 32, 1, 1)
    t = F.conv2d(xc, _bf(p["w1"]), stride=(stride, 1), padding=1)
    t = _bf(F.relu(t * ch(p["a1"]) + ch(p["b1"])))
    y = F.conv2d(t, _bf(p["w2"]), padding=1) * ch(p["a2"]) + ch(p["b2"])
    if stride == 2:
        res = _bf(F.conv2d(xc, _bf(p["wsc"]), stride=(2, 1)) * ch(p["asc"]) + ch(p["bsc"]))
    else:
        res = xc
    return _bf(F.relu(y + res)).permute(0, 2, 3, 1)


WS = [1, 15, 17, TW - 1, TW, TW + 1, 2 * TW + 3]
CASES = [(1, B, H, W) for H in (1, R1 - 1, R1, R1 + 1, 20) for W in WS for B in (1, 3)] + \
        [(2, B, H, W) for H in (2, 7, 8, 40) for W in WS for B in (1, 3)]


@pytest.mark.parametrize("stride,B,H,W", CASES)
def test_fused_equals_two_launches(gpu, stride, B, H, W):
    x = _input(B, H, W, 1000 * H + W + B)
    p = _params(stride, H + W)
    assert _same(_run(gpu, x, stride, p, 1), _run(gpu, x, stride, p, 0))


def _bands(stride, B, H, W):
    """Bands of the fused kernel's launch: images x row bands of R output rows x tiles of TW frames."""
    Ho, R = (H - 1) // stride + 1, (R1 if stride == 1 else R2)
    return B * ((Ho + R - 1) // R) * ((W + TW - 1) // TW)


def test_fused_equals_two_launches_b9(gpu):
    """B 9, H 40, W 598, stride 1 (14 MB): 450 bands, two per workgroup on a 256-CU device."""
    x = _input(9, 40, 598, 3)
    p = _params(1, 4)
    assert _same(_run(gpu, x, 1, p, 1), _run(gpu, x, 1, p, 0))


@pytest.mark.parametrize("stride", [1, 2])
def test_fused_equals_two_launches_wrapping_walk(gpu, stride):
    """The grid is one workgroup per CU at most, and the input ring has two slots: with more than 3 bands per CU
    every workgroup walks at least 4 bands, so both slots and the intermediate image are rewritten right after an
    earlier band's reads of them (what the band-top wait and the two barriers order).  H 40, W 598; B from the
    device's CU count (B 16, 800 bands, 25 MB on 256 CUs)."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    H, W = 40, 598
    B = (3 * cus) // _bands(stride, 1, H, W) + 1
    assert _bands(stride, B, H, W) > 3 * cus
    x = _input(B, H, W, 30 + stride)
    p = _params(stride, 40 + stride)
    assert _same(_run(gpu, x, stride, p, 1), _run(gpu, x, stride, p, 0))


@pytest.mark.parametrize("stride", [1, 2])
def test_fused_equals_two_launches_nan_inf(gpu, stride):
    """A NaN on a band edge (the last output row of the first band, as conv1 input rows go) and a +Inf on a tile
    edge (the last frame of the first tile): both reach neighbouring bands / tiles through the halo.  (The kernels'
    ReLU is fmaxf(v, 0), which turns a NaN into 0, so the outputs need not hold a NaN themselves; where they do,
    the positions must agree.)"""
    H, W = (2 * R1 + 3, 2 * TW + 5) if stride == 1 else (4 * R2 + 5, 2 * TW + 5)
    x = _input(2, H, W, 21)
    rows = R1 if stride == 1 else 2 * R2
    x[0, rows - 1, 20, 3] = float("nan")
    x[1, rows, TW - 1, 9] = float("inf")
    x[1, 2, TW, 30] = float("inf")
    p = _params(stride, 22)
    a, b = _run(gpu, x, stride, p, 1), _run(gpu, x, stride, p, 0)
    assert _same(a, b)


@pytest.mark.parametrize("stride,B,H,W", [(1, 3, R1 + 1, 2 * TW + 3), (1, 1, 20, TW + 1), (2, 3, 7, 2 * TW + 3)])
def test_fused_matches_reference(gpu, stride, B, H, W):
    x = _input(B, H, W, 1000 * H + W + B)
    p = _params(stride, H + W)
    got, ref = _run(gpu, x, stride, p, 1), _reference(x, stride, p)
    rel = float((got - ref).abs().max() / (ref.abs().max() + 1e-12))   # test_gpu_ops._rel_err
    print(f"stride {stride} B {B} H {H} W {W}: relative error {rel:.3e}")
    assert rel < 1e-2   # tests/test_gpu_ops.py::test_conv2d's bf16 bound


def test_fused_rejects_overlap_and_bad_arguments(gpu):
    p = {k: v.float().to(gpu) for k, v in _params(1, 1).items()}
    x = torch.zeros(1, 8, 16, 32, dtype=torch.bfloat16, device=gpu)
    args = [_lib.ptr(p[k]) for k in ("w1", "a1", "b1", "w2", "a2", "b2")]
    with pytest.raises(ValueError):      # out aliases the input
        _lib.call("sd_op_fcm_block", _lib.ptr(x), 1, 8, 16, 1, *args, None, None, None, _lib.ptr(x), 1, _lib.stream_ptr(gpu))
    with pytest.raises(ValueError):      # stride 2 needs its shortcut
        _lib.call("sd_op_fcm_block", _lib.ptr(x), 1, 8, 16, 2, *args, None, None, None, _lib.ptr(x), 1, _lib.stream_ptr(gpu))


MODEL_CHILD = r"""
import hashlib, os, sys
import numpy as np, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, os.path.join({repo!r}, "tests", "golden"))
from make_golden import tsvad_inputs
from speaker_diarization_amd.ts_vad.model import TSVADModel
from speaker_diarization_amd.weights import TSVADConfig, tsvad_state_dict, to_torch
dev = torch.device("cuda", 0)
outs = []
for rs, B, T, nl in ((6, 8, 598, 150), (4, 3, 398, 100)):   # rs_len seconds of 10-ms frames per window
    cfg = TSVADConfig.ots_vad_v1(rs_len=rs)
    sd = to_torch(tsvad_state_dict(cfg, seed=11))
    m = TSVADModel(cfg, device=dev, precision="bf16", max_batch=B)
    m.load_state_dict(sd)
    x, ts = tsvad_inputs(B, T, nl, seed=5)
    outs.append(m.forward(torch.from_numpy(x).to(dev), torch.from_numpy(ts).to(dev), nl).float().cpu())
    del m
torch.save(outs, {path!r})
"""


def test_model_logits_identical_with_and_without_fused_blocks(gpu, tmp_path):
    """TS-VAD ots_vad v1, bf16: SDIAR_NO_FCM_BLOCK=1 (two launches per FCM block) and the default give the same
    logits (child processes: the switch is read once)."""
    outs = []
    for off in (False, True):
        env = dict(os.environ)
        env.pop("SDIAR_NO_FCM_BLOCK", None)
        if off:
            env["SDIAR_NO_FCM_BLOCK"] = "1"
        path = str(tmp_path / f"logits_{int(off)}.pt")
        r = subprocess.run([sys.executable, "-c", MODEL_CHILD.format(repo=REPO, path=path)], env=env,
                           capture_output=True, text=True, timeout=110)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(torch.load(path, weights_only=True))
    for a, b in zip(*outs):
        assert a.shape == b.shape and _same(a, b)
