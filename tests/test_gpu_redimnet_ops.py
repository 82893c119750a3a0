"""The ReDimNetB2 test ops on the MI355X path (csrc/redimnet.hip through sd_op_redim_*), each against the CPU
restatement (tests/redimnet_ref.py) on the same inputs.

Tolerances.  fp32 and bf16x3: the project's fp32 bar, max|got - want| <= 1e-3 * max(1, max|want|).  bf16 ops are
compared with the fp32 restatement on the bf16-rounded inputs and weights, so only the kernel's own rounding points
count; a bf16 rounding is at most 2^-9 relative:
  block2d    h is rounded once and passes the He-scaled pointwise conv at a gain of about sqrt(2), the sum is rounded
             once: (1.5 + 1) * 2^-9 of the largest value, taken as 4 * 2^-9 to leave room for an unlucky alignment; both
             arms are held to it
  the others one rounding of the output: 2^-9 of the largest value, plus the fp32 bar
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import redimnet_ref as rr  # noqa: E402
from ecapa_ref import astp  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

CF = 1152
FP32_RTOL = 1e-3
BF = 2.0 ** -9


def bar(want, extra=0.0):
    return (FP32_RTOL + extra) * max(1.0, float(want.abs().max()))


def dev(gpu, *arrays):
    return [torch.as_tensor(a).to(gpu).contiguous() for a in arrays]


def bn_params(rng, c):
    w, b = rng.uniform(0.7, 1.3, c), rng.standard_normal(c) * 0.1
    m, v = rng.standard_normal(c) * 0.3, rng.uniform(0.5, 1.5, c)
    return [torch.from_numpy(a.astype(np.float32)) for a in (w, b, m, v)]


def fold(w, b, m, v, eps=1e-5):
    s = w / torch.sqrt(v + eps)
    return s, b - m * s


# ---------------------------------------------------------------- the 2-D block
def block_case(c, T, seed):
    rng = np.random.default_rng(seed)
    p = "blk."
    sd = {p + "dwconvs.0.weight": torch.from_numpy((rng.standard_normal((c, 4, 3, 3)) * np.sqrt(2 / 36)).astype(np.float32)),
          p + "dwconvs.0.bias": torch.from_numpy((rng.standard_normal(c) * 0.05).astype(np.float32)),
          p + "pwconv1.weight": torch.from_numpy((rng.standard_normal((c, c, 1, 1)) * np.sqrt(2 / c)).astype(np.float32)),
          p + "pwconv1.bias": torch.from_numpy((rng.standard_normal(c) * 0.05).astype(np.float32))}
    for k, a in zip(("weight", "bias", "running_mean", "running_var"), bn_params(rng, c)):
        sd[p + "norm." + k] = a
    x = torch.from_numpy(rng.standard_normal((2, T, CF)).astype(np.float32))     # two distinct windows
    return sd, x


def block_ref(sd, x, c):
    B, T, _ = x.shape
    y = rr.block2d(sd, "blk.", x.view(B, T, CF // c, c).permute(0, 3, 2, 1))
    return y.permute(0, 3, 2, 1).reshape(B, T, CF)


def run_block(gpu, sd, x, c, precision, use_generic):
    B, T, _ = x.shape
    dt = torch.bfloat16 if precision == 1 else torch.float32
    xd = x.to(gpu, dt).contiguous()
    out = torch.full((B, T, CF), float("nan"), device=gpu, dtype=dt)
    s, h = fold(*(sd["blk.norm." + k] for k in ("weight", "bias", "running_mean", "running_var")))
    a = dev(gpu, sd["blk.dwconvs.0.weight"], sd["blk.dwconvs.0.bias"], s, h, sd["blk.pwconv1.weight"].reshape(c, c),
            sd["blk.pwconv1.bias"])
    _lib.call("sd_op_redim_block2d", _lib.ptr(xd), B, T, c, *[_lib.ptr(t) for t in a], _lib.ptr(out), use_generic,
              precision, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return out


# T: one frame (every time tap but the centre is padding), shorter than the fused kernel's 8-row tile, and nine tiles
# plus a 5-row remainder
@pytest.mark.parametrize("T", [1, 5, 77])
@pytest.mark.parametrize("c", [16, 32, 64, 128])
def test_block2d_fp32(gpu, c, T):
    sd, x = block_case(c, T, 10 * c + T)
    want = block_ref(sd, x, c)
    for precision in (0, 2):
        got = run_block(gpu, sd, x, c, precision, 1).cpu()
        err = float((got - want).abs().max())
        print(f"block2d c={c} T={T} precision {precision}: max err {err:.3e} (bar {bar(want):.3e})")
        assert err <= bar(want)


@pytest.mark.parametrize("T", [1, 5, 77])
@pytest.mark.parametrize("c", [16, 32, 64, 128])
def test_block2d_bf16_both_arms(gpu, c, T):
    sd, x = block_case(c, T, 20 * c + T)
    x = x.bfloat16().float()
    sdr = dict(sd)
    sdr["blk.pwconv1.weight"] = sd["blk.pwconv1.weight"].bfloat16().float()    # the grouped conv's weights stay fp32
    want = block_ref(sdr, x, c)
    bound = bar(want, 4 * BF)
    for arm, use_generic in (("generic", 1), ("fused", 0)):
        got = run_block(gpu, sd, x, c, 1, use_generic)
        err = float((got.float().cpu() - want).abs().max())
        print(f"block2d bf16 c={c} T={T} {arm}: max err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, arm
        alone = run_block(gpu, sd, x[1:], c, 1, use_generic)                    # no neighbour's frames
        assert torch.equal(alone[0].view(torch.int16), got[1].view(torch.int16)), arm


def test_block2d_refuses_fused_fp32(gpu):
    sd, x = block_case(16, 1, 1)
    with pytest.raises(ValueError, match="the fused kernel is bf16"):
        run_block(gpu, sd, x, 16, 0, 0)


# ---------------------------------------------------------------- depthwise conv over time
# T: shorter than the half kernel of k = 59, just over the kernel, and one 64-frame tile plus a remainder
@pytest.mark.parametrize("T", [8, 61, 77])
@pytest.mark.parametrize("hC", [96, 288])
@pytest.mark.parametrize("k", [7, 59])
def test_dwconv1d(gpu, k, hC, T):
    rng = np.random.default_rng(k * 1000 + hC + T)
    w = torch.from_numpy((rng.standard_normal((hC, 1, k)) * np.sqrt(2 / k)).astype(np.float32))
    b = torch.from_numpy((rng.standard_normal(hC) * 0.05).astype(np.float32))
    bn = bn_params(rng, hC)
    x = torch.from_numpy(rng.standard_normal((2, T, hC)).astype(np.float32))
    y = F.conv1d(x.permute(0, 2, 1), w, b, padding=k // 2, groups=hC)
    want = F.gelu(F.batch_norm(y, bn[2], bn[3], bn[0], bn[1], False, 0.0, 1e-5)).permute(0, 2, 1).contiguous()
    s, h = fold(*bn)
    xd, wd, bd, sdv, hd = dev(gpu, x, w.reshape(hC, k), b, s, h)
    for out_bf16 in (0, 1):
        out = torch.full((2, T, hC), float("nan"), device=gpu, dtype=torch.bfloat16 if out_bf16 else torch.float32)
        _lib.call("sd_op_redim_dwconv1d", _lib.ptr(xd), 2, T, hC, k, _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(sdv),
                  _lib.ptr(hd), _lib.ptr(out), out_bf16, _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
        err = float((out.float().cpu() - want).abs().max())
        bound = bar(want, BF if out_bf16 else 0.0)
        print(f"dwconv1d k={k} hC={hC} T={T} bf16 out {out_bf16}: max err {err:.3e} (bound {bound:.3e})")
        assert err <= bound


# ---------------------------------------------------------------- stage mix
@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("n", [2, 7])
def test_stage_mix(gpu, n, bf16):
    rng = np.random.default_rng(n)
    rows = 2 * 13
    x = torch.from_numpy(rng.standard_normal((n, rows, CF)).astype(np.float32))
    if bf16:
        x = x.bfloat16().float()
    w = torch.softmax(torch.from_numpy((rng.standard_normal((n, CF)) * 0.5).astype(np.float32)), 0)
    want = (w[:, None, :] * x).sum(0)
    dt = torch.bfloat16 if bf16 else torch.float32
    xd = x.to(gpu, dt).contiguous()
    out = torch.full((rows, CF), float("nan"), device=gpu, dtype=dt)
    _lib.call("sd_op_redim_stage_mix", _lib.ptr(xd), n, rows, _lib.ptr(w.to(gpu).contiguous()), _lib.ptr(out), bf16,
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    err = float((out.float().cpu() - want).abs().max())
    bound = bar(want, BF if bf16 else 0.0)
    print(f"stage_mix n={n} bf16 {bf16}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ---------------------------------------------------------------- stem
@pytest.mark.parametrize("T", [1, 77])
def test_stem(gpu, T):
    rng = np.random.default_rng(T)
    w = torch.from_numpy((rng.standard_normal((16, 1, 3, 3)) * np.sqrt(2 / 9)).astype(np.float32))
    b = torch.from_numpy((rng.standard_normal(16) * 0.05).astype(np.float32))
    g = torch.from_numpy(rng.uniform(0.7, 1.3, 16).astype(np.float32))
    beta = torch.from_numpy((rng.standard_normal(16) * 0.05).astype(np.float32))
    fb = torch.from_numpy((rng.standard_normal((2, T, 72)) * 3.0).astype(np.float32))
    y = rr.ln_channels(F.conv2d(fb.permute(0, 2, 1).unsqueeze(1), w, b, padding=1), g, beta)
    want = rr.to1d(y).permute(0, 2, 1).contiguous()                         # (B, T, 1152), channel f * 16 + ch
    a = dev(gpu, fb, w.reshape(16, 9), b, g, beta)
    for out_bf16 in (0, 1):
        out = torch.full((2, T, CF), float("nan"), device=gpu, dtype=torch.bfloat16 if out_bf16 else torch.float32)
        _lib.call("sd_op_redim_stem", _lib.ptr(a[0]), 2, T, *[_lib.ptr(t) for t in a[1:]], _lib.ptr(out), out_bf16,
                  _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
        err = float((out.float().cpu() - want).abs().max())
        bound = bar(want, BF if out_bf16 else 0.0)
        print(f"stem T={T} bf16 out {out_bf16}: max err {err:.3e} (bound {bound:.3e})")
        assert err <= bound


# ---------------------------------------------------------------- attention with zero-padded heads
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("hC", [96, 144, 288])
def test_padded_head_attention(gpu, hC, precision):
    """q | k | v of 4 heads of hC / 4 values, zero-padded to 32 / 48 / 96 per head, with the scale of the TRUE width:
    the outputs' first hC / 4 values per head equal plain attention, the padding stays zero.  precision 2: q | k | v and
    the output stored in bf16 and the products on bf16 MFMA, as the bf16 trunk runs it; against fp32 attention on the
    bf16-rounded q | k | v, the output (a convex combination of v rows) is rounded once, 2^-9, and the probabilities'
    bf16 rounding adds at most another 2^-9 of the largest |v|: bound 3 * 2^-9 * max|v| with the fp32 bar on top."""
    T, S, nh = 77, 2, 4
    hd, hdp = hC // nh, rr.padded_width(hC // nh)
    rng = np.random.default_rng(hC)
    qkv = torch.from_numpy(rng.standard_normal((S, T, 3, nh, hd)).astype(np.float32))
    if precision == 2:
        qkv = qkv.bfloat16().float()
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))              # (S, nh, T, hd)
    want = (torch.softmax((q * hd ** -0.5) @ k.transpose(2, 3), -1) @ v).transpose(1, 2)   # (S, T, nh, hd)
    pad = torch.zeros(S, T, 3, nh, hdp)
    pad[..., :hd] = qkv
    out = torch.full((S, T, nh, hdp), float("nan"), device=gpu)
    _lib.call("sd_op_attention_scaled", _lib.ptr(pad.to(gpu).contiguous()), S, T, nh * hdp, nh, float(hd ** -0.5),
              _lib.ptr(out), precision, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    got = out.cpu()
    err = float((got[..., :hd] - want).abs().max())
    bound = bar(want) + (3 * BF * float(v.abs().max()) if precision == 2 else 0.0)
    print(f"padded attention hC={hC} ({hd} -> {hdp}) precision {precision}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert float(got[..., hd:].abs().max()) == 0.0


# ---------------------------------------------------------------- ASTP at 1152 channels
@pytest.mark.parametrize("x_bf16", [0, 1])
@pytest.mark.parametrize("T", [2, 77])
def test_astp_pool_1152(gpu, T, x_bf16):
    """x_bf16: the map stored in bf16 (the kernel's fp32 copy feeds the attention GEMMs); the statistics stay fp32 /
    fp64, so against float64 ASTP of the bf16-rounded map the fp32 bar holds in both forms."""
    rng = np.random.default_rng(T)
    C, H, B = CF, 128, 2
    sd = {"pool.linear1.weight": torch.from_numpy((rng.standard_normal((H, 3 * C, 1)) * np.sqrt(2 / (3 * C))).astype(np.float32)),
          "pool.linear1.bias": torch.from_numpy((rng.standard_normal(H) * 0.05).astype(np.float32)),
          "pool.linear2.weight": torch.from_numpy((rng.standard_normal((C, H, 1)) * 2 * np.sqrt(2 / H)).astype(np.float32)),
          "pool.linear2.bias": torch.from_numpy((rng.standard_normal(C) * 0.05).astype(np.float32))}
    x = torch.from_numpy((rng.standard_normal((B, T, C)) * 2.0).astype(np.float32))
    if x_bf16:
        x = x.bfloat16().float()
    want = astp({k: v.double() for k, v in sd.items()}, x.double().permute(0, 2, 1)).float()
    a = dev(gpu, x.bfloat16() if x_bf16 else x, sd["pool.linear1.weight"].reshape(H, 3 * C), sd["pool.linear1.bias"],
            sd["pool.linear2.weight"].reshape(C, H), sd["pool.linear2.bias"])
    stats = torch.full((B, 2 * C), float("nan"), device=gpu)
    _lib.call("sd_op_astp_pool_c", _lib.ptr(a[0]), x_bf16, B, T, C, *[_lib.ptr(t) for t in a[1:]], _lib.ptr(stats),
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    got = stats.cpu()
    # the mean half; the std half as variances (two frames leave them next to the 1e-7 clamp, where the square root
    # magnifies round-off, as tests/test_ecapa_host.py explains for its T = 2 golden)
    e_mean = float((got[:, :C] - want[:, :C]).abs().max())
    e_var = float((got[:, C:] ** 2 - want[:, C:] ** 2).abs().max())
    print(f"astp C=1152 T={T} bf16 map {x_bf16}: max err mean {e_mean:.3e} variance {e_var:.3e}")
    assert e_mean <= bar(want[:, :C]) and e_var <= bar(want[:, C:] ** 2)
