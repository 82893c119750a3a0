"""The kernels WavLM adds (csrc/wavlm.hip), through their test ops, each against tests/wavlm_ref.py or the torch formula.

Tolerances.  fp32 arms: the project's fp32 bar, max |got - ref| <= 1e-3 max(1, max |ref|).  bf16 arms: the reference is
computed in fp32 on the operands rounded to bf16 as the kernel rounds them, so what is left is the accumulation order
and the roundings the kernel adds, bounded from the format (bf16 has 8 significant bits: a value in [2^e, 2^(e+1)) is
rounded by at most half an ulp, 2^(e-8), so by at most 2^-8 of itself):
  conv layers 1-6 and pos_conv: operands only, fp32 accumulation and output: the fp32 bar (a bf16 map out, precision 2
    of the conv op: + 2^-8 max |ref|, and what the test states for the LayerNorm that reads a bf16 map);
  layer 0 with a bf16 map: the fp32 result rounded once: fp32 bar + 2^-8 max |ref|;
  attention: each P is rounded to bf16 for P V (the row sum keeps the unrounded values), so the output, a convex
    combination of v, moves by at most 2^-8 max |v|: fp32 bar + 2^-8 max |v|.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from speaker_diarization_amd import _lib  # noqa: E402
import wavlm_ref as wr  # noqa: E402

pytestmark = pytest.mark.gpu
A = "encoder.layers.0.self_attn."


def fp32_bar(ref):
    return 1e-3 * max(1.0, float(ref.abs().max()))


def rb(x):
    """fp32 values rounded to bf16 (round to nearest even, as the kernels round)."""
    return x.to(torch.bfloat16).float()


def check(got, ref, bound, what):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    e = float((got - ref).abs().max())
    print(f"{what}: max|got - ref| {e:.3e}  bound {bound:.3e}  max|ref| {float(ref.abs().max()):.3f}")
    assert e <= bound, (what, e, bound)


def dev(gpu, *ts):
    return [t.to(gpu).contiguous() for t in ts]


# ---------------------------------------------------------------- layer 0
@pytest.mark.parametrize("out_bf16", [0, 1])
@pytest.mark.parametrize("n", [400, 16000])
@pytest.mark.parametrize("mode", ["default", "layer_norm"])
def test_layer0(gpu, mode, n, out_bf16):
    B = 2
    rng = np.random.default_rng(11 + n)
    wav = torch.from_numpy((rng.standard_normal((B, n)) * 0.5 + 0.05).astype(np.float32))
    p = "feature_extractor.conv_layers.0."
    nk = p + ("2.1" if mode == "layer_norm" else "2")
    sd = {p + "0.weight": torch.from_numpy((rng.standard_normal((512, 1, 10)) * np.sqrt(0.2)).astype(np.float32)),
          nk + ".weight": torch.from_numpy((1 + 0.1 * rng.standard_normal(512)).astype(np.float32)),
          nk + ".bias": torch.from_numpy((0.1 * rng.standard_normal(512)).astype(np.float32))}
    ref = wr.conv_layer0(sd, wav, mode).transpose(1, 2).contiguous()
    T0 = (n - 10) // 5 + 1
    assert ref.shape == (B, T0, 512)
    d = dev(gpu, wav, sd[p + "0.weight"], sd[nk + ".weight"], sd[nk + ".bias"])
    out = torch.full((B, T0, 512), float("nan"), device=gpu, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    _lib.call("sd_op_wavlm_layer0", _lib.ptr(d[0]), B, n, _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]),
              int(mode == "layer_norm"), _lib.ptr(out), out_bf16, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    bound = fp32_bar(ref) + (2.0 ** -8 * float(ref.abs().max()) if out_bf16 else 0.0)
    check(out.cpu().float(), ref, bound, f"layer0 {mode} n={n} bf16={out_bf16}")


def test_layer0_group_norm_statistics_over_a_long_window_with_an_offset(gpu):
    """10 s of audio (31,999 frames) with a DC offset a hundred times the signal: a one-pass sum of squares in fp32
    would lose the variance; the chunked two-pass statistics merged in fp64 do not."""
    B, n = 1, 160000
    rng = np.random.default_rng(12)
    wav = torch.from_numpy((rng.standard_normal((B, n)) * 0.01 + 1.0).astype(np.float32))
    w = torch.from_numpy(rng.uniform(0.05, 0.15, (512, 1, 10)).astype(np.float32))
    g, b = torch.ones(512), torch.zeros(512)
    x = F.conv1d(wav.double().unsqueeze(1), w.double(), stride=5)
    ref = F.gelu((x - x.mean(-1, keepdim=True)) / (x.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt())
    ref = ref.float().transpose(1, 2).contiguous()
    T0 = ref.shape[1]
    assert T0 == 31999
    d = dev(gpu, wav, w, g, b)
    out = torch.full((B, T0, 512), float("nan"), device=gpu)
    _lib.call("sd_op_wavlm_layer0", _lib.ptr(d[0]), B, n, _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), 0,
              _lib.ptr(out), 0, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    # the conv output itself (about 1.0, ulp 1.2e-7) carries fp32 rounding of 6e-8 against a deviation of ~3e-3 after
    # the norm: ~2e-5 relative to a unit-variance output, far inside the bar
    check(out.cpu(), ref, fp32_bar(ref), "layer0 default, 31999 frames, offset 1.0")


# ---------------------------------------------------------------- conv layers 1-6
@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("k,T", [(3, 79), (2, 4), (3, 80), (2, 5)])
def test_strided_conv(gpu, k, T, ln, precision):
    """k 3 on 79 -> 39 and k 2 on 4 -> 2 (the issue's cases), and the other parity of each: 80 -> 39, 5 -> 2.
    precision 2: bf16 operands and a bf16 map out, the form layers 1-5 take in the model's bf16 mode; with the
    LayerNorm the raw conv result is stored in bf16 first and the norm reads that map."""
    B = 2
    rng = np.random.default_rng(20 + T)
    x = torch.from_numpy(rng.standard_normal((B, T, 512)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((512, 512, k)) * np.sqrt(2.0 / (512 * k))).astype(np.float32))
    g = torch.from_numpy((1 + 0.1 * rng.standard_normal(512)).astype(np.float32))
    b = torch.from_numpy((0.1 * rng.standard_normal(512)).astype(np.float32))
    xr, wq = (rb(x), rb(w)) if precision else (x, w)
    y = F.conv1d(xr.transpose(1, 2), wq, stride=2)
    extra = 0.0
    if ln:
        if precision == 2:
            # the stored conv map: where the kernel's sum and torch's fall on two sides of a rounding boundary the
            # LayerNorm input differs by one bf16 ulp, 2^-7 of a value of at most max |y|; the norm divides by the
            # row's standard deviation (>= 0.5 here, asserted) and multiplies by g (<= 1.5)
            assert float(y.std(dim=1).min()) >= 0.5 and float(g.abs().max()) <= 1.5
            extra += 2.0 ** -7 * float(y.abs().max()) / 0.5 * 1.5
            y = rb(y)
        y = F.layer_norm(y.transpose(1, 2), (512,), g, b).transpose(1, 2)
    ref = F.gelu(y).transpose(1, 2).contiguous()
    To = (T - k) // 2 + 1
    assert ref.shape == (B, To, 512) and To == {79: 39, 80: 39, 4: 2, 5: 2}[T]
    if precision == 2:
        extra += 2.0 ** -8 * float(ref.abs().max())          # the output rounded to bf16 once
    d = dev(gpu, x, w, g, b)
    out = torch.full((B, To, 512), float("nan"), device=gpu, dtype=torch.bfloat16 if precision == 2 else torch.float32)
    _lib.call("sd_op_wavlm_conv", _lib.ptr(d[0]), B, T, _lib.ptr(d[1]), k, _lib.ptr(d[2]) if ln else None,
              _lib.ptr(d[3]) if ln else None, _lib.ptr(out), precision, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    check(out.cpu().float(), ref, fp32_bar(ref) + extra, f"conv k{k} T={T} ln={ln} precision={precision}")


# ---------------------------------------------------------------- pos_conv
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("D", [768, 1024])
@pytest.mark.parametrize("T", [1, 2, 49, 130])
def test_pos_conv(gpu, T, D, precision):
    """Both pad edges (every T), a window shorter than the kernel (1, 2, 49) and longer (130: three 64-frame tiles)."""
    B = 2
    rng = np.random.default_rng(30 + T + D)
    x = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((D, D // 16, 128)) * np.sqrt(4.0 / (128 * D)) * 2).astype(np.float32))
    bias = torch.from_numpy((0.1 * rng.standard_normal(D)).astype(np.float32))
    xr, wq = (rb(x), rb(w)) if precision else (x, w)
    y = F.conv1d(xr.transpose(1, 2), wq, bias, padding=64, groups=16)[:, :, :-1]
    ref = x + F.gelu(y).transpose(1, 2)          # the residual stream stays fp32
    d = dev(gpu, x, w, bias)
    out = torch.full((B, T, D), float("nan"), device=gpu)
    _lib.call("sd_op_wavlm_pos_conv", _lib.ptr(d[0]), B, T, D, _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(out), precision,
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert float((ref - x).abs().max()) > 0.2     # the conv term is not small beside the bar, even from one tap
    check(out.cpu(), ref, fp32_bar(ref), f"pos_conv T={T} D={D} precision={precision}")


# ---------------------------------------------------------------- bias table + gated attention
@pytest.mark.parametrize("T,H", [(1, 12), (109, 12), (199, 16)])
def test_bias_table(gpu, T, H):
    emb = torch.from_numpy(np.random.default_rng(40).standard_normal((320, H)).astype(np.float32))
    ref = wr.bias_table({A + "relative_attention_bias.weight": emb}, T)
    assert ref.shape == (H, 2 * T - 1)
    out = torch.full((H, 2 * T - 1), float("nan"), device=gpu)
    e = emb.to(gpu)
    _lib.call("sd_op_wavlm_bias_table", _lib.ptr(e), T, H, _lib.ptr(out), _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)


def attention_case(T, H, seed, gates="seeded", zero_table=False):
    B, D = 2, H * 64
    rng = np.random.default_rng(seed)
    qkv = torch.from_numpy(rng.standard_normal((B * T, 3 * D)).astype(np.float32))
    qkv[:, :D] *= 2.0                                  # scores of standard deviation 2 before the bias
    xin = torch.from_numpy(rng.standard_normal((B * T, D)).astype(np.float32))
    gw = torch.from_numpy((0.5 * rng.standard_normal((8, 64)) / 8).astype(np.float32))
    gb = torch.from_numpy((0.5 * rng.standard_normal(8)).astype(np.float32))
    ga = torch.from_numpy((1 + 0.5 * rng.standard_normal(H)).astype(np.float32))
    if gates == "one":       # sigmoid(0) = 0.5 twice: 0.5 (0.5 * -2 - 1) + 2 = 1
        gw, gb, ga = torch.zeros(8, 64), torch.zeros(8), torch.full((H,), -2.0)
    table = torch.from_numpy((1.5 * rng.standard_normal((H, 2 * T - 1))).astype(np.float32))
    if zero_table:
        table = torch.zeros(H, 2 * T - 1)
    return dict(B=B, T=T, H=H, D=D, qkv=qkv, xin=xin, gw=gw, gb=gb, ga=ga, table=table)


def attention_gpu(c, gpu, precision):
    d = dev(gpu, c["qkv"], c["xin"], c["gw"], c["gb"], c["ga"], c["table"])
    out = torch.full((c["B"] * c["T"], c["D"]), float("nan"), device=gpu)
    _lib.call("sd_op_wavlm_attention", _lib.ptr(d[0]), _lib.ptr(d[1]), c["B"], c["T"], c["H"], _lib.ptr(d[2]),
              _lib.ptr(d[3]), _lib.ptr(d[4]), _lib.ptr(d[5]), _lib.ptr(out), precision, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return out.cpu()


def split_heads(c, precision):
    B, T, H, D = c["B"], c["T"], c["H"], c["D"]
    qkv = rb(c["qkv"]) if precision else c["qkv"]
    return [t.reshape(B, T, H, 64).permute(0, 2, 1, 3) for t in qkv.split(D, dim=1)]


def attention_bound(c, ref, precision):
    v = float(c["qkv"][:, 2 * c["D"]:].abs().max())
    return fp32_bar(ref) + (2.0 ** -8 * v if precision else 0.0)


def merge(o, c):
    return o.permute(0, 2, 1, 3).reshape(c["B"] * c["T"], c["D"])


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("H", [12, 16])
@pytest.mark.parametrize("T", [1, 2, 49, 109, 199])
def test_gated_attention(gpu, T, H, precision):
    c = attention_case(T, H, 50 + T + H)
    q, k, v = split_heads(c, precision)
    sd = {A + "grep_linear.weight": c["gw"], A + "grep_linear.bias": c["gb"], A + "grep_a": c["ga"].view(1, H, 1, 1)}
    gate = wr.gates(sd, 0, c["xin"].view(c["B"], T, c["D"]), H)
    assert gate.shape == (c["B"], H, T)
    if T > 1:
        assert float(gate.max() - gate.min()) > 0.5          # the gates differ across queries and heads
    ref = merge(wr.gated_attention(q, k, v, gate, c["table"]), c)
    check(attention_gpu(c, gpu, precision), ref, attention_bound(c, ref, precision),
          f"gated attention T={T} H={H} precision={precision}")


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("T,H", [(49, 12), (199, 16)])
def test_attention_with_all_gates_one(gpu, T, H, precision):
    c = attention_case(T, H, 60 + T, gates="one")
    q, k, v = split_heads(c, precision)
    ref = merge(wr.gated_attention(q, k, v, torch.ones(c["B"], H, T), c["table"]), c)
    check(attention_gpu(c, gpu, precision), ref, attention_bound(c, ref, precision),
          f"attention, gates 1, T={T} H={H} precision={precision}")


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("T,H", [(49, 12), (199, 16)])
def test_attention_with_a_zero_table_is_plain_softmax_attention(gpu, T, H, precision):
    c = attention_case(T, H, 70 + T, zero_table=True)
    q, k, v = split_heads(c, precision)
    ref = merge(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(64), dim=-1) @ v, c)
    check(attention_gpu(c, gpu, precision), ref, attention_bound(c, ref, precision),
          f"attention, zero table, T={T} H={H} precision={precision}")
