"""The two kernels w2v-BERT 2.0 adds (csrc/w2vbert.hip), through their test ops, each against an fp64 numpy reference.

Tolerances.  fp32 arms: 1e-5 max |ref|, the order of an exact-f32 MFMA accumulation over K = 64 (attention) / a 31-tap
fp32 FMA chain (conv mix) followed by fp32 softmax / LayerNorm arithmetic.  bf16 arms: the reference is computed on the
operands rounded to bf16 as the kernel rounds them, so what is left is the accumulation order and the roundings the
kernel adds, bounded from the format as in test_gpu_wavlm_ops.py (bf16 has 8 significant bits: a value is rounded by at
most 2^-8 of itself):
  attention: each P is rounded to bf16 for P V (the row sum keeps the unrounded values), so the output, a convex
    combination of v, moves by at most 2^-8 max |v|: fp32 bar + 2^-8 max |v|;
  conv mix: operands only on the way in, the fp32 result rounded once on the way out: fp32 bar + 2^-8 max |ref|
    (layer 0 of WavLM with a bf16 map out).
The fp32 bar of those two is the project's, 1e-3 max(1, max |ref|).
"""
import numpy as np
import pytest
import torch

from speaker_diarization_amd import _lib

pytestmark = pytest.mark.gpu
H, LEFT, RIGHT, C, K, TILE = 16, 64, 8, 1024, 31, 16
ATTN_T = [1, 9, 10, 16, 17, 64, 65, 66, 80, 200]
MIX_T = [1, TILE - 1, TILE, TILE + 1, 30, 31, 32, 200]


def rb(x):
    """fp32 values rounded to bf16 (round to nearest even, as the kernels round)."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def check(got, ref, bound, what):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    e = float(np.abs(got - ref).max())
    print(f"{what}: max|got - ref| {e:.3e}  bound {bound:.3e}  max|ref| {float(np.abs(ref).max()):.3f}")
    assert e <= bound, (what, e, bound)


# ---------------------------------------------------------------- relative-key attention
_attn = {}


def attention_case(T):
    """B = 2 windows; q scaled so that q . k / 8 and q . E / 8 both have a standard deviation near 2: sharp rows in
    which the distance term matters as much as the content term."""
    if T not in _attn:
        rng = np.random.default_rng(500 + T)
        B, D = 2, H * 64
        qkv = rng.standard_normal((B * T, 3 * D)).astype(np.float32)
        qkv[:, :D] *= 2.0
        dist = rng.standard_normal((LEFT + RIGHT + 1, 64)).astype(np.float32)
        _attn[T] = dict(B=B, T=T, D=D, qkv=qkv, dist=dist, ref={})
    return _attn[T]


def attention_ref(c, precision):
    """fp64: softmax((q k^T + q E[clamp(r - l, -64, 8) + 64]^T) / 8) v per window and head."""
    if precision not in c["ref"]:
        B, T, D = c["B"], c["T"], c["D"]
        qkv, E = (rb(c["qkv"]), rb(c["dist"])) if precision else (c["qkv"], c["dist"])
        q, k, v = (t.reshape(B, T, H, 64).transpose(0, 2, 1, 3).astype(np.float64) for t in np.split(qkv, 3, axis=1))
        pos = np.arange(T)
        idx = np.clip(pos[None, :] - pos[:, None], -LEFT, RIGHT) + LEFT          # [query l, key r]
        rel = np.take_along_axis(q @ E.astype(np.float64).T, np.broadcast_to(idx, (B, H, T, T)), axis=-1)
        s = (q @ k.transpose(0, 1, 3, 2) + rel) / 8.0
        p = np.exp(s - s.max(-1, keepdims=True))
        o = (p / p.sum(-1, keepdims=True)) @ v
        c["ref"][precision] = (o.transpose(0, 2, 1, 3).reshape(B * T, D), float(np.abs(rel / 8).std()),
                               float(np.abs(v).max()))
    return c["ref"][precision]


def attention_gpu(qkv, dist, B, T, gpu, precision):
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (qkv, dist)]
    out = torch.full((B * T, H * 64), float("nan"), device=gpu)
    _lib.call("sd_op_w2vbert_attention", _lib.ptr(d[0]), B, T, H, _lib.ptr(d[1]), _lib.ptr(out), precision,
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("T", ATTN_T)
def test_relative_key_attention(gpu, T, precision):
    """T 1: a single key; 9 / 10: the right clamp (+8) just inactive / just active; 16 / 17 and 64 / 65: query-tile and
    64-key-tile edges; 65 / 66: the left clamp (-64) just inactive / active; 80, 200: several tiles with both clamps."""
    c = attention_case(T)
    ref, rel_std, vmax = attention_ref(c, precision)
    if T > 1:
        assert rel_std > 0.5                                   # the distance term is not small beside q . k
    got = attention_gpu(c["qkv"], c["dist"], c["B"], T, gpu, precision)
    amax = float(np.abs(ref).max())
    bound = 1e-5 * amax if precision == 0 else 1e-3 * max(1.0, amax) + 2.0 ** -8 * vmax
    check(got, ref, bound, f"relative-key attention T={T} precision={precision}")


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("T", [17, 66])
def test_attention_windows_are_independent(gpu, T, precision):
    """Two windows with different content in one call equal two single-window calls bit for bit."""
    c = attention_case(T)
    both = attention_gpu(c["qkv"], c["dist"], 2, T, gpu, precision)
    for b in range(2):
        one = attention_gpu(c["qkv"][b * T:(b + 1) * T], c["dist"], 1, T, gpu, precision)
        assert np.array_equal(one.view(np.int32), both[b * T:(b + 1) * T].view(np.int32)), (T, b)


@pytest.mark.parametrize("precision", [0, 1])
def test_attention_with_a_zero_distance_embedding_is_plain_softmax_attention(gpu, precision):
    c = attention_case(80)
    qkv = rb(c["qkv"]) if precision else c["qkv"]
    q, k, v = (torch.from_numpy(t.reshape(2, 80, H, 64)).permute(0, 2, 1, 3).double() for t in np.split(qkv, 3, axis=1))
    ref = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).permute(0, 2, 1, 3).reshape(160, H * 64).numpy()
    got = attention_gpu(c["qkv"], np.zeros_like(c["dist"]), 2, 80, gpu, precision)
    amax = float(np.abs(ref).max())
    bound = 1e-5 * amax if precision == 0 else 1e-3 * max(1.0, amax) + 2.0 ** -8 * float(v.abs().max())
    check(got, ref, bound, f"attention, zero distance embedding, precision={precision}")


# ---------------------------------------------------------------- conv mix
_mix = {}


def mix_case(T):
    if T not in _mix:
        rng = np.random.default_rng(600 + T)
        x = rng.standard_normal((2, T, 2 * C)).astype(np.float32) * 1.5
        w = (rng.standard_normal((C, K)) / np.sqrt(K)).astype(np.float32)
        g = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
        b = (0.1 * rng.standard_normal(C)).astype(np.float32)
        _mix[T] = dict(T=T, x=x, w=w, g=g, b=b, ref={})
    return _mix[T]


def mix_ref(c, precision):
    """fp64: GLU over channels, left zero pad of 30 + depthwise k31 within each window, LayerNorm over C, swish."""
    if precision not in c["ref"]:
        x = (rb(c["x"]) if precision else c["x"]).astype(np.float64)
        T = c["T"]
        y = x[:, :, :C] / (1.0 + np.exp(-x[:, :, C:]))
        yp = np.concatenate([np.zeros((2, K - 1, C)), y], 1)
        w = c["w"].astype(np.float64)
        z = sum(yp[:, k:k + T] * w[:, k] for k in range(K))              # z[t] = sum_k w[k] y[t - 30 + k]
        z = (z - z.mean(-1, keepdims=True)) / np.sqrt(z.var(-1, keepdims=True) + 1e-5) * c["g"] + c["b"]
        c["ref"][precision] = z / (1.0 + np.exp(-z))
    return c["ref"][precision]


def mix_gpu(c, x, gpu, precision):
    B, T = x.shape[:2]
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (x, c["w"], c["g"], c["b"])]
    out = torch.full((B, T, C), float("nan"), device=gpu)
    _lib.call("sd_op_w2vbert_conv_mix", _lib.ptr(d[0]), B, T, _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]),
              _lib.ptr(out), precision, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("T", MIX_T)
def test_conv_mix(gpu, T, precision):
    """T 1, 30, 31, 32: windows shorter than, as long as and longer than the 31 taps; 15, 16, 17: the 16-frame time
    tile -+ 1; 200: 13 tiles.  B = 2, so every halo of the second window starts at a window boundary."""
    c = mix_case(T)
    ref = mix_ref(c, precision)
    got = mix_gpu(c, c["x"], gpu, precision)
    amax = float(np.abs(ref).max())
    bound = 1e-5 * amax if precision == 0 else 1e-3 * max(1.0, amax) + 2.0 ** -8 * amax
    check(got, ref, bound, f"conv mix T={T} precision={precision}")


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("T", [1, TILE + 1, 32])
def test_conv_mix_reads_no_halo_across_windows(gpu, T, precision):
    """Window order (huge, normal) and (normal, huge): the normal window's output is bit-identical to its output in
    the plain batch, so neither the left halo of window 1 nor anything of window 0 reads the neighbour's frames."""
    c = mix_case(T)
    plain = mix_gpu(c, c["x"], gpu, precision)
    for keep in (0, 1):
        x = c["x"].copy()
        x[1 - keep] = 1e30
        got = mix_gpu(c, x, gpu, precision)
        assert np.array_equal(got[keep].view(np.int32), plain[keep].view(np.int32)), (T, keep)
