"""The kernels SimAM-ResNet34 adds, through their test ops: the SimAM gate (sd_op_simam) and ASP (sd_op_asp_pool)
against float64 computed on the values the kernels read, the 64-channel stem (sd_op_stem_conv) and the trunk's 3x3
convs at the new widths (sd_op_res_conv up to 512 channels) against torch CPU convs of the bf16-rounded operands."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from speaker_diarization_amd import _lib  # noqa: E402
from test_gpu_res_conv import make, one_ulp_apart, reference, run  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-5                 # fp32 outputs against float64 (test_gpu_resnet_emb.py's TSTP_RTOL)
BF16_RTOL = 2.0 ** -8       # one bf16 rounding of the float64 result
ASP_CLAMP = np.float32(1e-5)

# (B, H, W, C): a stage-1-like map over two tiles of pixels, narrow maps, and the fewest pixels a stage-4 map can have
SIMAM_MAPS = [(2, 10, 3, 64), (2, 80, 9, 64), (1, 20, 5, 256), (2, 10, 1, 512), (2, 80, 15, 64)]


def crafted_nhwc(B, H, W, C, seed):
    """Random channels; constant ones (c % 7 == 0); offset ones (c % 11 == 3: mean 100 / std 0.1, c % 11 == 5: mean
    1000 / std 0.01); one NaN element (as crafted_map of test_gpu_resnet_emb.py, over a 2-D map)."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((B, H, W, C)).astype(np.float32)
    c = np.arange(C)
    const = c % 7 == 0
    y[..., const] = rng.standard_normal((B, 1, 1, int(const.sum()))).astype(np.float32) * 3
    o1, o2 = (c % 11 == 3) & ~const, (c % 11 == 5) & ~const
    y[..., o1] = (100 + 0.1 * rng.standard_normal((B, H, W, int(o1.sum())))).astype(np.float32)
    y[..., o2] = (1000 + 0.01 * rng.standard_normal((B, H, W, int(o2.sum())))).astype(np.float32)
    nan_at = (B - 1, min(1, H - 1), W - 1, 9)      # a random channel
    y[nan_at] = np.nan
    return y, const, nan_at


def simam64(y, r):
    """float64 on (B, H, W, C): relu(y sigmoid((y - mean)^2 / (4 (v + 1e-4)) + 0.5) + r), NaN kept by the ReLU."""
    n = y.shape[1] * y.shape[2] - 1
    with np.errstate(all="ignore"):
        d = (y - y.mean((1, 2), keepdims=True)) ** 2
        v = d.sum((1, 2), keepdims=True) / n
        z = y / (1.0 + np.exp(-(d / (4 * (v + 1e-4)) + 0.5)))
        if r is not None:
            z = z + r
        return np.where(z < 0, 0.0, z)


def simam_gpu(y, r, gpu):
    B, H, W, C = y.shape
    yd = y.to(gpu).contiguous()
    rd = r.to(gpu).contiguous() if r is not None else None
    out = torch.full_like(yd, -7.0)
    _lib.call("sd_op_simam", _lib.ptr(yd), _lib.ptr(rd), int(y.dtype == torch.bfloat16), B, H, W, C, _lib.ptr(out),
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SIMAM_MAPS, ids=["x".join(map(str, s)) for s in SIMAM_MAPS])
def test_simam_vs_float64(gpu, shape, dtype, residual):
    B, H, W, C = shape
    y, const, nan_at = crafted_nhwc(B, H, W, C, 7 + H * W + C)
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    yt = torch.from_numpy(y).to(td)
    rt = None
    if residual:
        rt = torch.from_numpy(np.random.default_rng(3 + C).standard_normal(shape).astype(np.float32)).to(td)
    y64 = yt.float().numpy().astype(np.float64)              # the (bf16-rounded) values the kernel reads
    r64 = rt.float().numpy().astype(np.float64) if residual else None
    want = simam64(y64, r64)
    got_t = simam_gpu(yt, rt, gpu)
    got = got_t.float().numpy().astype(np.float64)
    # a NaN poisons its (b, c) channel and nothing else
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN not where float64 puts it"
    assert nan[nan_at[0], :, :, nan_at[3]].all() and nan.sum() == H * W
    # constant channels: d = 0, v = 0 -> y sigmoid(0.5) + r
    cw = y64[..., const] / (1.0 + np.exp(-0.5)) + (r64[..., const] if residual else 0.0)
    cw = np.where(cw < 0, 0.0, cw)
    assert np.array_equal(want[..., const], cw)
    ok = ~nan
    rel = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
    rel[(got[ok] == 0) & (want[ok] == 0)] = 0.0
    # the kernel's constant channels against the closed form, within one rounding to the output type (half an ulp:
    # 2^-24 relative in fp32, 2^-8 in bf16)
    one = (2.0 ** -24 if dtype == "fp32" else 2.0 ** -8) * 1.001
    assert (np.abs(got[..., const] - cw) <= one * np.abs(cw)).all()
    tol = RTOL if dtype == "fp32" else BF16_RTOL
    print(f"simam {shape} {dtype} res={residual}: max rel err {rel.max():.3e} (bound {tol:.3e}); "
          f"constant channels max abs err {np.abs(got[..., const] - cw).max():.3e}")
    assert rel.max() <= tol
    # item 0 alone is bit-identical to item 0 of the batch
    if B > 1:
        alone = simam_gpu(yt[:1], rt[:1] if residual else None, gpu)
        it = torch.int16 if dtype == "bf16" else torch.int32
        assert torch.equal(alone.view(it), got_t[:1].view(it))


def asp64(x, w1, b1, s, h, w2, b2):
    """float64 ASP on x (B, T, C): [mu | sqrt(max(sum a (x - mu)^2, fp32 1e-5))], the variance itself (float64's
    E[x^2] - mu^2 loses it at mean 1000).  The attention's ReLU is the GEMM epilogue's maximum, which drops a NaN
    (np.fmax), so a NaN frame poisons its own channel's statistics only."""
    with np.errstate(all="ignore"):
        hid = np.fmax(x @ w1.T + b1, 0.0) * s + h
        e = hid @ w2.T + b2
        e = e - e.max(axis=1, keepdims=True)
        a = np.exp(e)
        a = a / a.sum(1, keepdims=True)
        mu = (a * x).sum(1)
        var = (a * (x - mu[:, None, :]) ** 2).sum(1)
        sg = np.sqrt(np.where(np.isnan(var), np.nan, np.maximum(var, np.float64(ASP_CLAMP))))
    return np.concatenate([mu, sg], 1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [1, 2, 3, 25, 75])
def test_asp_pool_vs_float64(gpu, T, dtype):
    B, C, H = 2, 5120, 128
    rng = np.random.default_rng(50 + T)
    # The map ASP reads is a ReLU output: non-negative channels, constant ones (c % 7 == 0), offset ones (c % 11 == 3:
    # mean 100 / std 0.1, c % 11 == 5: mean 1000 / std 0.01), one NaN element.  The fp32 attention GEMMs leave the
    # softmax weights a relative error of about 2e-6 against float64; on non-negative channels mu and sg inherit it
    # without cancellation (d var = sum da (x - mu)^2), which is what the 1e-5 bound allows for.
    x = np.abs(rng.standard_normal((B, T, C))).astype(np.float32)
    c = np.arange(C)
    const = c % 7 == 0
    x[:, :, const] = np.abs(rng.standard_normal((B, 1, int(const.sum())))).astype(np.float32) * 3
    o1, o2 = (c % 11 == 3) & ~const, (c % 11 == 5) & ~const
    x[:, :, o1] = (100 + 0.1 * rng.standard_normal((B, T, int(o1.sum())))).astype(np.float32)
    x[:, :, o2] = (1000 + 0.01 * rng.standard_normal((B, T, int(o2.sum())))).astype(np.float32)
    x[1, min(1, T - 1), 78] = np.nan                        # poisons channel 78 of item 1 and nothing else
    # attention.0 weighs the offset channels down by their size (0.01 at mean 100, 0.001 at mean 1000), so every
    # channel adds O(0.02) to a pre-activation of O(1).  With equal weights the 1000-valued channels alone would make
    # the fp32 GEMM's partial sums +-40, whose rounding (ulp 4e-6 over 1280 MFMA steps: 5e-5, measured 6e-5 on the
    # pooled statistics) is fp32 accumulation, the reference's own arithmetic, not the pooling under test.
    w1 = (rng.standard_normal((H, C)) * np.sqrt(2.0 / C)).astype(np.float32)
    w1[:, o1] *= 0.01
    w1[:, o2] *= 0.001
    b1 = (rng.standard_normal(H) * 0.05).astype(np.float32)
    s = rng.uniform(0.7, 1.3, H).astype(np.float32)
    h = (rng.standard_normal(H) * 0.1).astype(np.float32)
    w2 = (rng.standard_normal((C, H)) * 0.5 * np.sqrt(2.0 / H)).astype(np.float32)
    b2 = (rng.standard_normal(C) * 0.05).astype(np.float32)
    xt = torch.from_numpy(x)
    if dtype == "bf16":
        xt = xt.to(torch.bfloat16)
    x64 = xt.float().numpy().astype(np.float64)
    want = asp64(x64, *[a.astype(np.float64) for a in (w1, b1, s, h, w2, b2)])
    dev = [torch.from_numpy(a).to(gpu).contiguous() for a in (w1, b1, s, h, w2, b2)]
    stats = torch.full((B, 2 * C), -7.0, device=gpu)
    xd = xt.to(gpu).contiguous()
    _lib.call("sd_op_asp_pool", _lib.ptr(xd), int(dtype == "bf16"), B, T, C,
              *[_lib.ptr(a) for a in dev], _lib.ptr(stats), _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    got = stats.cpu().numpy()
    nan = np.isnan(want)
    assert nan.sum() == 2 and nan[1, 78] and nan[1, C + 78]
    assert np.array_equal(np.isnan(got), nan), "NaN not where float64 puts it"
    if T == 1:
        ok = ~nan[:, C:]
        assert (got[:, C:][ok] == np.sqrt(ASP_CLAMP)).all()  # weight 1, variance 0: sg is the clamp, bit for bit
        assert np.array_equal(got[0, :C], xt[0, 0].float().numpy())
        return
    assert (got[:, C:][:, const] == np.sqrt(ASP_CLAMP)).all()   # constant channels: variance <= rounding, clamped
    ok = ~nan
    rel = np.abs(got[ok].astype(np.float64) - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
    print(f"asp T={T} {dtype}: max rel err {rel.max():.3e}")
    assert rel.max() <= RTOL


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_asp_pool_signed_map_unscaled_weights(gpu, dtype):
    """The companion of the case above: a signed map and attention weights of one scale on every channel, the
    mean-1000 ones included.  The fp32 attention GEMM then sums 465 terms of about +-20 (pre-activations to +-1300,
    partial sums to +-2048, ulp 2.4e-4): over its 1280 accumulation steps the pre-activation carries 2.5e-3 (random
    rounding, ulp / sqrt(12) * sqrt(1280)) to 0.15 (every rounding one way), the scores 0.7 times that (|w2 row| over
    128 inputs), and a statistic that error times the channel's spread over time (<= ~1 here).  The bound is absolute,
    2e-2: 10 times the random-rounding estimate of 1.8e-3 and 5 times below the one-way worst case."""
    B, T, C, H = 2, 25, 5120, 128
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    c = np.arange(C)
    o1, o2 = c % 11 == 3, c % 11 == 5
    x[:, :, o1] = (100 + 0.1 * rng.standard_normal((B, T, int(o1.sum())))).astype(np.float32)
    x[:, :, o2] = (1000 + 0.01 * rng.standard_normal((B, T, int(o2.sum())))).astype(np.float32)
    w1 = (rng.standard_normal((H, C)) * np.sqrt(2.0 / C)).astype(np.float32)
    b1 = (rng.standard_normal(H) * 0.05).astype(np.float32)
    s = rng.uniform(0.7, 1.3, H).astype(np.float32)
    h = (rng.standard_normal(H) * 0.1).astype(np.float32)
    w2 = (rng.standard_normal((C, H)) * 0.5 * np.sqrt(2.0 / H)).astype(np.float32)
    b2 = (rng.standard_normal(C) * 0.05).astype(np.float32)
    xt = torch.from_numpy(x)
    if dtype == "bf16":
        xt = xt.to(torch.bfloat16)
    want = asp64(xt.float().numpy().astype(np.float64), *[a.astype(np.float64) for a in (w1, b1, s, h, w2, b2)])
    dev = [torch.from_numpy(a).to(gpu).contiguous() for a in (w1, b1, s, h, w2, b2)]
    stats = torch.full((B, 2 * C), -7.0, device=gpu)
    xd = xt.to(gpu).contiguous()
    _lib.call("sd_op_asp_pool", _lib.ptr(xd), int(dtype == "bf16"), B, T, C, *[_lib.ptr(a) for a in dev],
              _lib.ptr(stats), _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    got = stats.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    print(f"asp signed {dtype}: max abs err {err.max():.3e} (mu {err[:, :C].max():.3e}, sg {err[:, C:].max():.3e})")
    assert err.max() <= 2e-2


# (B, T, F) for the stem; the second spans several 256-thread workgroups and an odd map
@pytest.mark.parametrize("out_bf16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("shape", [(1, 2, 3), (2, 37, 80)], ids=["1x2x3", "2x37x80"])
def test_stem_conv_vs_cpu(gpu, shape, C, out_bf16):
    B, T, Fd = shape
    g = torch.Generator().manual_seed(11 + C + T)
    fb = torch.randn(B, T, Fd, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) * (2.0 / 9) ** 0.5
    al, be = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    ref = torch.relu(F.conv2d(fb.permute(0, 2, 1).unsqueeze(1), w, padding=1) * al[None, :, None, None]
                     + be[None, :, None, None]).permute(0, 2, 3, 1)          # (B, F, T, C)
    out = torch.full((B, Fd, T, C), -7.0, device=gpu, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    fbd, wd, ald, bed = (t.to(gpu).contiguous() for t in (fb, w, al, be))
    _lib.call("sd_op_stem_conv", _lib.ptr(fbd), B, T, Fd, _lib.ptr(wd), _lib.ptr(ald), _lib.ptr(bed), C, _lib.ptr(out),
              out_bf16, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    got = out.cpu().float()
    err = float((got - ref).abs().max())
    print(f"stem {shape} C={C} bf16={out_bf16}: max abs err {err:.3e}")
    if out_bf16:
        assert torch.allclose(got, ref.to(torch.bfloat16).float(), atol=2e-2, rtol=1e-2)
    else:
        assert torch.allclose(got, ref, atol=1e-5, rtol=1e-5)
    with pytest.raises(ValueError, match="32 or 64"):
        _lib.call("sd_op_stem_conv", _lib.ptr(fbd), B, T, Fd, _lib.ptr(wd), _lib.ptr(ald), _lib.ptr(bed), 48,
                  _lib.ptr(out), out_bf16, _lib.stream_ptr(gpu))


# every (Cin, Cout, stride) class the SimAM trunk adds, each on a map as small as 3 x 2 and on one that spans two
# tiles: (B, H, W, Cin, Cout, stride, residual, shortcut)
WIDE = [
    (1, 3, 2, 64, 64, 1, True, False), (1, 80, 20, 64, 64, 1, False, False),
    (1, 3, 2, 64, 128, 2, False, True), (1, 9, 40, 64, 128, 2, False, True),
    (1, 3, 2, 128, 256, 2, False, True), (1, 9, 40, 128, 256, 2, False, True),
    (1, 3, 2, 256, 512, 2, False, True), (1, 9, 40, 256, 512, 2, False, True),
    (2, 3, 2, 512, 512, 1, True, False), (1, 10, 30, 512, 512, 1, False, False),
]
WIDE_IDS = ["%dx%dx%d_%dto%d_s%d%s%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "_res" if c[6] else "", "_sc" if c[7] else "")
            for c in WIDE]


@pytest.mark.parametrize("case", WIDE, ids=WIDE_IDS)
def test_res_conv_at_the_new_widths(gpu, case):
    d = make(case)
    ref, ref_sc = reference(case, d)
    got, got_sc = run(case, d, gpu, generic=0)
    gen, gen_sc = run(case, d, gpu, generic=1)
    print(WIDE_IDS[WIDE.index(case)], "max|kernel - cpu| %.3e  max|generic - cpu| %.3e  max|kernel - generic| %.3e" % (
        (got.float() - ref).abs().max(), (gen.float() - ref).abs().max(), (got.float() - gen.float()).abs().max()))
    assert torch.allclose(got.float(), ref, atol=2e-2, rtol=1e-2)
    assert torch.allclose(gen.float(), ref, atol=2e-2, rtol=1e-2)
    assert one_ulp_apart(got, gen)
    if ref_sc is not None:
        assert torch.allclose(got_sc.float(), ref_sc, atol=2e-2, rtol=1e-2)
        assert torch.allclose(gen_sc.float(), ref_sc, atol=2e-2, rtol=1e-2)
        assert one_ulp_apart(got_sc, gen_sc)
