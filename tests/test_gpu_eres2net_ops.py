"""The kernels ERes2NetV2 adds, through their test ops: the Res2Net slice conv (sd_op_res2_conv3x3) against torch fp32
convs of the same bf16-rounded operands, and the in-block attentional fusion (sd_op_aff_gate) against float64 computed
on the values the kernel reads."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
WIDTHS = [24, 26, 48, 52, 96, 104, 192, 208]
SENTINEL = -7.0          # exact in bf16
# bf16 arms: max |got - reference| measured on MI355X (the kernels are deterministic), the largest case of each kind;
# the bounds are twice these.  Both kernels round an fp32 result to bf16 once: res2_conv3x3's lies in [0, 20] (half an
# ulp at 16 .. 20 is 6.25e-2; every case measured 5.98e-2 .. 6.25e-2), aff_gate's reaches 32 in these cases (half an
# ulp at 16 .. 32 again; 2.19e-2 at one pixel .. 6.25e-2), 4.81e-2 with the saturated tanh.
BF16_MEASURED = {"res2_conv3x3": 6.25e-2, "aff_gate": 6.25e-2, "aff_gate_saturated": 4.81e-2}
BF16_ATOL = {k: 2 * v for k, v in BF16_MEASURED.items()}
U = 2.0 ** -24           # fp32 unit round-off


def bf(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16)


def res2_case(B, H, W, width, slices, xi, oi, add, seed, positive=False):
    """Operands of one slice conv: x / add maps of `slices` slices (the input slice xi of x, slice 0 of add), weights
    whose outputs leave [0, 20] on both sides, and the sentinel-filled destination of `slices` slices (slice oi)."""
    rng = np.random.default_rng(seed)
    ld = slices * width
    x = bf(rng.standard_normal((B, H, W, ld)))
    a = bf(rng.standard_normal((B, H, W, ld))) if add else None
    w = (rng.standard_normal((width, width, 3, 3)) * np.sqrt(2.0 / (9 * width))).astype(np.float32)
    if positive:
        w = np.abs(w)
    alpha = rng.uniform(3.0, 7.0, width).astype(np.float32)
    beta = (6.0 + 4.0 * rng.standard_normal(width)).astype(np.float32)
    assert w.dtype == alpha.dtype == beta.dtype == np.float32      # the op reads fp32 device arrays
    return dict(B=B, H=H, W=W, width=width, ld=ld, xi=xi, oi=oi, x=x, add=a, w=torch.from_numpy(w),
                alpha=torch.from_numpy(alpha), beta=torch.from_numpy(beta))


def res2_reference(c):
    """torch fp32 on the bf16-rounded operands: clamp(alpha conv(x [+ add]) + beta, 0, 20), NHWC."""
    wd = c["width"]
    s = c["x"][..., c["xi"] * wd:(c["xi"] + 1) * wd].float()
    if c["add"] is not None:
        s = (s + c["add"][..., :wd].float()).to(torch.bfloat16).float()      # the MFMA operand is bf16
    y = F.conv2d(s.permute(0, 3, 1, 2), c["w"].to(torch.bfloat16).float(), padding=1)
    y = y * c["alpha"].view(1, -1, 1, 1) + c["beta"].view(1, -1, 1, 1)
    return torch.clamp(y, 0.0, 20.0).permute(0, 2, 3, 1)


def res2_gpu(c, gpu):
    wd, ld = c["width"], c["ld"]
    x = c["x"].to(gpu).contiguous()
    a = c["add"].to(gpu).contiguous() if c["add"] is not None else None
    out = torch.full((c["B"], c["H"], c["W"], ld), SENTINEL, device=gpu, dtype=torch.bfloat16)
    dev = [c[k].to(gpu).contiguous() for k in ("w", "alpha", "beta")]
    _lib.call("sd_op_res2_conv3x3", _lib.ptr(x), c["B"], c["H"], c["W"], ld, c["xi"] * wd, wd, _lib.ptr(a), ld, 0,
              _lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(out), ld, c["oi"] * wd,
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return out.cpu().float()


def res2_check(c, gpu, tag):
    wd, oi = c["width"], c["oi"]
    want = res2_reference(c)
    full = res2_gpu(c, gpu)
    got = full[..., oi * wd:(oi + 1) * wd]
    rest = torch.cat((full[..., :oi * wd], full[..., (oi + 1) * wd:]), -1)
    assert (rest == SENTINEL).all(), "a channel outside the destination slice was written"
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    err = float((got[ok] - want[ok]).abs().max())
    lo, hi = float((want[ok] == 0).float().mean()), float((want[ok] == 20).float().mean())
    print(f"res2_conv3x3 {tag}: max abs err {err:.3e}; outputs at 0: {lo:.3f}, at 20: {hi:.3f}")
    assert lo > 0.01 and hi > 0.01, "the case must drive outputs below 0 and above 20"
    assert err <= BF16_ATOL["res2_conv3x3"]
    return got, want


@pytest.mark.parametrize("add", [False, True], ids=["plain", "sum"])
@pytest.mark.parametrize("width", WIDTHS)
def test_res2_conv_every_width(gpu, width, add):
    # 20 x 9: a 14-row tile and a 6-row one, the 9-pixel rows narrower than a 16-pixel tile row; slice 1 of 2
    res2_check(res2_case(2, 20, 9, width, 2, 1, 1, add, 100 + width + add), gpu, f"w{width} 20x9 {'sum' if add else 'plain'}")


@pytest.mark.parametrize("shape", [(2, 5, 3), (1, 10, 40), (1, 80, 1)], ids=["5x3", "10x40", "80x1"])
@pytest.mark.parametrize("width", [24, 52, 208])
def test_res2_conv_maps(gpu, width, shape):
    # 5 x 3: the smallest stage-4 map (15 pixels of a 128-pixel tile); 10 x 40: 2 x 3 tiles; 80 x 1: one-pixel rows
    B, H, W = shape
    res2_check(res2_case(B, H, W, width, 2, 0, 1, True, 200 + width + H), gpu, f"w{width} {H}x{W}")


def test_res2_conv_unaligned_slice(gpu):
    """Width 26 in an unpadded 3-slice map: the source at byte offset 52 of 156-byte pixels, the destination at 104."""
    c = res2_case(2, 20, 9, 26, 3, 1, 2, True, 301)
    assert (c["xi"] * 26 * 2) % 16 != 0 and (c["ld"] * 2) % 16 != 0
    res2_check(c, gpu, "w26 slice 1 -> 2 of 3")


@pytest.mark.parametrize("width", [24, 26])
def test_res2_conv_nan_and_inf(gpu, width):
    """One NaN and one +inf input element.  The NaN reaches every output channel of the 3 x 3 pixels around it and
    nothing else (Hardtanh keeps it); the +inf (positive weights) gives +inf, clamped to 20.  No other channel of the
    destination map changes."""
    c = res2_case(1, 20, 9, width, 2, 1, 0, False, 400 + width, positive=True)
    c["x"][0, 3, 4, width + 5] = float("nan")
    c["x"][0, 15, 2, width + 1] = float("inf")
    got, want = res2_check(c, gpu, f"w{width} nan/inf")
    nan = torch.isnan(got)
    assert nan[0, 2:5, 3:6].all() and int(nan.sum()) == 9 * width
    assert (got[0, 14:17, 1:4] == 20.0).all()


# ------------------------------------------------------------------------------------------------ aff_gate
def aff_case(P, C, seed, dtype, saturate=False, nan=False):
    rng = np.random.default_rng(seed)
    I = C // 4
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    x = torch.from_numpy((4.0 * np.abs(rng.standard_normal((P, C)))).astype(np.float32)).to(td)
    y = torch.from_numpy((4.0 * rng.standard_normal((P, C))).astype(np.float32)).to(td)
    if nan:
        x[P // 2, 3] = float("nan")
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))   # noqa: E731
    c = dict(P=P, C=C, I=I, x=x, y=y, dtype=dtype,
             w1=f32(rng.standard_normal((I, 2 * C)) * np.sqrt(1.0 / (2 * C)) * 0.3), a1=f32(rng.uniform(0.7, 1.3, I)),
             c1=f32(rng.standard_normal(I) * 0.2), w2=f32(rng.standard_normal((C, I)) * np.sqrt(1.0 / I)),
             a2=f32(rng.uniform(0.7, 1.3, C) * (400.0 if saturate else 1.0)), c2=f32(rng.standard_normal(C) * 0.2))
    return c


def aff_reference(c):
    """float64 on the values the kernel reads; also the worst-case fp32 error bound of every output element."""
    x, y = c["x"].float().numpy().astype(np.float64), c["y"].float().numpy().astype(np.float64)
    w1, a1, c1, w2, a2, c2 = (c[k].numpy().astype(np.float64) for k in ("w1", "a1", "c1", "w2", "a2", "c2"))
    xy = np.concatenate((x, y), 1)
    with np.errstate(all="ignore"):
        pre = (xy @ w1.T) * a1 + c1
        h = pre / (1.0 + np.exp(-pre))
        att = (h @ w2.T) * a2 + c2
        t = np.tanh(att)
        out = x * (1.0 + t) + y * (1.0 - t)
        # fp32 accumulation over K terms: |fl(sum) - sum| <= K u sum |terms| (K = 2 C, then I), plus the affine's two
        # operations; SiLU is 1.1-Lipschitz and tanh 1-Lipschitz, expf / tanhf / the division within 4 u each
        K1, K2 = 2 * c["C"], c["I"]
        d_pre = (K1 + 2) * U * ((np.abs(xy) @ np.abs(w1).T) * np.abs(a1) + np.abs(c1))
        d_h = 1.1 * d_pre + 4 * U * np.abs(h)
        d_att = (K2 + 2) * U * ((np.abs(h) @ np.abs(w2).T) * np.abs(a2) + np.abs(c2)) + (d_h @ np.abs(w2).T) * np.abs(a2)
        d_t = d_att + 4 * U
        bound = (np.abs(x) + np.abs(y)) * d_t + 4 * U * (np.abs(x) + np.abs(y)) * (1.0 + np.abs(t))
    return out, t, bound


def aff_gpu(c, gpu):
    dev = [c[k].to(gpu).contiguous() for k in ("x", "y", "w1", "a1", "c1", "w2", "a2", "c2")]
    out = torch.full_like(dev[0], SENTINEL)
    _lib.call("sd_op_aff_gate", _lib.ptr(dev[0]), _lib.ptr(dev[1]), int(c["dtype"] == "bf16"), c["P"], c["C"], c["I"],
              *[_lib.ptr(a) for a in dev[2:]], _lib.ptr(out), _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return out.cpu().float().numpy().astype(np.float64)


def aff_check(c, gpu, tag, kind="aff_gate"):
    want, t, bound = aff_reference(c)
    got = aff_gpu(c, gpu)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got - want)[ok]
    print(f"{kind} {tag} {c['dtype']}: max abs err {err.max():.3e}; tanh {np.nanmin(t):.3f} .. {np.nanmax(t):.3f}, "
          f"|tanh| > 0.999: {(np.abs(t[ok]) > 0.999).mean():.3f}; fp32 bound max {bound[ok].max():.3e}")
    if c["dtype"] == "fp32":
        assert (err <= bound[ok]).all(), float((err - bound[ok]).max())
    else:
        assert err.max() <= BF16_ATOL[kind]
    return got, t


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("P", [1, 63, 200])
@pytest.mark.parametrize("C", [24, 26, 104, 208])
def test_aff_gate_vs_float64(gpu, C, P, dtype):
    # 1 pixel, 63 (one short of a 64-pixel workgroup), 200 (four workgroups, the last one partial)
    got, t = aff_check(aff_case(P, C, 500 + C + P, dtype), gpu, f"C{C} P{P}")
    if P > 1:
        assert np.ptp(t) > 0.1


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [26, 208])
def test_aff_gate_saturated_tanh(gpu, C, dtype):
    """|att| of hundreds: tanh is +-1 to the last bit on most elements, so out is 2 x or 2 y exactly there."""
    c = aff_case(63, C, 600 + C, dtype, saturate=True)
    got, t = aff_check(c, gpu, f"C{C} saturated", "aff_gate_saturated")
    assert (np.abs(t) == 1.0).mean() > 0.5
    x, y = c["x"].float().numpy().astype(np.float64), c["y"].float().numpy().astype(np.float64)
    assert np.array_equal(got[t == 1.0], 2 * x[t == 1.0]) and np.array_equal(got[t == -1.0], 2 * y[t == -1.0])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_aff_gate_nan_stays_in_its_pixel(gpu, dtype):
    c = aff_case(63, 104, 700, dtype, nan=True)
    got, _ = aff_check(c, gpu, "C104 nan")
    nan = np.isnan(got)
    assert nan[63 // 2].all() and int(nan.sum()) == 104      # the gate mixes every channel of the pixel, and no other
