"""res_conv.hip (the ResNet34 trunk's 3x3 convs, bf16 NHWC) through sd_op_res_conv: against F.conv2d on the CPU, against
the generic conv_gemm on the same arguments, NaN / Inf propagation through the ReLU, and run-to-run bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from speaker_diarization_amd import _lib

pytestmark = pytest.mark.gpu

# (B, H, W, Cin, Cout, stride, residual, shortcut)
CASES = [
    (2, 6, 37, 32, 32, 1, True, False),
    (2, 6, 37, 32, 64, 2, False, True),
    (1, 5, 19, 64, 64, 1, True, False),
    (2, 4, 5, 128, 256, 2, False, True),
    (3, 3, 3, 256, 256, 1, True, False),
    (1, 1, 1, 64, 64, 1, False, False),
    (1, 10, 130, 32, 32, 1, True, False),   # crosses a tile edge in W
]
IDS = ["%dx%dx%d_%dto%d_s%d%s%s" % (c[0], c[1], c[2], c[3], c[4], c[5], "_res" if c[6] else "", "_sc" if c[7] else "")
       for c in CASES]


def bf(t):
    return t.to(torch.bfloat16)


def make(case, seed=0):
    B, H, W, Cin, Cout, s, res, sc = case
    g = torch.Generator().manual_seed(1000 + seed + 7 * Cin + Cout + H * W)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    d = dict(x=bf(torch.randn(B, H, W, Cin, generator=g)),
             w=bf(torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).float(),
             alpha=torch.rand(Cout, generator=g) + 0.5, beta=torch.randn(Cout, generator=g) * 0.1,
             res=bf(torch.randn(B, Ho, Wo, Cout, generator=g)) if res else None, Ho=Ho, Wo=Wo)
    if sc:
        d.update(sc_w=bf(torch.randn(Cout, Cin, 1, 1, generator=g) * (1.0 / Cin) ** 0.5).float(),
                 sc_alpha=torch.rand(Cout, generator=g) + 0.5, sc_beta=torch.randn(Cout, generator=g) * 0.1)
    return d


def reference(case, d):
    """fp32 on the CPU with the same epilogue, bf16-rounded: (out, sc_out or None), NHWC floats."""
    s = case[5]
    x = d["x"].float().permute(0, 3, 1, 2)
    y = F.conv2d(x, d["w"], stride=s, padding=1) * d["alpha"][None, :, None, None] + d["beta"][None, :, None, None]
    if d["res"] is not None:
        y = y + d["res"].float().permute(0, 3, 1, 2)
    out = bf(torch.relu(y)).float().permute(0, 2, 3, 1)
    sc = None
    if "sc_w" in d:
        z = F.conv2d(x, d["sc_w"], stride=s) * d["sc_alpha"][None, :, None, None] + d["sc_beta"][None, :, None, None]
        sc = bf(z).float().permute(0, 2, 3, 1)
    return out, sc


def run(case, d, dev, generic):
    B, H, W, Cin, Cout, s, _, _ = case
    t = {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in d.items()}
    out = torch.zeros(B, d["Ho"], d["Wo"], Cout, dtype=torch.bfloat16, device=dev)
    sc_out = torch.zeros_like(out) if "sc_w" in d else None
    p = _lib.ptr
    _lib.call("sd_op_res_conv", p(t["x"]), B, H, W, Cin, p(t["w"]), Cout, s, p(t["alpha"]), p(t["beta"]), p(t["res"]),
              p(t.get("sc_w")), p(t.get("sc_alpha")), p(t.get("sc_beta")), p(out), p(sc_out), int(generic),
              _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return out.cpu(), (sc_out.cpu() if sc_out is not None else None)


def one_ulp_apart(a, b):
    """bf16 tensors at most one bf16 ulp apart: rtol 2^-7 on the decoded values, atol one ulp at the output's max."""
    a, b = a.float(), b.float()
    top = float(max(a.abs().max(), b.abs().max(), 1e-30))
    atol = 2.0 ** (np.floor(np.log2(top)) - 7)
    return bool((torch.abs(a - b) <= atol + 2.0 ** -7 * torch.minimum(a.abs(), b.abs())).all())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_res_conv_vs_cpu_and_generic(gpu, case):
    d = make(case)
    ref, ref_sc = reference(case, d)
    got, got_sc = run(case, d, gpu, generic=0)
    gen, gen_sc = run(case, d, gpu, generic=1)
    print(IDS[CASES.index(case)], "max|kernel - cpu| %.3e  max|generic - cpu| %.3e  max|kernel - generic| %.3e" % (
        (got.float() - ref).abs().max(), (gen.float() - ref).abs().max(), (got.float() - gen.float()).abs().max()))
    assert torch.allclose(got.float(), ref, atol=2e-2, rtol=1e-2)
    assert one_ulp_apart(got, gen)
    if ref_sc is not None:
        assert torch.allclose(got_sc.float(), ref_sc, atol=2e-2, rtol=1e-2)
        assert one_ulp_apart(got_sc, gen_sc)
    again, again_sc = run(case, d, gpu, generic=0)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16))
    if got_sc is not None:
        assert torch.equal(got_sc.view(torch.int16), again_sc.view(torch.int16))


def covered(h, w, Ho, Wo, s):
    """Output pixels whose 3x3 pad-1 window at stride s covers input pixel (h, w)."""
    return {(ho, wo) for ho in range(Ho) for wo in range(Wo) if abs(ho * s - h) <= 1 and abs(wo * s - w) <= 1}


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]], ids=[IDS[0], IDS[1], IDS[3]])
def test_res_conv_keeps_nan_and_inf(gpu, case):
    """torch.relu keeps NaN: a NaN input value makes every channel of exactly the covering output pixels NaN, a
    +Inf makes them +Inf or (negative weight, then ReLU) 0 exactly as in the fp32 CPU reference, and every other
    output value stays finite.  The shortcut output sees only the pixel it samples."""
    B, H, W, Cin, Cout, s, _, _ = case
    d = make(case, seed=3)
    nan_at, inf_at = (0, 2, 4, 5), (B - 1, H - 1, W - 2, 9)   # (b, h, w, c): different images
    d["x"][nan_at] = float("nan")
    d["x"][inf_at] = float("inf")
    ref, ref_sc = reference(case, d)
    got, got_sc = run(case, d, gpu, generic=0)
    Ho, Wo = d["Ho"], d["Wo"]
    nan_px = covered(nan_at[1], nan_at[2], Ho, Wo, s)
    inf_px = covered(inf_at[1], inf_at[2], Ho, Wo, s)
    assert nan_px and inf_px
    g = got.float()
    for b in range(B):
        for ho in range(Ho):
            for wo in range(Wo):
                v = g[b, ho, wo]
                if b == nan_at[0] and (ho, wo) in nan_px:
                    assert torch.isnan(v).all(), (b, ho, wo)
                elif b == inf_at[0] and (ho, wo) in inf_px:
                    assert not torch.isnan(v).any() and torch.equal(torch.isinf(v), torch.isinf(ref[b, ho, wo]))
                    assert torch.isinf(v).any(), (b, ho, wo)
                    assert (v[torch.isinf(v)] > 0).all()
                else:
                    assert torch.isfinite(v).all(), (b, ho, wo)
    assert torch.equal(torch.isnan(g), torch.isnan(ref)) and torch.equal(torch.isinf(g), torch.isinf(ref))
    if got_sc is not None:
        gs = got_sc.float()
        assert torch.equal(torch.isnan(gs), torch.isnan(ref_sc)) and torch.equal(torch.isinf(gs), torch.isinf(ref_sc))
        hit = nan_at[1] % s == 0 and nan_at[2] % s == 0
        assert bool(torch.isnan(gs[nan_at[0], nan_at[1] // s, nan_at[2] // s]).all()) == hit
        assert int(torch.isnan(gs).any(-1).sum()) == (1 if hit else 0)


def test_res_conv_rejects_what_it_cannot_compute(gpu):
    x = torch.zeros(1, 4, 4, 48, dtype=torch.bfloat16, device=gpu)
    w = torch.zeros(48, 48, 3, 3, device=gpu)
    out = torch.zeros(1, 4, 4, 48, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError, match="res_conv"):
        _lib.call("sd_op_res_conv", _lib.ptr(x), 1, 4, 4, 48, _lib.ptr(w), 48, 1, None, None, None, None, None, None,
                  _lib.ptr(out), None, 0, _lib.stream_ptr(gpu))
