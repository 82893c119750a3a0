"""The ECAPA-TDNN test ops on the MI355X path: the Res2 chain (sd_op_res2_chain) against a torch fp32 computation on
the same inputs, and attentive statistics pooling (sd_op_astp_pool) against a float64 numpy ASTP."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from speaker_diarization_amd import _lib

pytestmark = pytest.mark.gpu

G, NS, C = 128, 7, 1024
# (B, T): one frame, shorter than one dilated receptive field, an odd length over two windows, and a length that is
# four 64-frame tiles of the fused kernel plus a 45-frame remainder (and several 64- / 128-row GEMM tiles with window
# boundaries inside them)
SHAPES = [(1, 1), (1, 6), (2, 37), (2, 301)]


def chain_weights(seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((NS, G, G, 3)) * np.sqrt(2.0 / (3 * G))).astype(np.float32)
    bias = (rng.standard_normal((NS, G)) * 0.05).astype(np.float32)
    s = rng.uniform(0.7, 1.3, (NS, G)).astype(np.float32)
    h = (rng.standard_normal((NS, G)) * 0.1 - 0.3).astype(np.float32)
    return w, bias, s, h


def chain_ref(x, w, bias, s, h, dil):
    """x (B, T, 1024) fp32 channel-last -> the chain's output, fp32 on the CPU."""
    xt = x.permute(0, 2, 1)
    groups = torch.split(xt, G, 1)
    out, sp = [], None
    for i in range(NS):
        sp = groups[i] if i == 0 else sp + groups[i]
        sp = F.relu(F.conv1d(sp, torch.from_numpy(w[i]), torch.from_numpy(bias[i]), padding=dil, dilation=dil))
        sp = sp * torch.from_numpy(s[i])[None, :, None] + torch.from_numpy(h[i])[None, :, None]
        out.append(sp)
    out.append(groups[NS])
    return torch.cat(out, 1).permute(0, 2, 1).contiguous()


def run_chain(gpu, x, w, bias, s, h, dil, precision, use_generic=1):
    B, T, _ = x.shape
    dt = torch.bfloat16 if precision == 1 else torch.float32
    xd = x.to(gpu, dt).contiguous()
    out = torch.full((B, T, C), float("nan"), device=gpu, dtype=dt)
    wd, bd, sd, hd = (torch.from_numpy(a).to(gpu).contiguous() for a in (w, bias, s, h))
    _lib.call("sd_op_res2_chain", _lib.ptr(xd), B, T, dil, _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(sd), _lib.ptr(hd),
              _lib.ptr(out), use_generic, precision, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dil", [2, 3, 4])
@pytest.mark.parametrize("B,T", SHAPES)
def test_res2_chain_bf16(gpu, B, T, dil):
    """bf16 maps and weights, both arms, against torch fp32 on the same bf16-rounded inputs.  The generic arm (seven
    conv_gemm launches) is the yardstick: every stage output is rounded to bf16 once (2^-9 relative) and so is every
    stage input sp + split (2^-9); the He-scaled stage convs pass an error on at about unit gain, so seven stages
    accumulate at most 7 * 2 * 2^-9 of the largest activation.  The fused arm may err at most twice the generic arm's
    measured error (a different summation order)."""
    rng = np.random.default_rng(100 * T + dil)
    w, bias, s, h = chain_weights(T + dil)
    x = torch.from_numpy(np.abs(rng.standard_normal((B, T, C))).astype(np.float32)).bfloat16().float()
    wr = torch.from_numpy(w).bfloat16().float().numpy()
    want = chain_ref(x, wr, bias, s, h, dil)
    errs = {}
    for arm, use_generic in (("generic", 1), ("fused", 0)):
        got = run_chain(gpu, x, w, bias, s, h, dil, 1, use_generic)
        errs[arm] = float((got.float().cpu() - want).abs().max())
        assert torch.equal(got[..., NS * G:].cpu(), x[..., NS * G:].bfloat16()), arm     # group 7 passes through
        if B == 2:
            alone = run_chain(gpu, x[1:], w, bias, s, h, dil, 1, use_generic)
            assert torch.equal(alone[0].view(torch.int16), got[1].view(torch.int16)), arm   # no neighbour's frames
    bound = 14 * 2.0 ** -9 * float(want.abs().max())
    print(f"res2_chain bf16 B={B} T={T} dil={dil}: max err generic {errs['generic']:.3e} fused {errs['fused']:.3e} "
          f"(generic bound {bound:.3e}, max |y| {float(want.abs().max()):.2f})")
    assert errs["generic"] < bound
    assert errs["fused"] <= 2 * errs["generic"]


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("B,T,dil", [(1, 1, 2), (1, 6, 4), (2, 37, 3), (2, 301, 2)])
def test_res2_chain_fp32(gpu, B, T, dil, precision):
    rng = np.random.default_rng(7 * T + dil)
    w, bias, s, h = chain_weights(3 * T + dil)
    x = torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32))
    want = chain_ref(x, w, bias, s, h, dil)
    got = run_chain(gpu, x, w, bias, s, h, dil, precision).cpu()
    err = float((got - want).abs().max())
    # per stage: a 384-term fp32 dot product (sqrt(384) * 2^-24 ~ 2^-20 of its magnitude), or bf16x3's 2^-16 per
    # product (kernels.h); seven stages at about unit gain, relative to the largest activation
    bound = 7 * (2.0 ** -16 if precision == 2 else 2.0 ** -20) * float(want.abs().max())
    print(f"res2_chain precision {precision} B={B} T={T} dil={dil}: max err {err:.3e} (bound {bound:.3e})")
    assert err < bound
    assert torch.equal(got[..., NS * G:], x[..., NS * G:])


def test_res2_chain_fused_arm_is_bf16_only(gpu):
    w, bias, s, h = chain_weights(1)
    for precision in (0, 2):
        with pytest.raises(ValueError, match="the fused kernel is bf16"):
            run_chain(gpu, torch.zeros(1, 4, C), w, bias, s, h, 2, precision, use_generic=0)
    with pytest.raises(ValueError, match="dilation 1..4"):
        run_chain(gpu, torch.zeros(1, 4, C), w, bias, s, h, 5, 1, use_generic=0)


# ---------------------------------------------------------------- ASTP
CA, H = 1536, 128


def astp_weights(seed):
    rng = np.random.default_rng(seed)
    w1 = (rng.standard_normal((H, 3 * CA)) * np.sqrt(2.0 / (3 * CA))).astype(np.float32)
    b1 = (rng.standard_normal(H) * 0.05).astype(np.float32)
    w2 = (rng.standard_normal((CA, H)) * 2.0 * np.sqrt(2.0 / H)).astype(np.float32)
    b2 = (rng.standard_normal(CA) * 0.05).astype(np.float32)
    return w1, b1, w2, b2


def astp_ref(x, w1, b1, w2, b2):
    """float64 numpy ASTP with the global context: x (B, T, C) -> (B, 2 C)."""
    x = x.astype(np.float64)
    T = x.shape[1]
    mean = x.mean(1, keepdims=True)
    std = np.sqrt(x.var(1, ddof=1, keepdims=True) + 1e-7)
    xin = np.concatenate([x, np.broadcast_to(mean, x.shape), np.broadcast_to(std, x.shape)], 2)
    a = np.tanh(xin @ w1.astype(np.float64).T + b1)
    e = a @ w2.astype(np.float64).T + b2
    e = np.exp(e - e.max(1, keepdims=True))
    al = e / e.sum(1, keepdims=True)
    m = (al * x).sum(1)
    var = (al * x * x).sum(1) - m * m
    return np.concatenate([m, np.sqrt(np.maximum(var, 1e-7))], 1), al


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("B,T", [(1, 2), (3, 37), (2, 598)])
def test_astp_pool(gpu, B, T, bf16):
    rng = np.random.default_rng(T)
    w1, b1, w2, b2 = astp_weights(T + 1)
    x = np.maximum(rng.standard_normal((B, T, CA)), 0.0).astype(np.float32)     # a ReLU output, like the trunk's
    x[:, :, 5] = 0.75       # constant over time: both stds are exactly sqrt(1e-7)
    x[:, :, 6] = 0.0
    xt = torch.from_numpy(x)
    if bf16:
        xt = xt.bfloat16()
        x = xt.float().numpy()
    want, al = astp_ref(x, w1, b1, w2, b2)
    xd = xt.to(gpu).contiguous()
    stats = torch.full((B, 2 * CA), float("nan"), device=gpu)
    wd = [torch.from_numpy(a).to(gpu).contiguous() for a in (w1, b1, w2, b2)]
    _lib.call("sd_op_astp_pool", _lib.ptr(xd), int(bf16), B, T, *[_lib.ptr(a) for a in wd], _lib.ptr(stats),
              _lib.stream_ptr(gpu))
    got = stats.cpu().numpy().astype(np.float64)
    err = np.abs(got - want).max()
    print(f"astp B={B} T={T} bf16={bf16}: max err {err:.3e}; largest weight {al.max():.3f} (uniform {1.0 / T:.4f})")
    assert err < 1e-4
    assert (got[:, [CA + 5, CA + 6]] == np.float64(np.float32(np.sqrt(1e-7)))).all()
    assert np.abs(got[:, 5] - 0.75).max() < 1e-6


def test_astp_pool_refuses_one_frame(gpu):
    w = [torch.from_numpy(a).to(gpu).contiguous() for a in astp_weights(0)]
    x = torch.zeros(1, 1, CA, device=gpu)
    stats = torch.zeros(1, 2 * CA, device=gpu)
    with pytest.raises(AssertionError, match="at least 2 frames"):
        _lib.call("sd_op_astp_pool", _lib.ptr(x), 0, 1, 1, *[_lib.ptr(a) for a in w], _lib.ptr(stats),
                  _lib.stream_ptr(gpu))
