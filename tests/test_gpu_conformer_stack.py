"""A whole torchaudio Conformer (2 - 3 layers of D 384, ffn 512, 8 heads, depthwise kernel 31; GroupNorm or folded
BatchNorm) through sd_op_conformer_stack -- the product's loader (the 1/2 fold, the GLU row interleave, the BatchNorm fold,
the row-program packing), then run_conformer per layer (use_generic 1) or run_conformer_stack's row programs
(use_generic 0) -- against oracle/torchaudio_conformer.py's Conformer in float64.

fp32 (precision 0, generic): atol = rtol = 1e-3 on the LayerNorm'd output.  bf16 (precision 1), fused and generic alike
and never against each other: max |out - oracle| <= 4 e_w, with e_w = max |oracle(GEMM weights and input rounded to
bf16) - oracle(exact)| computed per case from the float64 oracle alone.  The margin covers the activation operands,
rounded at as many points again, and the five bf16 intermediates per layer; a layout or statistics bug gives errors on
the scale of the activations, O(1) after the final LayerNorm.

Every case asserts its launch path through the profiler scope names.  The pw1 GEMM takes the GLU epilogue from 2048
rows (gemm_stream_supported: M >= 16 tiles of 128) and the register-A GEMM, with the tiled A layout, from 16384 rows
(gemm_areg_supported: M >= 64 tiles of 256): (8, 150) is below both (the depthwise conv applies the GLU on load),
(32, 150) has the GLU epilogue on gemm_stream, (112, 150) has it on gemm_areg with a_tiled.

Largest max |out - oracle| / e_w observed on an MI355X (every case prints its own; e_w is 0.018 - 0.025): fused 1.42
((4, 150), GroupNorm), generic bf16 1.55 ((4, 150) x 3 layers, GroupNorm), speaker streams 1.63 (GroupNorm; its output
is rounded to bf16 once more); fp32 generic: max |out - oracle| <= 3.8e-6."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conformer_ref as cr  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

D, FFN, NH, K = cr.D, 512, 8, 31


@functools.lru_cache(maxsize=None)
def _model(n_layers, group_norm):
    return cr.make_conformer(n_layers, FFN, NH, K, group_norm, seed=100 + 10 * n_layers + group_norm)


@functools.lru_cache(maxsize=2)
def _case(S, T, lens, n_layers, group_norm, spk=0):
    """(x, key_len, oracle output, e_w[, ts, mix]) of a case, shared by the runs that use it."""
    g = torch.Generator().manual_seed(S * 1000 + T + n_layers)
    m = _model(n_layers, group_norm)
    ts = mix = None
    if spk:
        NS, Tmix, ld = spk, T - 1, 200
        ts = torch.randn(S, D // 2, generator=g)
        mix = torch.randn(S // NS, Tmix, ld, generator=g)
        x = cr.speaker_rows(ts, mix[:, :, :D // 2], NS, T).reshape(S, T, D)
    else:
        x = torch.randn(S, T, D, generator=g)
    key_len = torch.randint(max(1, T // 3), T + 1, (S,), generator=g, dtype=torch.int32) if lens else None
    ref = cr.conformer_forward(m, x.double(), key_len)
    e_w = (cr.conformer_forward(cr.conformer_bf16_weights(m), cr.bf16r(x), key_len) - ref).abs().max().item()
    return x, key_len, ref, e_w, ts, mix


def _run(gpu, S, T, n_layers, group_norm, x, key_len, precision, use_generic, ts=None, mix=None, NS=0):
    w = cr.conformer_blob(_model(n_layers, group_norm).state_dict(), n_layers, group_norm).to(gpu)
    kl = key_len.to(gpu) if key_len is not None else None
    if ts is None:
        xd, tsd, mixd = x.contiguous().to(gpu), None, None
        out = torch.full((S * T + 64, D), float("nan"), device=gpu)
    else:
        xd, tsd, mixd = None, ts.contiguous().to(gpu), mix.contiguous().to(gpu)
        out = torch.full((S * T + 64, D), float("nan"), dtype=torch.bfloat16, device=gpu)
    with cr.profiled() as launches:
        _lib.call("sd_op_conformer_stack", _lib.ptr(xd), S, T, _lib.ptr(w), w.numel(), n_layers, FFN, NH, K,
                  int(group_norm), _lib.ptr(kl), precision, use_generic, _lib.ptr(tsd), _lib.ptr(mixd),
                  mix.shape[2] if mix is not None else 0, mix.shape[1] if mix is not None else 0, NS, _lib.ptr(out),
                  _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
    assert torch.isnan(out[S * T:].float()).all(), "rows past the output written"
    return out[:S * T].cpu(), launches


def _assert_fused_path(launches, n_layers, S, T, group_norm):
    """run_conformer_stack's launches: one FFN program, then per layer attention, the out-projection program, the pw1
    GEMM, the depthwise conv and the pw2 + FFN program; no stand-alone LayerNorm or GroupNorm pass."""
    rows = S * T
    assert launches.get("rowprog_ffn") == 1 and launches.get("rowprog_out") == n_layers
    assert launches.get("rowprog_pw2_ffn") == n_layers
    for absent in ("layernorm", "add_layernorm", "groupnorm_silu"):
        assert absent not in launches, launches
    if T <= 160:
        assert launches.get("mha_block") == n_layers and "attention_bf16" not in launches
    else:
        assert launches.get("attention_bf16") == n_layers and "mha_block" not in launches
    glu_epilogue = rows >= 2048
    assert launches.get("dwconv" if glu_epilogue else "glu_dwconv") == n_layers, launches
    assert ("glu_dwconv" if glu_epilogue else "dwconv") not in launches, launches
    if rows >= 16384:
        assert launches.get("gemm_areg") == n_layers and "gemm_stream" not in launches, launches
    elif glu_epilogue:
        assert launches.get("gemm_stream") == n_layers and "gemm_areg" not in launches, launches
    else:
        assert "gemm_stream" not in launches and "gemm_areg" not in launches, launches


def _assert_generic_path(launches, n_layers, group_norm):
    assert not any(k.startswith("rowprog") for k in launches), launches
    assert launches.get("layernorm") == n_layers and launches.get("add_layernorm") == 4 * n_layers, launches
    assert launches.get("groupnorm_silu", 0) == (n_layers if group_norm else 0), launches


@pytest.mark.parametrize("group_norm", [True, False], ids=["groupnorm", "batchnorm"])
@pytest.mark.parametrize("S,T", [(3, 37), (2, 161)])
def test_stack_fp32_generic(gpu, S, T, group_norm):
    """Pins the loader, the 1/2 fold, the GLU interleave and the BatchNorm fold in exact arithmetic."""
    x, key_len, ref, _, _, _ = _case(S, T, True, 2, group_norm)
    out, launches = _run(gpu, S, T, 2, group_norm, x, key_len, 0, 1)
    _assert_generic_path(launches, 2, group_norm)
    err = (out.double().reshape(S, T, D) - ref).abs().max().item()
    print(f"fp32 generic ({S}, {T}) group_norm {group_norm}: max |out - oracle| = {err:.3e}")
    torch.testing.assert_close(out.double().reshape(S, T, D), ref, atol=1e-3, rtol=1e-3)


# (S, T, key_len, layers): rows % 16 != 0 (every layout row-major) | tiled, below the GEMM thresholds | tiled, the GLU
# epilogue on gemm_stream | mha_block unsupported (T > 160): the attention() fallback | key_len | the middle program
# (pre + 2 FFNs + y) between two others | the GLU epilogue on gemm_areg with the tiled A
BF16_CASES = [(4, 150, False, 2), (8, 150, False, 2), (32, 150, False, 2), (2, 161, False, 2), (6, 37, True, 2),
              (4, 150, False, 3), (112, 150, False, 2)]


# the largest case runs with GroupNorm only (the CPU oracle is its cost)
BF16_PARAMS = [c + (gn,) for c in BF16_CASES for gn in (True, False) if gn or c[0] < 100]


@pytest.mark.parametrize("use_generic", [0, 1], ids=["fused", "generic"])
@pytest.mark.parametrize("S,T,lens,n_layers,group_norm", BF16_PARAMS,
                         ids=["S%d-T%d-%s-L%d-%s" % (s, t, "lens" if le else "whole", nl, "groupnorm" if gn else "batchnorm")
                              for s, t, le, nl, gn in BF16_PARAMS])
def test_stack_bf16(gpu, S, T, lens, n_layers, group_norm, use_generic):
    x, key_len, ref, e_w, _, _ = _case(S, T, lens, n_layers, group_norm)
    out, launches = _run(gpu, S, T, n_layers, group_norm, x, key_len, 1, use_generic)
    if use_generic:
        _assert_generic_path(launches, n_layers, group_norm)
    else:
        _assert_fused_path(launches, n_layers, S, T, group_norm)
    err = (out.double().reshape(S, T, D) - ref).abs().max().item()
    print(f"bf16 {'generic' if use_generic else 'fused'} ({S}, {T}) x {n_layers} group_norm {group_norm}: "
          f"e_w = {e_w:.3e}, max |out - oracle| / e_w = {err / e_w:.3f}")
    assert err <= 4 * e_w


@pytest.mark.parametrize("group_norm", [True, False], ids=["groupnorm", "batchnorm"])
def test_stack_speaker_streams(gpu, group_norm):
    """The first program builds its rows from ts / mix (the last mix frame reads as zero), the last writes bf16 rows in
    the speakers-to-channels layout."""
    B, NS, T = 2, 4, 150
    S = B * NS
    x, _, ref, e_w, ts, mix = _case(S, T, False, 2, group_norm, spk=NS)
    out, launches = _run(gpu, S, T, 2, group_norm, x, None, 1, 0, ts=ts, mix=mix, NS=NS)
    _assert_fused_path(launches, 2, S, T, group_norm)
    want = cr.speakers_to_channels(ref.reshape(S * T, D), NS, T).reshape(S * T, D)
    err = (out.double() - want).abs().max().item()
    print(f"speaker streams group_norm {group_norm}: e_w = {e_w:.3e}, max |out - oracle| / e_w = {err / e_w:.3f}")
    assert err <= 4 * e_w
