"""The conformer stack at the geometry of TS-VAD's conformer back ends -- D 384, 4 heads of 96, FFN 1536, depthwise kernel
31, eval BatchNorm1d folded into the depthwise conv, 2 layers -- through sd_op_conformer_stack, against
oracle.tsvad_ref.conformer(group_norm=False) in float64.

mha_block is 8 heads of 48 only, so at 4 heads the fused stack (use_generic 0) runs the in-projection GEMM + attention()
between its row programs, with the programs' tiled layouts off for the attention operands; the row programs run at
hidden 1536.  T covers 1, the 15-frame halo of the depthwise conv (15, 16, 31), the 16-token tile (15, 16), and the
rs_len 4 / 8 label lengths 100 and 200; S = 3 makes S * T no multiple of 16 for odd T (every layout row-major),
(4, 100) is the tiled case.

A. fp32 and bf16x3 (use_generic 1): max |out - ref| <= 1e-4 max |ref| (measured: fp32 <= 7.5e-7, bf16x3 <= 7.8e-6).
B. bf16, use_generic 1 (run_conformer per layer: existing code) and 0 (the fused stack), each against float64, as
   max |out - ref| / max |ref|.  The fused path's bound is twice the largest figure MEASURED on the generic path over the
   cases (on an MI355X; the kernels are deterministic): the fused path keeps its residual stream in fp32 registers and
   rounds at fewer points, so it may not be worse than that.  The generic path is held to the same bound.
C. use_generic 0 launches rowprog_* and attention_bf16, never mha_block, and two calls agree bit for bit."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conformer_ref as cr  # noqa: E402
from oracle import tsvad_ref as tr  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

D, FFN, NH, K, LAYERS = cr.D, 1536, 4, 31, 2
CASES = [(3, 1), (3, 15), (3, 16), (3, 31), (3, 100), (3, 200), (4, 100)]
IDS = ["S%d-T%d" % c for c in CASES]
EXACT_RTOL = 1e-4
# max |out - ref| / max |ref| of the generic bf16 path (precision 1, use_generic 1) per case, measured on an MI355X
MEASURED = {(3, 1): 4.377e-3, (3, 15): 3.325e-3, (3, 16): 3.897e-3, (3, 31): 4.230e-3, (3, 100): 3.383e-3,
            (3, 200): 2.914e-3, (4, 100): 3.271e-3}
# the fused path on the same cases, for the record (not part of any bound)
MEASURED_FUSED = {(3, 1): 3.368e-3, (3, 15): 3.462e-3, (3, 16): 3.755e-3, (3, 31): 3.096e-3, (3, 100): 3.333e-3,
                  (3, 200): 2.627e-3, (4, 100): 2.810e-3}
BF16_RTOL = 2 * max(MEASURED.values())   # 8.75e-3
assert set(MEASURED) == set(CASES)


@functools.lru_cache(maxsize=None)
def _model():
    return cr.make_conformer(LAYERS, FFN, NH, K, False, seed=4096)


@functools.lru_cache(maxsize=None)
def _case(S, T):
    """(x, float64 reference) of a case, computed once and shared."""
    x = torch.randn(S, T, D, generator=torch.Generator().manual_seed(100 * S + T))
    sd = {k: v.detach() for k, v in _model().state_dict().items()}
    with torch.no_grad():
        ref = tr.conformer(x.double(), torch.full((S,), T), sd, "", num_layers=LAYERS, nh=NH, group_norm=False)
    return x, ref


def _run(gpu, S, T, precision, use_generic):
    x, _ = _case(S, T)
    w = cr.conformer_blob(_model().state_dict(), LAYERS, False).to(gpu)
    out = torch.full((S * T + 64, D), float("nan"), device=gpu)
    xd = x.contiguous().to(gpu)
    with cr.profiled() as launches:
        _lib.call("sd_op_conformer_stack", _lib.ptr(xd), S, T, _lib.ptr(w), w.numel(), LAYERS, FFN,
                  NH, K, 0, None, precision, use_generic, None, None, 0, 0, 0, _lib.ptr(out), _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
    assert torch.isnan(out[S * T:]).all(), "rows past the output written"
    return out[:S * T].cpu().reshape(S, T, D), launches


def _rel_err(out, ref):
    return ((out.double() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("precision", [0, 2], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("S,T", CASES, ids=IDS)
def test_exact_precisions(gpu, S, T, precision):
    _, ref = _case(S, T)
    out, launches = _run(gpu, S, T, precision, 1)
    assert not any(k.startswith("rowprog") or k == "mha_block" for k in launches), launches
    err = _rel_err(out, ref)
    print(f"precision {precision} ({S}, {T}): max |out - ref| / max |ref| = {err:.3e} (max |ref| {ref.abs().max():.3f})")
    assert err <= EXACT_RTOL


@pytest.mark.parametrize("use_generic", [1, 0], ids=["generic", "fused"])
@pytest.mark.parametrize("S,T", CASES, ids=IDS)
def test_bf16(gpu, S, T, use_generic):
    _, ref = _case(S, T)
    out, _ = _run(gpu, S, T, 1, use_generic)
    err = _rel_err(out, ref)
    print(f"bf16 {'generic' if use_generic else 'fused'} ({S}, {T}): max |out - ref| / max |ref| = {err:.3e}")
    assert torch.isfinite(out).all()
    assert err <= BF16_RTOL


@pytest.mark.parametrize("S,T", CASES, ids=IDS)
def test_fused_path_and_repeatability(gpu, S, T):
    a, launches = _run(gpu, S, T, 1, 0)
    assert launches.get("rowprog_ffn") == 1 and launches.get("rowprog_out") == LAYERS, launches
    assert launches.get("rowprog_pw2_ffn") == LAYERS, launches
    assert "mha_block" not in launches and launches.get("attention_bf16") == LAYERS, launches
    for absent in ("layernorm", "add_layernorm", "groupnorm_silu"):
        assert absent not in launches, launches
    b, _ = _run(gpu, S, T, 1, 0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
