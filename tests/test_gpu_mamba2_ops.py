"""sd_op_mamba2_stack (the bidirectional Mamba2BlockV2 stage: RMSNorm, in_proj, causal conv, SSD scan, gated RMSNorm,
out_proj, residuals) on the MI355X against the fp64 CPU restatement (tests/mamba2_ref.py), without a trunk in front."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mamba2_ref as mr  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

# max|out - ref| / max|ref| measured on MI355X over mr.OP_CASES (the kernels are deterministic), the largest per
# precision; the bound is twice that.  fp32: exact-f32 MFMA GEMMs and an fp32 scan against fp64.  bf16x3: the GEMMs as
# bf16 hi + lo splits.  bf16: bf16 GEMM operands, zxbcdt / g / the output stored as bf16, the scan itself in fp32.
# The bf16 figure is the (E 64, d_state 16, 2 layers, L 65) case's; the next largest are 3.07e-2 and 2.02e-2 (two layers,
# L 64 / 65), every other case is under 1.3e-2: a few elements of a long two-layer scan whose decay sits at the knee of
# exp(dt A) move by percents when the GEMM operands and zxbcdt are rounded to bf16 (dt_raw itself stays fp32).
MEASURED = {"fp32": 2.135e-06, "bf16x3": 3.088e-05, "bf16": 5.307e-02}
BOUND = {p: 2 * v for p, v in MEASURED.items()}
assert BOUND["fp32"] <= 1e-4 and BOUND["bf16x3"] <= 1e-4   # an fp32 figure above 1e-4 is a bug to find, not a bound

_ref = {}


def reference(case):
    if case not in _ref:
        sd, x = mr.op_case(case)
        _ref[case] = mr.mamba2_block_v2(mr.to_double(sd), "", x.double())
    return _ref[case]


def run_op(sd, x, case, precision, gpu):
    E, expand, d_state, _, n_layer, _ = case
    R, L = x.shape[:2]
    w = mr.flat_weights(sd, n_layer).to(gpu)
    xd = x.to(gpu).contiguous()
    out = torch.empty(R, L, 2 * E, device=gpu, dtype=torch.float32)
    _lib.call("sd_op_mamba2_stack", _lib.ptr(xd), R, L, E, _lib.ptr(w), w.numel(), n_layer, d_state, expand,
              _lib.PRECISION[precision], _lib.ptr(out), _lib.stream_ptr(gpu))
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("case", mr.OP_CASES, ids=str)
def test_stack_vs_restatement(gpu, case, precision):
    sd, x = mr.op_case(case)
    want = reference(case)
    got = run_op(sd, x, case, precision, gpu).cpu().double()
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max() / want.abs().max())
    print(f"mamba2_stack {case} {precision}: max|diff| / max|ref| = {err:.3e} (max|ref| {float(want.abs().max()):.3f})")
    assert err < BOUND[precision]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_calls_bit_identical(gpu, precision):
    case = (64, 2, 128, 3, 2, 65)
    sd, x = mr.op_case(case)
    a = run_op(sd, x, case, precision, gpu)
    b = run_op(sd, x, case, precision, gpu)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sequences_are_independent(gpu, precision):
    """R = 3 equals rows 0-2 of the R = 6 call built by stacking three more sequences, bit for bit."""
    case = (64, 2, 128, 3, 2, 65)
    sd, x = mr.op_case(case)
    more = torch.cat([x, mr.stack_input(3, 65, 64, seed=77)])
    a = run_op(sd, x, case, precision, gpu)
    b = run_op(sd, more, case, precision, gpu)
    assert torch.equal(a.view(torch.int32), b[:3].view(torch.int32))


def test_argument_checks(gpu):
    case = (64, 2, 16, 3, 1, 5)
    sd, x = mr.op_case(case)
    w = mr.flat_weights(sd, 1).to(gpu)
    xd = x.to(gpu)
    out = torch.empty(3, 5, 128, device=gpu)

    def call(d_state=16, expand=2, n=None, E=64):
        _lib.call("sd_op_mamba2_stack", _lib.ptr(xd), 3, 5, E, _lib.ptr(w), w.numel() if n is None else n, 1, d_state,
                  expand, 0, _lib.ptr(out), _lib.stream_ptr(gpu))
    with pytest.raises(ValueError, match="d_state"):
        call(d_state=100)
    with pytest.raises(ValueError, match="expand"):
        call(expand=3, E=32)    # 3 * 32 = 96 is no multiple of the head dimension 64; refused before x is read
    with pytest.raises(ValueError, match="weights must hold"):
        call(n=w.numel() - 1)
    call()
