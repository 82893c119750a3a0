"""The conformer conv module's kernels (ops.hip glu_dwconv: the fp32 kernel, the bf16 generic kernel, the bf16 packed
kernels dwconv_pp / dwconv_pk in their three run lengths; groupnorm_silu) through sd_op_glu_dwconv against a plain
float64 restatement (tests/conformer_ref.py conv_module_ref: F.glu, F.conv1d(groups=C), F.group_norm(1 group), F.silu),
at the shapes where each dispatch rule of glu_dwconv() and each tail begins.

Which kernel a case reaches follows from its shape alone (glu_dwconv() in ops.hip); the case lists say which one that
is.  The profiler scope tells the GLU-on-load launch ("glu_dwconv") from the plain one ("dwconv") and counts the
groupnorm_silu launches; every case asserts those.

Every S > 1 case scales its sequences by 1, 3, 0.3, ... so a halo row or a partial sum taken from the neighbouring
sequence shows; the bias has a non-zero mean so the E[y^2] - E[y]^2 form of the GroupNorm statistics has something to
cancel; outputs carry 64 guard rows of NaN.  The mode-1 partial sums are held to conformer_ref.conv_partial_bound, the
worst case of the fp32 arithmetic derived from the number formats (observed on an MI355X: at most 0.061 of it)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conformer_ref as cr  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

FP32_TOL = dict(atol=1e-4, rtol=1e-4)      # tests/test_gpu_ops.py
BF16_TOL = dict(atol=2e-2, rtol=1e-2)      # against the bf16-rounded reference (test_gemm_bf16, test_add_layernorm)
GUARD = 64

# (S, T, C, k, glu_in, io_bf16), grouped by the kernel glu_dwconv() picks
FP32 = [(S, T, C, k, g, 0) for (S, T, C, k) in
        [(1, 1, 384, 31), (3, 7, 384, 31),      # T < pad
         (2, 64, 384, 31), (2, 65, 384, 15),    # the 64-row time tile and one row past it
         (2, 150, 384, 31),
         (2, 70, 48, 7),                        # C % 64 != 0
         (2, 33, 80, 1)]
        for g in (0, 1)]                        # glu_dwconv_kernel<false>: time tile 64, runs of 8 rows
BF16_GENERIC = [(S, T, C, k, g, 1) for (S, T, C, k) in
                [(2, 160, 384, 7), (2, 161, 384, 7),   # k not in {15, 31}; the 160-row tile and one row past it
                 (2, 170, 48, 31), (3, 9, 80, 15)]     # C % 64 != 0
                for g in (0, 1)]                       # glu_dwconv_kernel<true>: time tile 160
# dwconv_pp (glu_in 0, k in {15, 31}, C % 64 == 0, T <= 152), run length 9 for T <= 72, 13 for T <= 104, else 19
BF16_PP = ([(2, T, 384, k, 0, 1) for k in (15, 31) for T in (1, 14, 72, 73, 104, 105, 152)]
           + [(2, 73, 64, 31, 0, 1), (2, 152, 64, 31, 0, 1), (3, 14, 64, 15, 0, 1), (2, 105, 64, 15, 0, 1)]
           # at most resident / 6 <= 341 workgroups per channel block: every workgroup walks more than one sequence
           + [(700, 24, 384, 31, 0, 1)])
# dwconv_pk; dwconv_pk_runlen (fewest staged rows cdiv(T, 8 R) (8 R + k - 1) over R in 9, 13, 19) gives, for k = 15
# and k = 31 alike: T 153 -> 13, T 161 -> 13 (above dwconv_pp's T <= 152); with glu_in T 9 -> 9, T 72 -> 9, T 150 -> 19
BF16_PK = ([(2, T, 384, k, 0, 1) for k in (15, 31) for T in (153, 161)]
           + [(S, T, 384, k, 1, 1) for k in (15, 31) for (S, T) in ((3, 9), (2, 72), (2, 150))])
CASES = FP32 + BF16_GENERIC + BF16_PP + BF16_PK


@functools.lru_cache(maxsize=4)
def _inputs(case):
    S, T, C, k, glu_in, bf = case
    g = torch.Generator().manual_seed(((((S * 1009 + T) * 1009 + C) * 37 + k) * 2 + glu_in) * 2 + bf)
    x = torch.randn(S, T, (2 if glu_in else 1) * C, generator=g, dtype=torch.float64)
    scale = torch.tensor([1.0, 3.0, 0.3, 2.0, 0.5])[torch.arange(S) % 5].double()
    x = x * scale[:, None, None]
    x = cr.bf16r(x) if bf else x.float().double()          # exactly what the kernel reads
    w = (torch.randn(C, k, generator=g) / k ** 0.5).double()
    bias = (0.5 + 0.1 * torch.randn(C, generator=g)).double()
    gn_g = (torch.rand(C, generator=g) + 0.5).double()
    gn_b = (0.1 * torch.randn(C, generator=g)).double()
    refs = {m: cr.conv_module_ref(x, w, bias, k, bool(glu_in), m, gn_g, gn_b, bool(bf)) for m in (0, 1, 2)}
    bounds = cr.conv_partial_bound(x, w, bias, k, bool(glu_in), bool(bf))
    return x, w, bias, gn_g, gn_b, refs, bounds


def _id(case):
    return "S%d-T%d-C%d-k%d-glu%d-%s" % (case[:5] + ("bf16" if case[5] else "fp32",))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_conv_module(gpu, case, mode):
    S, T, C, k, glu_in, bf = case
    x, w, bias, gn_g, gn_b, refs, (b_sum, b_sq) = _inputs(case)
    dt = torch.bfloat16 if bf else torch.float32
    nblk = (C + 63) // 64
    if glu_in:      # the kernel's column order: 32-wide groups [16 values | 16 gates]
        xi = torch.empty_like(x)
        xi[..., cr.glu_interleave_perm(C)] = x
    else:
        xi = x
    xd = xi.to(dt).contiguous().to(gpu)
    y = torch.full((S * T + GUARD, C), float("nan"), dtype=dt, device=gpu)
    part = torch.full((S * nblk * 2 + GUARD,), float("nan"), device=gpu)
    f32 = [t.float().contiguous().to(gpu) for t in (w, bias, gn_g, gn_b)]
    with cr.profiled() as launches:
        _lib.call("sd_op_glu_dwconv", _lib.ptr(xd), S, T, C, _lib.ptr(f32[0]), _lib.ptr(f32[1]), k, glu_in, bf, mode,
                  _lib.ptr(f32[2]) if mode == 2 else None, _lib.ptr(f32[3]) if mode == 2 else None, _lib.ptr(y),
                  _lib.ptr(part) if mode else None, _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
    assert launches == {("glu_dwconv" if glu_in else "dwconv"): 1, **({"groupnorm_silu": 1} if mode == 2 else {})}
    y, part = y.cpu(), part.cpu()
    assert torch.isnan(y[S * T:].float()).all(), "guard rows written"
    assert torch.isnan(part[S * nblk * 2 if mode else 0:]).all(), "partial sums written past their end"
    out, _, pref = refs[mode]
    got = y[:S * T].double().reshape(S, T, C)
    want = cr.bf16r(out) if bf else out
    err = (got - want).abs()
    print(f"{_id(case)} mode {mode}: max |y - ref| = {err.max().item():.3e}, max |ref| = {want.abs().max().item():.3e}")
    tol = BF16_TOL if bf else FP32_TOL
    torch.testing.assert_close(got, want, **tol)
    if mode == 1:
        p = part[:S * nblk * 2].double().reshape(S, nblk, 2)
        r1 = ((p[..., 0] - pref[..., 0]).abs() / b_sum).max().item()
        r2 = ((p[..., 1] - pref[..., 1]).abs() / b_sq).max().item()
        print(f"  partial sums: error / bound = {r1:.3f} (sum), {r2:.3f} (sum of squares)")
        assert r1 <= 1.0 and r2 <= 1.0
