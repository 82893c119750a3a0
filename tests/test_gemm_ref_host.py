"""CPU self-tests of tests/gemm_ref.py, on every case of the GPU matrix (tests/test_gpu_gemm_paths.py) restricted to
its first 64 and last 64 output rows:

  * exactness: the `exact` data's product, emulated in fp32 in three summation orders (forward, reversed, chunks of 32),
    equals the float64 reference bit for bit -- the premise under which a kernel must match the reference bit for bit
    whatever its accumulation order;
  * sensitivity: each value-only mutation of the reference (a dropped K chunk, a shifted channel slice, alpha / beta of
    the neighbouring column, the activation before the residual, a prologue applied to the padding, beta in every
    split-K slab) moves at least half of the output elements it can reach beyond the case's tolerance, so a kernel
    with that bug cannot pass."""
import pytest
import torch

import gemm_ref as gr


def _rows(case):
    M = case.M
    return torch.arange(M) if M <= 128 else torch.cat([torch.arange(64), torch.arange(M - 64, M)])


_DATA = {}


def _data(case, mode):
    key = (case.name, mode)
    if key not in _DATA:
        _DATA.clear()                                    # one case's tensors at a time
        _DATA[key] = gr.make_data(case, mode)
    return _DATA[key]


def test_matrix_is_consistent():
    names = [c.name for c in gr.CASES]
    assert len(set(names)) == len(names)
    for c in gr.CASES:
        assert c.M >= 1 and c.K % 8 == 0 and c.ld >= c.a_coff + c.Cin
        assert c.skinny == (c.M <= 16) or c.pre           # <= 16 rows reach a tile kernel only with a prologue
        if c.precision != 1 and not c.skinny:            # the fp32 tile kernels take fp32 tensors only
            assert not c.a_bf16 and not c.out_bf16 and c.res != "bf16"
        if not c.a_tiled and c.kw * c.kh == 1 and not c.skinny:
            assert c.ld >= c.a_coff + c.Cin + gr.PAD_COLS    # room for the NaN sentinel columns


def _sum_orders(a, w):
    """a (R, K), w (N, K) float32 -> the three fp32 sums of products, each a (R, N) float32."""
    R, K = a.shape
    fwd = torch.zeros(R, w.shape[0], dtype=torch.float32)
    rev = fwd.clone()
    chunks = fwd.clone()
    part = fwd.clone()
    for k in range(K):
        fwd += a[:, k:k + 1] * w[:, k]
        rev += a[:, K - 1 - k:K - k] * w[:, K - 1 - k]
        part += a[:, k:k + 1] * w[:, k]
        if k % 32 == 31 or k == K - 1:
            chunks += part
            part.zero_()
    return fwd, rev, chunks


@pytest.mark.parametrize("case", [c for c in gr.CASES if "exact" in c.modes], ids=lambda c: c.name)
def test_exact_data_sums_exactly_in_fp32(case):
    d = _data(case, "exact")
    rows = _rows(case)
    a, w = gr.im2col(case, d, rows), gr.weights(case, d)
    # the operands are what they claim to be: bf16 values, so no rounding happens on the way into the kernel
    assert torch.equal(gr.bf16r(a), a) and torch.equal(gr.bf16r(w), w)
    for k in ("alpha", "beta", "res", "post_s", "post_h", "gate", "s", "h"):
        if k in d:
            assert torch.equal(gr.bf16r(d[k]), d[k]), k
    acc64 = a @ w.t()
    assert float((a.abs() @ w.abs().t()).max()) / float(w.abs()[w != 0].min()) * 4 < 2 ** 24
    for got in _sum_orders(a.float(), w.float()):
        assert torch.equal(got.double(), acc64)
    # the whole linear epilogue in fp32, without FMA, gives the float64 reference exactly
    if case.act in (gr.NONE, gr.RELU, gr.CLAMP20) and not case.glu:
        ref, _ = gr.reference(case, d, rows)
        x = acc64.float()
        if case.alpha:
            x = x * d["alpha"].float()
        if case.beta:
            x = x + d["beta"].float()
        if case.res:
            x = x + d["res"][rows].float()
        x = gr._act(x, case.act)
        if case.post:
            x = x * d["post_s"].float() + d["post_h"].float()
        if case.gate_seg:
            x = x * d["gate"][rows // (case.Wo * case.Ho), (rows % case.Wo) // case.gate_seg].float()
        assert torch.equal(x.double(), ref)
    if case.act == gr.CLAMP20:                            # accumulators on both sides of the clamp
        pre = acc64 * d["alpha"] + d["beta"]
        assert (pre < 0).any() and (pre > 20).any()


def _reachable(case, rows, mut):
    """Rows of `rows` the mutation can change: all, or for the padding mutation those that read a padded tap."""
    c = case
    if mut != "pre_pad":
        return torch.ones(len(rows), dtype=torch.bool)
    wo, ho = rows % c.Wo, (rows // c.Wo) % c.Ho
    hit = torch.zeros(len(rows), dtype=torch.bool)
    for i in range(c.kh):
        for j in range(c.kw):
            hi, wi = ho * c.sh - c.ph + i * c.dh, wo * c.sw - c.pw + j * c.dw
            hit |= (hi < 0) | (hi >= c.H) | (wi < 0) | (wi >= c.W)
    return hit


@pytest.mark.parametrize("case,mode", gr.CASE_MODES, ids=gr.CASE_IDS)
def test_mutations_are_detected(case, mode):
    d = _data(case, mode)
    rows = _rows(case)
    ref, tol = gr.reference(case, d, rows)
    target, bound = gr.expected(case, mode, ref, tol)
    assert torch.isfinite(ref).all() and torch.isfinite(bound).all()
    # the reference passes its own check
    assert ((ref - target).abs() <= bound + (2.0 ** -8 * ref.abs() if case.out_bf16 else 0)).all()
    ran = 0
    for mut in gr.MUTATIONS:
        if not gr.applies(case, mut, mode):
            continue
        ran += 1
        bad, _ = gr.reference(case, d, rows, mut)
        got = gr.bf16r(bad) if case.out_bf16 else gr.f32r(bad)      # what a kernel with the bug would store
        moved = (got - target).abs() > bound
        reach = _reachable(case, rows, mut)
        assert reach.any(), mut
        frac = float(moved[reach].double().mean())
        assert frac >= 0.5, f"{mut}: only {frac:.3f} of the reachable elements move beyond the tolerance"
    assert ran >= 1
