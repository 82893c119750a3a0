"""Every GEMM kernel behind conv_gemm at its tile and feature edges, through sd_op_conv_gemm (the production dispatch,
no route override) against tests/gemm_ref.py in float64.

Each case asserts the launch name it is built for, puts NaN in every A column outside the channel slice and around the
output block, and compares either bit for bit (`exact` data, see gemm_ref) or within the derived fp32 accumulation
bound (`random` data).  tests/test_gemm_ref_host.py shows on the CPU that these checks see a dropped K chunk, a shifted
slice, a neighbour's alpha / beta, a misplaced activation, a transformed pad and a repeated split-K beta."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import conformer_ref as cr  # noqa: E402
import gemm_ref as gr  # noqa: E402

from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

GEMM_NAMES = ("gemm_bf16_reg", "gemm_dma", "gemm_dma_splitk", "gemm_ring", "gemm_stream", "gemm_areg",
              "gemm_skinny_bf16", "gemm_skinny_f32", "conv_gemm_f32", "conv_gemm_bf16x3", "fcm_conv3x3_band")
NAN = float("nan")


def _bits(x):
    """float64 -> bf16 bits (int16)."""
    return x.to(torch.float32).to(torch.bfloat16).view(torch.int16)


def _dev(x, bf16, gpu):
    return (_bits(x) if bf16 else x.to(torch.float32)).contiguous().to(gpu)


def _f32(d, key, gpu):
    return d[key].to(torch.float32).contiguous().to(gpu) if key in d else None


def _nan_buf(shape, bf16, gpu):
    return torch.full(shape, NAN, dtype=torch.bfloat16 if bf16 else torch.float32, device=gpu)


def _report(got, target, bound, what):
    err = (got - target).abs()
    bad = ~(err <= bound)                                  # NaN counts as bad
    worst = float((err / bound.clamp(min=1e-300)).max()) if bound.any() else float(err.max())
    print(f"{what}: max err {float(err[~err.isnan()].max()) if (~err.isnan()).any() else NAN:.3e}, "
          f"worst err / bound {worst:.3f}, {int(bad.sum())} of {bad.numel()} beyond the bound")
    if bad.any():
        m, n = [int(v) for v in bad.nonzero()[0]]
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound; first at (m {m}, n {n}): "
                    f"got {float(got[m, n])!r}, want {float(target[m, n])!r} +- {float(bound[m, n]):.3e}")


def _launch_check(launches, kernel):
    ran = {k: v for k, v in launches.items() if k.split(" ")[0] in GEMM_NAMES and v}
    assert ran == {kernel: 1}, f"built for {kernel}, ran {ran}"


def _run(op, gpu, clamp_route=0):
    """One sd_op_conv_gemm call under the launch counters -> {name: launches}.  An argument error raises ValueError; a
    GPU runtime error ends the session (nothing more is started on a device that has faulted)."""
    lib = _lib.load()
    try:
        if clamp_route:
            _lib.call("sd_debug_clamp_route", clamp_route)
        with cr.profiled() as launches:
            status = lib.sd_op_conv_gemm(ctypes.byref(op), _lib.stream_ptr(gpu))
            try:
                torch.cuda.synchronize()
            except RuntimeError as e:
                pytest.exit(f"GPU error after sd_op_conv_gemm: {e}", returncode=3)
    finally:
        if clamp_route:
            _lib.call("sd_debug_clamp_route", 0)
    try:
        _lib.check(status, "sd_op_conv_gemm")
    except _lib.SdiarError as e:
        pytest.exit(f"GPU error in sd_op_conv_gemm: {e}", returncode=3)
    return launches


def _op_for(c, d, gpu, keep, with_A=True):
    """The sd_gemm_op of case c on data d and its NaN-filled output allocation; `keep` holds the device tensors."""
    def put(t):
        keep.append(t)
        return t.data_ptr() if t is not None else None

    shape, (o_sb, o_sh, o_sw, o_sn) = gr.out_shape(c)
    op = _lib.GemmOp()
    op.precision = c.precision
    if with_A:
        # A: NaN in every column outside [a_coff, a_coff + Cin)
        A = d["A"].clone()
        A[..., :c.a_coff] = NAN
        A[..., c.a_coff + c.Cin:] = NAN
        A = A.reshape(-1, c.ld)
        if c.a_tiled:
            A = gr.tile_a(A, c.K)
        op.A = put(_dev(A, c.a_bf16, gpu))
    op.a_bf16, op.a_tiled = int(c.a_bf16), int(c.a_tiled)
    op.B, op.H, op.W, op.Cin, op.lda, op.a_coff = c.B, c.H, c.W, c.Cin, c.ld, c.a_coff
    op.kh, op.kw, op.sh, op.sw, op.ph, op.pw, op.dh, op.dw = c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, c.dh, c.dw
    op.w, op.N = put(_f32(d, "w", gpu)), c.N
    op.pre_scale, op.pre_shift = put(_f32(d, "s", gpu)), put(_f32(d, "h", gpu))
    op.alpha, op.beta = put(_f32(d, "alpha", gpu)), put(_f32(d, "beta", gpu))
    if c.res:
        op.res, op.res_bf16, op.res_ld = put(_dev(d["res"], c.res == "bf16", gpu)), int(c.res == "bf16"), c.N
    op.act = c.act
    op.post_scale, op.post_shift = put(_f32(d, "post_s", gpu)), put(_f32(d, "post_h", gpu))
    if c.gate_seg:
        op.gate, op.gate_seg, op.gate_nseg = put(_f32(d, "gate", gpu)), c.gate_seg, c.gate_nseg
    out = _nan_buf(shape, c.out_bf16, gpu)
    op.out, op.out_bf16 = put(out), int(c.out_bf16)
    op.o_sb, op.o_sh, op.o_sw, op.o_sn = o_sb, o_sh, o_sw, o_sn
    op.glu = int(c.glu)
    op.ln_eps = 1e-5
    return op, out


def _check_out(c, mode, d, out, what):
    ref, tol = gr.reference(c, d)
    target, bound = gr.expected(c, mode, ref, tol)
    buf = out.cpu().to(torch.float64)
    got, outside = gr.out_view(c, buf)
    assert buf[outside].isnan().all(), f"{what}: wrote outside the M x N block"
    _report(got, target, bound, what)
    return got


@pytest.mark.parametrize("case,mode", gr.CASE_MODES, ids=gr.CASE_IDS)
def test_conv_gemm_path(gpu, case, mode):
    c = case
    d = gr.make_data(c, mode)
    keep = []                                              # device tensors alive until the stream is drained
    op, out = _op_for(c, d, gpu, keep)
    ks_dev = slabs = None
    if c.splitk:
        ks_dev = torch.zeros(1, dtype=torch.int32, device=gpu)
        slabs = _nan_buf((5, c.M, c.N), False, gpu)        # 4 slabs the op may use and a sentinel
        keep += [ks_dev, slabs]
        op.ksplit_out, op.slabs, op.slab_cap = ks_dev.data_ptr(), slabs.data_ptr(), 4

    launches = _run(op, gpu, c.clamp_route)
    _launch_check(launches, c.kernel)

    what = f"{c.name}/{mode} ({c.kernel})"
    if c.splitk:
        target, bound = gr.expected(c, mode, *gr.reference(c, d))
        ks = int(ks_dev.item())
        assert 1 < ks <= 4, ks
        s = slabs.cpu().double()
        assert s[ks:].isnan().all(), "a slab beyond the split count was written"
        assert out.isnan().all(), "the split launch wrote the plain output"
        _report(s[:ks].sum(0), target, bound, what)       # beta counted once: slab 0 only
        return
    _check_out(c, mode, d, out, what)


# ---------------------------------------------------------------- the <= 16-row kernel's prologues and K-V epilogue
FP32_TOL = dict(atol=gr.FP32_ATOL, rtol=gr.FP32_RTOL)
SK = "gemm_skinny_bf16"


def _rows_case(name, M, N, K, **kw):
    """A skinny case whose A rows are built in LDS by a prologue: K-wide rows, no sentinel columns to put."""
    return gr.lin(name, SK, M, N, K, lda=K, a_bf16=False, out_bf16=False, **kw)


def _prologue_gemm(gpu, c, d, fill, mode="random"):
    """Runs case c with the op fields `fill(op, put)` sets instead of A -> (out, ln_out read back or None)."""
    keep = []
    op, out = _op_for(c, d, gpu, keep, with_A=False)

    def put(t):
        keep.append(t)
        return t.data_ptr()
    ln_out = fill(op, put)
    _launch_check(_run(op, gpu), c.kernel)
    return out, (ln_out.cpu().double() if ln_out is not None else None)


@pytest.mark.parametrize("ln_t", ["none", "f32", "bf16"])
@pytest.mark.parametrize("K", [256, 1024])
def test_skinny_layernorm_prologue(gpu, K, ln_t):
    M, N = 7, 100
    c = _rows_case(f"skinny_ln_{K}_{ln_t}", M, N, K, res="f32")
    d = gr.make_data(c, "random")
    g = torch.Generator().manual_seed(K + len(ln_t))
    x = (torch.randn(M, K, generator=g) * 3 + 1).double()
    t = torch.randn(M, K, generator=g)
    t = (t.to(torch.bfloat16) if ln_t == "bf16" else t).double()
    gam, bet = torch.randn(K, generator=g).double(), torch.randn(K, generator=g).double()
    v = x + (t if ln_t != "none" else 0)
    ln_ref = (v - v.mean(1, keepdim=True)) / (v.var(1, unbiased=False, keepdim=True) + 1e-5).sqrt() * gam + bet

    def fill(op, put):
        ln_out = _nan_buf((M + 1, K), False, gpu)
        op.ln_x, op.ln_g, op.ln_b, op.ln_out = put(_dev(x, False, gpu)), put(_dev(gam, False, gpu)), \
            put(_dev(bet, False, gpu)), put(ln_out)
        if ln_t != "none":
            op.ln_t, op.ln_t_bf16 = put(_dev(t, ln_t == "bf16", gpu)), int(ln_t == "bf16")
        return ln_out
    out, ln_out = _prologue_gemm(gpu, c, d, fill)
    assert ln_out[M:].isnan().all()
    torch.testing.assert_close(ln_out[:M], ln_ref, **FP32_TOL)
    # the GEMM on the kernel's own rows: the LayerNorm's error stays out of the GEMM's bound
    d["A"] = ln_out[:M].reshape(1, 1, M, K)
    _check_out(c, "random", d, out, c.name)


def test_skinny_layernorm_in_place_is_refused(gpu):
    """ln_out == ln_x: the skinny kernel refuses it (workgroup 0 would overwrite rows the others still read) and no
    other kernel has the prologue, so conv_gemm raises."""
    M, N, K = 7, 100, 256
    c = _rows_case("skinny_ln_alias", M, N, K)
    d = gr.make_data(c, "random")
    x = torch.randn(M, K).double()

    def fill(op, put):
        xd = _dev(x, False, gpu)
        op.ln_x = op.ln_out = put(xd)
        op.ln_g, op.ln_b = put(torch.ones(K, device=gpu)), put(torch.zeros(K, device=gpu))
        fill.x = xd
    with pytest.raises(ValueError, match="skinny path only"):
        _prologue_gemm(gpu, c, d, fill)
    assert torch.equal(fill.x.cpu().double(), x.float().double())


def test_skinny_l2norm_prologue(gpu):
    M, N, K = 7, 100, 512
    c = _rows_case("skinny_l2norm", M, N, K)
    d = gr.make_data(c, "random")
    x = (torch.randn(M, K, generator=torch.Generator().manual_seed(1)) * 2).double()

    def fill(op, put):
        ln_out = _nan_buf((M + 1, K), False, gpu)
        op.pro_mode, op.ln_x, op.ln_out = 1, put(_dev(x, False, gpu)), put(ln_out)
        return ln_out
    out, ln_out = _prologue_gemm(gpu, c, d, fill)
    assert ln_out[M:].isnan().all()
    torch.testing.assert_close(ln_out[:M], x / x.norm(dim=1, keepdim=True), **FP32_TOL)
    d["A"] = ln_out[:M].reshape(1, 1, M, K)
    _check_out(c, "random", d, out, c.name)


@pytest.mark.parametrize("mode", ["exact", "random"])
def test_skinny_slot_init_prologue(gpu, mode):
    """pro_mode 2: row r = ln_x[r / pro_C] + pro_p[r % pro_C], one fp32 add (exact on the integer data)."""
    M, N, K, C = 12, 100, 64, 3
    c = _rows_case("skinny_slot_init", M, N, K, act=gr.RELU)
    d = gr.make_data(c, mode)
    g = torch.Generator().manual_seed(2)
    if mode == "exact":
        x, pp = torch.randint(-2, 3, (M // C, K), generator=g).double(), torch.randint(-1, 2, (C, K), generator=g).double()
    else:
        x, pp = torch.randn(M // C, K, generator=g).double(), torch.randn(C, K, generator=g).double()
    rows = gr.f32r(x.repeat_interleave(C, 0) + pp.repeat(M // C, 1))

    def fill(op, put):
        ln_out = _nan_buf((M + 1, K), False, gpu)
        op.pro_mode, op.pro_C, op.ln_x, op.pro_p, op.ln_out = 2, C, put(_dev(x, False, gpu)), put(_dev(pp, False, gpu)), \
            put(ln_out)
        return ln_out
    out, ln_out = _prologue_gemm(gpu, c, d, fill)
    assert ln_out[M:].isnan().all() and torch.equal(ln_out[:M], rows)
    d["A"] = rows.reshape(1, 1, M, K)
    _check_out(c, mode, d, out, f"{c.name}/{mode}")


@pytest.mark.parametrize("mode", ["exact", "random"])
@pytest.mark.parametrize("cursor,pad,n_valid", [(1, 3, 40), (20, 0, 25), (12, 9, 40)],
                         ids=["before_row0", "past_n_valid", "pad9"])
def test_skinny_gather_window_prologue(gpu, mode, cursor, pad, n_valid):
    """pro_mode 3: the rows a stride-1 k3 conv reads are history rows [cursor - pad, ...), zero outside [0, n_valid);
    cursor and n_valid are device ints.  History rows from n_valid on hold NaN: they must read as 0."""
    Wo, kw, Cin, N, hist = 8, 3, 64, 100, 40
    W = Wo + kw - 1
    c = gr.Case("skinny_gather_window", SK, W=W, Cin=Cin, N=N, kw=kw, lda=Cin, a_bf16=False, out_bf16=False)
    d = gr.make_data(c, mode)
    g = torch.Generator().manual_seed(3)
    h = (torch.randint(-3, 4, (hist, Cin), generator=g) if mode == "exact" else torch.randn(hist, Cin, generator=g)).double()
    src = torch.arange(W) + cursor - pad
    ok = (src >= 0) & (src < n_valid)
    d["A"] = (h[src.clamp(0, hist - 1)] * ok[:, None]).reshape(1, 1, W, Cin)

    def fill(op, put):
        hd = h.clone()
        hd[n_valid:] = NAN
        op.pro_mode, op.pro_pad, op.ln_x = 3, pad, put(_dev(hd, False, gpu))
        op.pro_cursor = put(torch.tensor([cursor], dtype=torch.int32, device=gpu))
        op.pro_nvalid = put(torch.tensor([n_valid], dtype=torch.int32, device=gpu))
    out, _ = _prologue_gemm(gpu, c, d, fill)
    _check_out(c, mode, d, out, f"{c.name}/{mode}")


@pytest.mark.parametrize("out_bf16", [False, True])
def test_skinny_kv_out(gpu, out_bf16):
    """Columns n >= kv_col0 also go to kv_out[(cursor kv_mult + m) kv_ld + n - kv_col0], and nothing else does."""
    M, N, K, mult, cursor = 3, 96, 64, 3, 5
    col0, kv_ld, kv_rows = N // 3, N - N // 3 + 8, (cursor + 2) * mult
    c = gr.lin("skinny_kv_out", SK, M, N, K, a_bf16=False, out_bf16=out_bf16)
    d = gr.make_data(c, "exact")
    keep = []
    op, out = _op_for(c, d, gpu, keep)
    kv = _nan_buf((kv_rows, kv_ld), out_bf16, gpu)
    cur = torch.tensor([cursor], dtype=torch.int32, device=gpu)
    op.kv_out, op.kv_cursor, op.kv_mult, op.kv_col0, op.kv_ld = kv.data_ptr(), cur.data_ptr(), mult, col0, kv_ld
    _launch_check(_run(op, gpu), c.kernel)
    got = _check_out(c, "exact", d, out, c.name)
    kvh = kv.cpu().double()
    r0 = cursor * mult
    assert torch.equal(kvh[r0:r0 + M, :N - col0], got[:, col0:])
    kvh[r0:r0 + M, :N - col0] = NAN
    assert kvh.isnan().all(), "kv_out written outside its rows / columns"
