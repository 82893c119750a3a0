"""The conformer row programs (rowprog.hip rowprog_kernel, with rowprog_pack_pre / rowprog_pack_ffn) one program at a
time through sd_op_rowprog, against tests/conformer_ref.py: rowprog_ref64 (the header formula of rowprog.hip in
float64, weights as given) and rowprog_emu64 (the same with a bf16 rounding at each MFMA operand the kernel rounds).

The fp32 output's tolerance comes from the references alone, per case: with e_max = max |emu64 - ref64| and
e_mean = mean |emu64 - ref64|, a case requires max |Xo - emu64| <= e_max and mean |Xo - emu64| <= e_mean / 10.  A
correct kernel differs from emu64 only where its fp32 arithmetic lands on the other side of a bf16 rounding boundary
(measured on the CPU, the emulation in float32 against float64: 0.12 - 0.34 e_max, 0.002 - 0.01 e_mean); a dropped bias,
a wrong 1/2, a swapped fragment or another row's statistics moves the mean by e_mean or far more.  bf16 outputs (y, yt):
atol 2e-2, rtol 1e-2 against bf16(emu64).  Every output buffer has guard rows of NaN past row M.

Largest ratios observed on an MI355X over this module's cases (every case prints its own): max |Xo - emu64| / e_max =
0.426 (pre + 2 FFNs + y, hidden 64, M 600), mean |Xo - emu64| / (e_mean / 10) = 0.123 (the same program, M 127); the
one-GEMM program (rowprog_out) has no activation rounding and stays at 0.000 / 0.001."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conformer_ref as cr  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

D = cr.D
GUARD = 64
BF16_TOL = dict(atol=2e-2, rtol=1e-2)
NAN = float("nan")


# ---------------------------------------------------------------- inputs
def _gain(g):
    return torch.rand(D, generator=g) + 0.5


def _bias(g, n=D):
    return 0.1 * torch.randn(n, generator=g)


def make_ffn(g, hidden, post):
    return dict(ln_g=_gain(g), ln_b=_bias(g), W1=torch.randn(hidden, D, generator=g) / D ** 0.5, b1=_bias(g, hidden),
                W2=0.5 * torch.randn(D, hidden, generator=g) / hidden ** 0.5, b2=_bias(g),
                post_g=_gain(g) if post else None, post_b=_bias(g) if post else None)


def make_pre(g, M):
    return dict(A=torch.randn(M, D, generator=g).to(torch.bfloat16), W0=torch.randn(D, D, generator=g) / D ** 0.5,
                b0=_bias(g))


def make_program(seed, M, pre, n_ffn, y, hidden=512):
    """(X, pre, ffns, y) of a program: post_g on the FFN that is its layer's second (the one after a pre-GEMM, or the
    first of two)."""
    g = torch.Generator().manual_seed(seed)
    X = 1.5 * torch.randn(M, D, generator=g)
    p = make_pre(g, M) if pre else None
    ffns = [make_ffn(g, hidden, post=(i == 0 and (pre or n_ffn == 2))) for i in range(n_ffn)]
    return X, p, ffns, ((_gain(g), _bias(g)) if y else None)


# ---------------------------------------------------------------- the op
def run(gpu, M, X=None, spk=None, pre=None, ffns=(), y=None, flags=0, xo=True, yt=None, inplace=False, expect=0):
    """One sd_op_rowprog call.  X / pre['A'] are given row-major and laid out here as `flags` says; Xo / y come back
    row-major.  spk = dict(ts, mix (B, Tmix, ldmix), NS, T_seq); yt = dict(NS, T_seq).  Returns dict(Xo, y, yt, X)."""
    keep = []

    def dev(t, dtype=torch.float32):
        if t is None:
            return None
        keep.append(t.to(dtype).contiguous().to(gpu))
        return keep[-1].data_ptr()

    def guarded(rows, dtype, init=None):
        b = torch.full((rows + GUARD, D), NAN, dtype=dtype, device=gpu)
        if init is not None:
            b[:rows] = init.to(gpu)
        return b

    op = _lib.RowprogOp()
    op.M, op.flags = M, flags
    Xd = None
    if X is not None:
        Xd = guarded(M, torch.float32, cr.tile_x(X) if flags & 1 and M % 16 == 0 else X)
        op.X = Xd.data_ptr()
    if spk is not None:
        op.ts, op.mix = dev(spk["ts"]), dev(spk["mix"])
        op.ldmix, op.Tmix, op.NS, op.T_seq = spk["mix"].shape[2], spk["mix"].shape[1], spk["NS"], spk["T_seq"]
    if pre is not None:
        A = pre["A"]
        op.A = dev(cr.tile_a(A) if flags & 4 and M % 16 == 0 else A, torch.bfloat16)
        op.w0, op.b0 = dev(pre["W0"]), dev(pre["b0"])
        if pre.get("gn_T"):
            op.gn_partial, op.gn_g, op.gn_b = dev(pre["gn_partial"]), dev(pre["gn_g"]), dev(pre["gn_b"])
            op.gn_T, op.gn_nblk = pre["gn_T"], D // 64
    op.n_ffn = len(ffns)
    for i, f in enumerate(ffns):
        for k in ("ln_g", "ln_b", "b1", "b2", "post_g", "post_b"):
            setattr(op.ffn[i], k, dev(f[k]))
        op.ffn[i].w1, op.ffn[i].w2 = dev(f["W1"]), dev(f["W2"])
        op.ffn[i].hidden = f["W1"].shape[0]
    Xo = yb = ytb = None
    if xo:
        Xo = Xd if inplace else guarded(M, torch.float32)
        op.Xo = Xo.data_ptr()
    if y is not None:
        yb = guarded(M, torch.bfloat16)
        op.y, op.y_g, op.y_b = yb.data_ptr(), dev(y[0]), dev(y[1])
    if yt is not None:
        ytb = guarded(M, torch.bfloat16)
        op.yt, op.yt_NS, op.T_seq = ytb.data_ptr(), yt["NS"], yt["T_seq"]
    x_before = Xd.clone() if Xd is not None else None
    with cr.profiled() as launches:
        status = _lib.load().sd_op_rowprog(ctypes.byref(op), _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
    assert status == expect, (status, _lib.load().sd_last_error())
    if status:      # refused: nothing launched, nothing written
        assert launches == {}, launches
        assert all(torch.isnan(b.float()).all() for b in (Xo, yb, ytb) if b is not None and b is not Xd)
        return None
    name = ("rowprog_pw2_ffn" if ffns else "rowprog_out") if pre is not None else \
        ("rowprog_ffn" if len(ffns) == 1 else "rowprog")
    assert launches == {name: 1}, launches
    out = {}
    for k, b in (("Xo", Xo), ("y", yb), ("yt", ytb)):
        if b is None:
            continue
        assert torch.isnan(b[M:].float()).all(), f"{k}: rows past M written"
        out[k] = b[:M].cpu()
    if "Xo" in out and flags & 2:
        out["Xo"] = cr.untile_x(out["Xo"])
    if "y" in out and flags & 8:
        out["y"] = cr.untile_a(out["y"])
    if Xd is not None and not inplace:
        assert torch.equal(Xd.view(torch.int32), x_before.view(torch.int32)), "the input X was written"
    return out


def check(tag, out, X64, pre, ffns, y, yt=None):
    """Xo against emu64 under the bounds derived from |emu64 - ref64|; y / yt against bf16(emu64)."""
    ref, _ = cr.rowprog_ref64(X64, pre, ffns, y)
    emu, emu_y = cr.rowprog_emu64(X64, pre, ffns, y)
    e_max, e_mean = (emu - ref).abs().max().item(), (emu - ref).abs().mean().item()
    if "Xo" in out:
        d = (out["Xo"].double() - emu).abs()
        d_max, d_mean = d.max().item(), d.mean().item()
        print(f"{tag}: e_max {e_max:.3e} e_mean {e_mean:.3e}; max |Xo - emu64| / e_max = {d_max / max(e_max, 1e-300):.3f}, "
              f"mean |Xo - emu64| / (e_mean / 10) = {d_mean / max(e_mean / 10, 1e-300):.3f}")
        assert d_max <= e_max and d_mean <= e_mean / 10, (d_max, e_max, d_mean, e_mean)
    if "y" in out:
        torch.testing.assert_close(out["y"].double(), cr.bf16r(emu_y), **BF16_TOL)
    if "yt" in out:
        want = cr.speakers_to_channels(cr.bf16r(emu), yt["NS"], yt["T_seq"]).reshape(-1, D)
        torch.testing.assert_close(out["yt"].double(), want, **BF16_TOL)


# ---------------------------------------------------------------- programs
# (pre, n_ffn, y): rowprog_ffn <1,0,2> | rowprog_out <1,0,1> | the last layer's rowprog_pw2_ffn <1,0,3> | the middle
# layers' <1,0,5> | the two runtime-dispatched forms <1,0>
PROGRAMS = [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 2, 1), (0, 2, 1), (0, 0, 1)]


@pytest.mark.parametrize("prog,hidden", [(p, h) for p in PROGRAMS for h in ((512, 64, 1024) if p[1] else (0,))],
                         ids=lambda v: "pre%d-ffn%d-y%d" % v if isinstance(v, tuple) else "h%d" % v)
def test_programs(gpu, prog, hidden):
    pre, n_ffn, y = prog
    M = 600                                                 # 4 tiles and a tail of 88 rows
    X, p, ffns, yy = make_program(1000 * hidden + 100 * pre + 10 * n_ffn + y, M, pre, n_ffn, y, hidden)
    out = run(gpu, M, X=X, pre=p, ffns=ffns, y=yy)
    check(f"program {prog} hidden {hidden}", out, X.double(), p, ffns, yy)


def test_program_hidden_32(gpu):
    """One up / down piece pair per FFN: the shortest weight ring (P = 12 + 2 pieces per tile)."""
    M = 600
    X, p, ffns, yy = make_program(32, M, 1, 1, 0, 32)
    check("hidden 32", run(gpu, M, X=X, pre=p, ffns=ffns, y=yy), X.double(), p, ffns, yy)


# ---------------------------------------------------------------- row counts
@pytest.mark.parametrize("M", [1, 15, 16, 127, 128, 129, 600])
def test_row_counts(gpu, M):
    X, p, ffns, yy = make_program(7000 + M, M, 1, 2, 1, 512)
    check(f"M {M}", run(gpu, M, X=X, pre=p, ffns=ffns, y=yy), X.double(), p, ffns, yy)


def test_more_tiles_than_workgroups(gpu):
    """M = 256 * 128 + 200: more 128-row tiles than workgroups on a 256-CU device, so workgroups take a second tile,
    the weight ring runs across the tile boundary and rowprog() sets a non-zero stagger."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    if cus > 256:
        pytest.skip(f"{cus} CUs: 258 tiles do not exceed one tile per workgroup here")
    M = 256 * 128 + 200
    X, p, ffns, yy = make_program(4242, M, 1, 2, 1, 64)
    check(f"M {M}", run(gpu, M, X=X, pre=p, ffns=ffns, y=yy), X.double(), p, ffns, yy)


# ---------------------------------------------------------------- tiled layouts
@pytest.mark.parametrize("M", [16, 592, 4800])
def test_tiled_layouts_bit_identical(gpu, M):
    """x_tiled (1), xo_tiled (2), a_tiled (4), y_tiled (8), each alone and all together: the row-major call's bits."""
    X, p, ffns, yy = make_program(9000 + M, M, 1, 1, 1, 64)
    base = run(gpu, M, X=X, pre=p, ffns=ffns, y=yy)
    for flags in (1, 2, 4, 8, 15):
        out = run(gpu, M, X=X, pre=p, ffns=ffns, y=yy, flags=flags)
        assert torch.equal(out["Xo"].view(torch.int32), base["Xo"].view(torch.int32)), flags
        assert torch.equal(out["y"].view(torch.int16), base["y"].view(torch.int16)), flags
    if M == 592:
        check(f"tiled base M {M}", base, X.double(), p, ffns, yy)


@pytest.mark.parametrize("flags", [1, 2, 4, 8])
def test_tiled_layouts_need_whole_groups(gpu, flags):
    """M % 16 != 0 with any tiled flag: SD_ERR_INVALID, no launch, no output row written (run() asserts both)."""
    X, p, ffns, yy = make_program(77, 40, 1, 1, 1, 64)
    assert run(gpu, 40, X=X, pre=p, ffns=ffns, y=yy, flags=flags, expect=_lib.SD_ERR_INVALID) is None


# ---------------------------------------------------------------- GroupNorm on load
@pytest.mark.parametrize("S,gn_T", [(8, 150), (16, 37), (16, 7)])
def test_groupnorm_on_load(gpu, S, gn_T):
    """S gn_T is a multiple of 16 but gn_T is not: 16-row tiles straddle sequences of distinct means and scales.  M =
    1200 / 592 / 112 all leave a dead tail in the last 128-row tile."""
    M = S * gn_T
    assert M % 16 == 0 and M % 128 != 0
    g = torch.Generator().manual_seed(100 * S + gn_T)
    X, p, ffns, yy = make_program(5000 + gn_T, M, 1, 1, 1, 64)
    mean = 2.0 * torch.randn(S, 1, 1, generator=g)
    scale = torch.tensor([1.0, 3.0, 0.3, 2.0])[torch.arange(S) % 4].reshape(S, 1, 1)
    A = (mean + scale * torch.randn(S, gn_T, D, generator=g)).to(torch.bfloat16).reshape(M, D)
    a64 = A.double().reshape(S, gn_T, D // 64, 64)
    partial = torch.stack([a64.sum((1, 3)), (a64 * a64).sum((1, 3))], -1).float()      # (S, 6, 2)
    gn_g, gn_b = _gain(g), _bias(g)
    pg = dict(p, A=A, gn_T=gn_T, gn_g=gn_g, gn_b=gn_b, gn_partial=partial)
    out = run(gpu, M, X=X, pre=pg, ffns=ffns, y=yy)
    check(f"GroupNorm on load T {gn_T}", out, X.double(), pg, ffns, yy)
    # the same program fed silu(GroupNorm(A)) computed in torch
    An = cr.gn_silu_rows(A.double(), gn_T, gn_g.double(), gn_b.double()).to(torch.bfloat16)
    plain = run(gpu, M, X=X, pre=dict(p, A=An), ffns=ffns, y=yy)
    torch.testing.assert_close(out["Xo"], plain["Xo"], **BF16_TOL)
    torch.testing.assert_close(out["y"].float(), plain["y"].float(), **BF16_TOL)


# ---------------------------------------------------------------- speaker source and sink
SPK = dict(B=2, NS=4, T_seq=150, Tmix=149, ldmix=200)


def _speaker_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    B, NS, T, Tmix, ld = (SPK[k] for k in ("B", "NS", "T_seq", "Tmix", "ldmix"))
    ts = 1.5 * torch.randn(B * NS, D // 2, generator=g)
    mix = 1.5 * torch.randn(B, Tmix, ld, generator=g)        # columns 192 .. 199 are padding the kernel never reads
    return ts, mix, cr.speaker_rows(ts, mix[:, :, :D // 2], NS, T)


def test_speaker_source(gpu):
    ts, mix, X = _speaker_inputs(11)
    M = X.shape[0]
    _, _, ffns, yy = make_program(12, M, 0, 1, 1, 512)
    out = run(gpu, M, spk=dict(ts=ts, mix=mix, NS=SPK["NS"], T_seq=SPK["T_seq"]), ffns=ffns, y=yy)
    check("speaker source", out, X.double(), None, ffns, yy)
    # no FFN: the rows come back as they were built (frame Tmix = 149 of every sequence reads as zero)
    out = run(gpu, M, spk=dict(ts=ts, mix=mix, NS=SPK["NS"], T_seq=SPK["T_seq"]), y=yy)
    assert torch.equal(out["Xo"], X)


def test_speaker_sink(gpu):
    M = SPK["B"] * SPK["NS"] * SPK["T_seq"]
    X, p, ffns, _ = make_program(13, M, 1, 1, 0, 512)
    geo = dict(NS=SPK["NS"], T_seq=SPK["T_seq"])
    both = run(gpu, M, X=X, pre=p, ffns=ffns, yt=geo)
    check("speaker sink", both, X.double(), p, ffns, None, yt=geo)
    # Xo = null: only yt is written (run() asserts that the input rows and their guard rows are untouched)
    only = run(gpu, M, X=X, pre=p, ffns=ffns, yt=geo, xo=False)
    assert "Xo" not in only and torch.equal(only["yt"].view(torch.int16), both["yt"].view(torch.int16))


# ---------------------------------------------------------------- in place
@pytest.mark.parametrize("flags", [0, 1], ids=["rowmajor", "tiled-in"])
def test_in_place(gpu, flags):
    """Xo == X, as the stack's programs run (the last one tiled -> row-major): the out-of-place bits."""
    M = 592
    X, p, ffns, yy = make_program(21, M, 1, 1, 0, 64)
    base = run(gpu, M, X=X, pre=p, ffns=ffns, flags=flags)
    out = run(gpu, M, X=X, pre=p, ffns=ffns, flags=flags, inplace=True)
    assert torch.equal(out["Xo"].view(torch.int32), base["Xo"].view(torch.int32))
