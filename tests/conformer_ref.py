"""Plain float64 CPU references for the fused conformer path (rowprog.hip, ops.hip glu_dwconv / groupnorm_silu,
encoder.cpp run_conformer_stack) and the host-side layout transforms its tests need.  Nothing here touches a GPU:
`python -m tests.conformer_ref` (or `python tests/conformer_ref.py`) runs a self-check of the references against each
other."""
import contextlib
import math

import torch
import torch.nn.functional as F

D = 384
U32 = 2.0 ** -24          # fp32 unit roundoff


def bf16r(x):
    """x rounded to bf16 (through fp32, as the kernels round their fp32 values), back in float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


@contextlib.contextmanager
def profiled():
    """Collects {ProfScope name: launches} of the library calls made inside the block (sd_prof_enable / sd_prof_query):
    the tests assert with it that a case took the launch path it names."""
    from speaker_diarization_amd import _lib
    lib = _lib.load()
    lib.sd_prof_enable(1)
    lib.sd_prof_reset()
    out = {}
    try:
        yield out
    finally:
        out.update({k: v["launches"] for k, v in _lib.prof_stats().items()})
        lib.sd_prof_reset()
        lib.sd_prof_enable(0)


# ---------------------------------------------------------------- layouts
def tile_a(x):
    """Rows of 384 (any leading shape, rows % 16 == 0) -> the row programs' bf16 MFMA-fragment layout (kernels.h
    RowProgArgs::a_tiled, also y_tiled and mha_block's): 16-row group g, fragment kk (features 32 kk ..), lane
    l = row % 16 + 16 q holds features 32 kk + 8 q .. + 7 of row 16 g + l % 16."""
    r = x.reshape(-1, 16, D // 32, 4, 8)                    # (group, row, kk, q, 8)
    return r.permute(0, 2, 3, 1, 4).contiguous().reshape(x.shape)


def untile_a(x):
    r = x.reshape(-1, D // 32, 4, 16, 8)                    # (group, kk, q, row, 8)
    return r.permute(0, 3, 1, 2, 4).contiguous().reshape(x.shape)


def tile_x(x):
    """Rows of 384 -> the fp32 residual layout (kernels.h RowProgArgs::x_tiled): feature 16 ft + 4 q + r of row
    16 g + l at float ((g * 24 + ft) * 64 + l + 16 q) * 4 + r."""
    r = x.reshape(-1, 16, D // 16, 4, 4)                    # (group, row l, ft, q, r)
    return r.permute(0, 2, 3, 1, 4).contiguous().reshape(x.shape)


def untile_x(x):
    r = x.reshape(-1, D // 16, 4, 16, 4)                    # (group, ft, q, row l, r)
    return r.permute(0, 3, 1, 2, 4).contiguous().reshape(x.shape)


def glu_interleave_perm(C):
    """perm[r] = column of original pointwise_conv1 channel r (values 0 .. C - 1, gates C .. 2 C - 1) in the 32-wide
    [16 values | 16 gates] order (kernels.h glu_interleave_row)."""
    r = torch.arange(2 * C)
    gate = r >= C
    c = torch.where(gate, r - C, r)
    return (c // 16) * 32 + gate.long() * 16 + c % 16


def speaker_rows(ts, mix, NS, T_seq):
    """The TS-VAD speaker-stream input rows (kernels.h RowProgArgs::x_ts): ts (B NS, 192), mix (B, Tmix, 192) ->
    (B NS T_seq, 384) with row (s, t) = [ts[s] | mix[s // NS][t]], zeros for t >= Tmix."""
    Sq, SE = ts.shape
    B, Tmix, _ = mix.shape
    m = torch.zeros(B, T_seq, SE, dtype=mix.dtype)
    m[:, :min(Tmix, T_seq)] = mix[:, :T_seq]
    m = m[:, None].expand(B, NS, T_seq, SE).reshape(Sq, T_seq, SE)
    return torch.cat([ts[:, None].expand(Sq, T_seq, SE), m], -1).reshape(Sq * T_seq, 2 * SE)


def speakers_to_channels(x, NS, T_seq):
    """(B NS T_seq, E) speaker-major rows -> (B, T_seq, NS E)."""
    E = x.shape[-1]
    return x.reshape(-1, NS, T_seq, E).permute(0, 2, 1, 3).reshape(-1, T_seq, NS * E)


# ---------------------------------------------------------------- conv module
def conv_module_ref(x, w, bias, k, glu_in, mode, gn_g=None, gn_b=None, io_bf16=False, eps=1e-5):
    """The conformer conv module's middle (torchaudio _ConvolutionModule.sequential[1:5]) in float64.

    x: float64 (S, T, C), or with glu_in the pointwise_conv1 output (S, T, 2 C) in ORIGINAL channel order [values |
    gates]; already holding exactly the values the kernel reads (bf16-representable when io_bf16).  w (C, k), bias (C).
    mode 0: silu(conv); 1: conv; 2: silu(group_norm(conv, 1 group per sequence)).  With io_bf16 the values the kernel
    stores as bf16 are rounded here too: the GLU product it stages (glu_dwconv_kernel<true> / dwconv_pk_kernel:
    pack_bf16x2(a * sigmoid(g))) and, in mode 2, the pre-norm y that groupnorm_silu reads back; the GroupNorm
    statistics come from the unrounded conv values, as the kernels' partial sums do.
    Returns (out, conv, partial): out (S, T, C) before the final bf16 store, conv (S, T, C) unrounded, partial
    (S, cdiv(C, 64), 2) = (sum, sum of squares) of conv per sequence and 64-channel block."""
    S, T, _ = x.shape
    C = w.shape[0]
    xg = F.glu(x, dim=-1) if glu_in else x
    if glu_in and io_bf16:
        xg = bf16r(xg)
    conv = F.conv1d(xg.transpose(1, 2), w[:, None, :], bias, padding=(k - 1) // 2, groups=C).transpose(1, 2)
    nblk = (C + 63) // 64
    partial = torch.zeros(S, nblk, 2, dtype=torch.float64)
    for b in range(nblk):
        blk = conv[:, :, 64 * b:64 * b + 64]
        partial[:, b, 0] = blk.sum((1, 2))
        partial[:, b, 1] = (blk * blk).sum((1, 2))
    if mode == 0:
        out = F.silu(conv)
    elif mode == 1:
        out = conv
    else:
        y = bf16r(conv) if io_bf16 else conv
        mean = conv.mean((1, 2), keepdim=True)
        var = conv.var((1, 2), unbiased=False, keepdim=True)
        out = F.silu((y - mean) / torch.sqrt(var + eps) * gn_g + gn_b)
    return out, conv, partial


def conv_partial_bound(x, w, bias, k, glu_in, io_bf16):
    """Worst-case error of the kernels' fp32 partial sums against conv_module_ref's, from the number formats alone:
    (bound on the sums, bound on the sums of squares), each (S, cdiv(C, 64)).

    With u = 2^-24: a conv value is bias + k FMAs in fp32, relative error <= (k + 1) u of A = |bias| + sum |w| |x|;
    a thread adds at most T of them and the block tree adds 8 levels, <= (T + 8) u of the sum of magnitudes.  With
    glu_in the staged input a * sigmoid(g) carries the hardware exp / rcp error, <= e_in = (8 + 2 |g|) u (v_exp_f32 of
    -g log2(e): the argument's rounding scales with |g|); in bf16 that only matters where the float64 product lies
    within e_in of a bf16 rounding boundary, where the staged value may be the neighbouring bf16 number: those
    elements contribute one bf16 ulp each, through |w|."""
    C = w.shape[0]
    T = x.shape[1]
    aw = w.abs()[:, None, :]
    pad = (k - 1) // 2

    def absconv(v):
        return F.conv1d(v.transpose(1, 2), aw, None, padding=pad, groups=C).transpose(1, 2)

    if glu_in:
        p = F.glu(x, dim=-1)
        e_in = (8 + 2 * x[..., C:].abs()) * U32
        if io_bf16:
            ulp = torch.exp2(torch.floor(torch.log2(p.abs().clamp_min(1e-300))) - 7)
            to_boundary = ulp / 2 - (p - bf16r(p)).abs()
            dx = torch.where(to_boundary <= e_in * p.abs(), ulp, torch.zeros_like(p))
            xa = bf16r(p).abs()
        else:
            dx = e_in * p.abs()
            xa = p.abs()
    else:
        xa = x.abs()
        dx = torch.zeros_like(x)
    A = absconv(xa) + (bias.abs() if bias is not None else 0)
    dy = (k + 1) * U32 * A + absconv(dx)            # per conv value
    e1 = dy + (T + 8) * U32 * A
    e2 = 2 * A * dy + (T + 9) * U32 * A * A
    nblk = (C + 63) // 64
    b1 = torch.stack([e1[:, :, 64 * b:64 * b + 64].sum((1, 2)) for b in range(nblk)], 1)
    b2 = torch.stack([e2[:, :, 64 * b:64 * b + 64].sum((1, 2)) for b in range(nblk)], 1)
    return b1, b2


# ---------------------------------------------------------------- row programs
def _ln(x, g=None, b=None, eps=1e-5):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    y = (x - m) / torch.sqrt(v + eps)
    return y if g is None else y * g + b


def gn_silu_rows(A, gn_T, g, b, eps=1e-5, partial=None):
    """silu(GroupNorm(A)) with one group per gn_T consecutive rows (the conv module's GroupNorm(1, C) per sequence).
    partial (S, nblk, 2): take the statistics from these (sum, sum of squares) partial sums instead, mean = sum / n,
    var = sumsq / n - mean^2 clamped at 0 (groupnorm_silu_kernel's and the row program's form, in float64)."""
    a = A.reshape(-1, gn_T, A.shape[-1])
    if partial is None:
        m = a.mean((1, 2), keepdim=True)
        v = a.var((1, 2), unbiased=False, keepdim=True)
    else:
        n = gn_T * A.shape[-1]
        m = (partial[..., 0].double().sum(1) / n).reshape(-1, 1, 1)
        v = (partial[..., 1].double().sum(1).reshape(-1, 1, 1) / n - m * m).clamp_min(0)
    return F.silu((a - m) / torch.sqrt(v + eps) * g + b).reshape(A.shape)


def rowprog_ref64(X, pre=None, ffns=(), y=None, eps=1e-5):
    """The row program of rowprog.hip's header formula in float64, weights exactly as given:
        acc = X;  acc += A W0^T + b0;  per FFN: acc += W2 silu(W1 LN(acc) + b1) + b2, acc = LN_post(acc);  y = LN_y(acc)
    X (M, 384) float64; pre = dict(A, W0, b0[, gn_T, gn_g, gn_b]); ffns = dicts(ln_g, ln_b, W1, b1, W2, b2[, post_g,
    post_b]) with W2 / b2 as the kernel consumes them (no 1/2 applied here); y = (y_g, y_b).  Returns (acc, y or None)."""
    acc = X.clone()
    if pre is not None:
        a = pre["A"].double()
        if pre.get("gn_T"):
            a = gn_silu_rows(a, pre["gn_T"], pre["gn_g"].double(), pre["gn_b"].double(), eps)
        acc = acc + F.linear(a, pre["W0"].double(), pre["b0"].double())
    for f in ffns:
        h = F.silu(F.linear(_ln(acc, f["ln_g"].double(), f["ln_b"].double(), eps), f["W1"].double(), f["b1"].double()))
        acc = acc + F.linear(h, f["W2"].double(), f["b2"].double())
        if f.get("post_g") is not None:
            acc = _ln(acc, f["post_g"].double(), f["post_b"].double(), eps)
    return acc, (_ln(acc, y[0].double(), y[1].double(), eps) if y is not None else None)


def rowprog_emu64(X, pre=None, ffns=(), y=None, eps=1e-5, rnd=bf16r):
    """rowprog_ref64's arithmetic in float64 with a bf16 rounding exactly where rowprog_kernel rounds an MFMA operand
    (rowprog.hip line numbers):
      * A is bf16 in HBM (:312-318); with the GroupNorm-on-load the operand is bf16(silu(GN(A))) (:351-355, pack_bf16x2);
      * W0: rowprog_pack_pre -> put_frag's f2bf (:552, :567);
      * W1 diag(ln_g), the product formed in fp32 by rowprog_pack_ffn (:583) and rounded by put_frag (:592); the folded
        bias b1' = b1 + W1 ln_b uses the unrounded W1 and stays fp32 (:581-586);
      * W2: put_frag (:593);
      * the normalised row (x - mean) rstd of each FFN, packed by pack_bf16x2 (:400-401);
      * silu(hidden + b1'), packed by pack_bf16x2 (:437-440).
    Nothing else is rounded: the accumulator (the MFMA's fp32 registers), every LayerNorm's statistics and affine
    (ln_stats, :139-155; :466-469; :512-515) and the biases (add_bias, :158) are fp32 in the kernel and float64 here.
    rnd = (lambda v: v) turns the rounding off; the result then equals rowprog_ref64's (the self-check below)."""
    acc = X.clone()
    if pre is not None:
        a = pre["A"].double()
        if pre.get("gn_T"):
            # the statistics from the partial sums the kernel is handed (an input of the program: :325-336), when given
            a = rnd(gn_silu_rows(a, pre["gn_T"], pre["gn_g"].double(), pre["gn_b"].double(), eps,
                                 pre.get("gn_partial") if rnd is bf16r else None))
        acc = acc + a @ rnd(pre["W0"].double()).t() + pre["b0"].double()
    for f in ffns:
        W1, g = f["W1"], f["ln_g"]
        # the packer multiplies in fp32; with the rounding off (self-check) keep the product exact
        W1f = (W1.float() * g.float()).double() if rnd is bf16r else W1.double() * g.double()
        b1f = f["b1"].double() + W1.double() @ f["ln_b"].double()
        xh = rnd(_ln(acc, eps=eps))
        h = rnd(F.silu(xh @ rnd(W1f).t() + b1f))
        acc = acc + h @ rnd(f["W2"].double()).t() + f["b2"].double()
        if f.get("post_g") is not None:
            acc = _ln(acc, f["post_g"].double(), f["post_b"].double(), eps)
    return acc, (_ln(acc, y[0].double(), y[1].double(), eps) if y is not None else None)


# ---------------------------------------------------------------- stack
CONFORMER_KEYS = (
    ["ffn1.sequential.%s" % s for s in ("0.weight", "0.bias", "1.weight", "1.bias", "4.weight", "4.bias")]
    + ["self_attn_layer_norm.weight", "self_attn_layer_norm.bias", "self_attn.in_proj_weight",
       "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
       "conv_module.layer_norm.weight", "conv_module.layer_norm.bias"]
    + ["conv_module.sequential.%s" % s for s in ("0.weight", "0.bias", "2.weight", "2.bias", "3.weight", "3.bias",
                                                 "3.running_mean", "3.running_var", "5.weight", "5.bias")]
    + ["ffn2.sequential.%s" % s for s in ("0.weight", "0.bias", "1.weight", "1.bias", "4.weight", "4.bias")]
    + ["final_layer_norm.weight", "final_layer_norm.bias"])


def conformer_blob(sd, n_layers, group_norm):
    """The flat fp32 weight array sd_op_conformer_stack takes (include/sdiar.h), from a Conformer state_dict."""
    parts = []
    for i in range(n_layers):
        for k in CONFORMER_KEYS:
            if group_norm and "running_" in k:
                continue
            parts.append(sd[f"conformer_layers.{i}.{k}"].detach().float().reshape(-1))
    return torch.cat(parts).contiguous()


def make_conformer(n_layers, ffn_dim, nh, kernel, group_norm, seed):
    """oracle.torchaudio_conformer.Conformer in float64 with every parameter away from its initial value (LayerNorm
    and norm gains U(0.5, 1.5), biases 0.1 N(0, 1), BatchNorm running statistics N(0, 0.3) / U(0.5, 1.5))."""
    from oracle.torchaudio_conformer import Conformer
    g = torch.Generator().manual_seed(seed)
    m = Conformer(D, nh, ffn_dim, n_layers, kernel, use_group_norm=group_norm).double().eval()
    with torch.no_grad():
        for name, p in list(m.named_parameters()) + list(m.named_buffers()):
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith("running_var"):
                p.copy_(torch.rand(p.shape, generator=g, dtype=torch.float64) + 0.5)
            elif name.endswith("running_mean"):
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3)
            elif p.dim() == 1 and name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g, dtype=torch.float64) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.1)
            else:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) / math.sqrt(fan_in))
            p.copy_(p.float().double())          # the GPU sees fp32 weights: keep them exactly representable
    return m


def conformer_forward(m, x, key_len=None):
    S, T, _ = x.shape
    lengths = key_len.long() if key_len is not None else torch.full((S,), T, dtype=torch.long)
    with torch.no_grad():
        return m(x, lengths)[0]


def conformer_bf16_weights(m):
    """A copy of the model with every weight matrix (the GEMM operands: the Linear, in-projection and 1x1 conv
    weights) rounded to bf16; vectors and the depthwise taps, which the kernels keep in fp32, stay exact."""
    import copy
    r = copy.deepcopy(m)
    with torch.no_grad():
        for name, p in r.named_parameters():
            if p.dim() >= 2 and "conv_module.sequential.2." not in name:
                p.copy_(bf16r(p))
    return r


# ---------------------------------------------------------------- self-check
def _self_check():
    g = torch.Generator().manual_seed(0)

    def rn(*s, scale=1.0):
        return torch.randn(*s, generator=g, dtype=torch.float64) * scale

    def gain():
        return torch.rand(D, generator=g, dtype=torch.float64) + 0.5

    M, H = 96, 64
    X = rn(M, D, scale=1.5)
    pre = dict(A=bf16r(rn(M, D)), W0=rn(D, D, scale=D ** -0.5), b0=rn(D, scale=0.1), gn_T=48, gn_g=gain(),
               gn_b=rn(D, scale=0.1))
    ffns = [dict(ln_g=gain(), ln_b=rn(D, scale=0.1), W1=rn(H, D, scale=D ** -0.5), b1=rn(H, scale=0.1),
                 W2=rn(D, H, scale=0.5 * H ** -0.5), b2=rn(D, scale=0.1), post_g=gain() if i == 0 else None,
                 post_b=rn(D, scale=0.1) if i == 0 else None) for i in range(2)]
    y = (gain(), rn(D, scale=0.1))
    r, ry = rowprog_ref64(X, pre, ffns, y)
    e, ey = rowprog_emu64(X, pre, ffns, y, rnd=lambda v: v)
    d = max((r - e).abs().max().item(), (ry - ey).abs().max().item())
    assert d < 1e-11, d
    eb, _ = rowprog_emu64(X, pre, ffns, y)
    db = (eb - r).abs().max().item()
    assert 1e-4 < db < 0.2, db                       # the bf16 emulation differs from ref64 by bf16-sized errors
    for t in (torch.float32, torch.bfloat16):
        v = torch.randn(64, D, generator=g).to(t)
        assert torch.equal(untile_a(tile_a(v)), v) and torch.equal(untile_x(tile_x(v)), v)
    # tile_x against the address formula of kernels.h
    v = torch.arange(32 * D, dtype=torch.float32).reshape(32, D)
    tx = tile_x(v).reshape(-1)
    ta = tile_a(v).reshape(-1)
    for row, f in ((0, 0), (5, 7), (17, 100), (31, 383)):
        gq, l = divmod(row, 16)
        ft, q, rr = f // 16, (f % 16) // 4, f % 4
        assert tx[((gq * 24 + ft) * 64 + l + 16 * q) * 4 + rr] == v[row, f]
        kk, q8, j = f // 32, (f % 32) // 8, f % 8
        assert ta[((gq * 12 + kk) * 64 + l + 16 * q8) * 8 + j] == v[row, f]
    # conv module: the GLU interleave undone, partial sums consistent
    C, k, S, T = 48, 7, 2, 9
    x = rn(S, T, 2 * C)
    w, b = rn(C, k, scale=k ** -0.5), rn(C, scale=0.1) + 0.5
    perm = glu_interleave_perm(C)
    xi = torch.empty_like(x)
    xi[..., perm] = x
    assert torch.equal(xi[..., 0:16], x[..., 0:16]) and torch.equal(xi[..., 16:32], x[..., C:C + 16])
    out, conv, part = conv_module_ref(x, w, b, k, True, 1)
    assert torch.allclose(part[:, 0, 0], conv.sum((1, 2)))
    ts, mix = rn(4, 192), rn(2, 5, 192)
    rows = speaker_rows(ts, mix, 2, 6).reshape(4, 6, D)
    assert torch.equal(rows[3, 2, :192], ts[3]) and torch.equal(rows[3, 2, 192:], mix[1, 2]) and (rows[:, 5, 192:] == 0).all()
    print(f"conformer_ref self-check ok: |emu64(no rounding) - ref64| = {d:.2e}, |emu64 - ref64| = {db:.2e}")


if __name__ == "__main__":
    _self_check()
