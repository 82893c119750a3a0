"""Plain float64 reference of conv_gemm (kernels.h ConvGemmArgs) and the case matrix of tests/test_gpu_gemm_paths.py.
Nothing here touches a GPU; tests/test_gemm_ref_host.py checks the reference against itself on the CPU.

The reference multiplies exactly the operand values the kernel multiplies:
  * the bf16 tile kernels (gemm_bf16_reg, gemm_dma, gemm_ring, gemm_stream, gemm_areg): A and W rounded to bf16 (RNE);
    with the BN-ReLU prologue a' = relu(a s + h) is formed in fp32 first and then rounded;
  * gemm_skinny: A as given (fp32, or the bf16 values of a bf16 A), W rounded to bf16 at precision 1, else fp32;
  * conv_gemm_f32 / conv_gemm_bf16x3: fp32 operands.
im2col is tap-major (k = (i kw + j) Cin + c); padded taps contribute 0 (the prologue is not applied to them).
Epilogue, in the order of the kernels: x = acc alpha + beta + res; x = act(x); x = x post_scale + post_shift;
x *= gate[b, wo / gate_seg, n].  GLU: channel c = a_c sigmoid(g_c) of torch-order rows [values | gates].

Two kinds of data.

`exact`: A and res are small integers, W = (small integer) 2^e with 2^e the power of two nearest below 1 / sqrt(K), s,
alpha, post_scale and gate are powers of two, h, beta and post_shift small multiples of 1/4.  All are bf16 values.  With
|a'| <= 7.5 in units of 1/4 (30 units), |w| <= 2 units of 2^e and K <= 4864, every partial sum of products is an integer
of at most 30 * 2 * 4864 < 2^19 units of 2^(e-2): exactly representable in fp32 in ANY summation order, on MFMA or
VALU.  The linear epilogue adds multiples of that unit below 2^24 units, so it is exact with or without FMA contraction.
Hence for act in {none, relu, clamp20} the kernel must give the reference BIT FOR BIT (after one RNE rounding to bf16
for a bf16 output).  tests/test_gemm_ref_host.py proves the premise by summing in fp32 in three orders.

`random`: randn A and W / sqrt(K).  The bound per element, for any accumulation order with one rounding (or one
truncation) of relative size 2^-23 per step: after K products and K - 1 additions the error of acc is at most
2^-23 K sum|a'||w'| to first order; the epilogue's few operations (alpha, beta, res, post, gate: at most 8 roundings,
doubled for a prologue's fp32 rounding of a') are covered by 16 more steps on the epilogue's own magnitude.  So
    E = 2^-23 (K + 16) S,   S = |alpha| sum|a'||w'| + |beta| + |res|,
S carried through max(1, |post_scale|), + |post_shift| and max(1, |gate|).  Nothing is assumed about MFMA's internal
order or rounding.  A bf16 output adds the RNE half ulp 2^-8 (|ref| + E).  The transcendental activations (sigmoid,
SiLU, both GELUs, GLU) add the project's FP32_TOL (atol = rtol = 1e-4) in both kinds of data.  Split-K sums of slabs
use the same bound (every slab's error is bounded by its own share of S).  No constant is tuned against kernel output.
"""
import dataclasses
import math
import zlib

import torch

FP32_ATOL = FP32_RTOL = 1e-4     # tests/test_gpu_ops.py FP32_TOL
NONE, RELU, SIGMOID, SILU, CLAMP20, GELU, GELU_TANH = range(7)
TRANSCENDENTAL = (SIGMOID, SILU, GELU, GELU_TANH)
PAD_COLS = 8                     # sentinel columns behind the A slice, and behind the N output columns
PAD_ROWS = 64                    # sentinel rows behind the M output rows


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kernel: str                  # the ProfScope launch name the case is built for
    B: int = 1
    H: int = 1
    W: int = 1
    Cin: int = 8
    N: int = 4
    precision: int = 1           # 0 fp32, 1 bf16 MFMA, 2 bf16x3
    a_bf16: bool = True
    lda: int = 0                 # 0: a_coff + Cin + PAD_COLS
    a_coff: int = 0
    kh: int = 1
    kw: int = 1
    sh: int = 1
    sw: int = 1
    ph: int = 0
    pw: int = 0
    dh: int = 1
    dw: int = 1
    a_tiled: bool = False
    pre: bool = False
    alpha: bool = True
    beta: bool = True
    res: str = ""                # "", "f32" or "bf16"
    act: int = NONE
    post: bool = False
    gate_seg: int = 0
    gate_nseg: int = 0
    out_bf16: bool = True
    transposed: bool = False     # out (B, N, Wo): o_sn = Wo, o_sw = 1
    glu: bool = False
    splitk: bool = False
    clamp_route: int = 0
    modes: tuple = ("exact", "random")

    @property
    def Ho(self):
        return (self.H + 2 * self.ph - self.dh * (self.kh - 1) - 1) // self.sh + 1

    @property
    def Wo(self):
        return (self.W + 2 * self.pw - self.dw * (self.kw - 1) - 1) // self.sw + 1

    @property
    def M(self):
        return self.B * self.Ho * self.Wo

    @property
    def K(self):
        return self.kh * self.kw * self.Cin

    @property
    def ld(self):
        return self.lda or self.a_coff + self.Cin + PAD_COLS

    @property
    def n_out(self):
        return self.N // 2 if self.glu else self.N

    @property
    def skinny(self):
        return self.kernel.startswith("gemm_skinny")

    @property
    def bf16_operands(self):
        return self.precision == 1 and not self.skinny


def lin(name, kernel, M, N, K, **kw):
    """A linear layer of M rows as conv_gemm sees it: B 1, H 1, W M."""
    return Case(name, kernel, W=M, Cin=K, N=N, **kw)


# ---------------------------------------------------------------- the matrix
# Thresholds as read from conv_gemm_bf16 and the *_supported predicates: ring and stream from 2048 rows (8 RBM /
# 16 SBM), areg from 16384 (64 RB); stream K % 64 == 0, 192 <= K <= 768, its 128-column form for K <= 384 and
# N >= 128; ring N >= 96, prologue K <= kRingMaxK = 1024, fp32 out / post affine only for N > 128; the <= 16-row
# kernel takes whatever it supports BEFORE any bf16 dispatch (so a 1-row case reaches the register kernel only with a
# prologue, which the skinny kernel refuses); `big` tiles (BM 128) from 512 tiles of 128 rows.
def _bf16_cases():
    R, S, D, G, A = "gemm_ring", "gemm_stream", "gemm_dma", "gemm_bf16_reg", "gemm_areg"
    big = 255 * 128 + 10         # cdiv(M, 128) = 256 row tiles, x 2 column tiles = 512
    c = [
        lin("ring_narrow_ktail", R, 2085, 96, 72, pre=True),
        lin("ring_narrow_slice", R, 2085, 128, 640, lda=1024, a_coff=32, pre=True, act=RELU),
        lin("ring_wide_f32_maxk", R, 2085, 132, 1024, pre=True, out_bf16=False),
        lin("ring_wide_k1032", R, 2085, 256, 1032, act=SIGMOID),
        lin("ring_wide_post", R, 2085, 260, 512, post=True, act=RELU),
        lin("ring_wide_k448", R, 2085, 512, 448, act=SILU, alpha=False),
        lin("stream64_tail", S, 2049, 68, 192, act=RELU),
        lin("stream128_maxk", S, 2049, 132, 384, act=SIGMOID, out_bf16=False),
        lin("stream64_n128", S, 2049, 128, 448, lda=512, a_coff=32, act=SILU),
        lin("stream64_maxk", S, 2049, 96, 768, out_bf16=False),
        lin("stream64_glu", S, 2064, 64, 384, glu=True),
        lin("stream128_glu", S, 2064, 160, 384, glu=True),
        lin("areg_tail7", A, 16391, 768, 384, lda=400, a_coff=8, act=SILU),
        lin("areg_k192_sigmoid", A, 16391, 768, 192, act=SIGMOID, alpha=False),
        lin("areg_tiled_k192", A, 16400, 1536, 192, lda=192, a_tiled=True, act=RELU, out_bf16=False),
        lin("areg_tiled_glu", A, 16400, 768, 384, lda=384, a_tiled=True, glu=True),
        lin("dma_slice_pre", D, 700, 128, 256, lda=512, a_coff=64, pre=True, act=RELU),
        lin("dma_bn32_tails", D, 65, 36, 360, pre=True),
        lin("dma_res_bf16", D, 300, 130, 1536, res="bf16", act=SILU),
        lin("dma_res_f32_vec", D, 300, 132, 256, res="f32", act=RELU, out_bf16=False),   # the 4-column fast epilogue
        lin("dma_res_f32_tail", D, 300, 130, 256, res="f32", act=RELU),                 # rows of 138: the general one
        Case("dma_gate", D, B=2, W=250, Cin=128, N=64, gate_seg=100, gate_nseg=3),
        Case("dma_k3_dil2_pre_pad", D, B=2, W=70, Cin=128, N=32, kw=3, dw=2, pw=2, pre=True),
        Case("dma_k5_stride2", D, B=3, W=61, Cin=64, N=40, kw=5, sw=2, pw=2, act=RELU),
        Case("dma_3x3_cin64", D, B=2, H=9, W=20, Cin=64, N=40, kh=3, kw=3, sh=2, ph=1, pw=1, pre=True, act=RELU),
        # tall maps stay on this kernel when they carry a residual or a gate: its three 128-row tiles
        lin("dma_big_bn32", D, big, 36, 72, res="bf16"),
        Case("dma_big_bn64", D, B=2, W=big // 2, Cin=72, N=68, gate_seg=4000, gate_nseg=5, act=RELU),
        lin("dma_big_bn128", D, big, 132, 72, res="f32", out_bf16=False),
        lin("dma_clamp20", D, 333, 40, 136, act=CLAMP20),
        lin("reg_clamp20_route1", G, 333, 40, 136, act=CLAMP20, clamp_route=1),
        lin("dma_transposed", D, 333, 40, 72, transposed=True, out_bf16=False),
        lin("splitk_2048", "gemm_dma_splitk", 500, 256, 2048, alpha=False, splitk=True, out_bf16=False),
        lin("splitk_2056", "gemm_dma_splitk", 500, 256, 2056, alpha=False, splitk=True, out_bf16=False),
        # the register-staged kernel: fp32 A (rounded on staging -> random data only)
        lin("reg_f32a_64x32", G, 1, 4, 8, a_bf16=False, pre=True, modes=("random",)),
        lin("reg_f32a_64x128", G, 257, 130, 136, a_bf16=False, res="f32", out_bf16=False, modes=("random",)),
        lin("reg_f32a_64x128_tall", G, 4099, 132, 64, a_bf16=False, modes=("random",)),
        lin("reg_f32a_128x32", G, big, 36, 8, a_bf16=False, act=RELU, modes=("random",)),
        lin("reg_f32a_128x64", G, big, 68, 8, a_bf16=False, modes=("random",)),
        lin("reg_f32a_128x128", G, big, 132, 8, a_bf16=False, modes=("random",)),
        lin("reg_gelu", G, 200, 68, 96, act=GELU),
        lin("reg_gelu_tanh", G, 70, 36, 40, act=GELU_TANH, out_bf16=False),
        lin("reg_post_n128", G, 2085, 128, 64, post=True, act=RELU),
        Case("reg_3x3_cin32", G, B=2, H=10, W=21, Cin=32, N=40, kh=3, kw=3, sh=2, ph=1, pw=1, pre=True),
        lin("reg_res_f32", G, 257, 68, 136, a_bf16=False, res="f32", act=RELU),
        Case("reg_gate", G, B=2, W=250, Cin=72, N=36, a_bf16=False, gate_seg=100, gate_nseg=3),
        lin("reg_transposed", G, 333, 40, 72, a_bf16=False, transposed=True),
    ]
    return c


def _exact_cases():
    out = []
    big = 255 * 128 + 10
    for prec, kern in ((0, "conv_gemm_f32"), (2, "conv_gemm_bf16x3")):
        def f(name, M, N, K, **kw):
            return lin(f"p{prec}_{name}", kern, M, N, K, precision=prec, a_bf16=False, out_bf16=False, **kw)
        out += [
            f("res_relu", 70, 36, 40, res="f32", act=RELU),
            f("pre", 70, 36, 40, pre=True),
            f("clamp20", 70, 36, 40, act=CLAMP20),
            f("gelu", 70, 36, 40, act=GELU),
            f("gelu_tanh", 70, 36, 40, act=GELU_TANH),
            Case(f"p{prec}_gate_post_silu", kern, B=2, W=100, Cin=96, N=68, precision=prec, a_bf16=False,
                 out_bf16=False, gate_seg=40, gate_nseg=3, post=True, act=SILU),
            f("transposed_sigmoid", 300, 132, 64, transposed=True, act=SIGMOID),
            Case(f"p{prec}_k3_pre_pad", kern, B=2, W=35, Cin=32, N=36, kw=3, pw=1, pre=True, precision=prec,
                 a_bf16=False, out_bf16=False),
            # K 104 (3 k-tiles of 32 and a tail of 8): bf16x3 drops lo x lo and rounds both lo parts, up to 3 * 2^-18
            # per product by its format, which the fp32 bound 2^-23 (K + 16) S can hold only from K + 16 >= 96
            f("big_bn32", big, 36, 104, act=RELU),
            f("big_bn64", big, 68, 104, post=True),
            f("big_bn128", big, 132, 104, res="f32"),
        ]
    return out


def _skinny_cases():
    B, F = "gemm_skinny_bf16", "gemm_skinny_f32"

    def f(name, kern, M, N, K, **kw):
        kw.setdefault("a_bf16", False)
        return lin(name, kern, M, N, K, precision=1 if kern == B else 0, **kw)
    return [
        f("skinny_1x4x8", B, 1, 4, 8, out_bf16=False),
        f("skinny_16x4x8_f32w", F, 16, 4, 8, out_bf16=False, act=RELU),
        f("skinny_7x100x352_res", F, 7, 100, 352, res="f32"),
        f("skinny_7x100x352_abf", B, 7, 100, 352, a_bf16=True, out_bf16=False),
        f("skinny_16x256x352_res_bf16", B, 16, 256, 352, res="bf16", act=SILU),
        f("skinny_1x256x4864", B, 1, 256, 4864, out_bf16=False),
        f("skinny_1x100x4864_f32w", F, 1, 100, 4864, out_bf16=False),
        f("skinny_7x100x352_transposed", F, 7, 100, 352, transposed=True, out_bf16=False, act=SIGMOID),
        f("skinny_7x2052x8_nc4", F, 7, 2052, 8, out_bf16=False),
        # the k19 look-ahead conv of the streaming FS-EEND chunk: the taps are consecutive rows, so lda == Cin
        Case("skinny_k19_conv", B, W=26, Cin=256, N=256, kw=19, lda=256, a_bf16=False, out_bf16=False),
    ]


CASES = _bf16_cases() + _exact_cases() + _skinny_cases()
CASE_IDS = [f"{c.name}-{m}" for c in CASES for m in c.modes]
CASE_MODES = [(c, m) for c in CASES for m in c.modes]


# ---------------------------------------------------------------- data
def bf16r(x):
    """x rounded to fp32 and then to bf16 (RNE), as the kernels round their fp32 values; float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def f32r(x):
    return x.to(torch.float32).to(torch.float64)


def _pick(g, values, shape):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def make_data(case, mode):
    """Every tensor float64 and finite (the GPU test puts its NaN sentinels around them).  A: (B, H, W, lda), the
    columns outside the slice hold values too: the a_coff mutation of the host tests reads them."""
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.name}/{mode}".encode()))
    K, N, M = c.K, c.N, c.M
    d = {}
    if mode == "exact":
        e = 2.0 ** -math.floor(math.log2(K) / 2 + 0.5)
        d["A"] = torch.randint(-3, 4, (c.B, c.H, c.W, c.ld), generator=g).double()
        d["w"] = torch.randint(-2, 3, (N, c.Cin, c.kh, c.kw), generator=g).double() * e
        if c.pre:
            d["s"] = _pick(g, [0.5, 1.0, 2.0], (c.Cin,))
            d["h"] = _pick(g, [0.25, 0.5, 0.75, 1.0, 1.25, 1.5], (c.Cin,))
        # relu / clamp20 cases sit mostly above 0 so that a changed sum shows in the output; clamp20 spreads wider
        # (accumulators on both sides of [0, 20])
        off = {RELU: 8.0, CLAMP20: 10.0}.get(c.act, 0.0)
        # ... with a residual the sum sits below 0 and the residual lifts it above: act(x) + res != act(x + res)
        lift = 16.0 if c.res and c.act in (RELU, CLAMP20) else 0.0
        off -= lift
        if c.alpha:
            d["alpha"] = _pick(g, [2.0, 4.0, 8.0] if c.act == CLAMP20 else [0.5, 1.0, 2.0], (N,))
        if c.beta:
            d["beta"] = _pick(g, [-2.0, -1.25, -0.75, -0.25, 0.25, 0.5, 1.0, 1.75], (N,)) + off
        if c.res:
            d["res"] = torch.randint(-4, 5, (M, N), generator=g).double() + lift
        if c.post:
            d["post_s"] = _pick(g, [0.5, 1.0, 2.0], (N,))
            d["post_h"] = _pick(g, [-1.0, -0.25, 0.25, 0.75], (N,))
        if c.gate_seg:
            d["gate"] = _pick(g, [0.25, 0.5, 1.0, 2.0], (c.B, c.gate_nseg, N))
    else:
        A = torch.randn(c.B, c.H, c.W, c.ld, generator=g)
        d["A"] = (A.to(torch.bfloat16) if c.a_bf16 else A).double()
        d["w"] = (torch.randn(N, c.Cin, c.kh, c.kw, generator=g) / math.sqrt(K)).double()
        if c.pre:
            d["s"] = (torch.rand(c.Cin, generator=g) + 0.5).double()
            d["h"] = (torch.rand(c.Cin, generator=g) * 0.5 + 0.1).double()
        off = {RELU: 3.0, CLAMP20: 10.0}.get(c.act, 0.0)
        lift = 6.0 if c.res and c.act in (RELU, CLAMP20) else 0.0
        off -= lift
        if c.alpha:
            d["alpha"] = ((torch.rand(N, generator=g) + 0.5) * (8.0 if c.act == CLAMP20 else 1.0)).double()
        if c.beta:
            d["beta"] = (torch.randn(N, generator=g) * 0.1 + 0.3).double() + off
        if c.res:
            r = torch.randn(M, N, generator=g)
            d["res"] = ((r + lift).to(torch.bfloat16) if c.res == "bf16" else r + lift).double()
        if c.post:
            d["post_s"] = (torch.rand(N, generator=g) + 0.5).double()
            d["post_h"] = (torch.randn(N, generator=g) * 0.3).double()
        if c.gate_seg:
            d["gate"] = torch.sigmoid(torch.randn(c.B, c.gate_nseg, N, generator=g)).float().double()
    return d


# ---------------------------------------------------------------- layouts (kernels.h)
def tile_a(x, K):
    """Rows of K (rows % 16 == 0, K % 32 == 0) -> RowProgArgs::a_tiled's fragment layout: row 16 g + l, feature
    32 kk + 8 q + j at ((g K/32 + kk) 64 + l + 16 q) 8 + j."""
    r = x.reshape(-1, 16, K // 32, 4, 8)                 # (g, l, kk, q, j)
    return r.permute(0, 2, 3, 1, 4).contiguous().reshape(-1, K)


def out_shape(case):
    """Shape of the output allocation (with its sentinel rows / columns) and the four strides (o_sb, o_sh, o_sw, o_sn)."""
    c = case
    if c.transposed:                                     # (B, N, Wo) + a sentinel tail of PAD_ROWS rows of Wo
        assert c.Ho == 1
        return (c.B * c.N + PAD_ROWS, c.Wo), (c.N * c.Wo, 0, 1, c.Wo)
    ldo = c.n_out + PAD_COLS
    return (c.M + PAD_ROWS, ldo), (c.Ho * c.Wo * ldo, c.Wo * ldo, ldo, 1)


def out_view(case, buf):
    """The (M, n_out) block of the output allocation `buf` (shape out_shape), and a mask of the allocation's elements
    outside it."""
    c = case
    mask = torch.ones(buf.shape, dtype=torch.bool)
    if c.transposed:
        mask[:c.B * c.N] = False
        return buf[:c.B * c.N].reshape(c.B, c.N, c.Wo).permute(0, 2, 1).reshape(c.M, c.N), mask
    mask[:c.M, :c.n_out] = False
    return buf[:c.M, :c.n_out], mask


# ---------------------------------------------------------------- reference
def _act(x, act):
    if act == RELU:
        return x.clamp(min=0)
    if act == SIGMOID:
        return torch.sigmoid(x)
    if act == SILU:
        return x * torch.sigmoid(x)
    if act == CLAMP20:
        return x.clamp(0, 20)
    if act == GELU:
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))
    if act == GELU_TANH:
        return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    return x


def im2col(case, d, rows, mut=None):
    """(len(rows), K) float64: the A operand rows of output rows `rows`, prologue and operand rounding applied."""
    c = case
    A = d["A"]
    c0 = c.a_coff + (8 if mut == "acoff8" else 0)
    wo = rows % c.Wo
    t = rows // c.Wo
    ho, b = t % c.Ho, t // c.Ho
    cols = []
    for i in range(c.kh):
        for j in range(c.kw):
            hi, wi = ho * c.sh - c.ph + i * c.dh, wo * c.sw - c.pw + j * c.dw
            ok = (hi >= 0) & (hi < c.H) & (wi >= 0) & (wi < c.W)
            v = A[b, hi.clamp(0, c.H - 1), wi.clamp(0, c.W - 1), c0:c0 + c.Cin]
            if mut == "pre_pad":
                v = v * ok[:, None]                       # the pad read as 0 BEFORE the prologue
            if c.pre:
                v = f32r((v * d["s"] + d["h"]).clamp(min=0))
            if mut != "pre_pad":
                v = v * ok[:, None]
            cols.append(v)
    a = torch.cat(cols, 1)
    return bf16r(a) if c.bf16_operands else a


def weights(case, d):
    """(N, K) float64, tap-major, rounded as the kernel's packed weights are."""
    c = case
    w = d["w"].permute(0, 2, 3, 1).reshape(c.N, c.K)
    return bf16r(w) if c.precision == 1 else f32r(w)


def epilogue(case, d, acc, s_acc, rows, mut=None):
    """acc, s_acc: (R, N) products and their absolute-value sums -> (ref, S) of the linear + activation + post + gate
    epilogue (before any GLU)."""
    c = case
    N = c.N
    nn = (torch.arange(N) + 1) % N if mut == "ab_next" else torch.arange(N)
    x, s = acc, s_acc
    if c.alpha:
        x, s = x * d["alpha"][nn], s * d["alpha"][nn].abs()
    if c.beta:
        x, s = x + d["beta"][nn], s + d["beta"][nn].abs()
    if mut == "beta_slabs":
        x = x + d["beta"][nn]                             # a second slab carrying beta too
    if c.res:
        r = d["res"][rows]
        if mut == "act_first":
            x = _act(x, c.act) + r
        else:
            x = _act(x + r, c.act)
        s = s + r.abs()
    else:
        x = _act(x, c.act)
    if c.post:
        x, s = x * d["post_s"] + d["post_h"], s * d["post_s"].abs().clamp(min=1) + d["post_h"].abs()
    if c.gate_seg:
        wo = rows % c.Wo
        b = rows // (c.Wo * c.Ho)
        gt = d["gate"][b, wo // c.gate_seg]
        x, s = x * gt, s * gt.abs().clamp(min=1)
    return x, s


def reference(case, d, rows=None, mut=None):
    """(ref, tol) float64 (R, n_out) for output rows `rows` (default all): the unrounded reference and the per-element
    bound of the module docstring for random data (`tol_exact` gives the bound of exact data)."""
    c = case
    rows = torch.arange(c.M) if rows is None else rows
    a = im2col(c, d, rows, mut)
    w = weights(c, d)
    if mut == "drop_k8":
        a = a[:, :-8]
        w = w[:, :-8]
    acc = a @ w.t()
    s_acc = a.abs() @ w.abs().t()
    x, s = epilogue(c, d, acc, s_acc, rows, mut)
    E = 2.0 ** -23 * (c.K + 16) * s
    if c.glu:
        h = c.N // 2
        va, vg, Ea, Eg = x[:, :h], x[:, h:], E[:, :h], E[:, h:]
        x = va * torch.sigmoid(vg)
        E = Ea + va.abs() * Eg / 4                        # |d sigmoid| <= 1/4
    tol = E
    if c.out_bf16:
        tol = tol + 2.0 ** -8 * (x.abs() + E)
    if c.act in TRANSCENDENTAL or c.glu:
        tol = tol + FP32_ATOL + FP32_RTOL * x.abs()
    return x, tol


def tol_exact(case, ref):
    """The bound of `exact` data: 0 (bit for bit, after the RNE rounding of a bf16 output) unless the activation is
    transcendental."""
    c = case
    if not (c.act in TRANSCENDENTAL or c.glu):
        return torch.zeros_like(ref)
    tol = FP32_ATOL + FP32_RTOL * ref.abs()
    return tol + 2.0 ** -8 * (ref.abs() + tol) if c.out_bf16 else tol


def expected(case, mode, ref, tol):
    """(target, bound) the kernel output is compared with: exact data -> the reference rounded as the output is."""
    if mode == "exact":
        t = tol_exact(case, ref)
        if case.out_bf16 and not t.any():
            return bf16r(ref), t
        return ref, t
    return ref, tol


MUTATIONS = ("drop_k8", "acoff8", "ab_next", "act_first", "pre_pad", "beta_slabs")


def applies(case, mut, mode="exact"):
    """Whether the mutation can show in the case.  One exclusion by magnitude: with random data at K = 4864 the
    worst-case fp32 bound itself, 2^-23 (K + 16) S with S ~ 0.64 sqrt(K), is 0.03 while 8 of 4864 columns contribute
    sqrt(8 / K) = 0.04: that data cannot resolve 8 columns (the exact data of the same case does, bit for bit)."""
    c = case
    if mut == "drop_k8" and mode == "random" and c.K > 2056:
        return False
    if mut == "ab_next":
        return c.alpha or c.beta
    if mut == "act_first":
        return bool(c.res) and c.act != NONE
    if mut == "pre_pad":
        return c.pre and (c.ph > 0 or c.pw > 0)
    if mut == "beta_slabs":
        return c.splitk
    if mut == "acoff8":
        return c.ld >= c.a_coff + c.Cin + 8
    if mut == "drop_k8":
        return c.K > 8
    return True
