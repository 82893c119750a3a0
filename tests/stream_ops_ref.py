"""Plain torch restatements of the FS-EEND streaming ops (csrc/stream_ops.hip), for the tests, and the cases both the
CPU and the GPU test run.  Restated from the contracts in csrc/kernels.h, not from the kernels: every function takes a
dtype (float64 is the yardstick, float32 the "same formula in torch float32" that sizes the fp32 bound) and works on
whole tensors with no tiling, no online softmax and no partials.

bf16: the caller hands in operands that are already bf16-representable (rb()) where the kernel reads bf16 (q / k / v,
the `t` operand, the weights); nothing else is rounded, as the fused kernels keep their intermediates in fp32.  The one
rounding of a bf16 output is the 2^-8 |ref element| term of bound_of(), so the reference's output stays unrounded.

`wrong=` selects a deliberately wrong implementation (test_stream_ops_host.py): the inputs of every case are chosen so
that each of them moves the result by at least 10 bounds.
"""
from __future__ import annotations

import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

HD = 64


def rb(x: torch.Tensor) -> torch.Tensor:
    """x rounded to bf16 (through float32, as a kernel's fp32 value is), in x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


# ---------------------------------------------------------------- bounds
def fp32_bound(ref64: torch.Tensor, ref32: torch.Tensor) -> float:
    """max(1e-5 max(1, max |ref|), 8 x the error of the same formula in torch float32)."""
    e32 = float((ref32.double() - ref64).abs().max())
    return max(1e-5 * max(1.0, float(ref64.abs().max())), 8.0 * e32)


def bound_of(ref64: torch.Tensor, ref32: torch.Tensor, bf16: bool) -> torch.Tensor:
    """Per-element bound: the fp32 bound, plus 2^-8 |ref element| for an output rounded to bf16."""
    b = torch.full_like(ref64, fp32_bound(ref64, ref32))
    return b + 2.0 ** -8 * ref64.abs() if bf16 else b


def worst(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> float:
    """Largest |got - want| / bound over the elements; a non-finite element counts as infinitely far."""
    d = (got.double() - want.double()).abs() / bound
    return float("inf") if not bool(torch.isfinite(d).all()) else float(d.max())


# ---------------------------------------------------------------- decode attention
def visible(pos: int, nq: int, delay: int, shift: int = 0) -> torch.Tensor:
    """(nq, pos + nq) bool: query i (at pos + i) sees key j iff j <= pos + i + delay (+ shift) and j < pos + nq."""
    i = torch.arange(nq)[:, None]
    j = torch.arange(pos + nq)[None, :]
    return j <= pos + i + delay + shift


def last_visible(pos: int, nq: int, delay: int, i: int) -> int:
    return min(pos + i + delay, pos + nq - 1)


def decode_attention(q, k, v, pos, scale, delay=0, dtype=torch.float64, wrong=None):
    """q (nseq, nq, nh, 64); k, v (nseq, >= pos + nq, nh, 64) -> (nseq, nq, nh, 64).
    wrong: ("drop", j) key j hidden from every query; ("drop_q", i, j) from query i; ("bound", +-1); ("heads",)."""
    nseq, nq, nh, _ = q.shape
    total = pos + nq
    q, k, v = q.to(dtype), k[:, :total].to(dtype), v[:, :total].to(dtype)
    vis = visible(pos, nq, delay, wrong[1] if wrong and wrong[0] == "bound" else 0)
    if wrong and wrong[0] == "drop":
        vis[:, wrong[1]] = False
    if wrong and wrong[0] == "drop_q":
        vis[wrong[1], wrong[2]] = False
    if wrong and wrong[0] == "heads":
        k = torch.roll(k, 1, dims=2)
        v = torch.roll(v, 1, dims=2)
    s = torch.einsum("sqhd,skhd->shqk", q, k) * scale
    s = s.masked_fill(~vis[None, None], float("-inf"))
    return torch.einsum("shqk,skhd->sqhd", torch.softmax(s, dim=-1), v)


def out_proj(o, w, b, dtype=torch.float64):
    """o (..., nh, 64) -> (..., nh * 64) = o W^T + b."""
    return F.linear(o.to(dtype).flatten(-2), w.to(dtype), b.to(dtype))


class AttnCase:
    def __init__(self, name, nseq, nh, nq, pos, delay=0, max_keys=256, layout="enc", big=False):
        self.name, self.nseq, self.nh, self.nq, self.pos, self.delay = name, nseq, nh, nq, pos, delay
        self.max_keys, self.layout, self.big = max_keys, layout, big
        self.total = pos + nq
        self.scale = 1.0 / math.sqrt(HD)

    def boundaries(self):
        """The keys on each side of a 64-tile and of a 256-block boundary (and, where a wave walks a second tile,
        of the 8192-key stride) that the history holds."""
        return [j for j in (63, 64, 255, 256, 8191, 8192) if j < self.total]

    def edges(self):
        lv0, lvn = last_visible(self.pos, self.nq, self.delay, 0), self.total - 1
        e = {0, lv0, lv0 + 1, lvn, *self.boundaries()}
        return sorted(j for j in e if 0 <= j < self.total)

    def wrongs(self):
        """The wrong implementations of this shape; one that leaves the visibility unchanged is no wrong one."""
        lv0 = last_visible(self.pos, self.nq, self.delay, 0)
        w = [("drop", 0), ("drop_q", 0, lv0), ("drop_q", self.nq - 1, self.total - 1)]
        w += [("drop", j) for j in self.boundaries()]
        w.append(("bound", -1))
        if not torch.equal(visible(self.pos, self.nq, self.delay, 1), visible(self.pos, self.nq, self.delay)):
            w.append(("bound", 1))
        if self.nh > 1:
            w.append(("heads",))
        return w

    def inputs(self, bf16: bool):
        """q, k, v (float32 tensors, bf16-representable when bf16), wo, bo.  Random operands alone leave an edge key
        one weight among thousands; here every query and every edge key share a direction u, so each edge key's logit
        sits about log(keys) + 2 above the rest and dropping it moves the output by far more than 10 bounds."""
        g = torch.Generator().manual_seed(zlib.crc32(self.name.encode()))
        rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
        nseq, nh, nq, total = self.nseq, self.nh, self.nq, self.total
        q, k, v = rn(nseq, nq, nh, HD), rn(nseq, total, nh, HD), rn(nseq, total, nh, HD)
        u = rn(nseq, 1, nh, HD)
        u = u / u.norm(dim=-1, keepdim=True)
        a = 4.0
        q = q + a * u
        lift = (math.log(total) + 2.0) / (a * self.scale)
        for j in self.edges():
            k[:, j] += lift * u[:, 0]
            v[:, j] *= 2.0
        if self.big:      # the last key (visible to the last query only): a logit about 30 times the others'
            k[:, total - 1] = 30.0 / (a * self.scale) * u[:, 0]
        D = nh * HD
        wo, bo = rn(D, D) / math.sqrt(D), rn(D) * 0.1
        if bf16:
            q, k, v, wo = rb(q), rb(k), rb(v), rb(wo)
        return q, k, v, wo, bo


ATTN_CASES = [
    AttnCase("one_key", 1, 4, 1, 0),
    AttnCase("k63", 1, 3, 2, 61),
    AttnCase("k64_delay", 1, 4, 8, 56, delay=2),
    AttnCase("k65_slots", 6, 1, 9, 56, layout="dec"),
    AttnCase("k255", 1, 4, 32, 223, max_keys=512),
    AttnCase("k256", 1, 3, 1, 255, max_keys=512),
    AttnCase("k257_delay", 6, 4, 8, 249, delay=2, max_keys=512),
    AttnCase("hollow_blocks", 6, 4, 8, 62, max_keys=2048, layout="dec"),
    AttnCase("two_tiles_per_wave", 1, 1, 9, 8291, max_keys=8448),
    AttnCase("two_tiles_one_query", 1, 1, 1, 8299, max_keys=8448),
    AttnCase("big_logit", 1, 4, 8, 592, max_keys=1024, big=True),
]


# ---------------------------------------------------------------- LayerNorm'd blocks
def layer_norm(x, g, b, eps):
    m = x.mean(-1, keepdim=True)
    var = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(var + eps) * g + b


def ln_add(x, t, g, b, eps, dtype):
    x = x.to(dtype) if t is None else x.to(dtype) + t.to(dtype)
    return layer_norm(x, g.to(dtype), b.to(dtype), eps)


def slot_block(x, t, g, b, w_in, b_in, w_out, b_out, c, C, nh, scale, eps=1e-5, dtype=torch.float64, wrong=None):
    """y = LN(x + t); qkv = y W_in^T + b_in; softmax over the C slots of the same frame, per head; out = o W_out^T +
    b_out.  Rows (c C, D) in (frame, slot) order.  Returns (out, y).
    wrong: "neighbour_frame", "k_half" (only the first half of the in-projection's K summed), "heads_short" (the last
    head's out-projection partial left out), "scale_twice" (scale on k as well as on q)."""
    n, D = c * C, x.shape[-1]
    hd = D // nh
    y = ln_add(x, t, g, b, eps, dtype)
    w_in, w_out = w_in.to(dtype), w_out.to(dtype)
    if wrong == "k_half":
        w_in = w_in.clone()
        w_in[:, D // 2:] = 0
    qkv = F.linear(y, w_in, b_in.to(dtype))
    q, k, v = (a.reshape(c, C, nh, hd) for a in qkv.split(D, dim=-1))
    if wrong == "neighbour_frame":
        k, v = torch.roll(k, -1, dims=0), torch.roll(v, -1, dims=0)
    s = torch.einsum("fihd,fjhd->fhij", q, k) * (scale * scale if wrong == "scale_twice" else scale)
    o = torch.einsum("fhij,fjhd->fihd", torch.softmax(s, dim=-1), v)
    if wrong == "heads_short":
        o = o.clone()
        o[:, :, nh - 1] = 0
    return F.linear(o.reshape(n, D), w_out, b_out.to(dtype)), y


def ffn_pair(x, t, g, b, w1, b1, w2, b2, eps=1e-5, dtype=torch.float64):
    """y = LN(x + t); out = relu(y W1^T + b1) W2^T + b2.  Returns (out, y)."""
    y = ln_add(x, t, g, b, eps, dtype)
    h = torch.relu(F.linear(y, w1.to(dtype), b1.to(dtype)))
    return F.linear(h, w2.to(dtype), b2.to(dtype)), y


def dec_scores(x, t, g, b, emb, C, eps=1e-5, dtype=torch.float64):
    """a = LN(x + t) over the (frame, slot) rows; scores[f, s] = emb[f] . a / |a|."""
    a = ln_add(x, t, g, b, eps, dtype)
    e = emb.to(dtype).repeat_interleave(C, dim=0)
    return (e * a).sum(-1) / a.norm(dim=-1)


def gather_window(hist, cursor, n_valid, pad, rows):
    """rows [cursor - pad, cursor - pad + rows) of hist, zero outside [0, n_valid)."""
    out = torch.zeros(rows, hist.shape[1], dtype=hist.dtype)
    for r in range(rows):
        s = cursor - pad + r
        if 0 <= s < n_valid:
            out[r] = hist[s]
    return out


# (c, C) -> n = 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16: every NR of slot_block_kernel and its LayerNorm rows past 8
SLOT_SHAPES = [(1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (1, 6), (1, 7), (1, 8), (2, 4), (3, 3), (2, 6), (5, 3), (2, 8),
               (4, 4)]
# (t, weights, out): None = no t operand, else bf16 or not
SLOT_DTYPES = [(None, False, False), (False, False, False), (True, True, True), (True, False, True),
               (False, True, False)]
SLOT_WRONGS = ("neighbour_frame", "k_half", "heads_short", "scale_twice")
FFN_ROWS = [1, 2, 3, 4, 7, 8]


def block_inputs(n, seed, t_mode, w_bf16, kind, F_=2048, D=256):
    """Operands of a slot block (kind "slot") or an FFN pair ("ffn") on n rows, as float32 tensors that are
    bf16-representable where the kernel reads bf16.  The in-projection is scaled so the slot logits spread over
    several units (a uniform softmax would hide a wrong key), and a quarter of the FFN's hidden units are biased far
    negative so relu kills them."""
    g_ = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g_)   # noqa: E731
    d = {"x": rn(n, D) * 1.5, "t": None if t_mode is None else rn(n, D),
         "g": 1 + 0.1 * rn(D), "b": 0.1 * rn(D)}
    if kind == "slot":
        d.update(w_in=rn(3 * D, D) * 2 / math.sqrt(D), b_in=0.1 * rn(3 * D), w_out=rn(D, D) / math.sqrt(D),
                 b_out=0.1 * rn(D))
        ws = ("w_in", "w_out")
    else:
        b1 = 0.1 * rn(F_)
        b1[::4] -= 50.0
        d.update(w1=rn(F_, D) / math.sqrt(D), b1=b1, w2=rn(D, F_) / math.sqrt(F_), b2=0.1 * rn(D))
        ws = ("w1", "w2")
    if t_mode:
        d["t"] = rb(d["t"])
    if w_bf16:
        for k in ws:
            d[k] = rb(d[k])
    return d


def np32(x):
    return np.ascontiguousarray(x.detach().cpu().numpy(), np.float32)
