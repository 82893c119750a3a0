"""CPU checks of what tests/test_gpu_stream_ops.py relies on: no GPU is needed.

1. The float64 restatements in stream_ops_ref.py satisfy the streaming identity: decode attention run chunk by chunk
   against the history, and the slot block, equal oracle/fseend_ref.py's whole-sequence causal attention / fusion layer.
2. The inputs of every GPU case are sharp enough: each wrong implementation of the issue's list (a dropped edge key, a
   causal bound off by one, swapped heads; a neighbouring frame's slots, a half in-projection, a missing head partial,
   a doubled scale) moves the float64 result by at least 10 bounds of that case's dtype at the worst element.  This is a
   condition on the inputs, not on the kernels.  ("scale applied to k" instead of q is the same function, q . k scale
   either way, so the wrong implementation used here is the scale on k as well as on q.)
3. The C ABI refuses, before any launch, the arguments the kernels do not take.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_ops_ref as ref  # noqa: E402
from oracle import fseend_ref  # noqa: E402
from oracle.tsvad_ref import mha  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402


def _mha_sd(D, seed):
    g = torch.Generator().manual_seed(seed)
    return {"a.in_proj_weight": torch.randn(3 * D, D, generator=g, dtype=torch.float64) * 2 / D ** 0.5,
            "a.in_proj_bias": torch.randn(3 * D, generator=g, dtype=torch.float64) * 0.1,
            "a.out_proj.weight": torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5,
            "a.out_proj.bias": torch.randn(D, generator=g, dtype=torch.float64) * 0.1}


@pytest.mark.parametrize("chunk,delay", [(1, 0), (3, 0), (5, 0), (14, 0), (14, 2)])
def test_chunked_decode_attention_is_the_causal_forward(chunk, delay):
    T, nh, D = 14, 4, 256
    sd = _mha_sd(D, 11)
    x = torch.randn(T, 1, D, generator=torch.Generator().manual_seed(12), dtype=torch.float64)
    want = mha(x, sd, "a.", nh, causal_mask=fseend_ref.causal_mask(T, delay).double())[:, 0]
    qkv = torch.nn.functional.linear(x[:, 0], sd["a.in_proj_weight"], sd["a.in_proj_bias"])
    q, k, v = (a.reshape(1, T, nh, 64) for a in qkv.split(D, dim=-1))
    got = torch.empty(T, D, dtype=torch.float64)
    for pos in range(0, T, chunk):
        nq = min(chunk, T - pos)
        o = ref.decode_attention(q[:, pos:pos + nq], k, v, pos, 0.125, delay)      # the history holds keys < pos + nq
        got[pos:pos + nq] = ref.out_proj(o, sd["a.out_proj.weight"], sd["a.out_proj.bias"])[0]
    assert (got - want).abs().max() < 1e-12


def test_slot_block_is_the_fusion_layers_slot_attention():
    c, C, nh, D = 3, 5, 4, 256
    sd = _mha_sd(D, 21)
    g = torch.Generator().manual_seed(22)
    x, t = (torch.randn(c * C, D, generator=g, dtype=torch.float64) for _ in range(2))
    lg, lb = 1 + 0.1 * torch.randn(D, generator=g, dtype=torch.float64), 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    out, y = ref.slot_block(x, t, lg, lb, sd["a.in_proj_weight"], sd["a.in_proj_bias"], sd["a.out_proj.weight"],
                            sd["a.out_proj.bias"], c, C, nh, 0.125)
    y_want = torch.nn.functional.layer_norm(x + t, (D,), lg, lb, 1e-5)
    want = fseend_ref._mha_bf(y_want.reshape(c, C, D), sd, "a.", nh).reshape(c * C, D)
    assert (y - y_want).abs().max() < 1e-12 and (out - want).abs().max() < 1e-12


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", ref.ATTN_CASES, ids=lambda c: c.name)
def test_attn_inputs_expose_every_wrong_implementation(case, bf16):
    q, k, v, wo, bo = case.inputs(bf16)
    r64 = ref.decode_attention(q, k, v, case.pos, case.scale, case.delay)
    r32 = ref.decode_attention(q, k, v, case.pos, case.scale, case.delay, torch.float32)
    bound = ref.bound_of(r64, r32, bf16)
    wrongs = case.wrongs()
    assert ("bound", -1) in wrongs and ("drop", 0) in wrongs
    for w in wrongs:
        bad = ref.decode_attention(q, k, v, case.pos, case.scale, case.delay, wrong=w)
        moved = ref.worst(ref.rb(bad) if bf16 else bad, r64, bound)
        print(f"{case.name} {'bf16' if bf16 else 'fp32'} {w}: {moved:.1f} bounds")
        assert moved >= 10, (case.name, w, moved)


@pytest.mark.parametrize("modes", ref.SLOT_DTYPES, ids=str)
@pytest.mark.parametrize("c,C", ref.SLOT_SHAPES)
def test_slot_inputs_expose_every_wrong_implementation(c, C, modes):
    t_mode, w_bf16, out_bf16 = modes
    d = ref.block_inputs(c * C, 100 * c + C, t_mode, w_bf16, "slot")
    args = (d["x"], d["t"], d["g"], d["b"], d["w_in"], d["b_in"], d["w_out"], d["b_out"], c, C, 4, 0.125)
    r64, _ = ref.slot_block(*args)
    r32, _ = ref.slot_block(*args, dtype=torch.float32)
    bound = ref.bound_of(r64, r32, out_bf16)
    for w in ref.SLOT_WRONGS:
        if w == "neighbour_frame" and c == 1:
            continue      # one frame has no neighbour
        if w == "scale_twice" and C == 1:
            continue      # one slot: the softmax is 1 whatever the logit
        bad, _ = ref.slot_block(*args, wrong=w)
        moved = ref.worst(ref.rb(bad) if out_bf16 else bad, r64, bound)
        print(f"slot ({c}, {C}) {'bf16' if out_bf16 else 'fp32'} {w}: {moved:.1f} bounds")
        assert moved >= 10, (c, C, w, moved)


# ---------------------------------------------------------------- refusals that need no device
def _i():
    return ctypes.c_int(-1)


def test_attn_decode_refuses_before_launching():
    a = 4096      # never dereferenced: every call below fails its argument check first
    ok = dict(q=a, q_tok=768, q_seq=0, k=a, v=a, kv_tok=512, kv_seq=0, out=a, o_tok=256, o_seq=0, nseq=1, nq=1, nh=4,
              scale=0.125, pos=a, delay=0, max_keys=256, bf=0, ws=a, n_blocks=1, cnt=None, wo=None, bo=None, o2=None,
              ws2=None, cnt2=None)

    def call(match, **kw):
        p = dict(ok, **kw)
        flag = _i()
        with pytest.raises(ValueError, match=match):
            _lib.call("sd_op_attn_decode", *p.values(), ctypes.byref(flag), None)
        assert flag.value in (-1, 0)

    call("null argument", q=None)
    call("null argument", pos=None)
    call("null argument", ws=None)
    call("1..32 queries", nq=0)
    call("1..32 queries", nq=33)
    call("workspace too small", max_keys=2048, n_blocks=7)
    call("bad argument", delay=-1)
    call("bad argument", max_keys=0)
    call("16-byte", k=a + 4)
    call("16-byte", kv_tok=514)
    call("together", wo=a)      # an out-projection without its counters
    assert _lib.load().sd_attn_decode_blocks(1) == 1 and _lib.load().sd_attn_decode_blocks(0) == 0


def test_fused_blocks_refuse_before_launching():
    a = 4096
    slot = dict(ln_x=a, ln_t=None, t_bf16=0, g=a, b=a, eps=1e-5, ln_out=a, w_in=a, b_in=a, w_out=a, b_out=a, w_bf16=0,
                out=a, out_bf16=0, ws=a, cnt=a, c=1, C=6, D=256, nh=4, scale=0.125)

    def refused(name, base, **kw):
        ran = _i()
        _lib.call(name, *dict(base, **kw).values(), ctypes.byref(ran), None)
        assert ran.value == 0      # the caller's fall-back path runs instead

    for kw in (dict(D=512, nh=8), dict(c=17, C=1), dict(c=1, C=9), dict(ws=None), dict(cnt=None), dict(nh=2),
               dict(ln_x=a + 4), dict(g=a + 8), dict(b=a + 4), dict(ln_out=a + 4), dict(w_in=a + 4), dict(w_out=a + 8),
               dict(ln_t=a + 4), dict(ln_t=a + 4, t_bf16=1)):
        refused("sd_op_stream_slot_block", slot, **kw)
    with pytest.raises(ValueError, match="null argument"):
        _lib.call("sd_op_stream_slot_block", *dict(slot, w_in=None).values(), ctypes.byref(_i()), None)
    ffn = dict(ln_x=a, ln_t=None, t_bf16=0, g=a, b=a, eps=1e-5, ln_out=a, w1=a, b1=a, w2=a, b2=a, w_bf16=0, out=a,
               out_bf16=0, ws=a, cnt=a, n=1, D=256, F=2048)
    for kw in (dict(n=9), dict(n=0), dict(F=1024), dict(D=512), dict(w1=a + 4), dict(w2=a + 4), dict(ws=None),
               dict(cnt=None)):
        refused("sd_op_stream_ffn_pair", ffn, **kw)


def test_copies_and_finishers_refuse_before_launching():
    a = 4096
    with pytest.raises(ValueError, match="16-byte multiples"):
        _lib.call("sd_op_kv_append", a, 1024, 2, 24, a, 1024, a, 1, None)
    with pytest.raises(ValueError, match="unaligned"):
        _lib.call("sd_op_kv_append", a + 8, 1024, 2, 32, a, 1024, a, 1, None)
    with pytest.raises(ValueError, match="bad argument"):
        _lib.call("sd_op_kv_append", a, 16, 2, 32, a, 1024, a, 1, None)
    with pytest.raises(ValueError, match="null argument"):
        _lib.call("sd_op_gather_window", a, 256, None, a, 9, 19, a, None)
    with pytest.raises(ValueError, match="null argument"):
        _lib.call("sd_op_cursor_advance", None, 1, None, None)
    for D in (0, 128, 320, 1280):
        with pytest.raises(ValueError, match="256/512/768/1024"):
            _lib.call("sd_op_stream_enc_finish", a, None, 0, a, a, 1e-5, 1, D, a, a, None, None)
        with pytest.raises(ValueError, match="256/512/768/1024"):
            _lib.call("sd_op_stream_dec_finish", a, None, 0, a, a, 1e-5, 1, 6, D, a, a, a, None)
