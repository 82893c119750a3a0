"""The w2v-BERT 2.0 trunk (speaker_diarization_amd.ssl.W2vBert, sd_w2vbert_*) on the MI355X path against the goldens of
transformers' Wav2Vec2BertModel (tests/golden/make_golden_w2vbert.py).

Tolerances.  fp32: max|x - golden| <= 1e-3 * max(1, max|golden|), the project's fp32 bar.  bf16: the bound was derived on
the CPU before any GPU run: tests/w2vbert_ref.py with emulate_bf16=True (every GEMM / attention operand rounded to bf16,
fp32 accumulation) against the same goldens gives BF16_EMULATED per case, and every case is bounded at twice the largest
(the project's margin for an error model).  BF16_MEASURED holds the GPU's maxima of one run beside them.  The errors
are those of a trunk whose seeded attention is sharp on purpose (scores of standard deviation ~3), on outputs of max
|x| ~ 4 .. 6.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import w2vbert_ref as ref  # noqa: E402
from w2vbert_cases import TRUNK, keep_frames, trunk_config, trunk_input  # noqa: E402
from speaker_diarization_amd.ssl import W2vBert  # noqa: E402
from speaker_diarization_amd.weights import to_torch, w2vbert_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_RTOL = 1e-3
# max|x - golden| of the CPU emulation of the bf16 mode (w2vbert_ref.trunk(..., emulate_bf16=True)), on the stored frames
BF16_EMULATED = {"w2vbert_t1": 1.818e-2, "w2vbert_t11": 4.163e-2, "w2vbert_t66": 3.579e-2, "w2vbert_t200": 3.514e-2}
assert set(BF16_EMULATED) == set(TRUNK)
BF16_BOUND = 2 * max(BF16_EMULATED.values())      # 8.33e-2
# max|x - golden| of one bf16 run on an MI355X
BF16_MEASURED = {"w2vbert_t1": 1.861e-2, "w2vbert_t11": 3.438e-2, "w2vbert_t66": 3.534e-2, "w2vbert_t200": 3.550e-2}
_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(layers, wseed, precision, gpu, max_batch=2, max_frames=200):
    key = (layers, wseed, precision, max_batch, max_frames)
    if key not in _models:
        m = W2vBert(trunk_config(layers), device=gpu, precision=precision, max_batch=max_batch, max_frames=max_frames)
        m.load_state_dict(to_torch(w2vbert_state_dict(trunk_config(layers), wseed)))
        _models[key] = m
    return _models[key]


def bar(g):
    return FP32_RTOL * max(1.0, float(np.abs(g).max()))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(TRUNK))
def test_forward_vs_reference_golden(gpu, name, precision):
    layers, B, T2, _, wseed, every = TRUNK[name]
    g = gold(name)
    frames = keep_frames(T2)
    x = torch.from_numpy(trunk_input(name)).to(gpu)
    m = model(layers, wseed, precision, gpu)
    out = m(x, output_hidden_states=True)
    assert len(out.hidden_states) == layers + 1 and torch.equal(out.hidden_states[-1], out.last_hidden_state)
    assert torch.equal(m(x), out.last_hidden_state)
    got = out.last_hidden_state.cpu().numpy()[:, frames]
    assert got.shape == g["x"].shape and np.isfinite(got).all()
    err = float(np.abs(got - g["x"]).max())
    cos = float((got * g["x"]).sum() / np.sqrt((got * got).sum() * (g["x"] * g["x"]).sum()))
    print(f"{name} {precision}: max|x diff| = {err:.3e} (|x| max {np.abs(g['x']).max():.3f}) cosine {cos:.6f}")
    assert err <= (BF16_BOUND if precision == "bf16" else bar(g["x"]))
    assert cos >= 0.99
    if every:
        for i, h in enumerate(out.hidden_states):
            e = float(np.abs(h.cpu().numpy()[:, frames] - g[f"layer_{i}"]).max())
            print(f"  hidden_states[{i}]: {e:.3e}")
            assert e <= (BF16_BOUND if precision == "bf16" else bar(g[f"layer_{i}"]))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_batch_compared_window_by_window(gpu, precision):
    """Five windows of 33 frames (three 16-frame conv tiles, three query tiles) in one call against one call each.  No
    kernel of the trunk mixes windows; the GEMM kernel that serves a shape may change with the row count, so the two
    are held to the precision's bar, not to bit equality."""
    layers, wseed = 2, TRUNK["w2vbert_t11"][4]
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((5, 33, 160)).astype(np.float32)).to(gpu)
    m = model(layers, wseed, precision, gpu, max_batch=5, max_frames=40)
    whole = m(x).cpu().numpy()
    each = np.concatenate([m(x[i:i + 1]).cpu().numpy() for i in range(5)])
    assert np.isfinite(whole).all()
    err = float(np.abs(whole - each).max())
    print(f"batch of 5 vs window by window, {precision}: {err:.3e}")
    assert err <= (BF16_BOUND if precision == "bf16" else bar(each))
    if precision == "fp32":
        want = ref.trunk(to_torch(w2vbert_state_dict(trunk_config(layers), wseed)), layers, x.cpu())[-1].numpy()
        assert np.abs(whole - want).max() <= bar(want)


def test_refusals_leave_the_handle_usable(gpu):
    layers, B, T2, _, wseed, _ = TRUNK["w2vbert_t11"]
    m = model(layers, wseed, "fp32", gpu)
    x = torch.from_numpy(trunk_input("w2vbert_t11")).to(gpu)
    with pytest.raises(ValueError, match="exceeds max_batch"):
        m(torch.zeros(3, 11, 160, device=gpu))
    with pytest.raises(ValueError, match="exceed max_frames"):
        m(torch.zeros(1, 201, 160, device=gpu))
    with pytest.raises(ValueError, match=r"expected \(B, T2, 160\)"):
        m(torch.zeros(1, 11, 80, device=gpu))
    with pytest.raises(ValueError, match="attention_mask"):
        m(x, attention_mask=torch.ones(B, T2))
    g = gold("w2vbert_t11")
    got = m(x).cpu().numpy()[:, keep_frames(T2)]
    assert np.abs(got - g["x"]).max() <= bar(g["x"])
    assert m.device_bytes > 2 * 30e6          # two layers of 30 M fp32 weights at least


def test_strict_load(gpu):
    cfg = trunk_config(2)
    sd = to_torch(w2vbert_state_dict(cfg, 1))
    sd.pop("encoder.layers.1.self_attn.distance_embedding.weight")
    with pytest.raises(RuntimeError, match="distance_embedding.weight"):
        W2vBert(cfg, device=gpu, precision="fp32", max_batch=1, max_frames=8).load_state_dict(sd)
    sd = to_torch(w2vbert_state_dict(cfg, 1))
    sd["encoder.layers.0.conv_module.depthwise_conv.weight"] = torch.zeros(1024, 1, 15)
    with pytest.raises(RuntimeError, match=r"depthwise_conv.weight must be \(1024,1,31\)"):
        W2vBert(cfg, device=gpu, precision="fp32", max_batch=1, max_frames=8).load_state_dict(sd)
    sd = to_torch(w2vbert_state_dict(trunk_config(3), 1))      # a deeper checkpoint: unexpected keys
    with pytest.raises(RuntimeError, match=r"encoder.layers.2"):
        W2vBert(cfg, device=gpu, precision="fp32", max_batch=1, max_frames=8).load_state_dict(sd)
