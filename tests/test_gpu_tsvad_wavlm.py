"""TS-VAD with the WavLM speech encoders on the raw waveform (speech_encoder_type "WavLM", variant 5, and
"WavLM_weight_sum" with wavlm_fuse_feat_post_norm, variant 6) on the MI355X path against the reference goldens
(tests/golden/make_golden_tsvad_wavlm.py, the reference MagicData TSVADModel).

Tolerances.  fp32: max|logit - golden| <= 1e-3 * max(1, max|golden|), the project's fp32 bar.  bf16: nobody had measured
this path; the maxima of one run are recorded per case in BF16_MEASURED and every case is bounded at twice the largest
(the convention of test_gpu_redimnet_emb.py).  The trunk's sharp seeded weights move layer outputs by about 0.28 at
|x| ~ 4 in bf16, so the 3e-2 cap of the other variants is not assumed.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from make_golden_tsvad_wavlm import CASES, NAN, RAISES, case_cfg, case_inputs  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.model import TSVADModel  # noqa: E402
from speaker_diarization_amd.ts_vad.pipeline import TSVADPipeline  # noqa: E402
from speaker_diarization_amd.ts_vad.windows import shard_batches  # noqa: E402
from speaker_diarization_amd.weights import to_torch, tsvad_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_RTOL = 1e-3
# bf16 (bf16 GEMM operands through the WavLM trunk, the head and the back end): max|logit - golden| of one run on an
# MI355X (max |logit| 0.88 .. 1.54)
BF16_MEASURED = {"tsvad_wavlm5_bp": 1.170e-2, "tsvad_wavlm5_rs4": 1.367e-2, "tsvad_wavlm5_pad2": 8.84e-3,
                 "tsvad_wavlm5_pad3": 9.04e-3, "tsvad_wavlm5_cut3": 8.28e-3, "tsvad_wavlm5_t1": 2.39e-3,
                 "tsvad_wavlm5_lg": 1.224e-2, "tsvad_wavlm6_bp": 1.271e-2, "tsvad_wavlm6_rs4": 1.798e-2,
                 "tsvad_wavlm6_pad3": 8.52e-3, "tsvad_wavlm6_lg": 1.645e-2, "tsvad_wavlm6_se256": 8.56e-3}
assert set(BF16_MEASURED) == set(CASES)
# 3.6e-2: above the 3e-2 cap of the other variants, below the smallest perturbation effect the golden generator
# recorded (zeroing wavlmproj.bias moves the Large goldens by 4.3e-2)
BF16_BOUND = 2 * max(BF16_MEASURED.values())
assert BF16_BOUND < 4.2e-2
_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(name, precision, gpu, max_batch=2):
    base = NAN[name][0] if name in NAN else name
    wseed = CASES[base][-1]
    v, geom, layers = CASES[base][:3]
    key = (v, geom["encoder_embed_dim"], layers, CASES[base][6], wseed, precision, max_batch)
    if key not in _models:
        cfg = case_cfg(base)
        m = TSVADModel(cfg, device=gpu, precision=precision, max_batch=max_batch)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)))
        _models[key] = m
    return _models[key]


def bar(g):
    return FP32_RTOL * max(1.0, float(np.abs(g).max()))


def inputs(name, gpu):
    (B, n, nl, wseed), wav, ts = case_inputs(name)
    return B, n, nl, torch.from_numpy(wav).to(gpu), torch.from_numpy(ts).to(gpu)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_vs_reference_golden(gpu, name, precision):
    B, n, nl, wav, ts = inputs(name, gpu)
    g = gold(name)["logits"]
    out = model(name, precision, gpu).forward(wav, ts, torch.zeros(B, 4, nl)).cpu().numpy()
    err = float(np.abs(out - g).max())
    print(f"{name} {precision}: max|logit diff| = {err:.3e} (|logit| max {np.abs(g).max():.3f})")
    assert out.shape == g.shape and np.isfinite(out).all()
    assert err <= (BF16_BOUND if precision == "bf16" else bar(g))


@pytest.mark.parametrize("base,nl", list(RAISES))
def test_label_lengths_beyond_three_frames_raise(gpu, base, nl):
    B, n, _, wav, ts = inputs(base, gpu)
    m = model(base, "fp32", gpu)
    gap = 5 - nl
    with pytest.raises(AssertionError, match=rf"label and ref_speech\(mix speech\) diff: {gap}, label len: {nl}"):
        m.forward(wav, ts, nl)
    g = gold(base)["logits"]                                   # the handle still works after a rejected call
    assert np.abs(m.forward(wav, ts, g.shape[-1]).cpu().numpy() - g).max() <= bar(g)


def test_rejected_calls_leave_the_handle_usable(gpu):
    name = "tsvad_wavlm5_bp"
    B, n, nl, wav, ts = inputs(name, gpu)
    m = model(name, "fp32", gpu)
    with pytest.raises(ValueError, match=r"expects the raw waveform \(B, n_samples\)"):
        m.forward(torch.zeros(B, 98, 80, device=gpu), ts, nl)
    with pytest.raises(ValueError, match="n_samples must be at least 400"):
        m.forward(torch.zeros(B, 396, device=gpu), ts, 1)
    with pytest.raises(ValueError, match="n_samples exceeds max_samples"):
        m.forward(torch.zeros(B, 64004, device=gpu), ts, 100)
    with pytest.raises(ValueError, match="bf16x3"):
        TSVADModel(case_cfg(name), device=gpu, precision="bf16x3", max_batch=1)
    g = gold(name)["logits"]
    assert np.abs(m.forward(wav, ts, nl).cpu().numpy() - g).max() <= bar(g)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_nan_window_bypasses_batchnorm(gpu, precision):
    name = "tsvad_wavlm5_nan"
    B, n, nl, wav, ts = inputs(name, gpu)
    bad = NAN[name][1]
    keep = [i for i in range(B) if i != bad]
    g, base = gold(name)["logits"], gold(NAN[name][0])["logits"]
    assert np.isnan(g[bad]).all() and np.isfinite(g[keep]).all()
    m = model(name, precision, gpu)
    tol = bar(g[keep]) if precision == "fp32" else BF16_BOUND
    out = m.forward(wav, ts, nl).cpu().numpy()
    assert np.isnan(out[bad]).all() and np.isfinite(out[keep]).all()
    print(f"nan {precision}: bypassed batch {np.abs(out[keep] - g[keep]).max():.3e}")
    assert np.abs(out[keep] - g[keep]).max() <= tol
    alone = m.forward(wav, ts, nl, forward_batch=1).cpu().numpy()
    assert np.isnan(alone[bad]).all()
    print(f"nan {precision}: forward_batch 1 {np.abs(alone[keep] - base[keep]).max():.3e}")
    assert np.abs(alone[keep] - base[keep]).max() <= tol
    if precision == "fp32":     # a reference batch wider than max_batch goes through _force
        one = model(name, precision, gpu, max_batch=1).forward(wav, ts, nl).cpu().numpy()
        assert np.isnan(one[bad]).all() and np.abs(one[keep] - g[keep]).max() <= tol


@pytest.mark.parametrize("name", ["tsvad_wavlm5_pad3", "tsvad_wavlm6_pad3"])
def test_batch_beyond_one_front_end_slice(gpu, name):
    """B = 9 windows of 3280 samples (the conv front end runs 8 at a time) against per-window forwards."""
    rng = np.random.default_rng(77)
    wav = torch.from_numpy((rng.standard_normal((9, 3280)) * 0.5).astype(np.float32)).to(gpu)
    ts = torch.from_numpy(rng.standard_normal((9, 4, 192)).astype(np.float32)).to(gpu)
    m = model(name, "fp32", gpu, max_batch=9)
    whole = m.forward(wav, ts, 5).cpu().numpy()
    each = np.concatenate([m.forward(wav[i:i + 1], ts[i:i + 1], 5).cpu().numpy() for i in range(9)])
    assert np.isfinite(whole).all() and np.abs(whole - each).max() <= bar(each)


@pytest.mark.parametrize("name", ["tsvad_wavlm5_bp", "tsvad_wavlm6_bp"])
def test_graph_replays_bit_identical(gpu, name):
    B, n, nl, wav, ts = inputs(name, gpu)
    m = model(name, "bf16", gpu)
    out = torch.empty(B, 4, nl, device=gpu)
    m.forward(wav, ts, nl, out=out)
    ref = out.clone()
    out.zero_()
    _lib.call("sd_tsvad_forward_graph", m._h, _lib.ptr(wav), _lib.ptr(ts), B, n, nl, _lib.ptr(out), 2, None,
              _lib.stream_ptr(gpu))
    m.status()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def test_strict_load(gpu):
    cfg = case_cfg("tsvad_wavlm6_bp")
    sd = to_torch(tsvad_state_dict(cfg, seed=1))
    sd.pop("wavlmproj.weight")
    with pytest.raises(RuntimeError, match="wavlmproj.weight"):
        TSVADModel(cfg, device=gpu, precision="fp32", max_batch=1).load_state_dict(sd)
    sd = to_torch(tsvad_state_dict(cfg, seed=1))
    sd["speech_down_or_up.0.weight"] = torch.zeros(192, 768, 5)
    with pytest.raises(RuntimeError, match=r"speech_down_or_up.0.weight must be \(speaker_embed_dim, 192, 5\)"):
        TSVADModel(cfg, device=gpu, precision="fp32", max_batch=1).load_state_dict(sd)


def test_pipeline_vs_per_window_forwards(gpu):
    """13 s + one label of seeded noise: windows of 100 labels shifted by 25, a 1-label tail window, reference batches
    of 4 (a batch boundary, and batches of different padded lengths); posteriors against per-window model calls
    assembled on the host, and the two-shard concatenation bit-identical to one rank."""
    name = "tsvad_wavlm6_bp"
    m = model(name, "fp32", gpu, max_batch=9)
    n_labels = 326
    rng = np.random.default_rng(123)
    wav = torch.from_numpy((rng.standard_normal(n_labels * 640) * 0.5).astype(np.float32)).to(gpu)
    ts = torch.from_numpy(rng.standard_normal((4, 192)).astype(np.float32)).to(gpu)
    pipe = TSVADPipeline(m, segment_shift=1, batch_size=4)
    plan = pipe.plan(n_labels)
    assert plan.lens[-1] == 1 and plan.n_win > 8
    logits = pipe.window_logits(wav, ts, plan)
    post = pipe.average(logits, plan).cpu().numpy()
    # per-window calls, each zero-padded to its reference batch's longest window as the collater does
    acc, cnt = np.zeros((4, n_labels)), np.zeros(n_labels)
    for b0, b1 in plan.batches(4):
        longest = int(plan.wave_n[b0:b1].max())
        for w in range(b0, b1):
            x = torch.zeros(1, longest, device=gpu)
            s, k = int(plan.wave_start[w]), int(plan.wave_n[w])
            x[0, :k] = wav[s:s + k]
            nl = int(plan.lens[b0:b1].max())
            lg = m.forward(x, ts[None], nl).cpu().numpy()[0]
            a, e = int(plan.starts[w]), int(plan.ends[w])
            acc[:, a:e] += 1.0 / (1.0 + np.exp(-lg[:, :e - a].astype(np.float64)))
            cnt[a:e] += 1
    want = acc / cnt
    err = float(np.abs(post - want).max())
    print(f"pipeline vs per-window forwards: max|posterior diff| = {err:.3e}")
    assert np.isfinite(post).all() and err <= 1e-3
    parts = []
    for rank in range(2):
        w0, w1 = shard_batches(plan, 4, 2, rank)
        parts.append(pipe.window_logits(wav, ts, plan, w0, w1))
    both = torch.cat(parts, 0)
    assert torch.equal(both.view(torch.int32), logits.view(torch.int32))
