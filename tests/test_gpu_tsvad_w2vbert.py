"""TS-VAD with the w2v-BERT 2.0 speech encoder (speech_encoder_type "w2v-bert2", variant 7) on the MI355X path against
the reference goldens (tests/golden/make_golden_w2vbert.py, the reference MagicData TSVADModel).

Tolerances.  fp32: max|logit - golden| <= 1e-3 * max(1, max|golden|), the project's fp32 bar.  bf16: derived on the CPU
before any GPU run: tests/w2vbert_ref.py's tsvad_forward with emulate_bf16=True (every GEMM / attention operand of the
trunk, the down conv and the back end rounded to bf16, fp32 accumulation) against the same goldens gives BF16_EMULATED
per case; every case is bounded at twice the largest.  BF16_MEASURED holds the GPU's maxima of one run beside them.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import w2vbert_ref as ref  # noqa: E402
from w2vbert_cases import NAN, RAISES, TSVAD, tsvad_cfg, tsvad_inputs  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.frontend import kaldi_fbank, window_cmn  # noqa: E402
from speaker_diarization_amd.ts_vad.model import TSVADModel  # noqa: E402
from speaker_diarization_amd.ts_vad.pipeline import TSVADPipeline  # noqa: E402
from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_RTOL = 1e-3
# max|logit - golden| of the CPU emulation of the bf16 mode (max |logit| 0.77 .. 1.98)
BF16_EMULATED = {"tsvad_w2vbert_t100": 7.247e-3, "tsvad_w2vbert_rs4": 7.830e-3, "tsvad_w2vbert_t22_l5": 6.857e-3,
                 "tsvad_w2vbert_t22_l6": 7.233e-3, "tsvad_w2vbert_t2": 3.087e-3, "tsvad_w2vbert_se256": 7.188e-3,
                 "tsvad_w2vbert_cut": 7.213e-3, "tsvad_w2vbert_nan": 5.384e-3}
assert set(BF16_EMULATED) == set(TSVAD) | set(NAN)
BF16_BOUND = 2 * max(BF16_EMULATED.values())      # 1.566e-2
# max|logit - golden| of one bf16 run on an MI355X
BF16_MEASURED = {"tsvad_w2vbert_t100": 6.983e-3, "tsvad_w2vbert_rs4": 6.982e-3,
                 "tsvad_w2vbert_t22_l5": 6.985e-3, "tsvad_w2vbert_t22_l6": 7.940e-3,
                 "tsvad_w2vbert_t2": 2.090e-3, "tsvad_w2vbert_se256": 7.014e-3, "tsvad_w2vbert_cut": 9.427e-3,
                 "tsvad_w2vbert_nan": 6.060e-3}
assert set(BF16_MEASURED) == set(BF16_EMULATED) and max(BF16_MEASURED.values()) <= BF16_BOUND
_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(name, precision, gpu, max_batch=2):
    base = NAN[name][0] if name in NAN else name
    key = TSVAD[base][3:6] + (TSVAD[base][7], precision, max_batch)
    if key not in _models:
        cfg = tsvad_cfg(base)
        m = TSVADModel(cfg, device=gpu, precision=precision, max_batch=max_batch)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=TSVAD[base][7])))
        _models[key] = m
    return _models[key]


def bar(g):
    return FP32_RTOL * max(1.0, float(np.abs(g).max()))


def inputs(name, gpu):
    (B, T, nl, wseed), x, ts = tsvad_inputs(name)
    return B, T, nl, torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(TSVAD))
def test_forward_vs_reference_golden(gpu, name, precision):
    B, T, nl, x, ts = inputs(name, gpu)
    g = gold(name)["logits"]
    out = model(name, precision, gpu).forward(x, ts, torch.zeros(B, 4, nl)).cpu().numpy()
    err = float(np.abs(out - g).max())
    print(f"{name} {precision}: max|logit diff| = {err:.3e} (|logit| max {np.abs(g).max():.3f})")
    assert out.shape == g.shape and np.isfinite(out).all()
    assert err <= (BF16_BOUND if precision == "bf16" else bar(g))


@pytest.mark.parametrize("base,nl", list(RAISES))
def test_label_lengths_beyond_three_frames_raise(gpu, base, nl):
    B, T, _, x, ts = inputs(base, gpu)
    m = model(base, "fp32", gpu)
    gap = ref.mix_frames(T) - nl
    with pytest.raises(AssertionError, match=rf"label and ref_speech\(mix speech\) diff: {gap}, label len: {nl}"):
        m.forward(x, ts, nl)
    g = gold(base)["logits"]                                   # the handle still works after a rejected call
    assert np.abs(m.forward(x, ts, g.shape[-1]).cpu().numpy() - g).max() <= bar(g)


def test_rejected_calls_leave_the_handle_usable(gpu):
    name = "tsvad_w2vbert_t100"
    B, T, nl, x, ts = inputs(name, gpu)
    m = model(name, "fp32", gpu)
    with pytest.raises(ValueError, match="even number of fbank frames.*is invalid for input of size"):
        m.forward(x[:, :99].contiguous(), ts, nl)
    with pytest.raises(ValueError, match="exceed max_fbank_frames"):
        m.forward(torch.zeros(B, 402, 80, device=gpu), ts, 100)
    with pytest.raises(ValueError, match="bf16x3"):
        TSVADModel(tsvad_cfg(name), device=gpu, precision="bf16x3", max_batch=1)
    g = gold(name)["logits"]
    assert np.abs(m.forward(x, ts, nl).cpu().numpy() - g).max() <= bar(g)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_nan_window_reaches_only_what_the_reference_lets_it_reach(gpu, precision):
    """A NaN in window 1: its logits are NaN, and the reference skips both BatchNorms for the whole batch (the golden);
    as a batch of its own (forward_batch 1) the other window is the NaN-free golden's."""
    name = "tsvad_w2vbert_nan"
    B, T, nl, x, ts = inputs(name, gpu)
    bad = NAN[name][1]
    keep = [i for i in range(B) if i != bad]
    g, base = gold(name)["logits"], gold(NAN[name][0])["logits"]
    assert np.isnan(g[bad]).all() and np.isfinite(g[keep]).all()
    m = model(name, precision, gpu)
    tol = bar(g[keep]) if precision == "fp32" else BF16_BOUND
    out = m.forward(x, ts, nl).cpu().numpy()
    assert np.isnan(out[bad]).all() and np.isfinite(out[keep]).all()
    print(f"nan {precision}: bypassed batch {np.abs(out[keep] - g[keep]).max():.3e}")
    assert np.abs(out[keep] - g[keep]).max() <= tol
    alone = m.forward(x, ts, nl, forward_batch=1).cpu().numpy()
    assert np.isnan(alone[bad]).all()
    print(f"nan {precision}: forward_batch 1 {np.abs(alone[keep] - base[keep]).max():.3e}")
    assert np.abs(alone[keep] - base[keep]).max() <= tol


def test_batch_compared_window_by_window(gpu):
    """Five windows of 66 frames in one call against one call each (fp32, the fp32 bar)."""
    rng = np.random.default_rng(78)
    x = torch.from_numpy(rng.standard_normal((5, 66, 80)).astype(np.float32)).to(gpu)
    ts = torch.from_numpy(rng.standard_normal((5, 4, 192)).astype(np.float32)).to(gpu)
    m = model("tsvad_w2vbert_t100", "fp32", gpu, max_batch=5)
    whole = m.forward(x, ts, 17).cpu().numpy()
    each = np.concatenate([m.forward(x[i:i + 1], ts[i:i + 1], 17).cpu().numpy() for i in range(5)])
    assert np.isfinite(whole).all() and np.abs(whole - each).max() <= bar(each)
    with pytest.raises(ValueError, match="exceeds max_batch"):
        out = torch.empty(6, 4, 17, device=gpu)
        _lib.call("sd_tsvad_forward", m._h, _lib.ptr(torch.zeros(6, 66, 80, device=gpu)),
                  _lib.ptr(torch.zeros(6, 4, 192, device=gpu)), 6, 66, 17, _lib.ptr(out), _lib.stream_ptr(gpu))


def test_default_depth_builds_and_loads_strictly(gpu):
    """select_encoder_layer_nums=6, the recipe's depth: builds, loads a reference-keyed state dict strictly, runs."""
    cfg = TSVADConfig(speech_encoder_type="w2v-bert2", select_encoder_layer_nums=6)
    sd = to_torch(tsvad_state_dict(cfg, seed=5))
    m = TSVADModel(cfg, device=gpu, precision="bf16", max_batch=1)
    m.load_state_dict(sd)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 22, 80)).astype(np.float32)).to(gpu)
    ts = torch.from_numpy(np.random.default_rng(6).standard_normal((1, 4, 192)).astype(np.float32)).to(gpu)
    assert torch.isfinite(m.forward(x, ts, 6)).all()
    sd.pop("speech_encoder.masked_spec_embed")
    with pytest.raises(RuntimeError, match="masked_spec_embed"):
        TSVADModel(cfg, device=gpu, precision="bf16", max_batch=1).load_state_dict(sd)


def test_pipeline_vs_restatement_window_by_window(gpu):
    """6 s + one label of seeded noise: windows of 100 labels shifted by 25 and a 1-label tail window (2 fbank frames),
    reference batches of 2; the pipeline's window logits against tests/w2vbert_ref.py applied to each window's fbank +
    CMN rows (taken from the same front end), zero-padded to its reference batch's longest as the collater does."""
    name = "tsvad_w2vbert_t100"
    m = model(name, "fp32", gpu, max_batch=4)
    cfg, wseed = tsvad_cfg(name), TSVAD[name][7]
    sd = to_torch(tsvad_state_dict(cfg, seed=wseed))
    n_labels = 151
    rng = np.random.default_rng(124)
    wav = torch.from_numpy((rng.standard_normal(n_labels * 640) * 0.5).astype(np.float32)).to(gpu)
    ts = torch.from_numpy(rng.standard_normal((4, 192)).astype(np.float32)).to(gpu)
    pipe = TSVADPipeline(m, segment_shift=1, batch_size=2)
    plan = pipe.plan(n_labels)
    assert plan.lens[-1] == 1 and plan.fbank_n[-1] == 2 and plan.n_win == 7 and (plan.fbank_n % 2 == 0).all()
    logits = pipe.window_logits(wav, ts, plan).cpu().numpy()
    feats = kaldi_fbank(wav, n_mels=80)
    worst = 0.0
    for b0, b1 in plan.batches(2):
        T_out, nl = int(plan.fbank_n[b0:b1].max()), int(plan.lens[b0:b1].max())
        fs = torch.from_numpy(plan.fbank_start[b0:b1].astype(np.int32)).to(gpu)
        fn = torch.from_numpy(plan.fbank_n[b0:b1].astype(np.int32)).to(gpu)
        rows = window_cmn(feats, fs, fn, T_out).cpu()
        want = ref.tsvad_forward(sd, cfg, rows, ts.cpu()[None].expand(b1 - b0, -1, -1), nl).numpy()
        got = logits[b0:b1, :, :nl]
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.abs(got - want).max() <= bar(want), (b0, b1)
        assert (logits[b0:b1, :, nl:] == 0).all()
    print(f"pipeline vs restatement, window by window: max|logit diff| = {worst:.3e}")
    post = pipe.posteriors(wav, ts, n_labels)
    assert post.shape == (4, n_labels) and torch.isfinite(post).all()
