"""TS-VAD with the ReDimNetB2 speech encoder (speech_encoder_type "ReDimNetB2", variant 4) on the MI355X path against
the reference goldens (tests/golden/make_golden_redimnet.py, the reference MagicData TSVADModel) and the CPU
restatement (tests/redimnet_ref.py).

Tolerances.  fp32 and bf16x3: max|logit - golden| <= 1e-3 * max(1, max|golden|), the project's fp32 bar.  bf16: the maxima
of one run are recorded per case in BF16_MEASURED and every case is bounded at twice the largest.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from make_golden_redimnet import SE_TYPE, TSVAD_CASES, TSVAD_NAN, TSVAD_RAISES, tsvad_inputs72  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.model import TSVADModel  # noqa: E402
from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = TSVADConfig(speech_encoder_type=SE_TYPE)
FP32_RTOL = 1e-3
# bf16 (bf16 maps through the trunk, then the bf16 back end): max|logit - golden| of one run on an MI355X
# (max |logit| 0.68 .. 1.63)
BF16_MEASURED = {"tsvad_redimnet_gap0": 8.24e-3, "tsvad_redimnet_rs4": 9.00e-3, "tsvad_redimnet_pad2": 1.05e-2,
                 "tsvad_redimnet_pad3": 9.10e-3, "tsvad_redimnet_cut3": 8.65e-3}
assert 2 * max(BF16_MEASURED.values()) < 3e-2   # the project's loosest bf16 bound
_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(wseed, precision, gpu, cfg=CFG):
    key = (wseed, precision, cfg.speaker_embed_dim)
    if key not in _models:
        m = TSVADModel(cfg, device=gpu, precision=precision, max_batch=2)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)))
        _models[key] = m
    return _models[key]


def bar(g):
    return FP32_RTOL * max(1.0, float(np.abs(g).max()))


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("name", list(TSVAD_CASES))
def test_forward_vs_reference_golden(gpu, name, precision):
    """gap 0, the rs_len 4 window, pad 2, pad 3 and cut 3 of the MagicData length rule."""
    (B, T, nl, _, wseed), x, ts = tsvad_inputs72(name)
    g = gold(name)["logits"]
    m = model(wseed, precision, gpu)
    out = m.forward(torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu), torch.zeros(B, 4, nl)).cpu().numpy()
    err = float(np.abs(out - g).max())
    print(f"{name} {precision}: max|logit diff| = {err:.3e} (|logit| max {np.abs(g).max():.3f})")
    assert out.shape == g.shape and np.isfinite(out).all()
    assert err <= (2 * max(BF16_MEASURED.values()) if precision == "bf16" else bar(g))


@pytest.mark.parametrize("base,nl", list(TSVAD_RAISES))
def test_label_lengths_beyond_three_frames_raise(gpu, base, nl):
    (B, T, _, _, wseed), x, ts = tsvad_inputs72(base)
    m = model(wseed, "fp32", gpu)
    xd, tsd = torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu)
    gap = (T - 1) // 4 + 1 - nl
    with pytest.raises(AssertionError, match=rf"label and ref_speech\(mix speech\) diff: {gap}, label len: {nl}"):
        m.forward(xd, tsd, nl)
    g = gold(base)["logits"]                                   # the handle still works after a rejected call
    out = m.forward(xd, tsd, g.shape[-1]).cpu().numpy()
    assert np.abs(out - g).max() <= bar(g)


def test_rejected_calls_leave_the_handle_usable(gpu):
    (B, T, nl, _, wseed), x, ts = tsvad_inputs72("tsvad_redimnet_gap0")
    m = model(wseed, "fp32", gpu)
    tsd = torch.from_numpy(ts).to(gpu)
    with pytest.raises(AssertionError, match="expects 72-dim fbank"):
        m.forward(torch.zeros(B, T, 80, device=gpu), tsd, nl)
    with pytest.raises(ValueError, match="fbank frames exceed max_fbank_frames"):
        m.forward(torch.zeros(B, 399, 72, device=gpu), tsd, 100)
    g = gold("tsvad_redimnet_gap0")["logits"]
    assert np.abs(m.forward(torch.from_numpy(x).to(gpu), tsd, nl).cpu().numpy() - g).max() <= bar(g)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_nan_window_bypasses_batchnorm(gpu, precision):
    name = "tsvad_redimnet_nan"
    (B, T, nl, _, wseed), x, ts = tsvad_inputs72(name)
    bad = TSVAD_NAN[name][1]
    keep = [i for i in range(B) if i != bad]
    g, base = gold(name)["logits"], gold(TSVAD_NAN[name][0])["logits"]
    assert np.isnan(g[bad]).all() and np.isfinite(g[keep]).all()
    m = model(wseed, precision, gpu)
    xd, tsd = torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu)
    tol = bar(g[keep]) if precision == "fp32" else 2 * max(BF16_MEASURED.values())
    out = m.forward(xd, tsd, nl).cpu().numpy()
    assert np.isnan(out[bad]).all() and np.isfinite(out[keep]).all()
    print(f"nan {precision}: bypassed batch {np.abs(out[keep] - g[keep]).max():.3e}")
    assert np.abs(out[keep] - g[keep]).max() <= tol
    alone = m.forward(xd, tsd, nl, forward_batch=1).cpu().numpy()
    assert np.isnan(alone[bad]).all()
    print(f"nan {precision}: forward_batch 1 {np.abs(alone[keep] - base[keep]).max():.3e}")
    assert np.abs(alone[keep] - base[keep]).max() <= tol


def test_speaker_embed_dim_256_vs_restatement(gpu):
    """proj_layer (2 * 256 != 384) behind the ReDimNetB2 encoder, against the CPU restatement at fp32."""
    import redimnet_ref as rr
    cfg = TSVADConfig(speech_encoder_type=SE_TYPE, speaker_embed_dim=256)
    B, T, nl, wseed = 2, 38, 10, 951
    rng = np.random.default_rng(952)
    x = torch.from_numpy(rng.standard_normal((B, T, 72)).astype(np.float32))
    ts = torch.from_numpy(rng.standard_normal((B, 4, 256)).astype(np.float32))
    want = rr.tsvad_forward(to_torch(tsvad_state_dict(cfg, seed=wseed)), cfg, x, ts, nl).numpy()
    got = model(wseed, "fp32", gpu, cfg).forward(x.to(gpu), ts.to(gpu), nl).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"redimnet proj 256 fp32: max|logit diff| = {err:.3e} (|logit| max {np.abs(want).max():.3f})")
    assert err <= bar(want)


def test_graph_replays_bit_identical(gpu):
    (B, T, nl, _, wseed), x, ts = tsvad_inputs72("tsvad_redimnet_gap0")
    m = model(wseed, "bf16", gpu)
    xd, tsd = torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu)
    out = torch.empty(B, 4, nl, device=gpu)
    m.forward(xd, tsd, nl, out=out)
    ref = out.clone()
    out.zero_()
    _lib.call("sd_tsvad_forward_graph", m._h, _lib.ptr(xd), _lib.ptr(tsd), B, T, nl, _lib.ptr(out), 2, None,
              _lib.stream_ptr(gpu))
    m.status()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def test_strict_load(gpu):
    sd = to_torch(tsvad_state_dict(CFG, seed=1))
    sd.pop("speech_encoder.backbone.stage2.2.conv_block.pwconv1.weight")
    m = TSVADModel(CFG, device=gpu, precision="fp32", max_batch=1)
    with pytest.raises(RuntimeError, match="stage2.2.conv_block.pwconv1.weight"):
        m.load_state_dict(sd)
    sd = to_torch(tsvad_state_dict(CFG, seed=1))
    sd["speech_down_or_up.0.weight"] = torch.zeros(192, 1536, 5)
    m = TSVADModel(CFG, device=gpu, precision="fp32", max_batch=1)
    with pytest.raises(RuntimeError, match=r"speech_down_or_up.0.weight must be \(speaker_embed_dim, 1152, 5\)"):
        m.load_state_dict(sd)
