"""TS-VAD with the WavLM speech encoders (variants 5 / 6), host side: the torch restatement (tests/tsvad_wavlm_ref.py)
against every reference golden of tests/golden/make_golden_tsvad_wavlm.py at the fp32 bar, the configuration rules, the
state_dict layout against the reference's stored key list, the frame arithmetic and the waveform window plan."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import tsvad_wavlm_ref as ref  # noqa: E402
from make_golden_tsvad_wavlm import CASES, NAN, RAISES, case_cfg, case_inputs  # noqa: E402
from speaker_diarization_amd.ssl.wavlm import WavLMConfig, num_frames  # noqa: E402
from speaker_diarization_amd.ts_vad.windows import plan_windows  # noqa: E402
from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_layout, tsvad_state_dict  # noqa: E402

GOLD = os.path.join(HERE, "golden")
FP32_RTOL = 1e-3


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(CASES) + list(NAN))
def test_restatement_vs_reference_golden(name):
    (B, n, nl, wseed), wav, ts = case_inputs(name)
    cfg = case_cfg(name)
    g = gold(name)["logits"]
    with torch.no_grad():
        out = ref.tsvad_forward(to_torch(tsvad_state_dict(cfg, seed=wseed)), cfg, torch.from_numpy(wav),
                                torch.from_numpy(ts), nl).numpy()
    keep = np.isfinite(g)
    assert (np.isfinite(out) == keep).all()
    err = float(np.abs(out[keep] - g[keep]).max())
    print(f"{name}: max|logit diff| = {err:.3e}")
    assert err <= FP32_RTOL * max(1.0, float(np.abs(g[keep]).max()))


@pytest.mark.parametrize("base,nl", list(RAISES))
def test_restatement_label_rule(base, nl):
    (B, n, _, wseed), wav, ts = case_inputs(base)
    cfg = case_cfg(base)
    with pytest.raises(AssertionError, match=r"label and ref_speech\(mix speech\) diff"), torch.no_grad():
        ref.tsvad_forward(to_torch(tsvad_state_dict(cfg, seed=wseed)), cfg, torch.from_numpy(wav), torch.from_numpy(ts), nl)


def test_variant_rules():
    w = WavLMConfig()
    for se in ("WavLM", "WavLM_weight_sum"):      # the bare configurations stay unsupported, now saying why
        with pytest.raises(ValueError, match="unsupported TS-VAD configuration.*wavlm_cfg is missing"):
            TSVADConfig(speech_encoder_type=se).variant
    c5 = TSVADConfig(speech_encoder_type="WavLM", wavlm_cfg=w)
    assert c5.variant == 5 and c5.backend == 0 and c5.waveform_input and c5.wavlm_encoder_layers == 6
    assert c5.effective_wavlm_cfg().encoder_layers == 6 and w.encoder_layers == 12
    c6 = TSVADConfig(speech_encoder_type="WavLM_weight_sum", wavlm_cfg=w, wavlm_fuse_feat_post_norm=True)
    assert c6.variant == 6 and c6.backend == 0 and c6.wavlm_encoder_layers == 12
    with pytest.raises(ValueError, match=r"model.py:1206-1213.*view"):
        TSVADConfig(speech_encoder_type="WavLM_weight_sum", wavlm_cfg=w).variant
    for kw in (dict(single_backend_type="mamba2"), dict(single_backend_type="mamba2", multi_backend_type="mamba2"),
               dict(single_backend_type="conformer_ots_vad", multi_backend_type="lstm_ots_vad"),
               dict(ots_vad_style="v1")):
        with pytest.raises(ValueError, match="transformer single and multi back ends only"):
            TSVADConfig(speech_encoder_type="WavLM", wavlm_cfg=w, **kw).variant
    with pytest.raises(ValueError, match="encoder_embed_dim"):
        TSVADConfig(speech_encoder_type="WavLM", wavlm_cfg=WavLMConfig(dict(encoder_embed_dim=512))).variant
    with pytest.raises(ValueError, match="encoder_layers must be 1..24"):   # after the override
        TSVADConfig(speech_encoder_type="WavLM", wavlm_cfg=w, select_encoder_layer_nums=0).variant
    assert not TSVADConfig().waveform_input and TSVADConfig().variant == 0


def test_layout_matches_reference_keys():
    keys = gold("tsvad_wavlm_keys")
    assert "is invalid for input of size" in str(keys["post_norm_false_raises"])
    assert (keys["perturbation.fp32_bars"] >= 10).all() and len(keys["perturbation.names"]) == 11
    for tag, name in (("v5_bp_l2_se192", "tsvad_wavlm5_bp"), ("v5_lg_l2_se192", "tsvad_wavlm5_lg"),
                      ("v6_bp_l3_se192", "tsvad_wavlm6_bp"), ("v6_lg_l2_se192", "tsvad_wavlm6_lg"),
                      ("v6_bp_l3_se256", "tsvad_wavlm6_se256")):
        want = {n: tuple(int(d) for d in s.split(",") if d) for n, s in zip(keys[tag + ".names"], keys[tag + ".shapes"])}
        cfg = case_cfg(name)
        lay = {n: tuple(s) for n, s, _ in tsvad_layout(cfg)}
        assert lay == want, (set(lay) ^ set(want))
        sd = tsvad_state_dict(cfg, seed=3)
        assert {k: tuple(v.shape) for k, v in sd.items()} == want
    sd = tsvad_state_dict(case_cfg("tsvad_wavlm6_bp"), seed=3)
    w = sd["weights.weight"][0]
    assert w.max() - w.min() > 1.0 and len(set(np.round(w, 2))) == len(w)      # clearly non-uniform


def test_frame_arithmetic():
    for n, T, T3 in ((64000, 199, 100), (16000, 49, 25), (3280, 10, 5), (640, 1, 1)):
        assert num_frames(n) == T == ref.wavlm_frames(n) and ref.mix_frames(n) == T3


def test_waveform_window_plan_matches_collater_padding():
    """13 s at 25 labels / s: windows of 100 labels shifted by 25 with a 1-label tail when n_labels = 326; each
    batch's windows are the raw samples zero-padded to the batch's longest (ts_vad_dataset.py:693-707)."""
    plan = plan_windows(326, 4, 1)
    assert plan.lens[-1] == 1 and plan.samples_per_label == 640
    assert (plan.wave_n == plan.lens * 640).all() and (plan.wave_start == plan.starts * 640).all()
    wav = np.random.default_rng(0).standard_normal(326 * 640).astype(np.float32)
    for b0, b1 in plan.batches(4):
        rows = [wav[s * 640:e * 640] for s, e in zip(plan.starts[b0:b1], plan.ends[b0:b1])]
        longest = max(len(r) for r in rows)
        assert longest == int(plan.wave_n[b0:b1].max())
        padded = np.stack([np.pad(r, (0, longest - len(r))) for r in rows])
        for i, w in enumerate(range(b0, b1)):
            n = int(plan.wave_n[w])
            assert (padded[i, :n] == wav[plan.wave_start[w]:plan.wave_start[w] + n]).all() and (padded[i, n:] == 0).all()
