"""TS-VAD with the ECAPA-TDNN speech encoder (speech_encoder_type ecapa_channel_1024_wespeaker) on the MI355X path
against the reference goldens (tests/golden/make_golden_ecapa.py) and the CPU restatement (tests/ecapa_ref.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from make_golden_ecapa import ECAPA_CASES, ECAPA_NAN_CASES, SE_TYPE, ecapa_case_inputs  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.model import TSVADModel  # noqa: E402
from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = TSVADConfig(speech_encoder_type=SE_TYPE)
FP32_ATOL = 1e-3
# bf16: bf16 maps through the trunk's 28 convs (21 of them a sequential chain per block), then the bf16 back end.
# Measured max|logit - golden| on MI355X: BF16_MEASURED below (the kernels are deterministic); the bound is twice
# the largest, for other seeds.
BF16_MEASURED = {"tsvad_ecapa_rs4": 7.05e-3, "tsvad_ecapa_rs4_short": 7.83e-3, "tsvad_ecapa_tiny": 9.86e-3,
                 "tsvad_ecapa_t6": 6.04e-3}
BF16_ATOL = 2 * max(BF16_MEASURED.values())   # 1.97e-2
assert BF16_ATOL < 3e-2   # the project's loosest bf16 bound

_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(wseed, precision, gpu, cfg=CFG):
    key = (wseed, precision, cfg.speaker_embed_dim)
    if key not in _models:
        m = TSVADModel(cfg, device=gpu, precision=precision, max_batch=4)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)))
        _models[key] = m
    return _models[key]


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("name", list(ECAPA_CASES))
def test_forward_vs_reference_golden(gpu, name, precision):
    (B, T, nl, _, wseed, _), x, ts = ecapa_case_inputs(name)
    g = gold(name)
    m = model(wseed, precision, gpu)
    out = m.forward(torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu), torch.zeros(B, 4, nl)).cpu().numpy()
    err = np.abs(out - g["logits"]).max()
    print(f"{name} {precision}: max|logit diff| = {err:.3e} (|logit| max {np.abs(g['logits']).max():.3f})")
    assert err < (BF16_ATOL if precision == "bf16" else FP32_ATOL)


@pytest.mark.parametrize("name", list(ECAPA_CASES))
def test_down_conv_output_vs_reference_golden(gpu, name):
    """sd_tsvad_debug_buffer(which=0): the stride-4 conv + bias, (B, T3, 192) channel-last; the golden is the
    reference's speech_down_or_up output, i.e. BatchNorm1d + ReLU of it."""
    (B, T, nl, _, wseed, _), x, ts = ecapa_case_inputs(name)
    g = gold(name)
    m = model(wseed, "fp32", gpu)
    m.forward(torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu), nl)
    p, n = ctypes.c_void_p(), ctypes.c_int64()
    _lib.call("sd_tsvad_debug_buffer", m._h, 0, ctypes.byref(p), ctypes.byref(n))
    T3 = g["speech_enc"].shape[-1]
    assert T3 == (T - 1) // 4 + 1 and n.value >= B * T3 * 192 * 4
    host = np.empty(B * T3 * 192, np.float32)
    assert ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(host.ctypes.data), p, ctypes.c_size_t(host.nbytes), 2) == 0
    sd = tsvad_state_dict(CFG, seed=wseed)
    q = "speech_down_or_up.1.bn."
    y = host.reshape(B, T3, 192).astype(np.float64)
    y = (y - sd[q + "running_mean"]) / np.sqrt(sd[q + "running_var"].astype(np.float64) + 1e-5) * sd[q + "weight"] + sd[q + "bias"]
    enc = np.maximum(y, 0.0).transpose(0, 2, 1)
    err = np.abs(enc - g["speech_enc"]).max()
    print(f"{name}: max|speech_enc diff| = {err:.3e} (max {g['speech_enc'].max():.3f})")
    assert err < 1e-4


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_nan_window_bypasses_batchnorm(gpu, precision):
    name = "tsvad_ecapa_nan"
    (B, T, nl, _, wseed, _), x, ts = ecapa_case_inputs(name)
    bad = ECAPA_NAN_CASES[name][1]
    keep = [i for i in range(B) if i != bad]
    g, base = gold(name)["logits"], gold(ECAPA_NAN_CASES[name][0])["logits"]
    m = model(wseed, precision, gpu)
    xd, tsd = torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu)
    tol = FP32_ATOL if precision == "fp32" else BF16_ATOL
    out = m.forward(xd, tsd, nl).cpu().numpy()
    assert np.isnan(out[bad]).all() and np.isfinite(out[keep]).all()
    print(f"nan {precision}: bypassed batch {np.abs(out[keep] - g[keep]).max():.3e}")
    assert np.abs(out[keep] - g[keep]).max() < tol
    alone = m.forward(xd, tsd, nl, forward_batch=1).cpu().numpy()
    assert np.isnan(alone[bad]).all()
    print(f"nan {precision}: forward_batch 1 {np.abs(alone[keep] - base[keep]).max():.3e}")
    assert np.abs(alone[keep] - base[keep]).max() < tol


def test_bf16_ring_gemm_batch_vs_fp32(gpu):
    """Three 398-frame windows give 1194 GEMM rows, from which the trunk's 1x1 convs (ReLU, then BatchNorm in the
    epilogue) run on the ring GEMM instead of the register-staged kernel the goldens' smaller shapes take.  Reference:
    the fp32 handle, itself within 1e-3 of the goldens."""
    rng = np.random.default_rng(933)
    x = torch.from_numpy(rng.standard_normal((3, 398, 80)).astype(np.float32)).to(gpu)
    ts = torch.from_numpy(rng.standard_normal((3, 4, 192)).astype(np.float32)).to(gpu)
    want = model(777, "fp32", gpu).forward(x, ts, 100).cpu().numpy()
    got = model(777, "bf16", gpu).forward(x, ts, 100).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"ecapa bf16 B=3 T=398 vs fp32: max|logit diff| = {err:.3e} (|logit| max {np.abs(want).max():.3f})")
    assert np.isfinite(got).all() and err < BF16_ATOL


def test_shape_errors(gpu):
    m = model(777, "fp32", gpu)
    x = torch.zeros(1, 398, 80, device=gpu)
    ts = torch.zeros(1, 4, 192, device=gpu)
    with pytest.raises(AssertionError, match=r"label and ref_speech\(mix speech\) diff: -2"):
        m.forward(x, ts, 102)      # (398 - 1) // 4 + 1 = 100 mix frames
    with pytest.raises(AssertionError, match=r"label and ref_speech\(mix speech\) diff: 3"):
        m.forward(x, ts, 97)
    with pytest.raises(ValueError, match="fbank frames exceed max_fbank_frames"):
        m.forward(torch.zeros(1, 399, 80, device=gpu), ts, 100)
    m.forward(x, ts, 100)   # the handle still works


def test_strict_load(gpu):
    sd = to_torch(tsvad_state_dict(CFG, seed=1))
    sd["speech_encoder.pool.linear1.weight"] = torch.zeros(128, 4608, 1)
    m = TSVADModel(CFG, device=gpu, precision="fp32", max_batch=1)
    with pytest.raises(RuntimeError, match="speech_encoder.pool.linear1.weight"):
        m.load_state_dict(sd)
    sd = to_torch(tsvad_state_dict(CFG, seed=1))
    sd.pop("speech_encoder.layer3.se_res2block.1.convs.3.weight")
    m = TSVADModel(CFG, device=gpu, precision="fp32", max_batch=1)
    with pytest.raises(RuntimeError, match="se_res2block.1.convs.3.weight"):
        m.load_state_dict(sd)
    sd = to_torch(tsvad_state_dict(CFG, seed=1))
    sd["speech_encoder.layer2.se_res2block.1.convs.0.weight"] = torch.zeros(128, 128, 5)
    m = TSVADModel(CFG, device=gpu, precision="fp32", max_batch=1)
    with pytest.raises(RuntimeError, match=r"layer2.se_res2block.1.convs.0.weight must be \(128, 128, 3\)"):
        m.load_state_dict(sd)


def test_graph_replays_bit_identical(gpu):
    (B, T, nl, _, wseed, _), x, ts = ecapa_case_inputs("tsvad_ecapa_rs4_short")
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


def test_pipeline_vs_restatement(gpu):
    """An 8-s, 4-speaker meeting through TSVADPipeline.posteriors at fp32 = sigmoid + overlap mean of the CPU
    restatement's logits on the reference loop's windows (oracle.pipeline_ref, imported)."""
    import ecapa_ref as er
    from oracle.pipeline_ref import overlap_average, plan, window_batches
    from speaker_diarization_amd.synth import make_meeting, speaker_embeddings
    from speaker_diarization_amd.ts_vad.pipeline import TSVADPipeline
    mt = make_meeting(8.0, n_spk=4, seed=21)
    ts = speaker_embeddings(4, seed=21)
    n_lab = mt.labels.shape[1]
    sd = to_torch(tsvad_state_dict(CFG, seed=777))
    ws = plan(n_lab, CFG.rs_len, 1)
    logits = np.zeros((len(ws), 4, CFG.rs_len * 25), np.float32)
    for b0, wb, ref, tsb, L in window_batches(mt.wav, ts, ws, 8):
        logits[b0:b0 + len(wb), :, :L] = er.tsvad_forward(sd, CFG, ref, tsb, L).numpy()
    want = overlap_average(logits, [s for s, _ in ws], [e - s for s, e in ws], n_lab)
    m = model(777, "fp32", gpu)
    pipe = TSVADPipeline(m, segment_shift=1, batch_size=8)
    post = pipe.posteriors(torch.from_numpy(mt.wav).to(gpu), torch.from_numpy(ts).to(gpu), n_lab).cpu().numpy()
    err = np.abs(post - want).max()
    print(f"pipeline ecapa fp32: max|post diff| = {err:.3e}")
    assert err < 1e-3


def test_speaker_embed_dim_256_vs_restatement(gpu):
    """proj_layer (2 * 256 != 384) behind the ECAPA encoder, against the CPU restatement at fp32."""
    import ecapa_ref as er
    cfg = TSVADConfig(speech_encoder_type=SE_TYPE, speaker_embed_dim=256)
    B, T, nl, wseed = 2, 38, 10, 931
    rng = np.random.default_rng(932)
    x = torch.from_numpy(rng.standard_normal((B, T, 80)).astype(np.float32))
    ts = torch.from_numpy(rng.standard_normal((B, 4, 256)).astype(np.float32))
    want = er.tsvad_forward(to_torch(tsvad_state_dict(cfg, seed=wseed)), cfg, x, ts, nl).numpy()
    got = model(wseed, "fp32", gpu, cfg).forward(x.to(gpu), ts.to(gpu), nl).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"ecapa proj 256 fp32: max|logit diff| = {err:.3e} (|logit| max {np.abs(want).max():.3f})")
    assert err < 1e-3
