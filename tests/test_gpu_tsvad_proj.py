"""TS-VAD with proj_layer (speaker_embed_dim 256 / 512 against the 384-wide back end) on the MI355X path: the split
speaker-input stage (sd_op_speaker_input_proj) against float64, the models against the reference goldens
(tests/golden/make_golden_resnet_emb.py), and enrollment audio -> ResNet34 embeddings -> TS-VAD end to end against
the CPU restatement (tests/resnet_emb_ref.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import embed_wav  # noqa: E402
from make_golden_resnet_emb import PROJ_CASES, proj_config, proj_inputs  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.model import TSVADModel  # noqa: E402
from speaker_diarization_amd.weights import (TSVADConfig, resnet34_embed_state_dict, sinusoid_pe, to_torch,  # noqa: E402
                                             tsvad_state_dict)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_ATOL = 1e-3
OP_FP32_ATOL = 1e-5
# bf16, measured max abs error on MI355X (deterministic kernels); the bounds are twice the largest.
# stage: sd_op_speaker_input_proj against float64 (bf16 operands of both GEMMs, outputs O(1)); model: logits against
# the goldens.
BF16_MEASURED_OP = {(256, 10): 5.49e-3, (256, 8): 6.05e-3, (512, 10): 5.30e-3, (512, 8): 5.16e-3}   # (SE, Tmix)
BF16_MEASURED = {"rn34": 5.90e-3, "rn34_tiny": 5.44e-3, "campp": 6.50e-3, "rn34_nan": 5.80e-3}
BF16_OP_ATOL = 2 * max(BF16_MEASURED_OP.values())   # 1.21e-2 on rows of magnitude ~1-3
BF16_ATOL = 2 * max(BF16_MEASURED.values())         # 1.30e-2, below the 1.79e-2 of the SE-192 ResNet34 model's test

_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(gpu, name, precision):
    cfg, wseed = proj_config(name), PROJ_CASES[name][5]
    key = (cfg.speech_encoder_type, wseed, precision)
    if key not in _models:
        m = TSVADModel(cfg, device=gpu, precision=precision, max_batch=4)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)))
        _models[key] = m
    return _models[key]


_stage_ref = {}


def stage_case(SE, Tmix, B=2, NS=4, T=10, E=384):
    """Seeded inputs of the stage and its float64 result, with and without the BatchNorm bypass (computed once)."""
    key = (SE, Tmix)
    if key not in _stage_ref:
        rng = np.random.default_rng(SE + Tmix)
        d = dict(ts=rng.standard_normal((B, NS, SE)), mix=rng.standard_normal((B, Tmix, SE)) * 1.5,
                 w=rng.uniform(-1, 1, (E, 2 * SE)) / np.sqrt(2 * SE), bias=rng.standard_normal(E) * 0.05,
                 bn_a=rng.uniform(0.7, 1.4, SE), bn_b=rng.standard_normal(SE) * 0.1,
                 pe=sinusoid_pe(T, E)[:, 0].astype(np.float64))
        d = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in d.items()}
        want = {}
        for bypass in (False, True):
            mix = d["mix"].double()
            a = torch.relu(mix if bypass else mix * d["bn_a"].double() + d["bn_b"].double())
            a = F.pad(a, (0, 0, 0, T - Tmix))                                   # frames t >= Tmix: zeros
            cat = torch.cat((d["ts"].double()[:, :, None, :].expand(B, NS, T, SE),
                             a[:, None].expand(B, NS, T, SE)), -1)
            want[bypass] = (F.linear(cat, d["w"].double(), d["bias"].double()) + d["pe"].double()).numpy()
        _stage_ref[key] = (d, want)
    return _stage_ref[key]


@pytest.mark.parametrize("bypass", [False, True], ids=["bn", "bypass"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("Tmix", [10, 8])
@pytest.mark.parametrize("SE", [256, 512])
def test_speaker_input_proj_vs_float64(gpu, SE, Tmix, precision, bypass):
    B, NS, T, E = 2, 4, 10, 384
    d, want = stage_case(SE, Tmix)
    t = {k: v.to(gpu).contiguous() for k, v in d.items()}
    grp = torch.tensor([1 if bypass else 0], dtype=torch.int32, device=gpu)
    out = torch.full((B * NS * T, E), 9.0, device=gpu)
    xb = torch.zeros(B * NS * T, E, dtype=torch.bfloat16, device=gpu)
    p = _lib.ptr
    _lib.call("sd_op_speaker_input_proj", p(t["ts"]), p(t["mix"]), B, NS, T, Tmix, SE, E, p(t["w"]), p(t["bias"]),
              p(t["pe"]), p(t["bn_a"]), p(t["bn_b"]), p(grp), B, p(out), p(xb), 1 if precision == "bf16" else 0,
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(B, NS, T, E)
    err = float(np.abs(got - want[bypass]).max())
    print(f"speaker_input_proj SE={SE} Tmix={Tmix} {precision} bypass={bypass}: max abs err {err:.3e}")
    assert torch.equal(xb.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))   # the bf16 copy of the rows
    assert err <= (OP_FP32_ATOL if precision == "fp32" else BF16_OP_ATOL)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["rn34", "rn34_tiny", "campp"])
def test_forward_vs_reference_golden(gpu, name, precision):
    _, B, T, nl = PROJ_CASES[name][:4]
    x, ts = proj_inputs(name)
    want = gold("tsvad_proj")[f"{name}.logits"]
    m = model(gpu, name, precision)
    out = m.forward(torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu), nl).cpu().numpy()
    err = float(np.abs(out - want).max())
    print(f"tsvad_proj {name} {precision}: max|logit diff| = {err:.3e} (|logit| max {np.abs(want).max():.3f})")
    assert err <= (BF16_ATOL if precision == "bf16" else FP32_ATOL)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_nan_target_embedding(gpu, precision):
    name = "rn34_nan"
    _, B, T, nl, _, _, nan_at = PROJ_CASES[name]
    x, ts = proj_inputs(name)
    bad = nan_at[0]
    keep = [i for i in range(B) if i != bad]
    want = gold("tsvad_proj")[f"{name}.logits"]      # the reference on the same NaN batch (backend_down's BN bypassed)
    m = model(gpu, name, precision)
    out = m.forward(torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu), nl).cpu().numpy()
    assert np.isnan(out[bad]).all() and np.isfinite(out[keep]).all()
    err = float(np.abs(out[keep] - want[keep]).max())
    print(f"tsvad_proj {name} {precision}: other windows max|logit diff| = {err:.3e}")
    assert err <= (BF16_ATOL if precision == "bf16" else FP32_ATOL)


def test_graph_replays_bit_identical(gpu):
    name = "rn34"
    _, B, T, nl = PROJ_CASES[name][:4]
    x, ts = proj_inputs(name)
    m = model(gpu, name, "bf16")
    xd, tsd = torch.from_numpy(x).to(gpu), torch.from_numpy(ts).to(gpu)
    out = torch.empty(B, 4, nl, device=gpu)
    m.forward(xd, tsd, nl, out=out)
    ref = out.clone()
    out.zero_()
    _lib.call("sd_tsvad_forward_graph", m._h, _lib.ptr(xd), _lib.ptr(tsd), B, T, nl, _lib.ptr(out), 2, None,
              _lib.stream_ptr(gpu))
    m.status()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def test_ots_vad_with_proj_raises_at_create(gpu):
    with pytest.raises(ValueError, match="proj_layer"):
        TSVADModel(TSVADConfig.ots_vad_v1(speaker_embed_dim=256), device=gpu, precision="fp32", max_batch=1)


def test_se512_runs(gpu):
    cfg = TSVADConfig(speaker_embed_dim=512)
    m = TSVADModel(cfg, device=gpu, precision="fp32", max_batch=2)
    sd = to_torch(tsvad_state_dict(cfg, seed=3))
    m.load_state_dict(sd)
    import resnet_emb_ref as er
    rng = np.random.default_rng(12)
    x = torch.from_numpy(rng.standard_normal((2, 38, 80)).astype(np.float32))
    ts = torch.from_numpy(rng.standard_normal((2, 4, 512)).astype(np.float32))
    want = er.tsvad_forward(sd, cfg, x, ts, 10).numpy()
    out = m.forward(x.to(gpu), ts.to(gpu), 10).cpu().numpy()
    err = float(np.abs(out - want).max())
    print(f"tsvad_proj CAM++ SE 512 fp32 vs restatement: {err:.3e}")
    assert err <= FP32_ATOL


def test_enrollment_to_posteriors_end_to_end(gpu):
    """Enrollment wavs of 4 speakers -> ResNet34 extract_embed -> mean over chunks -> TSVADPipeline.posteriors on an
    8-s meeting with the ResNet34 SE-256 model, fp32, against the CPU restatement on the reference loop's windows
    (oracle.pipeline_ref, imported)."""
    import resnet_emb_ref as er
    from oracle.pipeline_ref import overlap_average, plan, window_batches
    from speaker_diarization_amd.synth import make_meeting
    from speaker_diarization_amd.ts_vad.embedding import ResNet34, extract_embed
    from speaker_diarization_amd.ts_vad.pipeline import TSVADPipeline
    cfg = TSVADConfig(speech_encoder_type="resnet34_wespeaker", speaker_embed_dim=256)
    esd = to_torch(resnet34_embed_state_dict(41, 256, False))
    tsd = to_torch(tsvad_state_dict(cfg, seed=42))
    wavs = [np.round(embed_wav(6.5 if i else 3.0, 300 + i) * 32768).astype(np.int16).astype(np.float64) / 32768.0
            for i in range(4)]
    ts_ref = np.stack([er.extract_embed(esd, w).mean(0).numpy() for w in wavs])
    ext = ResNet34(80, 256, two_emb_layer=False, device=gpu, precision="fp32", max_batch=2).load_state_dict(esd)
    ts = torch.stack([extract_embed(w, ext).mean(0) for w in wavs])
    e_err = float(np.abs(ts.cpu().numpy() - ts_ref).max())
    print(f"end to end: embeddings max abs err {e_err:.3e} (std {ts_ref.std():.3f})")
    assert e_err <= FP32_ATOL
    mt = make_meeting(8.0, n_spk=4, seed=21)
    n_lab = mt.labels.shape[1]
    ws = plan(n_lab, cfg.rs_len, 1)
    logits = np.zeros((len(ws), 4, cfg.rs_len * 25), np.float32)
    for b0, wb, ref, tsb, L in window_batches(mt.wav, ts_ref, ws, 8):
        logits[b0:b0 + len(wb), :, :L] = er.tsvad_forward(tsd, cfg, ref, tsb, L).numpy()
    want = overlap_average(logits, [s for s, _ in ws], [e - s for s, e in ws], n_lab)
    m = TSVADModel(cfg, device=gpu, precision="fp32", max_batch=8)
    m.load_state_dict(tsd)
    pipe = TSVADPipeline(m, segment_shift=1, batch_size=8)
    post = pipe.posteriors(torch.from_numpy(mt.wav).to(gpu), ts, n_lab).cpu().numpy()
    err = float(np.abs(post - want).max())
    print(f"end to end: max|post diff| = {err:.3e}")
    assert err <= FP32_ATOL
