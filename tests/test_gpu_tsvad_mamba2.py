"""TS-VAD with Mamba2 back ends (single_backend_type "mamba2", multi_backend_type "transformer" or "mamba2") on the
MI355X path against the CPU restatement (tests/mamba2_ref.py; parity unpinned: mamba_ssm is CUDA-only, so no reference
run exists).  The scan runs along the windows of each reference forward call, so forward_batch is part of every case."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mamba2_ref as mr  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.model import TSVADModel  # noqa: E402
from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu

WSEED = 777
MAX_BATCH = 70
FP32_ATOL = 1e-3
# bf16: max|logit - restatement| measured on MI355X per case (the kernels are deterministic); the bound is twice the
# largest and must stay under the project's loosest bf16 bound.
BF16_MEASURED = {(1, "b1"): 5.32e-3, (1, "b3"): 1.085e-2, (1, "b5_fb2"): 6.29e-3, (1, "b70"): 9.06e-3,
                 (2, "b1"): 5.94e-3, (2, "b3"): 6.45e-3, (2, "b5_fb2"): 8.93e-3, (2, "b70"): 1.176e-2}
BF16_ATOL = 2 * max(BF16_MEASURED.values())   # 2.35e-2
assert BF16_ATOL < 3e-2

# back end 1 at the recipe's d_state 128, back end 2 at the reference default 64
CFGS = {1: dict(multi_backend_type="transformer", d_state=128), 2: dict(multi_backend_type="mamba2", d_state=64)}
# name: (B, T_fbank, label frames, forward_batch): the tiny CAM++ shape (38 frames -> 10 labels); B = 70 with 5 label
# frames so that one sequence crosses the 64-window tile of a reference batch
CASES = {"b1": (1, 38, 10, 0), "b3": (3, 38, 10, 0), "b5_fb2": (5, 38, 10, 2), "b70": (70, 18, 5, 0)}

_models, _sd, _want = {}, {}, {}


def config(backend, **kw):
    return TSVADConfig(single_backend_type="mamba2", **CFGS[backend], **kw)


def state(backend, se=192):
    if (backend, se) not in _sd:
        _sd[backend, se] = to_torch(tsvad_state_dict(config(backend, speaker_embed_dim=se), seed=WSEED))
    return _sd[backend, se]


def model(backend, precision, gpu, se=192):
    key = (backend, precision, se)
    if key not in _models:
        m = TSVADModel(config(backend, speaker_embed_dim=se), device=gpu, precision=precision, max_batch=MAX_BATCH)
        m.load_state_dict(state(backend, se))
        _models[key] = m
    return _models[key]


def inputs(B, T_fb, se=192, seed=4100):
    rng = np.random.default_rng(seed + B)
    return (torch.from_numpy(rng.standard_normal((B, T_fb, 80)).astype(np.float32)),
            torch.from_numpy(rng.standard_normal((B, 4, se)).astype(np.float32)))


def restatement(backend, name):
    """The reference loop over forward calls of forward_batch windows, computed once per case."""
    if (backend, name) not in _want:
        B, T, nl, fb = CASES[name]
        x, ts = inputs(B, T)
        _want[backend, name] = mr.tsvad_forward_grouped(state(backend), config(backend), x, ts, nl, fb).numpy()
    return _want[backend, name]


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("backend", [1, 2])
def test_forward_vs_restatement(gpu, backend, name, precision):
    B, T, nl, fb = CASES[name]
    x, ts = inputs(B, T)
    want = restatement(backend, name)
    got = model(backend, precision, gpu).forward(x.to(gpu), ts.to(gpu), nl, forward_batch=fb).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"mamba2 backend {backend} {name} {precision}: max|logit diff| = {err:.3e} (|logit| max {np.abs(want).max():.3f})")
    assert np.isfinite(got).all()
    assert err < (BF16_ATOL if precision == "bf16" else FP32_ATOL)


def test_speaker_embed_dim_256(gpu):
    """proj_layer (2 * 256 != 384) runs before the back end and keeps working in front of the Mamba2 one."""
    cfg = config(1, speaker_embed_dim=256)
    x, ts = inputs(3, 38, se=256)
    want = mr.tsvad_forward(state(1, 256), cfg, x, ts, 10).numpy()
    got = model(1, "fp32", gpu, se=256).forward(x.to(gpu), ts.to(gpu), 10).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"mamba2 proj 256 fp32: max|logit diff| = {err:.3e}")
    assert err < FP32_ATOL


@pytest.mark.parametrize("backend", [1, 2])
def test_group_scope_is_honoured(gpu, backend):
    """The scan never crosses forward_batch groups: groups of 2 and one group of 5 are different functions."""
    B, T, nl, _ = CASES["b5_fb2"]
    x, ts = inputs(B, T)
    m = model(backend, "fp32", gpu)
    grouped = m.forward(x.to(gpu), ts.to(gpu), nl, forward_batch=2).cpu().numpy()
    whole = m.forward(x.to(gpu), ts.to(gpu), nl, forward_batch=0).cpu().numpy()
    diff = np.abs(grouped - whole).max()
    print(f"backend {backend}: forward_batch 2 vs 0 differ by {diff:.3e}")
    assert diff > FP32_ATOL
    want = mr.tsvad_forward(state(backend), config(backend), x, ts, nl).numpy()
    assert np.abs(whole - want).max() < FP32_ATOL


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_nan_window_poisons_its_group(gpu, precision):
    """One NaN window: the scan and backend_down carry it to every window of its reference forward call, and to no
    other group."""
    B, T, nl, fb = CASES["b5_fb2"]
    x, ts = inputs(B, T)
    x = x.clone()
    x[2, 5, 0] = float("nan")          # group 1 = windows 2, 3
    want = restatement(1, "b5_fb2")
    got = model(1, precision, gpu).forward(x.to(gpu), ts.to(gpu), nl, forward_batch=fb).cpu().numpy()
    assert np.isnan(got[2:4]).all()
    keep = [0, 1, 4]
    assert np.isfinite(got[keep]).all()
    err = np.abs(got[keep] - want[keep]).max()
    print(f"nan {precision}: other groups {err:.3e}")
    assert err < (BF16_ATOL if precision == "bf16" else FP32_ATOL)


@pytest.mark.parametrize("backend", [1, 2])
def test_graph_replays_bit_identical(gpu, backend):
    B, T, nl, _ = CASES["b3"]
    x, ts = inputs(B, T)
    m = model(backend, "bf16", gpu)
    xd, tsd = x.to(gpu), ts.to(gpu)
    out = torch.empty(B, 4, nl, device=gpu)
    m.forward(xd, tsd, nl, out=out)
    ref = out.clone()
    out.zero_()
    _lib.call("sd_tsvad_forward_graph", m._h, _lib.ptr(xd), _lib.ptr(tsd), B, T, nl, _lib.ptr(out), 2, None,
              _lib.stream_ptr(gpu))
    m.status()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def test_strict_load(gpu):
    cfg = config(2)
    sd = dict(state(2))
    sd.pop("multi_backend.backward_blocks.1.mixer.A_log")
    m = TSVADModel(cfg, device=gpu, precision="fp32", max_batch=1)
    with pytest.raises(RuntimeError, match=r"multi_backend.backward_blocks.1.mixer.A_log"):
        m.load_state_dict(sd)
    sd = dict(state(2))
    sd["single_backend.forward_blocks.0.mixer.in_proj.weight"] = torch.zeros(3352, 384)   # d_state 128's shape
    m = TSVADModel(cfg, device=gpu, precision="fp32", max_batch=1)
    with pytest.raises(RuntimeError, match=r"single_backend.forward_blocks.0.mixer.in_proj.weight.*\(3224, 384\)"):
        m.load_state_dict(sd)
    sd = dict(state(2))
    sd["single_backend.layers.0.norm1.weight"] = torch.ones(384)   # a transformer key the Mamba2 model does not have
    m = TSVADModel(cfg, device=gpu, precision="fp32", max_batch=1)
    with pytest.raises(RuntimeError, match="single_backend.layers.0.norm1.weight"):
        m.load_state_dict(sd)


def test_create_refusals(gpu):
    def create(**kw):
        conf = dict(variant=0, max_num_speaker=4, rs_len=4, max_batch=1, max_fbank_frames=398, precision=0,
                    num_transformer_layer=2, num_attention_head=4, transformer_embed_dim=384,
                    transformer_ffn_embed_dim=1536, speaker_embed_dim=192, backend=1, d_state=128, expand=4)
        conf.update(kw)
        h = ctypes.c_void_p()
        try:
            _lib.call("sd_tsvad_create", ctypes.byref(_lib.TsvadConfig(**conf)), ctypes.byref(h))
        finally:
            if h:
                _lib.call("sd_tsvad_destroy", h)
    for variant in (1, 2, 3, 4):
        with pytest.raises(ValueError, match="backend"):
            create(variant=variant)
    with pytest.raises(ValueError, match="backend"):
        create(backend=3)
    with pytest.raises(ValueError, match="d_state"):
        create(d_state=100)
    with pytest.raises(ValueError, match="d_state"):
        create(d_state=272)
    with pytest.raises(ValueError, match="expand"):
        create(transformer_embed_dim=96, speaker_embed_dim=48, expand=1)   # 96 is no multiple of the head dimension 64
    create()
    create(backend=0, d_state=0, expand=0)   # a zero-initialised tail is today's model


def test_reference_batch_must_fit(gpu):
    m = TSVADModel(config(1), device=gpu, precision="fp32", max_batch=2)
    x, ts = inputs(3, 38)
    with pytest.raises(ValueError, match="max_batch"):
        m.forward(x.to(gpu), ts.to(gpu), 10)


def test_pipeline_vs_restatement(gpu):
    """An 8-s, 4-speaker meeting through TSVADPipeline.posteriors at fp32 with batch_size 8 = sigmoid + overlap mean of
    the restatement's logits on the reference loop's batches of 8 windows (oracle.pipeline_ref)."""
    from oracle.pipeline_ref import overlap_average, plan, window_batches
    from speaker_diarization_amd.synth import make_meeting, speaker_embeddings
    from speaker_diarization_amd.ts_vad.pipeline import TSVADPipeline
    cfg = config(1)
    mt = make_meeting(8.0, n_spk=4, seed=21)
    ts = speaker_embeddings(4, seed=21)
    n_lab = mt.labels.shape[1]
    ws = plan(n_lab, cfg.rs_len, 1)
    logits = np.zeros((len(ws), 4, cfg.rs_len * 25), np.float32)
    for b0, wb, ref, tsb, L in window_batches(mt.wav, ts, ws, 8):
        logits[b0:b0 + len(wb), :, :L] = mr.tsvad_forward(state(1), cfg, ref, tsb, L, form="chunked").numpy()
    want = overlap_average(logits, [s for s, _ in ws], [e - s for s, e in ws], n_lab)
    pipe = TSVADPipeline(model(1, "fp32", gpu), segment_shift=1, batch_size=8)
    post = pipe.posteriors(torch.from_numpy(mt.wav).to(gpu), torch.from_numpy(ts).to(gpu), n_lab).cpu().numpy()
    err = np.abs(post - want).max()
    print(f"pipeline mamba2 fp32: max|post diff| = {err:.3e}")
    assert err < 1e-3
