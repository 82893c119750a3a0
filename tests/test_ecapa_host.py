"""ECAPA-TDNN (speech_encoder_type ecapa_channel_1024_wespeaker, and the 192-d extractor): configuration, key layouts,
the torch-functional restatement against the reference goldens, seeded weights, and the C API's argument checks for
the new handle kind.  No GPU."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.weights import (TSVADConfig, ecapa_embed_layout, ecapa_embed_state_dict,  # noqa: E402
                                             ecapa_layout, to_torch, tsvad_layout, tsvad_state_dict)
import ecapa_ref as er  # noqa: E402
from make_golden import embed_wav  # noqa: E402
from make_golden_ecapa import (ECAPA_CASES, ECAPA_NAN_CASES, EMB_CASES, EMB_EXTRACT, EMB_T2, SE_TYPE,  # noqa: E402
                               ecapa_case_inputs, emb_inputs)

GOLD = os.path.join(HERE, "golden")
CFG = TSVADConfig(speech_encoder_type=SE_TYPE)


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def test_config_variants():
    assert CFG.variant == 3
    assert TSVADConfig().variant == 0
    assert TSVADConfig.ots_vad_v1().variant == 1
    assert TSVADConfig(speech_encoder_type="resnet34_wespeaker").variant == 2


def test_v1_style_with_ecapa_raises():
    with pytest.raises(ValueError, match="ots_vad_style v1 is built for CAM\\+\\+_ots_vad"):
        TSVADConfig(speech_encoder_type=SE_TYPE, single_backend_type="conformer_ots_vad",
                    multi_backend_type="lstm_ots_vad", ots_vad_style="v1").variant
    with pytest.raises(ValueError):
        TSVADConfig(speech_encoder_type=SE_TYPE, ots_vad_style="v1").variant
    with pytest.raises(ValueError, match="unsupported TS-VAD configuration"):
        TSVADConfig(speech_encoder_type=SE_TYPE, multi_backend_type="lstm_ots_vad").variant
    with pytest.raises(ValueError, match="unsupported TS-VAD configuration"):
        TSVADConfig(speech_encoder_type="ecapa_channel_512_wespeaker").variant


def _ref_keys(name):
    g = gold(name)
    return {str(n): tuple(int(d) for d in str(s).split(",") if d) for n, s in zip(g["names"], g["shapes"])}


@pytest.mark.parametrize("fixture,layout", [("tsvad_ecapa_keys", lambda: tsvad_layout(CFG)),
                                            ("ecapa_emb_keys", lambda: ecapa_embed_layout(192))])
def test_layout_matches_reference_keys(fixture, layout):
    ref = _ref_keys(fixture)
    lay = layout()
    ours = {n: tuple(s) for n, s, _ in lay}
    assert len(ours) == len(lay), "duplicate key in the layout"
    assert set(ours) == set(ref), (sorted(set(ours) - set(ref))[:5], sorted(set(ref) - set(ours))[:5])
    assert ours == ref


def test_encoder_layout_has_no_pool_or_embedding_head():
    lay = ecapa_layout()
    names = [n for n, _, _ in lay]
    convs = [(n, s) for n, s, _ in lay if ".convs." in n and n.endswith(".weight")]
    assert len(convs) == 21 and all(s == (128, 128, 3) for _, s in convs)
    assert not [n for n in names if ".pool." in n or n.startswith("speech_encoder.bn.") or
                n.startswith("speech_encoder.linear.")]
    emb = [n for n, _, _ in ecapa_embed_layout()]
    assert {"pool.linear1.weight", "pool.linear2.bias", "bn.running_var", "linear.weight"} <= set(emb)


@pytest.mark.parametrize("name", list(ECAPA_CASES))
def test_restatement_matches_reference(name):
    (B, T, nl, _, wseed, keep), x, ts = ecapa_case_inputs(name)
    g = gold(name)
    assert g["speech_enc"].shape == (B, 192, (T - 1) // 4 + 1) and g["logits"].shape == (B, 4, nl)
    sd = to_torch(tsvad_state_dict(CFG, seed=wseed))
    xt = torch.from_numpy(x)
    with torch.no_grad():
        enc = er.speech_encoder_out(sd, xt).numpy()
        logits = er.tsvad_forward(sd, CFG, xt, torch.from_numpy(ts), nl).numpy()
    print(name, "speech_enc err", np.abs(enc - g["speech_enc"]).max(), "logits err", np.abs(logits - g["logits"]).max())
    assert np.abs(enc - g["speech_enc"]).max() < 1e-5
    assert np.abs(logits - g["logits"]).max() < 1e-4
    if keep:
        with torch.no_grad():
            trunk = er.ecapa_time_out(sd, xt).numpy()
        assert g["trunk"].shape == (keep, 1536, T)
        assert np.abs(trunk[:keep] - g["trunk"]).max() < 1e-5


def test_nan_golden_shape():
    name = "tsvad_ecapa_nan"
    (B, T, nl, _, wseed, _), x, ts = ecapa_case_inputs(name)
    bad = ECAPA_NAN_CASES[name][1]
    g, base = gold(name)["logits"], gold(ECAPA_NAN_CASES[name][0])["logits"]
    keep = [i for i in range(B) if i != bad]
    assert np.isnan(g[bad]).all() and np.isfinite(g[keep]).all()
    assert np.abs(g[keep] - base[keep]).max() > 1e-3      # the batch's BatchNorm1D was bypassed
    sd = to_torch(tsvad_state_dict(CFG, seed=wseed))
    got = er.tsvad_forward(sd, CFG, torch.from_numpy(x), torch.from_numpy(ts), nl).numpy()
    assert np.isnan(got[bad]).all() and np.abs(got[keep] - g[keep]).max() < 1e-4


def test_embedding_restatement_matches_reference():
    g = gold("ecapa_emb")
    for name, (B, T, iseed, wseed, keep) in EMB_CASES.items():
        sd = to_torch(ecapa_embed_state_dict(wseed))
        emb, stats, tout = er.ecapa_embed(sd, torch.from_numpy(emb_inputs(B, T, iseed)))
        print(name, np.abs(emb.numpy() - g[f"{name}.emb"]).max(), np.abs(stats.numpy() - g[f"{name}.stats"]).max())
        assert np.abs(emb.numpy() - g[f"{name}.emb"]).max() < 1e-5
        assert np.abs(stats.numpy() - g[f"{name}.stats"]).max() < 1e-5
        if keep:
            assert np.abs(tout.numpy() - g[f"{name}.time_out"]).max() < 1e-5
    B, T, iseed, wseed = EMB_T2
    g = gold("ecapa_emb_t2")
    emb, stats, _ = er.ecapa_embed(to_torch(ecapa_embed_state_dict(wseed)), torch.from_numpy(emb_inputs(B, T, iseed)))
    assert np.isfinite(g["emb"]).all()
    assert np.abs(emb.numpy() - g["emb"]).max() < 1e-5
    assert np.abs(stats.numpy()[:, :1536] - g["stats"][:, :1536]).max() < 1e-5
    # Two frames leave weighted variances next to the 1e-7 clamp, where the reference's own fp32 sum(a x^2) - mean^2
    # cancels: both terms reach max|x|^2 (< 64 on this trunk, maximum ~7), so the difference carries up to
    # 64 * 2^-23 ~ 8e-6 of rounding per term, and sqrt() magnifies that without bound near zero.  Compared as variances.
    assert np.abs(stats.numpy()[:, 1536:] ** 2 - g["stats"][:, 1536:] ** 2).max() < 2e-5


def test_extract_restatement_matches_reference():
    """The reference extract_embed fixture = the restated extractor over the same 6-s chunks of the restated fbank."""
    from oracle import fbank_ref
    g = gold("ecapa_emb_extract")
    secs, bs, wav_seed, wseed = EMB_EXTRACT
    sd = to_torch(ecapa_embed_state_dict(wseed))
    assert list(g["batches"]) == [2, 1]
    for i, s in enumerate(secs):
        wav = np.round(embed_wav(s, wav_seed + i) * 32768).astype(np.int16).astype(np.float64) / 32768.0
        n, L = len(wav), 6 * 16000
        chunks = [(a, a + L) for a in range(0, n - L, 16000)] if n > L else [(0, n)]
        feats = []
        for a, b in chunks:
            f = torch.from_numpy(fbank_ref.fbank(wav[a:b].astype(np.float32).astype(np.float64), 80, 16000, scale=1.0,
                                                 window="povey"))
            feats.append((f - f.mean(0, keepdim=True)).float())
        emb, _, _ = er.ecapa_embed(sd, torch.stack(feats))
        err = np.abs(emb.numpy() - g[f"emb{i}"]).max()
        print("extract", i, emb.shape, "max err", err)
        assert emb.shape == g[f"emb{i}"].shape and err < 1e-5


def _digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        a = np.ascontiguousarray(v)
        h.update(k.encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def test_seeded_weights_are_byte_stable():
    assert _digest(tsvad_state_dict(CFG, seed=780)) == _digest(tsvad_state_dict(CFG, seed=780))
    assert _digest(ecapa_embed_state_dict(922)) == _digest(ecapa_embed_state_dict(922))
    assert _digest(ecapa_embed_state_dict(922)) != _digest(ecapa_embed_state_dict(921))
    sd = tsvad_state_dict(CFG, seed=777)
    # every BatchNorm of the trunk follows a ReLU: running statistics that a wrong-side BatchNorm would show
    m = sd["speech_encoder.layer2.se_res2block.1.bns.3.running_mean"]
    v = sd["speech_encoder.layer2.se_res2block.1.bns.3.running_var"]
    assert m.min() >= 0.2 and m.max() <= 0.6 and v.max() / v.min() > 2.0


NEW_SYMBOLS = ("sd_ecapa_create", "sd_ecapa_set_param", "sd_ecapa_finalize", "sd_ecapa_forward", "sd_ecapa_device_bytes",
               "sd_ecapa_destroy", "sd_ecapa_debug_stats", "sd_op_res2_chain", "sd_op_astp_pool")


def test_library_exports_new_symbols():
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTED and hasattr(lib, s), s


GOOD = dict(channels=1024, embed_dim=192, max_batch=1, max_frames=64, precision=0)


def test_create_rejects_other_channel_counts():
    h = ctypes.c_void_p()
    for ch in (512, 0, 2048):
        with pytest.raises(ValueError, match="builds channels 1024 only"):
            _lib.call("sd_ecapa_create", ctypes.byref(_lib.EcapaConfig(**dict(GOOD, channels=ch))), ctypes.byref(h))
        assert h.value is None
    with pytest.raises(ValueError, match="^sd_ecapa_create: precision must be 0 or 1$"):
        _lib.call("sd_ecapa_create", ctypes.byref(_lib.EcapaConfig(**dict(GOOD, precision=2))), ctypes.byref(h))
    with pytest.raises(ValueError, match="^sd_ecapa_create: null argument$"):
        _lib.call("sd_ecapa_create", None, ctypes.byref(h))


def test_lifecycle_without_a_device():
    """What the lifecycle answers before the library's first HIP call: a forward before finalize is a state error,
    NULL handles are refused or ignored like every other kind's.  (finalize itself uploads weights: set_param after
    finalize is covered on the GPU, tests/test_gpu_ecapa_emb.py.)"""
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.call("sd_ecapa_create", ctypes.byref(_lib.EcapaConfig(**GOOD)), ctypes.byref(h))
    try:
        assert h.value
        data = (ctypes.c_float * 4)(1.0, 2.0, 3.0, 4.0)
        shape = (ctypes.c_int64 * 1)(4)
        _lib.call("sd_ecapa_set_param", h, b"linear.bias", data, shape, 1)
        assert lib.sd_ecapa_forward(h, data, 1, 2, data, None, None) == _lib.SD_ERR_STATE
        assert lib.sd_ecapa_device_bytes(h) == 0
    finally:
        assert lib.sd_ecapa_destroy(h) == _lib.SD_OK
    with pytest.raises(ValueError, match="^sd_ecapa_set_param: null argument$"):
        _lib.call("sd_ecapa_set_param", None, b"w", data, shape, 1)
    with pytest.raises(ValueError, match="^sd_ecapa_finalize: null handle$"):
        _lib.call("sd_ecapa_finalize", None)
    assert lib.sd_ecapa_destroy(None) == _lib.SD_OK
    assert lib.sd_ecapa_device_bytes(None) == 0
