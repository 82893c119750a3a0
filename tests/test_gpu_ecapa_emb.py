"""The ECAPA-TDNN embedding extractor (ts_vad/embedding.py ECAPA_TDNN_GLOB_c1024, sd_ecapa_*) on the MI355X path
against the reference goldens (tests/golden/make_golden_ecapa.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from make_golden import embed_wav  # noqa: E402
from make_golden_ecapa import EMB_CASES, EMB_EXTRACT, EMB_T2, emb_inputs  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.embedding import ECAPA_TDNN_GLOB_c1024, FBank, extract_embed  # noqa: E402
from speaker_diarization_amd.weights import ecapa_embed_state_dict, to_torch  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(wseed, precision, gpu):
    key = (wseed, precision)
    if key not in _models:
        m = ECAPA_TDNN_GLOB_c1024(feat_dim=80, embed_dim=192, pooling_func="ASTP", device=gpu, precision=precision,
                                  max_batch=3, max_frames=598)
        m.load_state_dict(to_torch(ecapa_embed_state_dict(wseed)))
        _models[key] = m
    return _models[key]


def cosine(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(EMB_CASES))
def test_embeddings_vs_reference_golden(gpu, name, precision):
    B, T, iseed, wseed, keep = EMB_CASES[name]
    g = gold("ecapa_emb")
    m = model(wseed, precision, gpu)
    x = torch.from_numpy(emb_inputs(B, T, iseed)).to(gpu)
    emb = m(x).cpu().numpy()
    stats = m.pooled_stats(B).cpu().numpy()
    err, cos = np.abs(emb - g[f"{name}.emb"]).max(), cosine(emb, g[f"{name}.emb"]).min()
    serr = np.abs(stats - g[f"{name}.stats"]).max()
    print(f"{name} {precision}: max|emb diff| {err:.3e}  min cosine {cos:.6f}  max|stats diff| {serr:.3e}")
    if precision == "fp32":
        assert err < 1e-3 and serr < 1e-3
    else:
        assert cos >= 0.999
    if keep:
        tout = m(x, get_time_out=True)
        assert tout.shape == (B, 1536, T)
        terr = np.abs(tout.cpu().numpy() - g[f"{name}.time_out"]).max()
        print(f"{name} {precision}: max|time_out diff| {terr:.3e} (max {g[f'{name}.time_out'].max():.2f})")
        # bf16: the project's bf16 bar of 3e-2, here relative to the map's maximum (the logits it holds for are O(1))
        assert terr < (1e-3 if precision == "fp32" else 3e-2 * g[f"{name}.time_out"].max())


def test_two_frames(gpu):
    B, T, iseed, wseed = EMB_T2
    g = gold("ecapa_emb_t2")
    m = model(wseed, "fp32", gpu)
    x = torch.from_numpy(emb_inputs(B, T, iseed)).to(gpu)
    emb = m(x).cpu().numpy()
    err = np.abs(emb - g["emb"]).max()
    print(f"t2 fp32: max|emb diff| {err:.3e}")
    assert err < 1e-3
    assert np.abs(m(x, get_time_out=True).cpu().numpy() - g["time_out"]).max() < 1e-3


def test_one_frame_is_refused(gpu):
    m = model(EMB_T2[3], "fp32", gpu)
    x = torch.zeros(1, 1, 80, device=gpu)
    with pytest.raises(AssertionError, match="at least 2 fbank frames"):
        m(x)
    assert m(x, get_time_out=True).shape == (1, 1536, 1)     # the trunk itself runs on one frame
    assert torch.isfinite(m(torch.zeros(1, 2, 80, device=gpu))).all()   # the handle still works


def test_extract_embed_vs_reference_fixture(gpu):
    g = gold("ecapa_emb_extract")
    secs, bs, wav_seed, wseed = EMB_EXTRACT
    m = model(wseed, "fp32", gpu)
    for i, s in enumerate(secs):
        wav = np.round(embed_wav(s, wav_seed + i) * 32768).astype(np.int16).astype(np.float64) / 32768.0
        got = extract_embed(wav, m, batch_size=bs).cpu().numpy()
        err = np.abs(got - g[f"emb{i}"]).max()
        print(f"extract {i}: {got.shape} max|emb diff| {err:.3e}")
        assert got.shape == g[f"emb{i}"].shape and err < 1e-3
    # the extractor's FBank(mean_nor=True) feeds the model directly too
    wav = torch.from_numpy(embed_wav(3.0, wav_seed + 1)).float().to(gpu)
    wav = torch.round(wav * 32768) / 32768
    e = m(FBank(80, 16000, mean_nor=True)(wav)[None]).cpu().numpy()
    assert np.abs(e - g["emb1"]).max() < 1e-3


def test_lifecycle(gpu):
    lib = _lib.load()
    h = ctypes.c_void_p()
    conf = _lib.EcapaConfig(channels=1024, embed_dim=192, max_batch=1, max_frames=16, precision=0)
    _lib.call("sd_ecapa_create", ctypes.byref(conf), ctypes.byref(h))
    try:
        x = torch.zeros(1, 4, 80, device=gpu)
        e = torch.zeros(1, 192, device=gpu)
        assert lib.sd_ecapa_forward(h, _lib.ptr(x), 1, 4, _lib.ptr(e), None, None) == _lib.SD_ERR_STATE
        assert lib.sd_ecapa_device_bytes(h) == 0
        _lib.load_params("ecapa", h, ecapa_embed_state_dict(5))
        assert lib.sd_ecapa_device_bytes(h) > 0
        data = (ctypes.c_float * 1)(1.0)
        shape = (ctypes.c_int64 * 1)(1)
        assert lib.sd_ecapa_set_param(h, b"linear.bias", data, shape, 1) == _lib.SD_ERR_STATE
        assert lib.sd_ecapa_finalize(h) == _lib.SD_ERR_STATE
        _lib.call("sd_ecapa_forward", h, _lib.ptr(x), 1, 4, _lib.ptr(e), None, _lib.stream_ptr(gpu))
        torch.cuda.synchronize()
        assert torch.isfinite(e).all()
    finally:
        assert lib.sd_ecapa_destroy(h) == _lib.SD_OK


def test_strict_load(gpu):
    sd = to_torch(ecapa_embed_state_dict(5))
    sd["bn2.weight"] = torch.zeros(192)
    m = ECAPA_TDNN_GLOB_c1024(device=gpu, precision="fp32", max_batch=1, max_frames=16)
    with pytest.raises(RuntimeError, match="bn2.weight"):
        m.load_state_dict(sd)
    sd = to_torch(ecapa_embed_state_dict(5))
    sd.pop("pool.linear2.bias")
    m = ECAPA_TDNN_GLOB_c1024(device=gpu, precision="fp32", max_batch=1, max_frames=16)
    with pytest.raises(RuntimeError, match="pool.linear2.bias"):
        m.load_state_dict(sd)
