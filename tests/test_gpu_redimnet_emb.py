"""The ReDimNetB2 embedding extractor (ts_vad/embedding.py ReDimNetB2, sd_redimnet_*) on the MI355X path against the
reference goldens (tests/golden/make_golden_redimnet.py).

Tolerances.  fp32 and bf16x3: the project's fp32 bar, max|got - golden| <= 1e-3 * max(1, max|golden|).  bf16: nobody had
measured this trunk, so the maxima of one run are recorded per case in BF16_MEASURED and each case is bounded at twice
the largest of them (the convention of tests/test_gpu_tsvad_ecapa.py); both arms of the 2-D block are held to the same
bound against the same golden.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import redimnet_ref as rr  # noqa: E402
from make_golden_redimnet import EMB_CASES, FRAME_CASE, KEEP_FRAMES, T1_CASE, emb_inputs  # noqa: E402
from oracle import fbank_ref  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.embedding import ReDimNetB2, extract_embed  # noqa: E402
from speaker_diarization_amd.weights import redimnet_embed_state_dict, to_torch  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_RTOL = 1e-3
ALL_CASES = dict(EMB_CASES, **{FRAME_CASE[0]: FRAME_CASE[1]})
# bf16 against the fp32 goldens, one run on an MI355X: max |diff| of the embedding and of the stored frames per case
# (the fused and the generic arm of the 2-D block, whichever was larger) and the smallest embedding cosine seen
# (max |embedding| 5.0 .. 6.9, max |frame value| 5.9 .. 10.3).  fused / generic: emb t8 3.90e-2 / 4.43e-2, t77 3.25e-2 /
# 3.25e-2, t398 1.63e-2 / 1.64e-2, f24 4.58e-2 / 4.87e-2; frames t8 4.51e-2 / 4.75e-2, t77 9.62e-2 / 9.97e-2, t398
# 1.167e-1 / 7.59e-2, f24 1.168e-1 / 1.093e-1; cosine >= 0.999967 / 0.999963
BF16_MEASURED = {
    "emb": {"t8": 4.43e-2, "t77": 3.25e-2, "t398": 1.64e-2, "f24": 4.87e-2},
    "frames": {"t8": 4.75e-2, "t77": 9.97e-2, "t398": 1.167e-1, "f24": 1.168e-1},
    "min_cosine": 0.999963,
}
_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(wseed, precision, gpu):
    key = (wseed, precision)
    if key not in _models:
        m = ReDimNetB2(feat_dim=72, embed_dim=192, pooling_func="ASTP", device=gpu, precision=precision, max_batch=2,
                       max_frames=398)
        _models[key] = m.load_state_dict(to_torch(redimnet_embed_state_dict(wseed)))
    return _models[key]


def cosine(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def run_case(m, name, gpu):
    B, T, iseed, _ = ALL_CASES[name]
    x = torch.from_numpy(emb_inputs(B, T, iseed)).to(gpu)
    zero, emb = m(x)
    assert float(zero) == 0.0 and emb.shape == (B, 192)
    frames = m.get_frame_level_feat(x)
    assert frames.shape == (B, T, 1152)
    if name in KEEP_FRAMES:
        frames = frames[:, list(KEEP_FRAMES[name])]
    return emb.cpu().numpy(), frames.cpu().numpy()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", list(ALL_CASES))
def test_fp32_vs_reference_golden(gpu, name, precision):
    g = gold("redimnet_b2_emb")
    emb, frames = run_case(model(ALL_CASES[name][3], precision, gpu), name, gpu)
    ge, gf = g[f"{name}.emb"], g[f"{name}.frames"]
    e1, e2 = np.abs(emb - ge).max(), np.abs(frames - gf).max()
    b1, b2 = FP32_RTOL * max(1.0, np.abs(ge).max()), FP32_RTOL * max(1.0, np.abs(gf).max())
    print(f"{name} {precision}: max|emb diff| {e1:.3e} (bar {b1:.3e})  max|frames diff| {e2:.3e} (bar {b2:.3e})")
    assert np.isfinite(emb).all() and np.isfinite(frames).all()
    assert e1 <= b1 and e2 <= b2


@pytest.mark.parametrize("arm", ["fused", "generic"])
@pytest.mark.parametrize("name", list(ALL_CASES))
def test_bf16_vs_reference_golden(gpu, name, arm):
    g = gold("redimnet_b2_emb")
    m = model(ALL_CASES[name][3], "bf16", gpu).use_generic_blocks(arm == "generic")
    try:
        emb, frames = run_case(m, name, gpu)
    finally:
        m.use_generic_blocks(False)
    ge, gf = g[f"{name}.emb"], g[f"{name}.frames"]
    e1, e2, cos = np.abs(emb - ge).max(), np.abs(frames - gf).max(), cosine(emb, ge).min()
    print(f"{name} bf16 {arm}: max|emb diff| {e1:.3e}  max|frames diff| {e2:.3e}  min cosine {cos:.6f}  "
          f"(max|emb| {np.abs(ge).max():.2f}, max|frames| {np.abs(gf).max():.2f})")
    assert np.isfinite(emb).all() and np.isfinite(frames).all()
    assert e1 <= 2 * max(BF16_MEASURED["emb"].values())
    assert e2 <= 2 * max(BF16_MEASURED["frames"].values())
    assert 1.0 - cos <= 2 * (1.0 - BF16_MEASURED["min_cosine"])


def test_one_frame(gpu):
    g = gold("redimnet_b2_emb")
    name, (B, T, iseed, wseed) = T1_CASE
    m = model(wseed, "fp32", gpu)
    x = torch.from_numpy(emb_inputs(B, T, iseed)).to(gpu)
    with pytest.raises(AssertionError, match="at least 2 fbank frames"):
        m(x)
    with pytest.raises(AssertionError, match="at least 2 fbank frames"):      # the library's own refusal
        _lib.call("sd_redimnet_forward", m._h, _lib.ptr(x), B, T, _lib.ptr(torch.zeros(B, 192, device=gpu)), None,
                  _lib.stream_ptr(gpu))
    frames = m.get_frame_level_feat(x).cpu().numpy()      # the trunk itself runs on one frame
    gf = g[f"{name}.frames"]
    assert np.abs(frames - gf).max() <= FP32_RTOL * max(1.0, np.abs(gf).max())
    assert torch.isfinite(m(torch.zeros(1, 2, 72, device=gpu))[1]).all()      # the handle still works


def test_extract_embed_real_speech_vs_restatement(gpu):
    """extract_embed(..., n_mels=72) on two seconds of the vendored speech sample (one chunk: the whole file) against
    the CPU chain povey fbank (oracle) -> mean removal -> restatement."""
    wav = np.load(os.path.join(GOLD, "sample_wav.npz"))["pcm16"][:32000].astype(np.float32) / 32768.0
    wseed = EMB_CASES["t398"][3]
    m = model(wseed, "fp32", gpu)
    got = extract_embed(wav, m, batch_size=96, n_mels=72).cpu().numpy()
    fb = torch.from_numpy(np.asarray(fbank_ref.fbank(wav.astype(np.float64), 72, 16000, scale=1.0, window="povey"),
                                     np.float32))
    fb = fb - fb.mean(0, keepdim=True)
    want = rr.embed(to_torch(redimnet_embed_state_dict(wseed)), fb[None])[0].numpy()
    err = np.abs(got - want).max()
    print(f"extract_embed real speech: {got.shape} max|emb diff| {err:.3e} (max|emb| {np.abs(want).max():.2f})")
    assert got.shape == want.shape == (1, 192)
    assert err <= FP32_RTOL * max(1.0, np.abs(want).max())


def test_lifecycle(gpu):
    lib = _lib.load()
    h = ctypes.c_void_p()
    conf = _lib.RedimnetConfig(feat_dim=72, embed_dim=192, max_batch=1, max_frames=16, precision=0)
    _lib.call("sd_redimnet_create", ctypes.byref(conf), ctypes.byref(h))
    try:
        x = torch.zeros(1, 4, 72, device=gpu)
        e = torch.zeros(1, 192, device=gpu)
        assert lib.sd_redimnet_forward(h, _lib.ptr(x), 1, 4, _lib.ptr(e), None, None) == _lib.SD_ERR_STATE
        assert lib.sd_redimnet_device_bytes(h) == 0
        _lib.load_params("redimnet", h, redimnet_embed_state_dict(5))
        assert lib.sd_redimnet_device_bytes(h) > 0
        data = (ctypes.c_float * 1)(1.0)
        shape = (ctypes.c_int64 * 1)(1)
        assert lib.sd_redimnet_set_param(h, b"seg_1.bias", data, shape, 1) == _lib.SD_ERR_STATE
        assert lib.sd_redimnet_finalize(h) == _lib.SD_ERR_STATE
        big = torch.zeros(1, 17, 72, device=gpu)
        assert lib.sd_redimnet_forward(h, _lib.ptr(big), 1, 17, _lib.ptr(e), None, None) == _lib.SD_ERR_INVALID
        _lib.call("sd_redimnet_forward", h, _lib.ptr(x), 1, 4, _lib.ptr(e), None, _lib.stream_ptr(gpu))   # still works
        torch.cuda.synchronize()
        assert torch.isfinite(e).all()
    finally:
        assert lib.sd_redimnet_destroy(h) == _lib.SD_OK


def test_strict_load(gpu):
    sd = to_torch(redimnet_embed_state_dict(5))
    sd["seg_2.weight"] = torch.zeros(192, 192)
    m = ReDimNetB2(device=gpu, precision="fp32", max_batch=1, max_frames=16)
    with pytest.raises(RuntimeError, match="seg_2.weight"):
        m.load_state_dict(sd)
    sd = to_torch(redimnet_embed_state_dict(5))
    sd.pop("backbone.stage3.6.tcm.2.pwconv1.bias")
    m = ReDimNetB2(device=gpu, precision="fp32", max_batch=1, max_frames=16)
    with pytest.raises(RuntimeError, match="backbone.stage3.6.tcm.2.pwconv1.bias"):
        m.load_state_dict(sd)
    sd = to_torch(redimnet_embed_state_dict(5))
    sd["backbone.inputs_weights.4"] = torch.zeros(1, 4, 1152, 1)
    m = ReDimNetB2(device=gpu, precision="fp32", max_batch=1, max_frames=16)
    with pytest.raises(RuntimeError, match="backbone.inputs_weights.4 shape"):
        m.load_state_dict(sd)
