"""Golden vectors of the ResNet34 embedding extractor and of TS-VAD with proj_layer (speaker_embed_dim 256), by
running the REFERENCE modules (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_resnet_emb.py

Same method as make_golden_resnet.py: the reference ResNet34 / TSVADModel are loaded strict=True with the seeded
weights of speaker_diarization_amd.weights and run in eval on seeded inputs; only their outputs (and their
state_dict key names and shapes) are stored.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _stub, embed_wav, install_stubs  # noqa: E402

LIMIT = 650_000   # bytes per fixture, the bound make_golden_resnet.py asserts

# name: (B, T_fbank, two_emb_layer, input seed, weight seed, store stats and time_out)
EMB_CASES = {
    "t38": (2, 38, False, 61, 901, True),      # T' = 5
    "t17": (3, 17, False, 62, 902, False),     # T' = 3; odd maps at every stage (17 -> 9 -> 5 -> 3)
    "t200": (2, 200, False, 63, 903, False),   # T' = 25
    "t9": (1, 9, False, 64, 904, False),       # T' = 2, the shortest finite case
    "t8": (1, 8, False, 65, 905, False),       # T' = 1: all NaN
    "two": (2, 38, True, 66, 906, False),      # both embeddings
}
# extract_embed over whole wav files: (seconds per file, batch_size, wav seed, weight seed)
EMB_EXTRACT = ([7.5, 3.0], 96, 67, 907)
# TS-VAD with speaker_embed_dim 256, transformer_embed_dim 384: name: (speech_encoder_type, B, T_fbank, labels,
# input seed, weight seed, (window, speaker, feature) of a NaN in the target embeddings or None)
PROJ_SE = 256
PROJ_CASES = {
    "rn34": ("resnet34_wespeaker", 2, 198, 50, 71, 911, None),
    "rn34_tiny": ("resnet34_wespeaker", 2, 38, 10, 72, 912, None),
    "campp": ("CAM++", 2, 198, 50, 73, 913, None),
    "rn34_nan": ("resnet34_wespeaker", 2, 38, 10, 72, 912, (1, 2, 7)),
}


def emb_inputs(name):
    B, T, _, iseed = EMB_CASES[name][:4]
    return np.random.default_rng(iseed).standard_normal((B, T, 80)).astype(np.float32)


def proj_inputs(name):
    """(ref_speech (B, T_fb, 80), target_speech (B, 4, 256)) of a PROJ_CASES name."""
    _, B, T_fb, _, iseed, _, nan_at = PROJ_CASES[name]
    rng = np.random.default_rng(iseed)
    ref_speech = rng.standard_normal((B, T_fb, 80)).astype(np.float32)
    ts = rng.standard_normal((B, 4, PROJ_SE)).astype(np.float32)
    if nan_at is not None:
        ts[nan_at] = np.nan
    return ref_speech, ts


def proj_config(name):
    from speaker_diarization_amd.weights import TSVADConfig
    return TSVADConfig(speech_encoder_type=PROJ_CASES[name][0], speaker_embed_dim=PROJ_SE)


def _ref_dir():
    d = os.path.join(REF, "egs/alimeeting/ts_vad2")
    if d not in sys.path:
        sys.path.insert(0, d)


def keys_of(m):
    sd = m.state_dict()
    return (np.array(list(sd), dtype="U"),
            np.array([",".join(str(d) for d in v.shape) for v in sd.values()], dtype="U"))


def reference_resnet34(two_emb_layer):
    import torch
    install_stubs()
    _ref_dir()
    import resnet_wespeaker as R
    torch.manual_seed(0)
    m = R.ResNet34(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=two_emb_layer, speech_encoder=False)
    m.eval()
    return m


def reference_tsvad(speech_encoder_type):
    import torch
    from oracle.torchaudio_conformer import Conformer
    install_stubs(Conformer)
    _ref_dir()
    import model as ref_model
    ref_model.TSVADModel.load_speaker_encoder = lambda self, *a, **k: None
    mcfg = ref_model.TSVADConfig()
    mcfg.speech_encoder_type = speech_encoder_type
    mcfg.speaker_embed_dim = PROJ_SE
    dcfg = ref_model.TSVADDataConfig()
    dcfg.rs_len = 4
    torch.manual_seed(0)
    m = ref_model.TSVADModel(cfg=mcfg, task_cfg=dcfg)
    m.eval()
    return m


def save(name, out):
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape}, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < LIMIT, "golden larger than the largest one committed"


def make_embeddings(keys):
    import torch
    from speaker_diarization_amd.weights import resnet34_embed_state_dict, to_torch
    out = {}
    for name, (B, T, two, iseed, wseed, keep) in EMB_CASES.items():
        m = reference_resnet34(two)
        keys["resnet34_two" if two else "resnet34_one"] = keys_of(m)
        m.load_state_dict(to_torch(resnet34_embed_state_dict(wseed, 256, two)), strict=True)
        x = torch.from_numpy(emb_inputs(name))
        with torch.no_grad():
            a, b = m(x.clone())
            tout = m(x.clone(), get_time_out=True)
            stats = m.pool(tout.reshape(B, 256, 10, -1))
        out[f"{name}.emb"] = b.numpy().astype(np.float32)
        if two:
            out[f"{name}.emb_a"] = a.numpy().astype(np.float32)
        if keep:
            out[f"{name}.stats"] = stats.numpy().astype(np.float32)
            out[f"{name}.time_out"] = tout.numpy().astype(np.float32)
            dead = float((tout.std(-1) == 0).float().mean())
            print(f"{name}: channels constant over time {dead:.3f}")
        if name == "t200":
            std = float(b.std())
            print(f"{name}: embedding std {std:.3f}")
            assert 0.3 <= std <= 5.0, std   # the seeded model is alive through the pooled head
    assert np.isnan(out["t8.emb"]).all() and np.isfinite(out["t9.emb"]).all()
    save("resnet_emb", out)


def make_extract():
    """The reference extract_embed (generate_chunk_..._wespeaker_...py:143-176) on wav files written to a temp dir,
    with the checkpoint-loading extract_embeddings replaced by the seeded ResNet34 and kaldi.fbank by the restated
    oracle (torchaudio is absent), as make_golden.make_campp_extract does for CAM++."""
    import tempfile
    import wave as wave_mod
    import torch
    from oracle import fbank_ref
    from speaker_diarization_amd.weights import resnet34_embed_state_dict, to_torch
    secs, bs, wav_seed, wseed = EMB_EXTRACT
    m = reference_resnet34(False)
    m.load_state_dict(to_torch(resnet34_embed_state_dict(wseed, 256, False)), strict=True)

    def kaldi_fbank(waveform, num_mel_bins=23, sample_frequency=16000.0, dither=0.0, window_type="povey", **kw):
        assert dither == 0.0 and not kw, kw
        x = waveform[0].numpy().astype(np.float64)
        return torch.from_numpy(fbank_ref.fbank(x, num_mel_bins, int(sample_frequency), scale=1.0, window=window_type))

    sys.modules["torchaudio.compliance.kaldi"].fbank = kaldi_fbank

    def sf_read(path, start=0, stop=None):
        with wave_mod.open(path, "rb") as w:
            a = np.frombuffer(w.readframes(w.getnframes()), np.int16).astype(np.float64) / 32768.0
        return a[start:stop], 16000

    sys.modules["soundfile"].read = sf_read
    for n in ("ecapa_tdnn_wespeaker", "samresnet_wespeaker"):   # other extractors the script imports; not run
        _stub(n, **{k: None for k in ("ECAPA_TDNN_c1024", "ECAPA_TDNN_GLOB_c1024", "ECAPA_TDNN_c512",
                                      "ECAPA_TDNN_GLOB_c512", "SimAM_ResNet34_ASP", "SimAM_ResNet100_ASP")})
    import generate_chunk_speaker_embedding_from_wespeaker_for_diarization as G
    batches = []

    def extract_embeddings(args, batch):     # :96-140 minus the checkpoint load
        batches.append(len(batch))
        with torch.no_grad():
            e = m(torch.stack(batch))
        return e[-1].detach()

    G.extract_embeddings = extract_embeddings
    args = types.SimpleNamespace(length_embedding=6, step_embedding=1, batch_size=bs)
    fe = G.FBank(80, sample_rate=16000, mean_nor=True)
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for i, s in enumerate(secs):
            wav = embed_wav(s, wav_seed + i)
            path = os.path.join(td, f"spk{i}.wav")
            with wave_mod.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(np.round(wav * 32768).astype(np.int16).tobytes())
            out[f"emb{i}"] = G.extract_embed(args, path, fe).numpy().astype(np.float32)
    out["batches"] = np.array(batches, np.int64)
    save("resnet_emb_extract", out)


def make_proj(keys):
    import torch
    from speaker_diarization_amd.weights import to_torch, tsvad_state_dict
    out = {}
    models = {}
    for name, (enc, B, T_fb, n_lab, _, wseed, _) in PROJ_CASES.items():
        if enc not in models:
            models[enc] = reference_tsvad(enc)
            keys["tsvad_rn34_se256" if enc == "resnet34_wespeaker" else "tsvad_campp_se256"] = keys_of(models[enc])
        m = models[enc]
        m.load_state_dict(to_torch(tsvad_state_dict(proj_config(name), seed=wseed)), strict=True)
        ref_speech, ts = proj_inputs(name)
        with torch.no_grad():
            logits = m(torch.from_numpy(ref_speech), torch.from_numpy(ts), torch.zeros(B, 4, n_lab), num_updates=0)
        out[f"{name}.logits"] = logits.numpy().astype(np.float32)
        lg = out[f"{name}.logits"]
        if name in ("rn34", "campp"):
            amax, std = float(np.abs(lg).max()), float(lg.std(-1).mean())
            print(f"{name}: max|logit| {amax:.3f}  std over frames {std:.3f}")
            assert 0.5 <= amax <= 20.0 and std > 0.05, (amax, std)
    nan = out["rn34_nan.logits"]
    assert np.isnan(nan[1]).all() and np.isfinite(nan[0]).all()
    save("tsvad_proj", out)


def main():
    keys = {}
    make_embeddings(keys)
    make_extract()
    make_proj(keys)
    flat = {}
    for model, (names, shapes) in keys.items():
        flat[f"{model}.names"], flat[f"{model}.shapes"] = names, shapes
    save("resnet_emb_keys", flat)


if __name__ == "__main__":
    main()
