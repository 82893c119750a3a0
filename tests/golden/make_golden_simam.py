"""Golden vectors of the SimAM-ResNet34 (ASP) embedding extractor, by running the REFERENCE module (build container
only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_simam.py

Same method as make_golden_resnet_emb.py: the reference SimAM_ResNet34_ASP is loaded strict=True with the seeded
weights of speaker_diarization_amd.weights and run in eval on seeded inputs; only its outputs (and its state_dict key
names and shapes) are stored.  The script asserts that the seeded reference run is alive: embedding spread, SimAM
gates, attention weights and constant channels.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _stub, embed_wav, install_stubs  # noqa: E402

LIMIT = 650_000   # bytes per fixture, the bound make_golden_resnet_emb.py asserts

# name: (B, T_fbank, input seed, weight seed, store front and stats)
CASES = {
    "t38": (2, 38, 81, 921, True),      # T' = 5
    "t17": (3, 17, 82, 922, False),     # T' = 3; odd maps at every stage (17 -> 9 -> 5 -> 3)
    "t8": (1, 8, 83, 923, False),       # T' = 1: finite, sg = sqrt(1e-5)
    "t200": (2, 200, 84, 924, False),   # T' = 25, several tiles per map
}
# extract_embed over whole wav files: (seconds per file, batch_size, wav seed, weight seed)
EXTRACT = ([7.5, 3.0], 96, 87, 927)


def inputs(name):
    B, T, iseed = CASES[name][:3]
    return np.random.default_rng(iseed).standard_normal((B, T, 80)).astype(np.float32)


def _ref_dir():
    d = os.path.join(REF, "egs/alimeeting/ts_vad2")
    if d not in sys.path:
        sys.path.insert(0, d)


def reference_model():
    import torch
    install_stubs()
    _ref_dir()
    import samresnet_wespeaker as S
    torch.manual_seed(0)
    m = S.SimAM_ResNet34_ASP(in_planes=64, embed_dim=256, acoustic_dim=80, dropout=0, speech_encoder=False)
    m.eval()
    return m


def save(name, out):
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape}, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < LIMIT, "golden larger than the largest one committed"


def make_embeddings():
    import torch
    from speaker_diarization_amd.weights import simam_resnet34_state_dict, to_torch
    out = {}
    m = reference_model()
    sd0 = m.state_dict()
    keys = {"simam_resnet34.names": np.array(list(sd0), dtype="U"),
            "simam_resnet34.shapes": np.array([",".join(str(d) for d in v.shape) for v in sd0.values()], dtype="U")}
    for name, (B, T, _, wseed, keep) in CASES.items():
        m.load_state_dict(to_torch(simam_resnet34_state_dict(wseed, 256)), strict=True)
        x = torch.from_numpy(inputs(name))
        grabbed = {}
        last = m.front.layer4[-1]
        hook = last.bn2.register_forward_hook(lambda mod, i, o: grabbed.__setitem__("y", o.detach().clone()))
        with torch.no_grad():
            emb = m(x.clone())
            fr = m.front(x.clone().permute(0, 2, 1).unsqueeze(1))
            front = fr.reshape(B, -1, fr.shape[-1])
            stats = m.pooling(fr)
            w = m.pooling.attention(front)
        hook.remove()
        out[f"{name}.emb"] = emb.numpy().astype(np.float32)
        assert np.isfinite(out[f"{name}.emb"]).all(), name
        if keep:
            out[f"{name}.front"] = front.numpy().astype(np.float32)
            out[f"{name}.stats"] = stats.numpy().astype(np.float32)
        # --- the seeded reference run is alive
        y = grabbed["y"]
        n = y.shape[2] * y.shape[3] - 1
        d = (y - y.mean(dim=[2, 3], keepdim=True)).pow(2)
        g = torch.sigmoid(d / (4 * (d.sum(dim=[2, 3], keepdim=True) / n + 1e-4)) + 0.5)
        T4 = front.shape[-1]
        const = float((front.std(-1) == 0).float().mean()) if T4 > 1 else 0.0
        print(f"{name}: last-block gates {float(g.min()):.3f} .. {float(g.max()):.3f}; attention weight "
              f"{float(w.min()):.4f} .. {float(w.max()):.4f} (uniform {1.0 / T4:.4f}); constant channels {const:.3f}; "
              f"front max {float(front.max()):.2f}")
        assert float(g.max() - g.min()) > 0.02, "SimAM gates of the last block all within 0.01 of one value"
        if T4 > 1:
            assert float(w.max()) < 0.99 and float((w - 1.0 / T4).abs().max()) > 0.05 / T4, "attention uniform or one-hot"
            assert const < 0.05, const
        if name == "t200":
            std = float(emb.std())
            print(f"{name}: embedding std {std:.3f}")
            assert 0.3 <= std <= 5.0, std
    save("simam_emb", out)
    save("simam_emb_keys", keys)


def make_extract():
    """The reference extract_embed (generate_chunk_..._wespeaker_...py:143-176) on wav files written to a temp dir,
    with the checkpoint-loading extract_embeddings replaced by the seeded SimAM_ResNet34_ASP and kaldi.fbank by the
    restated oracle (torchaudio is absent), as make_golden_resnet_emb.make_extract does for ResNet34."""
    import tempfile
    import wave as wave_mod
    import torch
    from oracle import fbank_ref
    from speaker_diarization_amd.weights import simam_resnet34_state_dict, to_torch
    secs, bs, wav_seed, wseed = EXTRACT
    m = reference_model()
    m.load_state_dict(to_torch(simam_resnet34_state_dict(wseed, 256)), strict=True)

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
    _stub("ecapa_tdnn_wespeaker", **{k: None for k in ("ECAPA_TDNN_c1024", "ECAPA_TDNN_GLOB_c1024", "ECAPA_TDNN_c512",
                                                       "ECAPA_TDNN_GLOB_c512")})   # imported by the script; not run
    import generate_chunk_speaker_embedding_from_wespeaker_for_diarization as G
    batches = []

    def extract_embeddings(args, batch):     # :96-140 minus the checkpoint load
        batches.append(len(batch))
        with torch.no_grad():
            e = m(torch.stack(batch))
        assert not isinstance(e, tuple)      # :132-133 keeps the tensor as it is
        return e.detach()

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
    save("simam_emb_extract", out)


def main():
    make_embeddings()
    make_extract()


if __name__ == "__main__":
    main()
