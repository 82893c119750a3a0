"""Golden vectors of the ERes2NetV2 embedding extractor, by running the REFERENCE module (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eres2net.py [emb] [frames] [extract]

Same method as make_golden_simam.py: the reference ERes2NetV2 (egs/alimeeting/ts_vad2/ERes2NetV2.py; the frame-level
methods of egs/magicdata-ramc/ots_vad/ERes2NetV2.py) is loaded strict=True with the seeded weights of
speaker_diarization_amd.weights and run in eval on seeded inputs; only its outputs (and its state_dict key names and
shapes) are stored.  The script asserts that the seeded reference run is alive: the Hardtanh's upper clamp fires on a
share of the elements but not everywhere, the AFF gates' tanh neither vanishes nor saturates, and the embedding spread
is in the band the other generators use.
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _stub, embed_wav, install_stubs  # noqa: E402

LIMIT = 650_000   # bytes per fixture, the bound make_golden_resnet_emb.py asserts

# tag: (baseWidth, scale, expansion)
TRIPLES = {"base": (26, 2, 2), "w24": (24, 4, 4)}
# name: (B, T_fbank, input seed, weight seed)
CASES = {
    "t38": (2, 38, 91, 931),      # T' = 5; stats and the fuse34 frame map of window 0 are stored
    "t17": (3, 17, 92, 932),      # odd maps at every stage: 17 -> 9 -> 5 -> 3
    "t9": (1, 9, 93, 933),        # T' = 2: the smallest finite case
    "t8": (1, 8, 94, 934),        # T' = 1: NaN stds, all-NaN embedding; the frame map is finite
    "t200": (2, 200, 95, 935),    # T' = 25, several tiles per map
}
# base triple only: the frame-level outputs.  name: (B, T_fbank, input seed, weight seed)
FRAME_CASES = {
    "f17": (1, 17, 96, 936),      # get_frame_level_feat_frame_rate25 (1, 10240, 5), whole
    "f100": (1, 100, 97, 937),    # both outputs, (1, 10240, 13) and (1, 10240, 25), subsampled in time
}
F100_T = (0, 6, 12)               # stored frames of get_frame_level_feat
F100_T25 = (0, 12, 24)            # stored frames of get_frame_level_feat_frame_rate25
# extract_embed over whole wav files at the modelscope entry's triple: (seconds per file, batch_size, wav seed, weight seed)
EXTRACT = ([7.5, 3.0], 96, 98, 938)


def inputs(name):
    B, T, iseed = (CASES.get(name) or FRAME_CASES[name])[:3]
    return np.random.default_rng(iseed).standard_normal((B, T, 80)).astype(np.float32)


def _module(rel):
    """The reference ERes2NetV2 module under REF/`rel` (the two recipe directories hold one each, same name)."""
    d = os.path.join(REF, rel)
    pkg = os.path.join(REF, "egs/alimeeting")   # the magicdata copy imports ts_vad2.fusion / ts_vad2.pooling_layers_3d_speaker
    for n in ("ERes2NetV2", "fusion", "pooling_layers_3d_speaker", "pooling_layers"):
        sys.modules.pop(n, None)
    sys.path[:0] = [d, pkg]
    try:
        return importlib.import_module("ERes2NetV2")
    finally:
        sys.path.remove(d)
        sys.path.remove(pkg)


def reference_model(triple, rel="egs/alimeeting/ts_vad2"):
    import torch
    install_stubs()
    E = _module(rel)
    torch.manual_seed(0)
    bw, sc, ex = triple
    m = E.ERes2NetV2(feat_dim=80, embedding_size=192, m_channels=64, baseWidth=bw, scale=sc, expansion=ex,
                     pooling_func="TSTP", two_emb_layer=False)
    m.eval()
    return m


def save(name, out):
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape}, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < LIMIT, "golden larger than the largest one committed"


def frames(x):
    """(B, C, F, T) -> (B, F C, T) as get_frame_level_feat orders it."""
    return x.transpose(1, 3).flatten(2).permute(0, 2, 1)


def make_embeddings(tag):
    import torch
    from speaker_diarization_amd.weights import eres2netv2_state_dict, to_torch
    triple = TRIPLES[tag]
    m = reference_model(triple)
    sd0 = m.state_dict()
    keys = {f"{tag}.names": np.array(list(sd0), dtype="U"),
            f"{tag}.shapes": np.array([",".join(str(d) for d in v.shape) for v in sd0.values()], dtype="U")}
    out, maps = {}, {}
    clamp_share = []
    for name, (B, T, _, wseed) in CASES.items():
        m.load_state_dict(to_torch(eres2netv2_state_dict(wseed, *triple, 192)), strict=True)
        x = torch.from_numpy(inputs(name))
        grabbed = {}
        hooks = [m.fuse34.register_forward_hook(lambda mod, i, o: grabbed.__setitem__("fuse", o.detach().clone())),
                 m.pool.register_forward_hook(lambda mod, i, o: grabbed.__setitem__("stats", o.detach().clone())),
                 m.layer4.register_forward_hook(lambda mod, i, o: grabbed.__setitem__("out4", o.detach().clone())),
                 m.fuse34.local_att.register_forward_hook(
                     lambda mod, i, o: grabbed.__setitem__("t34", torch.tanh(o.detach()))),
                 m.layer3[-1].fuse_models[0].local_att.register_forward_hook(
                     lambda mod, i, o: grabbed.__setitem__("t3", torch.tanh(o.detach()))),
                 m.layer4[-1].fuse_models[-1].local_att.register_forward_hook(
                     lambda mod, i, o: grabbed.__setitem__("t4", torch.tanh(o.detach())))]
        with torch.no_grad():
            emb = m(x.clone())
        for h in hooks:
            h.remove()
        out[f"{name}.emb"] = emb.numpy().astype(np.float32)
        fu = grabbed["fuse"]
        T4 = fu.shape[-1]
        if name == "t8":
            assert T4 == 1 and bool(torch.isnan(emb).all()), "8 frames must give an all-NaN embedding"
            out[f"{name}.nan"] = np.isnan(out[f"{name}.emb"])
            maps[f"{name}.frame"] = frames(fu).numpy().astype(np.float32)
            assert np.isfinite(maps[f"{name}.frame"]).all()
        else:
            assert np.isfinite(out[f"{name}.emb"]).all(), name
        if name == "t38":
            out[f"{name}.stats"] = grabbed["stats"][:1].numpy().astype(np.float32)
            maps[f"{name}.frame"] = frames(fu)[:1].numpy().astype(np.float32)
        # --- the seeded reference run is alive
        o4 = grabbed["out4"]
        share = float((o4 == 20).float().mean())
        clamp_share.append(share)
        spans = {k: (float(grabbed[k].min()), float(grabbed[k].max()), float((grabbed[k].abs() > 0.999).float().mean()))
                 for k in ("t3", "t4", "t34")}
        print(f"{tag} {name}: out4 at the clamp {share:.4f}, zero {float((o4 == 0).float().mean()):.3f}; tanh "
              + "; ".join(f"{k} {a:.3f} .. {b:.3f} (|t| > 0.999: {s:.3f})" for k, (a, b, s) in spans.items()))
        assert share < 0.5, "the clamp at 20 fires nearly everywhere"
        for k, (a, b, s) in spans.items():
            assert b - a > 0.1 and s < 0.5, f"{k}: AFF tanh flat or saturated"
        if name == "t200":
            std = float(emb.std())
            print(f"{tag} {name}: embedding std {std:.3f}")
            assert 0.3 <= std <= 5.0, std
    assert max(clamp_share) > 0.01, "the clamp at 20 never fires on a non-trivial share of out4"
    save(f"eres2net_{tag}_emb", out)
    save(f"eres2net_{tag}_frames", maps)
    return keys


def make_frames():
    """get_frame_level_feat / get_frame_level_feat_frame_rate25 of the magicdata copy of the class (base triple)."""
    import torch
    from speaker_diarization_amd.weights import eres2netv2_state_dict, to_torch
    m = reference_model(TRIPLES["base"], "egs/magicdata-ramc/ots_vad")
    out = {}
    for name, (B, T, _, wseed) in FRAME_CASES.items():
        m.load_state_dict(to_torch(eres2netv2_state_dict(wseed, *TRIPLES["base"], 192)), strict=True)
        with torch.no_grad():
            f25 = m.get_frame_level_feat_frame_rate25(torch.from_numpy(inputs(name)))
            f = m.get_frame_level_feat(torch.from_numpy(inputs(name)))
        if name == "f17":
            assert tuple(f25.shape) == (1, 10240, 5), f25.shape
            out["f17.frame25"] = f25.numpy().astype(np.float32)
        else:
            assert tuple(f.shape) == (1, 10240, 13) and tuple(f25.shape) == (1, 10240, 25), (f.shape, f25.shape)
            out["f100.frame"] = f[:, :, list(F100_T)].numpy().astype(np.float32)
            out["f100.frame25"] = f25[:, :, list(F100_T25)].numpy().astype(np.float32)
            out["f100.frame_t"] = np.array(F100_T, np.int64)
            out["f100.frame25_t"] = np.array(F100_T25, np.int64)
    save("eres2net_base_frames2", out)


def make_extract():
    """The reference extract_embed (generate_chunk_speaker_embedding_from_modelscope_for_diarization.py:271-304) on wav
    files written to a temp dir, with the checkpoint download and load of extract_embeddings replaced by the seeded
    ERes2NetV2 at the script's (24, 4, 4) and kaldi.fbank by the restated oracle (torchaudio is absent), as
    make_golden_simam.make_extract does."""
    import tempfile
    import wave as wave_mod
    import torch
    from oracle import fbank_ref
    from speaker_diarization_amd.weights import eres2netv2_state_dict, to_torch
    secs, bs, wav_seed, wseed = EXTRACT
    m = reference_model(TRIPLES["w24"])
    m.load_state_dict(to_torch(eres2netv2_state_dict(wseed, *TRIPLES["w24"], 192)), strict=True)

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
    for n in ("modelscope", "modelscope.hub", "modelscope.hub.snapshot_download"):
        _stub(n, snapshot_download=None)
    d = os.path.join(REF, "egs/alimeeting/ts_vad2")
    if d not in sys.path:
        sys.path.insert(0, d)
    import generate_chunk_speaker_embedding_from_modelscope_for_diarization as G
    batches = []

    def extract_embeddings(args, batch):     # :215-268 minus the download and the checkpoint load
        batches.append(len(batch))
        with torch.no_grad():
            return m(torch.stack(batch)).detach()

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
    save("eres2net_extract", out)


def main():
    only = sys.argv[1:]
    if not only or "emb" in only:
        keys = {}
        for tag in TRIPLES:
            keys.update(make_embeddings(tag))
        save("eres2net_keys", keys)
    if not only or "frames" in only:
        make_frames()
    if not only or "extract" in only:
        make_extract()


if __name__ == "__main__":
    main()
