"""Golden vectors of the WavLM feature extractor, by running the REFERENCE module (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wavlm.py

Same method as make_golden_redimnet.py: the reference WavLM (egs/magicdata-ramc/ts_vad2/wavlm.py with modules.py beside
it) is loaded strict=True with the seeded weights of speaker_diarization_amd.weights.wavlm_state_dict and run in eval on
seeded waveforms; only seeds, state_dict key names / shapes, a weight digest, the reference's relative-position bucket
row and outputs at selected frames are stored.

The seeded weights must make the goldens sensitive to every term of the gated relative-position attention: for each
stored case long enough to have the term, zeroing relative_attention_bias.weight, grep_linear.weight, grep_linear.bias
(all layers), grep_a, the positional conv or q_proj.weight, and negating layer 0's GroupNorm / LayerNorm weight, must
each move the stored outputs by at least ten times the fp32 bar 1e-3 max(1, max |golden|).  k_proj.bias is exempt: it
cannot change a softmax over keys.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402
from make_golden_redimnet import state_digest  # noqa: E402

LIMIT = 650_000   # bytes per fixture, the bound the other generators assert
BUCKET_SPAN = 3000
DIGEST_SEED = 777
BASE_PLUS = dict(encoder_embed_dim=768, encoder_ffn_embed_dim=3072, encoder_attention_heads=12,
                 extractor_mode="default", layer_norm_first=False)
LARGE = dict(encoder_embed_dim=1024, encoder_ffn_embed_dim=4096, encoder_attention_heads=16,
             extractor_mode="layer_norm", layer_norm_first=True)
# name: (geometry, encoder_layers, B, n_samples, output_layer settings, input seed, weight seed)
CASES = {
    "bp_t1": (BASE_PLUS, 2, 2, 400, (2,), 101, 1001),
    "bp_t2": (BASE_PLUS, 2, 2, 720, (2,), 102, 1002),
    "bp_t49": (BASE_PLUS, 2, 2, 16000, (2,), 103, 1003),
    "bp_t109": (BASE_PLUS, 2, 1, 35000, (2,), 104, 1004),
    "bp_t199": (BASE_PLUS, 3, 1, 64000, (2, None), 105, 1005),
    "lg_t49": (LARGE, 2, 2, 16000, (None, 2), 106, 1006),
    "lg_t1": (LARGE, 2, 2, 400, (2,), 107, 1007),
}


def case_config(name):
    from speaker_diarization_amd.ssl.wavlm import WavLMConfig
    geom, layers = CASES[name][:2]
    return WavLMConfig(dict(geom, encoder_layers=layers))


def case_input(name):
    _, _, B, n, _, iseed, _ = CASES[name]
    return (np.random.default_rng(iseed).standard_normal((B, n)) * 0.5).astype(np.float32)


def keep_frames(T: int):
    return sorted({0, T // 2, T - 1})


def tag(output_layer) -> str:
    return "none" if output_layer is None else str(output_layer)


def reference_wavlm(cfg):
    import torch
    install_stubs()
    d = os.path.join(REF, "egs/magicdata-ramc/ts_vad2")
    if d not in sys.path:
        sys.path.insert(0, d)
    import wavlm as W
    torch.manual_seed(0)
    m = W.WavLM(W.WavLMConfig(dict(cfg.__dict__)))
    m.eval()
    return m


def run(m, wav, settings, frames):
    """{key: array at `frames`} of x per output_layer setting, of features and of every layer_results entry."""
    import torch
    out = {}
    with torch.no_grad():
        for ol in settings:
            (x, results), pm = m.extract_features(torch.from_numpy(wav), output_layer=ol, ret_layer_results=True)
            assert pm is None
            out[f"x_{tag(ol)}"] = x[:, frames].numpy().astype(np.float32)
            if ol is None:
                assert results == []
                continue
            assert len(results) == ol + 1 and all(z is None for _, z in results)
            for i, (h, _) in enumerate(results):
                assert h.shape == (x.shape[1], x.shape[0], x.shape[2])
                out[f"layer_{i}"] = h.transpose(0, 1)[:, frames].numpy().astype(np.float32)
        feats, _ = m.extract_features(torch.from_numpy(wav), ret_conv=True)
        out["features"] = feats[:, frames].numpy().astype(np.float32)
    return out


def mutations(sd, long_enough: bool):
    """name -> mutated copy of the seeded state dict."""
    import torch

    def edit(pred, fn):
        return {k: (fn(v) if pred(k) else v) for k, v in sd.items()}

    zero = torch.zeros_like
    norm0 = "feature_extractor.conv_layers.0.2"
    muts = {
        # the gain g and the bias: the whole conv (a zero v would make g v / |v| 0 / 0)
        "pos_conv": edit(lambda k: k.startswith("encoder.pos_conv.0.") and not k.endswith("original1"), zero),
        "layer0 norm sign": edit(lambda k: k in (norm0 + ".weight", norm0 + ".1.weight"), lambda v: -v),
    }
    if long_enough:
        for key in ("relative_attention_bias.weight", "grep_linear.weight", "grep_linear.bias", "grep_a",
                    "q_proj.weight"):
            muts[key] = edit(lambda k, key=key: k.endswith("self_attn." + key), zero)
    return muts


def main():
    import torch
    from speaker_diarization_amd.weights import to_torch, wavlm_state_dict
    keys = {}
    for gname, case in (("bp", "bp_t49"), ("lg", "lg_t49")):
        cfg = case_config(case)
        sd0 = reference_wavlm(cfg).state_dict()
        keys[f"{gname}.names"] = np.array(list(sd0), dtype="U")
        keys[f"{gname}.shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd0.values()], dtype="U")
        keys[f"{gname}.digest"] = np.array(state_digest(wavlm_state_dict(cfg, DIGEST_SEED)))
    keys["digest_seed"] = np.int64(DIGEST_SEED)
    m = reference_wavlm(case_config("bp_t49"))
    rel = torch.arange(-(BUCKET_SPAN - 1), BUCKET_SPAN)
    keys["buckets"] = m.encoder.layers[0].self_attn._relative_positions_bucket(rel).numpy().astype(np.int32)
    assert keys["buckets"].shape == (2 * BUCKET_SPAN - 1,) and keys["buckets"].max() == 319
    save("wavlm_keys", keys)

    for name, (_, _, B, n, settings, iseed, wseed) in CASES.items():
        cfg = case_config(name)
        m = reference_wavlm(cfg)
        sd = to_torch(wavlm_state_dict(cfg, wseed))
        m.load_state_dict(sd, strict=True)
        wav = case_input(name)
        with torch.no_grad():
            T = m.extract_features(torch.from_numpy(wav))[0].shape[1]
        frames = keep_frames(T)
        out = run(m, wav, settings, frames)
        full = np.concatenate([v.ravel() for k, v in out.items() if k.startswith("x_")])
        std, peak = float(full.std()), float(max(np.abs(v).max() for v in out.values()))
        print(f"{name}: T {T}  x std {std:.3f}  max |.| {peak:.3f}")
        assert all(np.isfinite(v).all() for v in out.values()), name
        assert 0.1 <= std <= 10.0, (name, std)
        bar = 1e-3 * max(1.0, peak)
        for mname, msd in mutations(sd, T >= 2).items():
            m.load_state_dict(msd, strict=True)
            got = run(m, wav, settings, frames)
            moved = max(float(np.abs(got[k] - out[k]).max()) for k in out if k.startswith("x_"))
            print(f"    {mname}: moves the stored x by {moved:.3g} ({moved / bar:.0f} bars)")
            assert moved >= 10 * bar, (name, mname, moved, bar)
        out.update(B=np.int64(B), n_samples=np.int64(n), T=np.int64(T), frames=np.array(frames, dtype=np.int64),
                   input_seed=np.int64(iseed), weight_seed=np.int64(wseed))
        save(f"wavlm_{name}", out)


def save(name, out):
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape}, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= LIMIT, "golden larger than the bound"


if __name__ == "__main__":
    main()
