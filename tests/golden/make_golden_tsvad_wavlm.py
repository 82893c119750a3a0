"""Golden logits of TS-VAD with the WavLM speech encoders ("WavLM", variant 5; "WavLM_weight_sum" with
wavlm_fuse_feat_post_norm, variant 6) by running the REFERENCE MagicData TSVADModel (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tsvad_wavlm.py

Same method as make_golden_redimnet.py.  The reference builds its encoder from cfg.speech_encoder_path, so a temporary
{"cfg", "model"} checkpoint is written from wavlm_state_dict; then tsvad_state_dict's seeded weights are loaded
strict=True and the model runs in eval on seeded waveforms.  Only seeds, logits and key names / shapes are stored.

Asserted here: every golden is finite (outside a NaN window) with a logit standard deviation in [0.1, 10]; each of the
perturbations of PERTURB moves the logits by at least ten fp32 bars (the observed factors are stored in
tsvad_wavlm_keys.npz); and WavLM_weight_sum without wavlm_fuse_feat_post_norm raises in the reference's forward.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402
from make_golden_wavlm import BASE_PLUS, LARGE  # noqa: E402

LIMIT = 650_000
# name: (variant, geometry, layers, B, n_samples, n_label, speaker_embed_dim, input seed, weight seed)
CASES = {
    "tsvad_wavlm5_bp": (5, BASE_PLUS, 2, 2, 16000, 25, 192, 201, 2001),
    "tsvad_wavlm5_rs4": (5, BASE_PLUS, 2, 1, 64000, 100, 192, 202, 2002),
    "tsvad_wavlm5_pad2": (5, BASE_PLUS, 2, 2, 3280, 7, 192, 203, 2003),
    "tsvad_wavlm5_pad3": (5, BASE_PLUS, 2, 2, 3280, 8, 192, 203, 2003),
    "tsvad_wavlm5_cut3": (5, BASE_PLUS, 2, 2, 3280, 2, 192, 203, 2003),
    "tsvad_wavlm5_t1": (5, BASE_PLUS, 2, 1, 640, 1, 192, 204, 2004),
    "tsvad_wavlm5_lg": (5, LARGE, 2, 2, 16000, 25, 192, 205, 2005),
    "tsvad_wavlm6_bp": (6, BASE_PLUS, 3, 2, 16000, 25, 192, 211, 2011),
    "tsvad_wavlm6_rs4": (6, BASE_PLUS, 3, 1, 64000, 100, 192, 212, 2012),
    "tsvad_wavlm6_pad3": (6, BASE_PLUS, 3, 2, 3280, 8, 192, 213, 2013),
    "tsvad_wavlm6_lg": (6, LARGE, 2, 2, 16000, 25, 192, 214, 2014),
    "tsvad_wavlm6_se256": (6, BASE_PLUS, 3, 2, 16000, 25, 256, 215, 2015),
}
RAISES = (("tsvad_wavlm5_pad3", 9), ("tsvad_wavlm5_pad3", 1))   # label lengths the reference asserts on (5 mix frames)
# name: (base case, window, sample of the NaN)
NAN = {"tsvad_wavlm5_nan": ("tsvad_wavlm5_bp", 1, 777)}
FP32_RTOL = 1e-3


def case_cfg(name):
    """The project's TSVADConfig of a case."""
    from speaker_diarization_amd.ssl.wavlm import WavLMConfig
    from speaker_diarization_amd.weights import TSVADConfig
    v, geom, layers, _, _, _, se, _, _ = CASES[NAN[name][0] if name in NAN else name]
    if v == 5:   # the checkpoint's own depth (two layers more) is overridden by select_encoder_layer_nums
        return TSVADConfig(speech_encoder_type="WavLM", wavlm_cfg=WavLMConfig(dict(geom, encoder_layers=layers + 2)),
                           select_encoder_layer_nums=layers, speaker_embed_dim=se)
    return TSVADConfig(speech_encoder_type="WavLM_weight_sum", wavlm_cfg=WavLMConfig(dict(geom, encoder_layers=layers)),
                       wavlm_fuse_feat_post_norm=True, speaker_embed_dim=se)


def case_inputs(name):
    base, nan_at = (NAN[name][0], NAN[name][1:]) if name in NAN else (name, None)
    _, _, _, B, n, n_lab, se, iseed, wseed = CASES[base]
    rng = np.random.default_rng(iseed)
    wav = (rng.standard_normal((B, n)) * 0.5).astype(np.float32)
    ts = rng.standard_normal((B, 4, se)).astype(np.float32)
    if nan_at is not None:
        wav[nan_at] = np.nan
    return (B, n, n_lab, wseed), wav, ts


def reference_tsvad(cfg, post_norm=True):
    """The reference TSVADModel of a project TSVADConfig (imports under the stubs of SURVEY Appendix A)."""
    import torch
    from oracle.torchaudio_conformer import Conformer
    from speaker_diarization_amd.weights import to_torch, wavlm_state_dict
    install_stubs(Conformer)
    d = os.path.join(REF, "egs/magicdata-ramc/ts_vad2")
    for q in (os.path.dirname(d), d):
        if q not in sys.path:
            sys.path.insert(0, q)
    import model as ref_model
    assert os.path.dirname(os.path.abspath(ref_model.__file__)) == os.path.abspath(d), ref_model.__file__
    mcfg = ref_model.TSVADConfig()
    mcfg.speech_encoder_type = cfg.speech_encoder_type
    mcfg.select_encoder_layer_nums = cfg.select_encoder_layer_nums
    mcfg.wavlm_fuse_feat_post_norm = post_norm
    mcfg.speaker_embed_dim = cfg.speaker_embed_dim
    dcfg = ref_model.TSVADDataConfig()
    dcfg.rs_len = 4
    w = cfg.wavlm_cfg
    with tempfile.TemporaryDirectory() as tmp:
        mcfg.speech_encoder_path = os.path.join(tmp, "wavlm.pt")
        torch.save({"cfg": dict(w.__dict__), "model": to_torch(wavlm_state_dict(w, 1))}, mcfg.speech_encoder_path)
        torch.manual_seed(0)
        m = ref_model.TSVADModel(cfg=mcfg, task_cfg=dcfg)
    m.eval()
    return m


def run(m, wav, ts, n_lab):
    import torch
    with torch.no_grad():
        return m(torch.from_numpy(wav), torch.from_numpy(ts), torch.zeros(wav.shape[0], 4, n_lab),
                 num_updates=0).numpy().astype(np.float32)


def perturbations(m, sd, variant, large):
    """name -> (state_dict, context manager factory) pairs as callables that run the perturbed model."""
    import contextlib
    import torch
    enc = m.speech_encoder
    real = enc.extract_features

    @contextlib.contextmanager
    def patched(fn):
        enc.extract_features = fn
        try:
            yield
        finally:
            enc.extract_features = real

    def edit(key, fn):
        out = dict(sd)
        out[key] = fn(sd[key].clone())
        return out

    p = {}
    if variant == 6:
        def shifted(src, **kw):   # hss[0:-1] instead of hss[1:]
            (x, res), pm = real(src, **kw)
            return (x, [res[0]] + res[:-1]), pm
        p["permute weights.weight"] = (edit("weights.weight", lambda w: torch.roll(w, 1, 1)), contextlib.nullcontext)
        p["layer selection shifted by one"] = (sd, lambda: patched(shifted))
        p["zero wavlmproj.bias"] = (edit("wavlmproj.bias", torch.zeros_like), contextlib.nullcontext)
        ident = edit("wavlmlnorm.weight", torch.ones_like)
        ident["wavlmlnorm.bias"] = torch.zeros_like(sd["wavlmlnorm.bias"])
        p["identity wavlmlnorm affine"] = (ident, contextlib.nullcontext)
    else:
        L = len(enc.encoder.layers)

        def fewer(src, **kw):     # one encoder layer fewer
            return real(src, output_layer=L - 1, **kw)
        p["one layer fewer"] = (sd, lambda: patched(fewer))
        if large:
            ln = enc.encoder.layer_norm

            @contextlib.contextmanager
            def no_final_ln():
                enc.encoder.layer_norm = torch.nn.Identity()
                try:
                    yield
                finally:
                    enc.encoder.layer_norm = ln
            p["skip final encoder.layer_norm"] = (sd, no_final_ln)
    return p


def save(name, out):
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape}, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < LIMIT, "golden larger than the largest one committed"


def main():
    import torch
    from speaker_diarization_amd.weights import to_torch, tsvad_state_dict
    models, keys, factors = {}, {}, {}
    for name in list(CASES) + list(NAN):
        base = NAN[name][0] if name in NAN else name
        v, geom, layers, _, _, _, se, _, _ = CASES[base]
        cfg = case_cfg(name)
        mk = (v, geom is LARGE, layers, se)
        if mk not in models:
            models[mk] = reference_tsvad(cfg)
            sd0 = models[mk].state_dict()
            tag = f"v{v}_{'lg' if geom is LARGE else 'bp'}_l{layers}_se{se}"
            keys[tag + ".names"] = np.array(list(sd0), dtype="U")
            keys[tag + ".shapes"] = np.array([",".join(str(d) for d in t.shape) for t in sd0.values()], dtype="U")
        m = models[mk]
        (B, n, n_lab, wseed), wav, ts = case_inputs(name)
        sd = to_torch(tsvad_state_dict(cfg, seed=wseed))
        m.load_state_dict(sd, strict=True)
        logits = run(m, wav, ts, n_lab)
        assert logits.shape == (B, 4, n_lab), logits.shape
        good = logits if name not in NAN else np.delete(logits, NAN[name][1], 0)
        if name in NAN:
            assert np.isnan(logits[NAN[name][1]]).all()
        std = float(good.std())
        print(f"{name}: logit std {std:.3f}  max |logit| {float(np.abs(good).max()):.3f}")
        assert np.isfinite(good).all() and 0.1 <= std <= 10.0, (name, std)
        save(name, dict(logits=logits, B=np.int64(B), n_samples=np.int64(n), n_label=np.int64(n_lab),
                        weight_seed=np.int64(wseed)))
        if name in ("tsvad_wavlm5_bp", "tsvad_wavlm5_lg", "tsvad_wavlm6_bp", "tsvad_wavlm6_lg"):
            bar = FP32_RTOL * max(1.0, float(np.abs(logits).max()))
            for what, (psd, ctx) in perturbations(m, sd, v, geom is LARGE).items():
                m.load_state_dict(psd, strict=True)
                with ctx():
                    moved = float(np.abs(run(m, wav, ts, n_lab) - logits).max())
                print(f"  {name}: {what}: moves the logits by {moved:.3e} = {moved / bar:.0f} fp32 bars")
                assert moved >= 10 * bar, (name, what, moved, bar)
                factors[f"{name}: {what}"] = moved / bar
            m.load_state_dict(sd, strict=True)
    for base, n_lab in RAISES:      # the reference asserts |gap| <= 3
        cfg = case_cfg(base)
        v, geom, layers, _, _, _, se, _, _ = CASES[base]
        m = models[(v, geom is LARGE, layers, se)]
        (B, n, _, wseed), wav, ts = case_inputs(base)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)), strict=True)
        try:
            run(m, wav, ts, n_lab)
        except AssertionError as e:
            print(f"labels {n_lab} at {n} samples: reference raises: {str(e)[:70]}")
        else:
            raise SystemExit(f"the reference accepted labels {n_lab} at {n} samples")
    # WavLM_weight_sum without wavlm_fuse_feat_post_norm: the reference's forward raises (model.py:1206-1213)
    cfg = case_cfg("tsvad_wavlm6_bp")
    m = reference_tsvad(cfg, post_norm=False)
    (B, n, n_lab, _), wav, ts = case_inputs("tsvad_wavlm6_bp")
    try:
        run(m, wav, ts, n_lab)
    except RuntimeError as e:
        raised = str(e)
        print("wavlm_fuse_feat_post_norm=False: reference raises:", raised[:90])
        assert "is invalid for input of size" in raised, raised
    else:
        raise SystemExit("the reference ran WavLM_weight_sum without wavlm_fuse_feat_post_norm")
    keys["post_norm_false_raises"] = np.array(raised[:200])
    keys["perturbation.names"] = np.array(list(factors), dtype="U")
    keys["perturbation.fp32_bars"] = np.array(list(factors.values()), np.float64)
    save("tsvad_wavlm_keys", keys)


if __name__ == "__main__":
    main()
