"""Golden logits of TS-VAD with the Whisper-PMFA speech encoder ("whisper", variant 8) by running the REFERENCE
MagicData TSVADModel (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tsvad_whisper.py

Same method as make_golden_tsvad_wavlm.py.  The stubbed `whisper` module gets the restated log_mel_spectrogram of
make_golden_whisper.py (FRONT END RESTATED).  The reference can only build the published ModelDimensions(), so
model.ModelDimensions is replaced by a factory returning the case's geometry; a temporary speech_encoder_path holds the
encoder's state_dict; then tsvad_state_dict's seeded weights are loaded strict=True and the model runs in eval on
seeded waveforms.  Only seeds, logits and key names / shapes are stored.

Asserted here: every golden is finite (outside a NaN window) with a logit standard deviation in [0.1, 10]; each of the
wrong implementations of `perturbations` moves the logits by at least ten fp32 bars (the factors are stored in
tsvad_whisper_keys.npz); label lengths 9 and 1 on 5 mix frames raise in the reference.
"""
from __future__ import annotations

import contextlib
import copy
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
from make_golden_whisper import published_log_mel, reference_module  # noqa: E402
from whisper_cases import NAN, PERTURB_CASE, PUBLISHED, RAISES, S, TSVAD, config, tsvad_cfg, tsvad_inputs  # noqa: E402

LIMIT = 650_000
FP32_RTOL = 1e-3


def reference_tsvad(we, cfg, meta=False):
    """The reference TSVADModel of a project TSVADConfig, its encoder at cfg's Whisper geometry."""
    import torch
    from oracle.torchaudio_conformer import Conformer
    from speaker_diarization_amd.weights import to_torch, whisper_state_dict
    sys.modules["torchaudio"].models.Conformer = Conformer
    d = os.path.join(REF, "egs/magicdata-ramc/ts_vad2")
    for q in (os.path.dirname(d), d):
        if q not in sys.path:
            sys.path.insert(0, q)
    import model as ref_model
    assert os.path.dirname(os.path.abspath(ref_model.__file__)) == os.path.abspath(d), ref_model.__file__
    w = cfg.effective_whisper_cfg()
    ref_model.ModelDimensions = lambda: we.ModelDimensions(
        n_mels=w.n_mels, n_audio_ctx=w.n_audio_ctx, n_audio_state=w.n_audio_state, n_audio_head=w.n_audio_head,
        n_audio_layer=w.n_audio_layer, layer_st=w.layer_st, layer_ed=w.layer_ed)
    mcfg = ref_model.TSVADConfig()
    mcfg.speech_encoder_type = "whisper"
    mcfg.whisper_n_mels = cfg.whisper_n_mels
    mcfg.speaker_embed_dim = cfg.speaker_embed_dim
    dcfg = ref_model.TSVADDataConfig()
    dcfg.rs_len = 4
    with tempfile.TemporaryDirectory() as tmp:
        mcfg.speech_encoder_path = os.path.join(tmp, "whisper.pt")
        if meta:      # names and shapes only: the encoder's checkpoint is empty (the reference loads it strict=False)
            torch.save({}, mcfg.speech_encoder_path)
            with torch.device("meta"):
                m = ref_model.TSVADModel(cfg=mcfg, task_cfg=dcfg)
            return m
        torch.save(to_torch(whisper_state_dict(w, 1)), mcfg.speech_encoder_path)
        torch.manual_seed(0)
        m = ref_model.TSVADModel(cfg=mcfg, task_cfg=dcfg)
    return m.eval()


def run(m, wav, ts, n_lab):
    import torch
    with torch.no_grad():
        return m(torch.from_numpy(wav), torch.from_numpy(ts), torch.zeros(wav.shape[0], 4, n_lab),
                 num_updates=0).numpy().astype(np.float32)


def perturbations(we, m, sd, w):
    """name -> (state_dict, context manager factory): wrong implementations of the variant."""
    import torch
    enc = m.speech_encoder

    def edit(**kv):
        out = dict(sd)
        out.update(kv)
        return out

    @contextlib.contextmanager
    def shifted():
        enc.layer_st, enc.layer_ed = w.layer_st - 1, w.layer_ed - 1
        try:
            yield
        finally:
            enc.layer_st, enc.layer_ed = w.layer_st, w.layer_ed

    @contextlib.contextmanager
    def stride1():
        conv2 = enc.conv2
        enc.conv2 = copy.deepcopy(conv2)
        enc.conv2.stride = (1,)
        real, state = we.F.gelu, {"n": 0}

        def gelu(x, **kw):   # the second GELU of the forward sees conv2's stride-1 output: subsample from frame 1
            state["n"] += 1
            return real(x[..., 1::2] if state["n"] == 2 else x, **kw)
        we.F.gelu = gelu
        try:
            yield
        finally:
            we.F.gelu = real
            enc.conv2 = conv2

    @contextlib.contextmanager
    def no_clamp():
        mod = sys.modules["whisper"]
        mod.log_mel_spectrogram = lambda a, n_mels=80: published_log_mel(a, n_mels, clamp=False)
        try:
            yield
        finally:
            mod.log_mel_spectrogram = published_log_mel

    pe = "speech_encoder.positional_embedding"
    return {
        "layer_st shifted by one": (sd, shifted),
        "positional table dropped": (edit(**{pe: torch.zeros_like(sd[pe])}), contextlib.nullcontext),
        "identity ln_post2 affine": (edit(**{"speech_encoder.ln_post2.weight": torch.ones_like(sd["speech_encoder.ln_post2.weight"]),
                                              "speech_encoder.ln_post2.bias": torch.zeros_like(sd["speech_encoder.ln_post2.bias"])}),
                                     contextlib.nullcontext),
        "conv2 at stride 1, subsampled from frame 1": (sd, stride1),
        "max - 8 clamp removed": (sd, no_clamp),
    }


def save(name, out):
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape}, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < LIMIT, "golden larger than the largest one committed"


def main():
    from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict
    we = reference_module()
    models, keys, factors = {}, {}, {}
    for name in list(TSVAD) + list(NAN):
        base = NAN[name][0] if name in NAN else name
        geom, n_mels, _, _, _, se, _, _ = TSVAD[base]
        cfg = tsvad_cfg(name)
        mk = (geom, n_mels, se)
        if mk not in models:
            models[mk] = reference_tsvad(we, cfg)
            sd0 = models[mk].state_dict()
            tag = f"{'s' if geom is S else 'wd'}_m{n_mels}_se{se}"
            keys[tag + ".names"] = np.array(list(sd0), dtype="U")
            keys[tag + ".shapes"] = np.array([",".join(str(d) for d in t.shape) for t in sd0.values()], dtype="U")
        m = models[mk]
        (B, n, n_lab, wseed), wav, ts = tsvad_inputs(name)
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
        if name in (PERTURB_CASE, "tsvad_whisper_tail", "tsvad_whisper_wide"):
            bar = FP32_RTOL * max(1.0, float(np.abs(logits).max()))
            for what, (psd, ctx) in perturbations(we, m, sd, cfg.effective_whisper_cfg()).items():
                if (what == "max - 8 clamp removed") != (name == "tsvad_whisper_tail"):
                    continue      # the clamp shows on the zero tail only; the tail case checks nothing else
                m.load_state_dict(psd, strict=True)
                with ctx():
                    moved = float(np.abs(run(m, wav, ts, n_lab) - logits).max())
                print(f"  {name}: {what}: moves the logits by {moved:.3e} = {moved / bar:.0f} fp32 bars")
                assert moved >= 10 * bar, (name, what, moved, bar)
                factors[f"{name}: {what}"] = moved / bar
            m.load_state_dict(sd, strict=True)
    for base, n_lab in RAISES:      # the reference asserts |gap| <= 3
        cfg = tsvad_cfg(base)
        geom, n_mels, _, _, _, se, _, _ = TSVAD[base]
        m = models[(geom, n_mels, se)]
        (B, n, _, wseed), wav, ts = tsvad_inputs(base)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)), strict=True)
        try:
            run(m, wav, ts, n_lab)
        except AssertionError as e:
            print(f"labels {n_lab} at {n} samples: reference raises: {str(e)[:70]}")
        else:
            raise SystemExit(f"the reference accepted labels {n_lab} at {n} samples")
    # the published 24-layer geometry: names and shapes only, on the meta device
    pub = TSVADConfig(speech_encoder_type="whisper", whisper_cfg=config(PUBLISHED))
    sd0 = reference_tsvad(we, pub, meta=True).state_dict()
    keys["published.names"] = np.array(list(sd0), dtype="U")
    keys["published.shapes"] = np.array([",".join(str(d) for d in t.shape) for t in sd0.values()], dtype="U")
    keys["perturbation.names"] = np.array(list(factors), dtype="U")
    keys["perturbation.fp32_bars"] = np.array(list(factors.values()), np.float64)
    save("tsvad_whisper_keys", keys)


if __name__ == "__main__":
    main()
