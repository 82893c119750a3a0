"""Golden vectors of the ReDimNetB2 embedding extractor and of TS-VAD with it as the speech encoder, by running the
REFERENCE modules (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_redimnet.py

Same method as make_golden_ecapa.py: the reference ReDimNetB2 (egs/magicdata-ramc/ts_vad2/redimnet_wespeaker.py, which
needs only pooling_layers_wespeaker beside it) is loaded strict=True with the seeded weights of
speaker_diarization_amd.weights and run in eval on seeded inputs; only seeds, outputs and state_dict key names / shapes
are stored.  Every reference frame-level map must be finite with a standard deviation in [0.1, 10], so that no fixture
is degenerate.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402

LIMIT = 650_000   # bytes per fixture, the bound make_golden_resnet.py asserts
N_MELS = 72
# extractor: name: (B, T_fbank, input seed, weight seed)
EMB_CASES = {"t8": (2, 8, 91, 931), "t77": (2, 77, 92, 932), "t398": (1, 398, 93, 933)}
# the full frame-level map
FRAME_CASE = ("f24", (2, 24, 94, 934))
# T = 1: a finite frame-level map, a non-finite embedding
T1_CASE = ("t1", (2, 1, 95, 935))
# frames of the longer maps that are stored (the whole 1152 channels of each)
KEEP_FRAMES = {"t8": (0, 7), "t77": (0, 38, 76), "t398": (0, 199, 397)}
DIGEST_SEED = 777
SE_TYPE = "ReDimNetB2"
# TS-VAD: name: (B, T_fbank, n_label, input seed, weight seed); 38 / 398 frames give 10 / 100 mix frames, 30 give 8
TSVAD_CASES = {
    "tsvad_redimnet_gap0": (2, 38, 10, 96, 941),
    "tsvad_redimnet_rs4": (2, 398, 100, 97, 942),
    "tsvad_redimnet_pad2": (2, 30, 10, 98, 943),
    "tsvad_redimnet_pad3": (2, 30, 11, 98, 943),
    "tsvad_redimnet_cut3": (2, 30, 5, 98, 943),
}
TSVAD_RAISES = (("tsvad_redimnet_pad3", 12), ("tsvad_redimnet_pad3", 4))     # label lengths the reference asserts on
# name: (base case, window, fbank frame, mel bin of the NaN)
TSVAD_NAN = {"tsvad_redimnet_nan": ("tsvad_redimnet_gap0", 1, 5, 0)}


def tsvad_inputs72(name):
    base, nan_at = (TSVAD_NAN[name][0], TSVAD_NAN[name][1:]) if name in TSVAD_NAN else (name, None)
    B, T_fb, n_lab, iseed, wseed = TSVAD_CASES[base]
    rng = np.random.default_rng(iseed)
    ref_speech = rng.standard_normal((B, T_fb, N_MELS)).astype(np.float32)
    ts = rng.standard_normal((B, 4, 192)).astype(np.float32)
    if nan_at is not None:
        ref_speech[nan_at] = np.nan
    return (B, T_fb, n_lab, iseed, wseed), ref_speech, ts


def emb_inputs(B, T, iseed):
    return np.random.default_rng(iseed).standard_normal((B, T, N_MELS)).astype(np.float32)


def state_digest(sd) -> str:
    """sha256 over the names, shapes and bytes of a seeded state_dict: byte stability of the seeding."""
    h = hashlib.sha256()
    for k, v in sd.items():
        a = np.ascontiguousarray(v)
        h.update(k.encode())
        h.update(str(a.shape).encode())
        h.update(str(a.dtype).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def reference_redimnet():
    import torch
    install_stubs()
    d = os.path.join(REF, "egs/magicdata-ramc/ts_vad2")
    if d not in sys.path:
        sys.path.insert(0, d)
    import redimnet_wespeaker as R
    torch.manual_seed(0)
    m = R.ReDimNetB2(feat_dim=N_MELS, embed_dim=192, pooling_func="ASTP", two_emb_layer=False)
    m.eval()
    return m


def reference_tsvad():
    """The reference MagicData TSVADModel with speech_encoder_type "ReDimNetB2" (imports under the stubs of SURVEY
    Appendix A; the checkpoint load of the speech encoder is skipped: the seeded weights are loaded strict=True)."""
    import torch
    from oracle.torchaudio_conformer import Conformer
    install_stubs(Conformer)
    d = os.path.join(REF, "egs/magicdata-ramc/ts_vad2")
    for q in (os.path.dirname(d), d):      # ERes2NetV2.py there imports ts_vad2.* as a package
        if q not in sys.path:
            sys.path.insert(0, q)
    import model as ref_model
    assert os.path.dirname(os.path.abspath(ref_model.__file__)) == os.path.abspath(d), ref_model.__file__
    ref_model.TSVADModel.load_speaker_encoder = lambda self, *a, **k: None
    mcfg = ref_model.TSVADConfig()
    mcfg.speech_encoder_type = SE_TYPE
    dcfg = ref_model.TSVADDataConfig()
    dcfg.rs_len = 4
    torch.manual_seed(0)
    m = ref_model.TSVADModel(cfg=mcfg, task_cfg=dcfg)
    m.eval()
    return m


def make_tsvad():
    import torch
    from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict
    cfg = TSVADConfig(speech_encoder_type=SE_TYPE)
    m = reference_tsvad()
    sd0 = m.state_dict()
    save("tsvad_redimnet_keys", dict(names=np.array(list(sd0), dtype="U"),
                                     shapes=np.array([",".join(str(d) for d in v.shape) for v in sd0.values()], dtype="U")))
    for name in list(TSVAD_CASES) + list(TSVAD_NAN):
        (B, T_fb, n_lab, iseed, wseed), ref_speech, ts = tsvad_inputs72(name)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)), strict=True)
        with torch.no_grad():
            x = torch.from_numpy(ref_speech)
            logits = m(x, torch.from_numpy(ts), torch.zeros(B, 4, n_lab), num_updates=0).numpy().astype(np.float32)
        assert logits.shape == (B, 4, n_lab), logits.shape
        out = dict(logits=logits, B=np.int64(B), T_fb=np.int64(T_fb), n_label=np.int64(n_lab),
                   input_seed=np.int64(iseed), weight_seed=np.int64(wseed))
        if name in TSVAD_CASES:
            with torch.no_grad():
                frames = m.speech_encoder.get_frame_level_feat(x.clone())
                enc = m.speech_down_or_up(frames.transpose(1, 2)).numpy().astype(np.float32)
            alive(name, frames)
            assert np.isfinite(logits).all() and float(logits.std(-1).mean()) > 0.02, float(logits.std(-1).mean())
            print(f"{name}: max|logit| {float(np.abs(logits).max()):.3f}  speech_enc non-zero {float((enc != 0).mean()):.3f}")
            out["speech_enc"] = enc
        save(name, out)
    for base, n_lab in TSVAD_RAISES:      # the reference asserts |gap| <= 3
        (B, T_fb, _, iseed, wseed), ref_speech, ts = tsvad_inputs72(base)
        try:
            with torch.no_grad():
                m(torch.from_numpy(ref_speech), torch.from_numpy(ts), torch.zeros(B, 4, n_lab), num_updates=0)
        except AssertionError as e:
            print(f"labels {n_lab} at T_fb {T_fb}: reference raises: {str(e)[:70]}")
        else:
            raise SystemExit(f"the reference accepted labels {n_lab} at T_fb {T_fb}")


def save(name, out):
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape}, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < LIMIT, "golden larger than the largest one committed"


def alive(name, frames):
    f = frames.numpy()
    std = float(f.std())
    print(f"{name}: frame-level map std {std:.3f}  max |x| {float(np.abs(f).max()):.3f}")
    assert np.isfinite(f).all(), name
    assert 0.1 <= std <= 10.0, (name, std)


def main():
    import torch
    from speaker_diarization_amd.weights import redimnet_embed_state_dict, to_torch
    m = reference_redimnet()
    sd0 = m.state_dict()
    keys = dict(names=np.array(list(sd0), dtype="U"),
                shapes=np.array([",".join(str(d) for d in v.shape) for v in sd0.values()], dtype="U"),
                n_params=np.int64(sum(p.numel() for p in m.parameters())),
                digest=np.array(state_digest(redimnet_embed_state_dict(DIGEST_SEED))), digest_seed=np.int64(DIGEST_SEED))
    assert len(sd0) == 548 and int(keys["n_params"]) == 4888241, (len(sd0), keys["n_params"])
    save("redimnet_b2_keys", keys)
    out = {}
    for name, (B, T, iseed, wseed) in list(EMB_CASES.items()) + [FRAME_CASE, T1_CASE]:
        m.load_state_dict(to_torch(redimnet_embed_state_dict(wseed)), strict=True)
        x = torch.from_numpy(emb_inputs(B, T, iseed))
        with torch.no_grad():
            zero, emb = m(x.clone())
            frames = m.get_frame_level_feat(x.clone())            # (B, T, 1152)
        assert float(zero) == 0.0 and tuple(frames.shape) == (B, T, 1152)
        alive(name, frames)
        if name == T1_CASE[0]:
            assert not np.isfinite(emb.numpy()).any()
            out[f"{name}.frames"] = frames.numpy().astype(np.float32)
            continue
        assert np.isfinite(emb.numpy()).all()
        print(f"{name}: embedding std {float(emb.std()):.3f}")
        assert 0.05 <= float(emb.std()) <= 20.0, float(emb.std())
        out[f"{name}.emb"] = emb.numpy().astype(np.float32)
        if name == FRAME_CASE[0]:
            out[f"{name}.frames"] = frames.numpy().astype(np.float32)
        else:
            out[f"{name}.frames"] = frames[:, list(KEEP_FRAMES[name])].numpy().astype(np.float32)
    save("redimnet_b2_emb", out)


if __name__ == "__main__":
    main()
    make_tsvad()
