"""Golden outputs of TS-VAD with the conformer back ends by running the REFERENCE MagicData TSVADModel (build container
only: it imports the reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tsvad_conformer.py

Same method as make_golden_w2vbert.py: egs/magicdata-ramc/ts_vad2/model.py is imported under stub modules for the
packages absent here, load_speaker_encoder is patched out, tsvad_state_dict's seeded weights are loaded strict=True (which
pins the key set, the BatchNorm buffers of the conv module included) and TSVADModel.forward runs in eval on seeded
inputs.  torchaudio is absent, so oracle.torchaudio_conformer.Conformer is installed as torchaudio.models.Conformer: the
goldens pin everything AROUND the conformer (the batch-first call with the positional encoding inside, proj_layer, the
speaker stacking, backend_down with its BatchNorm1D, the multi back end, fc) to a reference run, while the conformer
arithmetic itself stays "parity unpinned", as for ots_vad_style v1.

Writes tsvad_conf_t.npz (single "conformer" + multi "transformer"), tsvad_conf_c.npz ("conformer" for both) and
tsvad_conf_c_se256.npz (speaker_embed_dim 256: proj_layer): seeds, inputs, logits and the state-dict key list with
shapes.  Only data is stored; the weights are regenerated from the seed.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, install_stubs  # noqa: E402

# name: (multi_backend_type, speaker_embed_dim, B, T_fbank, label frames, input seed, weight seed)
CASES = {
    "tsvad_conf_t": ("transformer", 192, 3, 38, 10, 5100, 781),
    "tsvad_conf_c": ("conformer", 192, 3, 38, 10, 5101, 782),
    "tsvad_conf_c_se256": ("conformer", 256, 3, 38, 10, 5102, 783),
}


def case_cfg(name):
    from speaker_diarization_amd.weights import TSVADConfig
    multi, se = CASES[name][:2]
    return TSVADConfig(single_backend_type="conformer", multi_backend_type=multi, speaker_embed_dim=se)


def case_inputs(name):
    _, se, B, T, _, iseed, _ = CASES[name]
    rng = np.random.default_rng(iseed)
    return (rng.standard_normal((B, T, 80)).astype(np.float32), rng.standard_normal((B, 4, se)).astype(np.float32))


def reference_tsvad(cfg):
    import torch
    from oracle.torchaudio_conformer import Conformer
    install_stubs(Conformer)
    d = os.path.join(REF, "egs/magicdata-ramc/ts_vad2")
    for q in (os.path.dirname(d), d):
        if q not in sys.path:
            sys.path.insert(0, q)
    import model as ref_model
    assert os.path.dirname(os.path.abspath(ref_model.__file__)) == os.path.abspath(d), ref_model.__file__
    ref_model.TSVADModel.load_speaker_encoder = lambda self, *a, **k: None
    mcfg = ref_model.TSVADConfig()
    mcfg.speech_encoder_type = cfg.speech_encoder_type
    mcfg.single_backend_type = cfg.single_backend_type
    mcfg.multi_backend_type = cfg.multi_backend_type
    mcfg.speaker_embed_dim = cfg.speaker_embed_dim
    assert (mcfg.num_attention_head, mcfg.num_transformer_layer, mcfg.transformer_embed_dim,
            mcfg.transformer_ffn_embed_dim) == (cfg.num_attention_head, cfg.num_transformer_layer,
                                                cfg.transformer_embed_dim, cfg.transformer_ffn_embed_dim)
    dcfg = ref_model.TSVADDataConfig()
    dcfg.rs_len = cfg.rs_len
    torch.manual_seed(0)
    m = ref_model.TSVADModel(cfg=mcfg, task_cfg=dcfg)
    m.eval()
    assert isinstance(m.single_backend, Conformer) and not m.single_backend.use_group_norm
    return m


def main():
    import torch
    from speaker_diarization_amd.weights import to_torch, tsvad_state_dict
    for name, (multi, se, B, T, n_lab, iseed, wseed) in CASES.items():
        cfg = case_cfg(name)
        m = reference_tsvad(cfg)
        sd0 = m.state_dict()
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)), strict=True)
        ref, ts = case_inputs(name)
        with torch.no_grad():
            logits = m(torch.from_numpy(ref), torch.from_numpy(ts), torch.zeros(B, 4, n_lab),
                       num_updates=0).numpy().astype(np.float32)
        assert logits.shape == (B, 4, n_lab), logits.shape
        std = float(logits.std())
        print(f"{name}: logit std {std:.3f}  max |logit| {float(np.abs(logits).max()):.3f}")
        assert np.isfinite(logits).all() and 0.1 <= std <= 10.0, (name, std)
        out = dict(logits=logits, ref_speech=ref, ts=ts, B=np.int64(B), T_fb=np.int64(T), n_label=np.int64(n_lab),
                   input_seed=np.int64(iseed), weight_seed=np.int64(wseed), speaker_embed_dim=np.int64(se),
                   multi_backend_type=np.array(multi),
                   names=np.array(list(sd0), dtype="U"),
                   shapes=np.array([",".join(str(d) for d in t.shape) for t in sd0.values()], dtype="U"))
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(name, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 650_000


if __name__ == "__main__":
    main()
