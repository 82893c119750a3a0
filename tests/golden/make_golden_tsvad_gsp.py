"""Golden outputs of TS-VAD with speech_encoder_type "CAM++_frame_level_gsp_fc" by running the REFERENCE MagicData
TSVADModel (build container only: it imports the reference).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tsvad_gsp.py

Same method as make_golden_tsvad_conformer.py: egs/magicdata-ramc/ts_vad2/model.py is imported under stub modules for the
packages absent here, load_speaker_encoder is patched out, tsvad_state_dict's seeded weights are loaded strict=True (which
pins the key set: gsp_fc.* and the (SE, 256, 5) conv among them) and TSVADModel.forward runs in eval on seeded inputs, with
the transformer single and multi back ends.  A forward hook on speech_down_or_up captures its output (B, SE, T3), so the
new stage (frame statistics, gsp_fc, the conv, BatchNorm1D, ReLU) is pinned by itself as well as through the logits.

Writes tsvad_gsp.npz (T2 = 19 trunk frames, odd), tsvad_gsp_even.npz (T2 = 20) and tsvad_gsp_se256.npz
(speaker_embed_dim 256: proj_layer): seeds, inputs, logits, the hooked stage output and the state-dict key list with
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

ENCODER = "CAM++_frame_level_gsp_fc"
# name: (speaker_embed_dim, B, T_fbank, label frames, input seed, weight seed)
CASES = {
    "tsvad_gsp": (192, 3, 38, 10, 5200, 791),
    "tsvad_gsp_even": (192, 3, 40, 10, 5201, 792),
    "tsvad_gsp_se256": (256, 3, 38, 10, 5202, 793),
}


def case_cfg(name, **kw):
    from speaker_diarization_amd.weights import TSVADConfig
    return TSVADConfig(speech_encoder_type=ENCODER, speaker_embed_dim=CASES[name][0], **kw)


def case_inputs(name):
    se, B, T, _, iseed, _ = CASES[name]
    rng = np.random.default_rng(iseed)
    return (rng.standard_normal((B, T, 80)).astype(np.float32), rng.standard_normal((B, 4, se)).astype(np.float32))


def reference_tsvad(cfg):
    import torch
    install_stubs()
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
    assert tuple(m.gsp_fc.weight.shape) == (256, 2)
    return m


def main():
    import torch
    from speaker_diarization_amd.weights import to_torch, tsvad_state_dict
    for name, (se, B, T, n_lab, iseed, wseed) in CASES.items():
        cfg = case_cfg(name)
        m = reference_tsvad(cfg)
        sd0 = m.state_dict()
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)), strict=True)
        ref, ts = case_inputs(name)
        stage = []
        hook = m.speech_down_or_up.register_forward_hook(lambda mod, inp, out: stage.append(out.detach().clone()))
        with torch.no_grad():
            logits = m(torch.from_numpy(ref), torch.from_numpy(ts), torch.zeros(B, 4, n_lab),
                       num_updates=0).numpy().astype(np.float32)
        hook.remove()
        assert logits.shape == (B, 4, n_lab), logits.shape
        down = stage[0].numpy().astype(np.float32)
        T3 = ((T - 1) // 2 + 1 - 1) // 2 + 1
        assert len(stage) == 1 and down.shape == (B, se, T3), down.shape
        std = float(logits.std())
        print(f"{name}: logit std {std:.3f}  max |logit| {float(np.abs(logits).max()):.3f}  stage max "
              f"{float(down.max()):.3f}  stage zero fraction {float((down == 0).mean()):.2f}")
        assert np.isfinite(logits).all() and 0.1 <= std <= 10.0, (name, std)
        assert 0.05 <= float((down == 0).mean()) <= 0.95, "the stage's ReLU should cut some values and pass some"
        out = dict(logits=logits, speech_down_or_up=down, ref_speech=ref, ts=ts, B=np.int64(B), T_fb=np.int64(T),
                   n_label=np.int64(n_lab), input_seed=np.int64(iseed), weight_seed=np.int64(wseed),
                   speaker_embed_dim=np.int64(se),
                   names=np.array(list(sd0), dtype="U"),
                   shapes=np.array([",".join(str(d) for d in t.shape) for t in sd0.values()], dtype="U"))
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(name, os.path.getsize(path), "bytes", len(sd0), "keys")
        assert os.path.getsize(path) < 650_000


if __name__ == "__main__":
    main()
