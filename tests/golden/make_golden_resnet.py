"""Golden vectors of TS-VAD with the ResNet34 speech encoder, by running the REFERENCE modules (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_resnet.py

Same method as make_golden.py (whose stubs and inputs it imports): the reference TSVADModel is built with
speech_encoder_type "resnet34_wespeaker", loaded strict=True with the seeded weights of
speaker_diarization_amd.weights, run in eval on seeded inputs; only its outputs are stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs, tsvad_inputs  # noqa: E402

# name: (B, T_fbank, n_label, input seed, weight seed, store the trunk output)
RN34_CASES = {
    "tsvad_rn34_rs4": (2, 398, 100, 1234, 777, False),
    "tsvad_rn34_rs4_short": (3, 198, 50, 4321, 778, False),    # 198 -> 99 -> 50 -> 25: odd maps at two stages
    "tsvad_rn34_tiny": (2, 38, 10, 77, 780, True),             # stage-4 map 10 x 5
}
# name: (base case, window, fbank frame, mel bin of the NaN)
RN34_NAN_CASES = {"tsvad_rn34_nan": ("tsvad_rn34_rs4_short", 2, 5, 0)}


def rn34_case_inputs(name):
    base, nan_at = (RN34_NAN_CASES[name][0], RN34_NAN_CASES[name][1:]) if name in RN34_NAN_CASES else (name, None)
    case = RN34_CASES[base]
    B, T_fb, n_lab, iseed = case[:4]
    ref_speech, ts = tsvad_inputs(B, T_fb, n_lab, seed=iseed)
    if nan_at is not None:
        ref_speech[nan_at] = np.nan
    return case, ref_speech, ts


def reference_model():
    import torch
    from oracle.torchaudio_conformer import Conformer
    install_stubs(Conformer)
    sys.path.insert(0, os.path.join(REF, "egs/alimeeting/ts_vad2"))
    import model as ref_model  # reference TSVADModel
    ref_model.TSVADModel.load_speaker_encoder = lambda self, *a, **k: None
    mcfg = ref_model.TSVADConfig()
    mcfg.speech_encoder_type = "resnet34_wespeaker"
    dcfg = ref_model.TSVADDataConfig()
    dcfg.rs_len = 4
    torch.manual_seed(0)
    m = ref_model.TSVADModel(cfg=mcfg, task_cfg=dcfg)
    m.eval()
    return m


def main():
    import torch
    from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict

    cfg = TSVADConfig(speech_encoder_type="resnet34_wespeaker")
    m = reference_model()
    keys = m.state_dict()
    np.savez_compressed(os.path.join(HERE, "tsvad_rn34_keys.npz"),
                        names=np.array(list(keys), dtype="U"),
                        shapes=np.array([",".join(str(d) for d in v.shape) for v in keys.values()], dtype="U"))
    for name in list(RN34_CASES) + list(RN34_NAN_CASES):
        (B, T_fb, n_lab, iseed, wseed, keep_trunk), ref_speech, ts = rn34_case_inputs(name)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)), strict=True)
        with torch.no_grad():
            x = torch.from_numpy(ref_speech)
            logits = m(x, torch.from_numpy(ts), torch.zeros(B, 4, n_lab), num_updates=0).numpy().astype(np.float32)
            trunk = m.speech_encoder(x.clone(), get_time_out=True)
            enc = m.speech_down_or_up(trunk).numpy().astype(np.float32)
        out = dict(logits=logits, B=np.int64(B), T_fb=np.int64(T_fb), n_label=np.int64(n_lab),
                   input_seed=np.int64(iseed), weight_seed=np.int64(wseed))
        if name in RN34_CASES:
            out["speech_enc"] = enc
        if keep_trunk:
            out["trunk"] = trunk.numpy().astype(np.float32)
        if name == "tsvad_rn34_rs4":
            # the seeded model is alive through its 16 residual blocks
            amax, std, nz = float(np.abs(logits).max()), float(logits.std(-1).mean()), float((enc != 0).mean())
            print(f"{name}: max|logit| {amax:.3f}  std over frames {std:.3f}  speech_enc non-zero {nz:.3f}  "
                  f"trunk max {float(trunk.abs().max()):.3f}")
            assert 0.5 <= amax <= 20.0, amax
            assert std > 0.05, std
            assert nz > 0.30, nz
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(name, {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape},
              os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 650_000, "golden larger than the largest one committed"


if __name__ == "__main__":
    main()
