"""The gsp_down kernel (speech_encoder_type "CAM++_frame_level_gsp_fc") at the recipe's shape against the stage it
replaces in the CAM++ model, the speech_down_or_up conv GEMM: 64 windows at rs_len 6 (598 fbank frames, T2 = 299 trunk
frames, T3 = 150 mix frames), both models on the same build, bf16 and fp32.

    python tools/gsp_down_probe.py [--rounds 5] [--steps 10] [--out DIR]

Both times come from the library's own kernel timer (HIP events around each launch, SDIAR_PROF_DETAIL keys so the one
GEMM with N = speaker_embed_dim, 5 taps and the out_nonlinear prologue can be told from the others).  Per precision
the two models alternate for `rounds` rounds of `steps` forwards after a warm-up; per round the mean time per launch,
then the median over rounds and the spread (max - min).  GB/s: the bytes gsp_down has to move (the trunk map once, the
outputs once) over its time.  The last line is one JSON record.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

os.environ["SDIAR_PROF_DETAIL"] = "1"   # read once by the library, before its first GEMM

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

B, RS_LEN, T_FB, N_LABEL, SE = 64, 6, 598, 150, 192
T2 = (T_FB - 1) // 2 + 1
T3 = (T2 - 1) // 2 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from speaker_diarization_amd import _lib
    from speaker_diarization_amd.ts_vad.model import TSVADModel
    from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict
    lib = _lib.load()
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((B, T_FB, 80)).astype(np.float32)).cuda()
    ts = torch.from_numpy(rng.standard_normal((B, 4, SE)).astype(np.float32)).cuda()
    out = torch.empty(B, 4, N_LABEL, device="cuda")
    rec = dict(shape=dict(B=B, rs_len=RS_LEN, fbank_frames=T_FB, T2=T2, T3=T3, speaker_embed_dim=SE), rounds=a.rounds,
               steps=a.steps)

    def timed(m, pick):
        lib.sd_prof_reset()
        lib.sd_prof_enable(1)
        for _ in range(a.steps):
            m.forward(x, ts, N_LABEL, out=out)
        lib.sd_prof_enable(0)
        hits = {k: v for k, v in _lib.prof_stats().items() if pick(k)}
        lib.sd_prof_reset()
        assert len(hits) == 1, sorted(hits)
        (k, v), = hits.items()
        assert v["launches"] == a.steps, (k, v)
        return k, v["ms"] / v["launches"], v["bytes"] / v["launches"]

    for precision in ("bf16", "fp32"):
        models = {}
        for name, kw in (("gsp", dict(speech_encoder_type="CAM++_frame_level_gsp_fc")), ("campp", dict())):
            cfg = TSVADConfig(rs_len=RS_LEN, **kw)
            models[name] = TSVADModel(cfg, precision=precision, max_batch=B).load_state_dict(
                to_torch(tsvad_state_dict(cfg, seed=2025)))
            for _ in range(3):
                models[name].forward(x, ts, N_LABEL, out=out)
        pick = {"gsp": lambda k: k == "gsp_down",
                "campp": lambda k: f" N={SE} " in k and " taps=5" in k and k.endswith(" pre")}
        ms = {"gsp": [], "campp": []}
        keys, nbytes = {}, {}
        for r in range(a.rounds):
            for name in (("gsp", "campp") if r % 2 == 0 else ("campp", "gsp")):
                keys[name], t, nbytes[name] = timed(models[name], pick[name])
                ms[name].append(t)
        assert bool(torch.isfinite(out).all())
        g, c = np.array(ms["gsp"]), np.array(ms["campp"])
        rec[precision] = dict(
            gsp_down_us=round(float(np.median(g)) * 1e3, 2), gsp_down_spread_us=round(float(g.max() - g.min()) * 1e3, 2),
            gsp_down_bytes=nbytes["gsp"], gsp_down_GBps=round(nbytes["gsp"] / (float(np.median(g)) * 1e-3) / 1e9, 1),
            down_gemm_key=keys["campp"], down_gemm_us=round(float(np.median(c)) * 1e3, 2),
            down_gemm_spread_us=round(float(c.max() - c.min()) * 1e3, 2))
        print(precision, json.dumps(rec[precision]), flush=True)
        del models
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "gsp_down_probe.json"), "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
