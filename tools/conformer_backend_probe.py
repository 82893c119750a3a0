"""TS-VAD with conformer single and multi back ends (sd_tsvad_config.backend 5) at the recipe's shape: one bf16 forward
of 64 windows at rs_len 6 (598 fbank frames, 150 labels; 256 sequences of 150 frames through the single stack), with the
row programs (the fused stack at FFN hidden 1536, sd_debug_conformer_wide_route(1)) against the per-layer path
(SDIAR_NO_ROWPROG; also the shipped rule at this hidden size).

    python tools/conformer_backend_probe.py [--rounds 5] [--steps 20] [--warmup 5] [--out DIR]

The library reads SDIAR_NO_ROWPROG once, so every measurement is a fresh child process (`--arm`): per round one child per
arm, the order alternating from round to round.  A child builds the seeded model, warms up, times `steps` forwards with
device events and reports their median.  Per arm: the median over the rounds' medians and their spread (max - min).
The fused path is this back end's bf16 default only if its median beats the per-layer one by more than the larger of
the two spreads; the last JSON line carries both arms and that decision (DESIGN.md 5k records the run that set
conformer_stack_default_fused's rule).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

B, RS_LEN, T_FB, N_LABEL = 64, 6, 598, 150
ARMS = {"fused": {}, "per_layer": {"SDIAR_NO_ROWPROG": "1"}}


def child(arm, steps, warmup):
    import numpy as np
    import torch
    from speaker_diarization_amd import _lib
    from speaker_diarization_amd.ts_vad.model import TSVADModel
    from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict
    assert (os.environ.get("SDIAR_NO_ROWPROG") is not None) == (arm == "per_layer")
    _lib.call("sd_debug_conformer_wide_route", 1 if arm == "fused" else 0)
    cfg = TSVADConfig(single_backend_type="conformer", multi_backend_type="conformer", rs_len=RS_LEN)
    assert cfg.backend == 5
    m = TSVADModel(cfg, precision="bf16", max_batch=B).load_state_dict(to_torch(tsvad_state_dict(cfg, seed=2025)))
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((B, T_FB, 80)).astype(np.float32)).cuda()
    ts = torch.from_numpy(rng.standard_normal((B, 4, 192)).astype(np.float32)).cuda()
    out = torch.empty(B, 4, N_LABEL, device="cuda")
    for _ in range(warmup):
        m.forward(x, ts, N_LABEL, out=out, check=False)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m.forward(x, ts, N_LABEL, out=out, check=False)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    m.status()
    assert bool(torch.isfinite(out).all())
    lib = _lib.load()                      # one more forward under the library's timers: which path ran
    lib.sd_prof_reset()
    lib.sd_prof_enable(1)
    m.forward(x, ts, N_LABEL, out=out)
    lib.sd_prof_enable(0)
    programs = sum(v["launches"] for k, v in _lib.prof_stats().items() if k.startswith("rowprog"))
    lib.sd_prof_reset()
    assert (programs > 0) == (arm == "fused"), (arm, programs)
    ms = np.array(ms)
    print(json.dumps(dict(arm=arm, median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
                          steps=steps, checksum=float(out.double().abs().sum()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--arm", choices=list(ARMS), default=None, help="(internal) measure one arm in this process")
    a = ap.parse_args()
    if a.arm:
        child(a.arm, a.steps, a.warmup)
        return
    if a.rounds < 5:
        raise SystemExit("at least 5 alternating rounds per arm")
    import numpy as np
    runs = {k: [] for k in ARMS}
    for r in range(a.rounds):
        order = list(ARMS) if r % 2 == 0 else list(ARMS)[::-1]
        for arm in order:
            env = {k: v for k, v in os.environ.items() if k != "SDIAR_NO_ROWPROG"}
            env.update(ARMS[arm])
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:      # a child that failed ends the probe: nothing more is started on the device
                raise SystemExit(f"round {r} arm {arm} exited with {p.returncode}:\n{p.stdout}\n{p.stderr}")
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            rec["round"] = r
            runs[arm].append(rec)
            print(json.dumps(rec), flush=True)
    arms = {}
    for arm, recs in runs.items():
        med = np.array([x["median_ms"] for x in recs])
        arms[arm] = dict(median_ms=float(np.median(med)), spread_ms=float(med.max() - med.min()),
                         round_medians_ms=[round(float(v), 4) for v in med])
    gain = arms["per_layer"]["median_ms"] - arms["fused"]["median_ms"]
    bar = max(arms["fused"]["spread_ms"], arms["per_layer"]["spread_ms"])
    rec = dict(shape=dict(B=B, rs_len=RS_LEN, fbank_frames=T_FB, labels=N_LABEL, backend=5, precision="bf16"),
               rounds=a.rounds, steps=a.steps, arms=arms, gain_ms=float(gain), bar_ms=float(bar),
               keep_fused_default=bool(gain > bar))
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "conformer_backend_probe.json"), "w") as f:
            json.dump(dict(rec, runs=runs), f, indent=1)


if __name__ == "__main__":
    main()
