"""The w2v-BERT 2.0 trunk at the TS-VAD recipe's shape: B = 64 windows of 200 frames (4 s of fbank, paired), 6 layers,
bf16 and fp32, on the HIP path and on the stock-PyTorch path (tests/w2vbert_ref.py moved to the same GPU under
torch-ROCm, fp32 and autocast bf16) with the same seeded weights.

    python tools/w2vbert_probe.py [--steps 20] [--warmup 5] [--out profiles/r12/w2vbert]

Per configuration: warm-up, then `steps` timed forwards (HIP events around each): mean / min / max / standard
deviation, beside each other.  Then one more HIP forward under the library's own per-kernel event timers
(sd_prof_enable; SDIAR_PROF_DETAIL keys the GEMM families by shape), which is the per-kernel table.  One JSON line per
configuration, and the tables as text under --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

os.environ.setdefault("SDIAR_PROF_DETAIL", "1")     # read once by the library, before its first launch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

B, T2, LAYERS = 64, 200, 6


def setup():
    import numpy as np
    import torch
    from speaker_diarization_amd.ssl.w2vbert import W2vBertConfig
    from speaker_diarization_amd.weights import to_torch, w2vbert_state_dict
    cfg = W2vBertConfig(num_hidden_layers=LAYERS)
    sd = to_torch(w2vbert_state_dict(cfg, 2024))
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((B, T2, 160)).astype(np.float32))
    return cfg, sd, x.cuda()


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    t = torch.tensor(ms, dtype=torch.float64)
    return dict(mean=float(t.mean()), min=float(t.min()), max=float(t.max()), sigma=float(t.std(unbiased=False)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r12", "w2vbert"))
    args = ap.parse_args()
    import torch
    import w2vbert_ref as ref
    from speaker_diarization_amd import _lib
    from speaker_diarization_amd.ssl.w2vbert import W2vBert
    os.makedirs(args.out, exist_ok=True)
    cfg, sd, x = setup()
    sd_gpu = {k: v.cuda() for k, v in sd.items()}
    for precision in ("bf16", "fp32"):
        m = W2vBert(cfg, precision=precision, max_batch=B, max_frames=T2).load_state_dict(sd)
        hip = timed(lambda: m(x), args.steps, args.warmup)

        def torch_fwd():
            if precision == "bf16":
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return ref.trunk(sd_gpu, LAYERS, x)[-1]
            return ref.trunk(sd_gpu, LAYERS, x)[-1]

        base = timed(torch_fwd, args.steps, args.warmup)
        err = float((m(x) - ref.trunk(sd_gpu, LAYERS, x)[-1]).abs().max())
        _lib.load().sd_prof_reset()
        _lib.load().sd_prof_enable(1)
        m(x)
        torch.cuda.synchronize()
        _lib.load().sd_prof_enable(0)
        stats = sorted(_lib.prof_stats().items(), key=lambda kv: -kv[1]["ms"])
        lines = [f"{'kernel family':58s} {'launches':>8s} {'ms':>9s} {'TFLOP/s':>9s} {'GB/s':>9s}"]
        for name, s in stats:
            tf = s["flops"] / s["ms"] / 1e9 if s["ms"] > 0 else 0.0
            gb = s["bytes"] / s["ms"] / 1e6 if s["ms"] > 0 else 0.0
            lines.append(f"{name:58s} {s['launches']:8d} {s['ms']:9.3f} {tf:9.1f} {gb:9.0f}")
        total = sum(s["ms"] for _, s in stats)
        lines.append(f"{'sum of kernel times':58s} {'':8s} {total:9.3f}")
        with open(os.path.join(args.out, f"{precision}_kernels.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        print(json.dumps(dict(config=f"w2vbert_l{LAYERS}_{precision}", B=B, T2=T2, hip_ms=hip, torch_ms=base,
                              torch_over_hip=base["mean"] / hip["mean"], max_abs_diff_vs_torch_fp32=err,
                              device_bytes=m.device_bytes, kernel_ms_sum=total)), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
