"""The Whisper-PMFA encoder at the TS-VAD recipe's shape: B = 64 windows of 64000 samples (4 s), the published geometry
(1280 wide, 20 heads, 24 blocks, blocks 16..23 concatenated to 10240), bf16 and fp32, on the HIP path and on the
stock-PyTorch path (tests/whisper_ref.py moved to the same GPU under torch-ROCm, fp32 and autocast bf16) with the same
seeded weights.

    python tools/whisper_probe.py [--steps 20] [--warmup 5] [--out profiles/r13/whisper]

Per configuration: warm-up, then `steps` timed forwards (HIP events around each): mean / min / max / standard
deviation, beside each other.  Then one more HIP forward under the library's own per-kernel event timers
(sd_prof_enable; SDIAR_PROF_DETAIL keys the GEMM families by shape), which is the per-kernel table and the front end's
share.  One JSON line per configuration (also appended to probe.jsonl), and the tables as text under --out.
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

B, N = 64, 64000
FRONT_END = ("whisper_frames", "whisper_mel", "whisper_clamp", "K=400")     # the DFT GEMM is keyed by its K


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
    ap.add_argument("--layers", type=int, default=24, help="blocks (layer_st / layer_ed = layers - 8 .. layers - 1)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r13", "whisper"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import whisper_ref as ref
    from speaker_diarization_amd import _lib
    from speaker_diarization_amd.ssl.whisper import WhisperConfig, WhisperEncoder
    from speaker_diarization_amd.weights import to_torch, whisper_state_dict
    os.makedirs(args.out, exist_ok=True)
    cfg = WhisperConfig(n_audio_layer=args.layers, layer_st=args.layers - 8, layer_ed=args.layers - 1)
    sd = to_torch(whisper_state_dict(cfg, 2024))
    x = torch.from_numpy((np.random.default_rng(7).standard_normal((B, N)) * 0.5).astype(np.float32)).cuda()
    sd_gpu = {k: v.cuda() for k, v in sd.items()}
    T = (N // 160 - 1) // 2 + 1
    D, L = cfg.n_audio_state, args.layers
    # by arithmetic: per block 24 D^2 (projections + MLP) + 4 T D (attention) flops per row, plus the stem's convs
    flops = 2.0 * B * T * L * (12.0 * D * D + 2.0 * T * D) + 2.0 * B * (N // 160) * 3 * 80 * D + 2.0 * B * T * 3 * D * D
    with open(os.path.join(args.out, "probe.jsonl"), "a") as log:
        for precision in ("bf16", "fp32"):
            m = WhisperEncoder(cfg, precision=precision, max_batch=B, max_samples=N).load_state_dict(sd)
            hip = timed(lambda: m(x), args.steps, args.warmup)

            def torch_fwd():
                if precision == "bf16":
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        return ref.encoder(sd_gpu, cfg, x)
                return ref.encoder(sd_gpu, cfg, x)

            base = timed(torch_fwd, args.steps, args.warmup)
            err = float((m(x) - ref.encoder(sd_gpu, cfg, x)).abs().max())
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
            front = sum(s["ms"] for name, s in stats if any(k in name for k in FRONT_END))
            lines.append(f"{'sum of kernel times':58s} {'':8s} {total:9.3f}")
            lines.append(f"{'log-mel front end (frames, DFT GEMM, mel, clamp)':58s} {'':8s} {front:9.3f}")
            with open(os.path.join(args.out, f"{precision}_kernels.txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
            line = json.dumps(dict(config=f"whisper_l{L}_{precision}", B=B, n_samples=N, frames=T, hip_ms=hip,
                                   torch_ms=base, torch_over_hip=base["mean"] / hip["mean"],
                                   max_abs_diff_vs_torch_fp32=err, device_bytes=m.device_bytes, kernel_ms_sum=total,
                                   front_end_ms=front, tflop_by_arithmetic=flops / 1e12,
                                   tflops_achieved=flops / 1e9 / hip["mean"]))
            print(line, flush=True)
            log.write(line + "\n")
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
