"""Times of the TS-VAD Mamba2 back end at the MagicData recipe's shape (GPU box): 64 windows of rs_len 6 (598 fbank
frames, 150 label frames), d_state 128, expand 4, one reference batch of 64 (forward_batch 0).

  - the back-end-1 forward (single_backend mamba2, multi_backend transformer) in bf16 and bf16x3, and the same-shape
    forward of the transformer single back end (variant 0) as context: device events around `steps` forwards after
    `warm` warm-up forwards;
  - per kernel family, from the library's event timers in a run of their own (one stream, a forward per timed step):
    the SSD kernel alone (mamba2_scan) with its algorithmic bytes (zxbcdt read once, g written once) over its time, the
    two projections' GEMM paths (SDIAR_PROF_DETAIL names them by shape), the norm / finish passes;
  - the handle's device bytes (workspace included).
    SDIAR_PROF_DETAIL=1 python3 tools/mamba2_probe.py [steps] [warm]"""
import json
import os
import sys

import torch

sys.path.insert(0, ".")
from speaker_diarization_amd import _lib
from speaker_diarization_amd.ts_vad.model import TSVADModel
from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 3
B, T_FB, T_LAB = 64, 598, 150
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(3)
x = torch.randn(B, T_FB, 80, generator=g).to(dev)
ts = torch.randn(B, 4, 192, generator=g).to(dev)
lib = _lib.load()
out = {"shape": dict(B=B, T_fbank=T_FB, T_label=T_LAB, d_state=128, expand=4), "steps": steps}


def timed(m):
    for _ in range(warm):
        m.forward(x, ts, T_LAB)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        m.forward(x, ts, T_LAB, check=False)
    b.record()
    torch.cuda.synchronize()
    m.status()
    return a.elapsed_time(b) / steps


def kernels(m):
    lib.sd_prof_reset()
    lib.sd_prof_enable(1)
    for _ in range(steps):
        m.forward(x, ts, T_LAB)
    torch.cuda.synchronize()
    lib.sd_prof_enable(0)
    st = {k: v for k, v in _lib.prof_stats().items() if v["launches"]}
    lib.sd_prof_reset()
    return {k: dict(ms=v["ms"] / steps, launches=v["launches"] / steps, gb_s=v["bytes"] / v["ms"] / 1e6 if v["ms"] else 0.0,
                    tflops=v["flops"] / v["ms"] / 1e9 if v["ms"] else 0.0) for k, v in st.items()}


for name, cfg in (("mamba2_transformer", TSVADConfig(single_backend_type="mamba2", d_state=128, rs_len=6)),
                  ("transformer_transformer", TSVADConfig(rs_len=6))):
    for precision in ("bf16", "bf16x3"):
        m = TSVADModel(cfg, device=dev, precision=precision, max_batch=B)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=777)))
        r = {"forward_ms": timed(m), "device_bytes": m.device_bytes}
        k = kernels(m)
        r["kernel_ms_total"] = sum(v["ms"] for v in k.values())
        # the back end's own families, and every GEMM family by shape when SDIAR_PROF_DETAIL is set
        r["kernels"] = {n: v for n, v in sorted(k.items(), key=lambda kv: -kv[1]["ms"])
                        if n.startswith("mamba2") or " M=" in n or os.environ.get("MAMBA2_PROBE_ALL")}
        out[f"{name}/{precision}"] = r
        print(f"{name} {precision}: forward {r['forward_ms']:.3f} ms, kernels {r['kernel_ms_total']:.3f} ms, "
              f"device {r['device_bytes'] / 2**20:.0f} MiB", flush=True)
        for n, v in list(r["kernels"].items())[:14]:
            print(f"    {n:60s} {v['ms']:8.3f} ms x{v['launches']:.0f}  {v['gb_s']:8.1f} GB/s {v['tflops']:7.2f} TFLOP/s")
        del m
        torch.cuda.empty_cache()
print(json.dumps(out))
