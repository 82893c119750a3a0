"""WavLM.extract_features at the TS-VAD recipe's shape: B = 64 windows of 64,000 samples (199 frames), Base+ and Large
cut to 6 layers, bf16 and fp32, on the HIP path and on the stock-PyTorch path (tests/wavlm_ref.py moved to the same GPU
under torch-ROCm, fp32 and autocast bf16) with the same seeded weights.

    python tools/wavlm_probe.py [--steps 20] [--warmup 5] [--out profiles/r10/wavlm] [--no-trace]

Per configuration: warm-up, then `steps` timed forwards (HIP events around each), mean / min / max / standard deviation
beside each other; then the per-kernel split of the HIP path from a `rocprofv3 --kernel-trace --stats` run of its own
(a child process: this script with --child under the profiler).  The GEMM families are split by shape with the
library's own event timers (SDIAR_PROF_DETAIL keys carry M / N / K), which is where the times of conv layer 1 (K 1536
at a slice's layer-1 row count) and of the FFN GEMMs (N or K = ffn) come from; the attention, pos_conv and layer-0 times
are the trace's.  In bf16 each is quoted as a fraction of the bf16 MFMA roof (2.5 PFLOP/s dense) from its algorithmic
FLOPs.  One JSON line per configuration, and the tables as text under --out.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import signal
import subprocess
import sys
import tempfile

os.environ.setdefault("SDIAR_PROF_DETAIL", "1")     # read once by the library, before its first launch

HERE =os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

B, N_SAMPLES, LAYERS = 64, 64000, 6
BF16_ROOF = 2.5e15
GEOMETRIES = {
    "base_plus": dict(encoder_embed_dim=768, encoder_ffn_embed_dim=3072, encoder_attention_heads=12,
                      extractor_mode="default", layer_norm_first=False),
    "large": dict(encoder_embed_dim=1024, encoder_ffn_embed_dim=4096, encoder_attention_heads=16,
                  extractor_mode="layer_norm", layer_norm_first=True),
}


def setup(geom):
    import numpy as np
    import torch
    from speaker_diarization_amd.ssl.wavlm import WavLMConfig
    from speaker_diarization_amd.weights import to_torch, wavlm_state_dict
    cfg = WavLMConfig(dict(GEOMETRIES[geom], encoder_layers=LAYERS))
    sd = to_torch(wavlm_state_dict(cfg, 2024))
    wav = torch.from_numpy((np.random.default_rng(7).standard_normal((B, N_SAMPLES)) * 0.5).astype(np.float32))
    return cfg, sd, wav.cuda()


def hip_model(cfg, sd, precision):
    from speaker_diarization_amd.ssl.wavlm import WavLM
    return WavLM(cfg, precision=precision, max_batch=B, max_samples=N_SAMPLES).load_state_dict(sd)


def timed(fn, steps, warmup):
    import numpy as np
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
    ms = np.array(ms)
    return dict(mean_ms=float(ms.mean()), min_ms=float(ms.min()), max_ms=float(ms.max()), std_ms=float(ms.std()),
                steps=steps)


def flops(cfg):
    """Algorithmic FLOPs of one forward at (B, N_SAMPLES) of the three stages the roof fractions are quoted for."""
    from speaker_diarization_amd.ssl.wavlm import num_frames
    T, D, F, H = num_frames(N_SAMPLES), cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_attention_heads
    T1 = ((N_SAMPLES - 10) // 5 + 1 - 3) // 2 + 1
    return dict(conv1=2.0 * B * T1 * 512 * 1536, ffn=LAYERS * 2 * 2.0 * B * T * D * F,
                attention=LAYERS * 4.0 * B * H * T * T * 64, pos_conv=2.0 * B * T * D * 128 * (D // 16))


def child(geom, precision, steps):
    """The profiled run: HIP forwards only (the profiler wraps this process)."""
    import torch
    cfg, sd, wav = setup(geom)
    m = hip_model(cfg, sd, precision)
    for _ in range(steps):
        m.extract_features(wav)
    torch.cuda.synchronize()


def kernel_table(geom, precision, steps):
    """[(kernel, calls per forward, us per forward, share)] from a rocprofv3 --kernel-trace --stats child run."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--child", geom, precision, "--steps", str(steps)]
        # its own session, so that a time limit ends the profiler AND the python under it
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            _, err = proc.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            proc.communicate()
            raise RuntimeError("the rocprofv3 run passed its time limit")
        if proc.returncode != 0:
            raise RuntimeError(f"rocprofv3 run failed ({proc.returncode}):\n{err[-2000:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        rows = []
        with open(files[0], newline="") as f:
            for row in csv.DictReader(f):
                rows.append((row["Name"], int(row["Calls"]), float(row["TotalDurationNs"])))
    total = sum(ns for _, _, ns in rows) or 1.0
    rows.sort(key=lambda r: -r[2])
    return [(n, c / steps, ns / steps / 1e3, ns / total) for n, c, ns in rows]


def us_of(table, *needles):
    us = sum(us for n, _, us, _ in table if any(k in n for k in needles))
    if not us:
        raise RuntimeError(f"no kernel of the trace matches {needles}: {[n[:60] for n, _, _, _ in table]}")
    return us


def gemm_shapes(m, wav, steps):
    """{timer key: us per forward} of the library's event timers, the GEMM families keyed by shape."""
    import torch
    from speaker_diarization_amd import _lib
    lib = _lib.load()
    lib.sd_prof_reset()
    lib.sd_prof_enable(1)
    for _ in range(steps):
        m.extract_features(wav)
    torch.cuda.synchronize()
    lib.sd_prof_enable(0)
    st = {k: v["ms"] * 1e3 / steps for k, v in _lib.prof_stats().items() if v["launches"]}
    lib.sd_prof_reset()
    return st


def field(key, name):
    m = re.search(rf" {name}=(\d+)", key)
    return int(m.group(1)) if m else None


def stage_us(shapes, cfg):
    """us per forward of conv layer 1 and of the FFN GEMMs, by the shapes in the timer keys."""
    F = cfg.encoder_ffn_embed_dim
    T1 = ((N_SAMPLES - 10) // 5 + 1 - 3) // 2 + 1
    conv1 = sum(us for k, us in shapes.items() if field(k, "K") == 1536 and field(k, "M") in (8 * T1, (B % 8 or 8) * T1))
    ffn = sum(us for k, us in shapes.items() if field(k, "N") == F or field(k, "K") == F)
    if not conv1 or not ffn:
        raise RuntimeError(f"no timer key matches conv layer 1 / the FFN GEMMs: {sorted(shapes)}")
    return conv1, ffn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--only", default=None, help="geometry:precision, e.g. base_plus:bf16")
    ap.add_argument("--child", nargs=2, metavar=("GEOMETRY", "PRECISION"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.steps)
        return
    import torch
    import wavlm_ref as wr
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    for geom in GEOMETRIES:
        cfg, sd, wav = setup(geom)
        sd_gpu = {k: v.cuda() for k, v in sd.items()}
        for precision in ("bf16", "fp32"):
            if a.only and a.only != f"{geom}:{precision}":
                continue
            m = hip_model(cfg, sd, precision)
            hip = timed(lambda: m.extract_features(wav), a.steps, a.warmup)
            dev_bytes = m.device_bytes
            shapes = gemm_shapes(m, wav, max(3, a.steps // 4))
            del m

            def baseline():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16"):
                    return wr.extract_features(sd_gpu, cfg, wav)["x"]

            ref = timed(baseline, a.steps, a.warmup)

            def stage(fn):     # one stage of the baseline alone, under the same autocast
                def run():
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16"):
                        return fn()
                return timed(run, max(3, a.steps // 4), 2)["mean_ms"]

            def conv_stack():
                x = wr.conv_layer0(sd_gpu, wav, cfg.extractor_mode)
                for i in range(1, 7):
                    x = wr.conv_layer(sd_gpu, x, i, cfg.extractor_mode)
                return x

            feats = torch.randn(B, wr.frames(N_SAMPLES), cfg.encoder_embed_dim, device="cuda")
            torch_stage_ms = dict(conv_front_end=stage(conv_stack), pos_conv=stage(lambda: wr.pos_conv(sd_gpu, feats)))
            torch_stage_ms["encoder_rest"] = ref["mean_ms"] - sum(torch_stage_ms.values())
            rec = dict(geometry=geom, precision=precision, B=B, n_samples=N_SAMPLES, layers=LAYERS, hip=hip, torch=ref,
                       speedup=ref["mean_ms"] / hip["mean_ms"], device_bytes=dev_bytes, torch_stage_ms=torch_stage_ms)
            fl = flops(cfg)
            conv1_us, ffn_us = stage_us(shapes, cfg)
            rec["conv1_us"], rec["ffn_us"] = round(conv1_us, 1), round(ffn_us, 1)
            rec["timer_us"] = {k: round(us, 1) for k, us in sorted(shapes.items(), key=lambda kv: -kv[1])}
            roof = dict(conv1=fl["conv1"] / (conv1_us * 1e-6) / BF16_ROOF, ffn=fl["ffn"] / (ffn_us * 1e-6) / BF16_ROOF)
            lines = []
            if not a.no_trace:
                table = kernel_table(geom, precision, a.steps)
                attn_us, pos_us = us_of(table, "wavlm_attn"), us_of(table, "wavlm_pos_conv")
                rec["attention_us"], rec["pos_conv_us"] = round(attn_us, 1), round(pos_us, 1)
                rec["layer0_us"] = round(us_of(table, "wavlm_l0"), 1)
                rec["trace_total_us"] = round(sum(us for _, _, us, _ in table), 1)
                conv_gemm_us = sum(us for k, us in shapes.items() if (field(k, "taps") or 1) > 1)
                ln_us = sum(us for n, _, us, _ in table if "wavlm_ln_gelu" in n)
                rec["hip_stage_ms"] = dict(conv_front_end=round((rec["layer0_us"] + conv_gemm_us + ln_us) / 1e3, 3),
                                           pos_conv=round(pos_us / 1e3, 3))
                rec["hip_stage_ms"]["encoder_rest"] = round(
                    rec["trace_total_us"] / 1e3 - sum(rec["hip_stage_ms"].values()), 3)
                roof.update(attention=fl["attention"] / (attn_us * 1e-6) / BF16_ROOF,
                            pos_conv=fl["pos_conv"] / (pos_us * 1e-6) / BF16_ROOF)
                lines = [f"{us:10.1f} us  {calls:6.1f} calls  {share * 100:5.1f} %  {n[:100]}"
                         for n, calls, us, share in table]
            if precision == "bf16":
                rec["roof_fraction"] = {k: round(v, 4) for k, v in roof.items()}
            print(json.dumps(rec), flush=True)
            if a.out:
                with open(os.path.join(a.out, f"{geom}_{precision}.json"), "w") as f:
                    json.dump(rec, f, indent=1)
                if lines:
                    with open(os.path.join(a.out, f"{geom}_{precision}_kernels.txt"), "w") as f:
                        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
