"""ECAPA-TDNN probe: (a) the Res2 chain, fused (ecapa.hip, one launch) against generic (seven conv_gemm launches +
the adds), through sd_op_res2_chain at B = 64, T = 398, dilation 2, 3, 4; (b) the TS-VAD variant-3 bf16 forward at
B = 64, rs_len 4, with the per-family kernel table.

    python tools/ecapa_probe.py [--part chain|forward|both] [--batch 64] [--rounds 5] [--reps 5] [--out FILE]
Kernel time is the library's HIP-event timers (every family a call launched, summed), after a warm-up call of every
arm; in (a) the arms alternate round by round and each arm's spread over the rounds (min .. max) is printed beside its
mean, so a difference can be read against the same-binary noise.  (b) times the forward with device events around
`reps` forwards per round (min .. max over the rounds), then one profiled forward for the family table; the share of
peak of a family is the larger of FLOPs / bf16 MFMA peak and bytes / HBM peak over its time (FLOPs and bytes from the
shapes, as the launchers report them).  SDIAR_RES2_GENERIC=1 in the environment runs (b) with the generic chain.
One JSON line per record.
"""
import argparse
import json
import os
import sys

os.environ.setdefault("SDIAR_PROF_DETAIL", "1")   # GEMM families keyed by shape (read once by the library)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speaker_diarization_amd import _lib  # noqa: E402

BF16_PEAK_TFLOPS = 2500.0   # dense bf16 MFMA peak of an MI355X
HBM_PEAK_GBS = 8000.0
G, NS, C = 128, 7, 1024


def prof_families(fn, reps):
    lib = _lib.load()
    lib.sd_prof_reset()
    lib.sd_prof_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    lib.sd_prof_enable(0)
    return {k: v for k, v in _lib.prof_stats().items() if v["launches"]}


def probe_chain(B, T, dil, rounds, reps):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(T + dil)
    x = torch.randn(B, T, C, device=dev, generator=g).abs().bfloat16()
    w = torch.randn(NS, G, G, 3, device=dev, generator=g) * (2.0 / (3 * G)) ** 0.5
    bias = torch.randn(NS, G, device=dev, generator=g) * 0.05
    s = torch.rand(NS, G, device=dev, generator=g) * 0.6 + 0.7
    h = torch.randn(NS, G, device=dev, generator=g) * 0.1 - 0.3
    outs = [torch.empty(B, T, C, device=dev, dtype=torch.bfloat16) for _ in range(2)]
    st = _lib.stream_ptr(dev)
    p = _lib.ptr

    def call(generic):
        _lib.call("sd_op_res2_chain", p(x), B, T, dil, p(w), p(bias), p(s), p(h), p(outs[generic]), generic, 1, st)

    for arm in (0, 1):
        call(arm)
    torch.cuda.synchronize()
    diff = float((outs[0].float() - outs[1].float()).abs().max())
    ms = {0: [], 1: []}
    fam = {0: {}, 1: {}}
    for _ in range(rounds):
        for arm in (0, 1):
            stats = prof_families(lambda: call(arm), reps)
            stats.pop("pack_weight", None)            # the test op packs its weights per call; not part of either arm
            for k, v in stats.items():
                fam[arm][k] = round(v["ms"] / reps, 5)
            ms[arm].append(sum(v["ms"] for v in stats.values()) / reps)
    flops = 2.0 * B * T * G * 3 * G * NS
    rec = dict(part="chain", B=B, T=T, dilation=dil, gflop=flops / 1e9, max_abs_diff=diff)
    for arm, name in ((0, "fused"), (1, "generic")):
        v = ms[arm]
        mean = sum(v) / len(v)
        rec[name] = dict(ms_mean=mean, ms_min=min(v), ms_max=max(v), families=fam[arm],
                         tflops=flops / (mean * 1e-3) / 1e12, mfma_roof_frac=flops / (mean * 1e-3) / 1e12 / BF16_PEAK_TFLOPS)
    spread = max(rec["fused"]["ms_max"] - rec["fused"]["ms_min"], rec["generic"]["ms_max"] - rec["generic"]["ms_min"])
    rec["spread_ms"] = spread
    rec["fused_wins"] = rec["generic"]["ms_mean"] - rec["fused"]["ms_mean"] > spread
    return rec


def probe_forward(B, rounds, reps):
    from speaker_diarization_amd.ts_vad.model import TSVADModel
    from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_state_dict
    dev = torch.device("cuda", 0)
    cfg = TSVADConfig(speech_encoder_type="ecapa_channel_1024_wespeaker")
    m = TSVADModel(cfg, device=dev, precision="bf16", max_batch=B)
    m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=777)))
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, 398, 80, device=dev, generator=g)
    ts = torch.randn(B, 4, 192, device=dev, generator=g)
    out = torch.empty(B, 4, 100, device=dev)

    def fwd():
        m.forward(x, ts, 100, out=out, check=False)

    for _ in range(3):
        fwd()
    m.status()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fwd()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    stats = prof_families(fwd, reps)
    table = []
    for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["ms"]):
        t = v["ms"] / reps * 1e-3
        tf, gbs = v["flops"] / reps / t / 1e12, v["bytes"] / reps / t / 1e9
        f_mfma, f_hbm = tf / BF16_PEAK_TFLOPS, gbs / HBM_PEAK_GBS
        table.append(dict(family=k, launches=v["launches"] // reps, ms=round(v["ms"] / reps, 4), tflops=round(tf, 1),
                          gbs=round(gbs, 1), bound="mfma" if f_mfma >= f_hbm else "hbm",
                          peak_frac=round(max(f_mfma, f_hbm), 4)))
    return dict(part="forward", B=B, T_fbank=398, precision="bf16",
                chain="generic" if os.environ.get("SDIAR_RES2_GENERIC") else "fused",
                ms_mean=sum(ms) / len(ms), ms_min=min(ms), ms_max=max(ms), kernel_ms=sum(r["ms"] for r in table),
                families=table)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=("chain", "forward", "both"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fh = open(a.out, "a") if a.out else None
    recs = []
    if a.part in ("chain", "both"):
        recs += [lambda d=d: probe_chain(a.batch, 398, d, a.rounds, a.reps) for d in (2, 3, 4)]
    if a.part in ("forward", "both"):
        recs.append(lambda: probe_forward(a.batch, a.rounds, a.reps))
    for r in recs:
        line = json.dumps(r())
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()
