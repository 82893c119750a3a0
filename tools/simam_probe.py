"""SimAM-ResNet34 (ASP) embedding extractor: records, not gates (no earlier build ran this model).

    python tools/simam_probe.py [--reps 20] [--warmup 3] [--out profiles/simam/simam_probe.jsonl]
One JSON line per record:
  forward   one 96 x 598 batch (96 chunks of 6 s) through SimAM_ResNet34_ASP.forward in bf16 and fp32: device-event
            time per call over `reps` calls after `warmup` calls (median, min, max), then one separate pass of 3 calls
            under the library's HIP-event kernel timers for the per-family shares (convs, simam_stats, simam_apply, ASP,
            bottleneck);
  plain     the same forward built under sd_debug_simam_variant(1): the base-64 trunk with plain BasicBlocks (not a
            public model), so forward - plain is what SimAM costs;
  simam_bw  achieved bytes / s of the simam_stats and simam_apply families over the forward's 16 blocks against the HBM
            roofline, from the byte count of DESIGN.md section 5c (the timers' own `bytes` column: one read of the map
            for the statistics; a read of the map, a read of the shortcut and a write of the output for the apply).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.embedding import SimAM_ResNet34_ASP  # noqa: E402
from speaker_diarization_amd.weights import simam_resnet34_state_dict, to_torch  # noqa: E402

HBM_TBPS = 6.3   # achievable HBM bandwidth of an MI355X (8.0 spec)


def event_times(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), reps=reps, warmup=warmup)


def kernel_table(fn, calls=3):
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.sd_prof_reset()
    lib.sd_prof_enable(1)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    lib.sd_prof_enable(0)
    return {k: dict(ms=v["ms"] / calls, gbytes=v["bytes"] / calls / 1e9, launches=v["launches"] // calls)
            for k, v in _lib.prof_stats().items() if v["launches"]}


def build(dev, prec, sd, variant):
    """variant: sd_debug_simam_variant (0 shipped, 1 plain blocks)."""
    _lib.call("sd_debug_simam_variant", variant)
    try:
        return SimAM_ResNet34_ASP(device=dev, precision=prec).load_state_dict(sd)
    finally:
        _lib.call("sd_debug_simam_variant", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "simam", "simam_probe.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU only"
    dev = torch.device("cuda", 0)
    sd = to_torch(simam_resnet34_state_dict(777, 256))
    x = torch.randn(96, 598, 80, generator=torch.Generator().manual_seed(1)).to(dev)
    out = torch.empty(96, 256, device=dev)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        def emit(r):
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()

        for prec in ("bf16", "fp32"):
            med = {}
            for variant in (0, 1):
                plain = variant == 1
                m = build(dev, prec, sd, variant)
                r = dict(record=("forward", "plain")[variant], precision=prec, B=96, T=598,
                         **event_times(lambda: m(x, out=out), a.warmup, a.reps))
                fams = kernel_table(lambda: m(x, out=out))
                r.update(kernel_ms_sum=sum(v["ms"] for v in fams.values()), families=fams)
                med[variant] = r["ms_median"]
                emit(r)
                if variant == 0:
                    for fam in ("simam_stats", "simam_apply"):
                        f = fams[fam]
                        tbps = f["gbytes"] / f["ms"]          # GB / ms = TB / s
                        emit(dict(record="simam_bw", precision=prec, family=fam, ms=f["ms"], gbytes=f["gbytes"],
                                  launches=f["launches"], tbytes_per_s=tbps, hbm_roof_frac=tbps / HBM_TBPS))
                del m
                torch.cuda.empty_cache()
            emit(dict(record="simam_cost", precision=prec, ms=med[0] - med[1]))


if __name__ == "__main__":
    main()
