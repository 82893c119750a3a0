"""ERes2NetV2 embedding extractor: records, not gates (no earlier build ran this model).

    python tools/eres2net_probe.py [--reps 20] [--warmup 3] [--out profiles/eres2net/eres2net_probe.jsonl]
One JSON line per record, for both size triples at 96 x 598 (96 chunks of 6 s) and 1 x 598, in bf16 and fp32:
  forward   ERes2NetV2.forward: device-event time per call over `reps` calls after `warmup` calls (median, min, max),
            then one separate pass of 3 calls under the library's HIP-event kernel timers, split into stem, 1x1 GEMMs,
            res2_conv3x3 (the slice convs; conv_gemm's 3x3 form in fp32), aff_gate, layer3_ds + fuse34, TSTP + seg_1 and
            the element-wise rest;
  roofline  achieved FLOP/s and bytes/s of res2_conv3x3 and aff_gate over the forward against the MI355X roofs the other
            probes use (2500 TFLOP/s dense bf16 MFMA, 8000 GB/s HBM; aff_gate's arithmetic is fp32 VALU, so its share
            of the MFMA roof is shown only for scale), from the FLOP and byte counts the launchers record (the
            algorithm's: every input and output element once).
  clamp_route  bf16 only: the same forward with the Hardtanh-epilogue GEMMs on the register-staged kernel
            (sd_debug_clamp_route(1), the first form built) against the shipped rule (0: the LDS-DMA kernel where it
            applies), arms alternating in one process, 3 rounds of 5 calls each after 2 warm-up calls; per arm the median
            of the round medians and the extremes of all calls.
A step that takes longer than --step-timeout seconds ends the probe (the records so far are kept).  Runs no reference
code.  The kernel timers' keys carry M / N / K / taps here (SDIAR_PROF_DETAIL), which is how the GEMM families are split.
"""
import argparse
import json
import os
import re
import signal
import statistics
import sys

os.environ.setdefault("SDIAR_PROF_DETAIL", "1")     # read once by the library, before its first launch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.embedding import ERes2NetV2  # noqa: E402
from speaker_diarization_amd.weights import eres2netv2_state_dict, to_torch  # noqa: E402

BF16_PEAK_TFLOPS = 2500.0   # dense bf16 MFMA peak of an MI355X
HBM_PEAK_GBS = 8000.0
TRIPLES = {"base": (26, 2, 2), "w24": (24, 4, 4)}
GROUPS = ("stem", "gemm_1x1", "res2_conv3x3", "aff_gate", "layer3_ds_fuse34", "tstp_seg1", "other")


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
    return {k: dict(ms=v["ms"] / calls, gbytes=v["bytes"] / calls / 1e9, gflop=v["flops"] / calls / 1e9,
                    launches=v["launches"] // calls)
            for k, v in _lib.prof_stats().items() if v["launches"]}


def group_of(key, expansion):
    """The probe's group of one kernel-timer key (family name, plus ' M= N= K= taps=' on the GEMM families)."""
    fam = key.split(" ")[0]
    if fam == "fcm_conv1":
        return "stem"
    if fam in ("res2_conv3x3", "aff_gate"):
        return fam
    if fam in ("tstp_pool", "seg_linear"):
        return "tstp_seg1"
    if fam == "aff_blend":
        return "layer3_ds_fuse34"
    m = re.search(r" N=(\d+) K=(\d+) taps=(\d+)", key)
    if m:
        N, K, taps = (int(v) for v in m.groups())
        c3, c4 = 256 * expansion, 512 * expansion
        if taps == 9:
            return "layer3_ds_fuse34" if K == 9 * c3 else "res2_conv3x3"
        if (N == c4 // 4 and K == 2 * c4) or (N == c4 and K == c4 // 4):
            return "layer3_ds_fuse34"
        return "gemm_1x1"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join("profiles", "eres2net", "eres2net_probe.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU only"
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)

    def too_long(signum, frame):
        raise TimeoutError(f"a probe step took longer than {a.step_timeout} s")

    signal.signal(signal.SIGALRM, too_long)
    with open(a.out, "w") as fh:
        def emit(r):
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()

        for tag, (bw, sc, ex) in TRIPLES.items():
            sd = to_torch(eres2netv2_state_dict(777, bw, sc, ex, 192))
            for prec in ("bf16", "fp32"):
                for B in (96, 1):
                    signal.alarm(a.step_timeout)
                    m = ERes2NetV2(baseWidth=bw, scale=sc, expansion=ex, device=dev, precision=prec, max_batch=B)
                    m.load_state_dict(sd)
                    x = torch.randn(B, 598, 80, generator=torch.Generator().manual_seed(1)).to(dev)
                    out = torch.empty(B, 192, device=dev)
                    r = dict(record="forward", triple=tag, precision=prec, B=B, T=598,
                             device_bytes=m.device_bytes, **event_times(lambda: m(x, out=out), a.warmup, a.reps))
                    fams = kernel_table(lambda: m(x, out=out))
                    split = {g: 0.0 for g in GROUPS}
                    roof = {}
                    for key, f in fams.items():
                        g = group_of(key, ex)
                        split[g] += f["ms"]
                        if key.split(" ")[0] in ("res2_conv3x3", "aff_gate"):
                            roof[key] = f
                    r.update(kernel_ms_sum=sum(f["ms"] for f in fams.values()), split_ms=split, families=fams)
                    emit(r)
                    if prec == "bf16":
                        arms = {0: [], 1: []}
                        for _ in range(3):
                            for route in (1, 0):
                                _lib.call("sd_debug_clamp_route", route)
                                try:
                                    arms[route].append(event_times(lambda: m(x, out=out), 2, 5))
                                finally:
                                    _lib.call("sd_debug_clamp_route", 0)
                        emit(dict(record="clamp_route", triple=tag, precision=prec, B=B, rounds=3, reps=5, **{
                            f"{name}_{k}": fn(t[k] for t in arms[route])
                            for route, name in ((0, "shipped"), (1, "register_kernel"))
                            for k, fn in (("ms_median", statistics.median), ("ms_min", min), ("ms_max", max))}))
                    for fam, f in roof.items():
                        tf, gbs = f["gflop"] / f["ms"], f["gbytes"] / f["ms"] * 1e3     # GFLOP / ms = TFLOP / s
                        f_mfma, f_hbm = tf / BF16_PEAK_TFLOPS, gbs / HBM_PEAK_GBS
                        emit(dict(record="roofline", triple=tag, precision=prec, B=B, family=fam, ms=f["ms"],
                                  launches=f["launches"], tflops=tf, gbytes_per_s=gbs, mfma_roof_frac=f_mfma,
                                  hbm_roof_frac=f_hbm, bound="mfma" if f_mfma > f_hbm else "hbm"))
                    signal.alarm(0)
                    del m, x, out
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
