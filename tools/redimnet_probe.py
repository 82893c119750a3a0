"""ReDimNetB2 embedding extractor: records, not gates (no earlier build ran this model).

    python tools/redimnet_probe.py [--reps 10] [--warmup 2] [--out profiles/redimnet/redimnet_probe.jsonl]
One JSON line per record, at (B, T) = (96, 598) for the extractor (forward: trunk + ASTP + seg_1) and (64, 398) for the
trunk alone (get_frame_level_feat, the TS-VAD window shape), each in bf16 and fp32:
  forward   device-event time per call over `reps` calls after `warmup` calls (median, min, max), then one separate
            pass of 3 calls under the library's HIP-event kernel timers, per kernel family;
  roofline  achieved bytes/s of redim_block2d (bf16: the single-launch 2-D block) over the forward against 8000 GB/s of
            HBM, from the byte count its launcher records (the algorithm's: the map read once and written once);
  arms      bf16 only: the 2-D blocks as the single-launch kernel against the generic arm (grouped-conv kernel +
            conv_gemm, sd_redimnet_debug_generic), arms alternating in one process, 5 rounds of 5 calls each after 2
            warm-up calls; per arm the median of the round medians, the extremes of all calls and the spread of the
            round medians (the same-arm spread the gain is judged against).
A step that takes longer than --step-timeout seconds ends the probe (the records so far are kept).  Runs no reference
code.
"""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.embedding import ReDimNetB2  # noqa: E402
from speaker_diarization_amd.weights import redimnet_embed_state_dict, to_torch  # noqa: E402

HBM_PEAK_GBS = 8000.0
SHAPES = (("extractor", 96, 598), ("trunk", 64, 398))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join("profiles", "redimnet", "redimnet_probe.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU only"
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)

    def too_long(signum, frame):
        raise TimeoutError(f"a probe step took longer than {a.step_timeout} s")

    signal.signal(signal.SIGALRM, too_long)
    sd = to_torch(redimnet_embed_state_dict(777))
    with open(a.out, "w") as fh:
        def emit(r):
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()

        for what, B, T in SHAPES:
            for prec in ("bf16", "fp32"):
                signal.alarm(a.step_timeout)
                m = ReDimNetB2(device=dev, precision=prec, max_batch=B, max_frames=T)
                m.load_state_dict(sd)
                x = torch.randn(B, T, 72, generator=torch.Generator().manual_seed(1)).to(dev)
                out = torch.empty(B, 192, device=dev)
                fn = (lambda: m(x, out=out)) if what == "extractor" else (lambda: m.get_frame_level_feat(x))
                r = dict(record="forward", what=what, precision=prec, B=B, T=T, device_bytes=m.device_bytes,
                         **event_times(fn, a.warmup, a.reps))
                fams = kernel_table(fn)
                r.update(kernel_ms_sum=sum(f["ms"] for f in fams.values()), families=fams)
                emit(r)
                f = fams.get("redim_block2d")
                if f:
                    gbs = f["gbytes"] / f["ms"] * 1e3
                    emit(dict(record="roofline", what=what, precision=prec, B=B, T=T, family="redim_block2d", ms=f["ms"],
                              launches=f["launches"], gbytes=f["gbytes"], gbytes_per_s=gbs,
                              hbm_roof_frac=gbs / HBM_PEAK_GBS))
                if prec == "bf16":
                    arms = {0: [], 1: []}
                    for _ in range(a.rounds):
                        for generic in (1, 0):
                            m.use_generic_blocks(generic)
                            try:
                                arms[generic].append(event_times(fn, 2, 5))
                            finally:
                                m.use_generic_blocks(False)
                    rec = dict(record="arms", what=what, precision=prec, B=B, T=T, rounds=a.rounds, reps=5)
                    for generic, name in ((0, "fused"), (1, "generic")):
                        meds = [t["ms_median"] for t in arms[generic]]
                        rec.update({f"{name}_ms_median": statistics.median(meds),
                                    f"{name}_ms_min": min(t["ms_min"] for t in arms[generic]),
                                    f"{name}_ms_max": max(t["ms_max"] for t in arms[generic]),
                                    f"{name}_round_medians": meds, f"{name}_spread": max(meds) - min(meds)})
                    emit(rec)
                signal.alarm(0)
                del m, x, out
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
