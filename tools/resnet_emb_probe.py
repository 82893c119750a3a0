"""ResNet34 embedding extractor and TS-VAD proj_layer input stage: records, not gates (no earlier build ran them).

    python tools/resnet_emb_probe.py [--reps 20] [--warmup 3] [--out profiles/resnet_emb_probe.jsonl]
One JSON line per record:
  forward      one 96 x 598 batch (96 chunks of 6 s) through ResNet34.forward in bf16 and fp32: device-event time per
               call over `reps` calls after `warmup` calls (median, min, max), then one separate pass of 5 calls under
               the library's HIP-event kernel timers for the share of tstp_pool and seg_linear;
  extract      extract_embed over 4 x 2.5 min of audio (the shape of bench.py's `emb` workload): host clock around a
               step that ends in a device synchronise, 10-ms frames per second;
  proj_stage   sd_op_speaker_input_proj at B 640, T 100, NS 4, SE 256, E 384 (a 10-min C4 batch) in bf16 and fp32.
               The op also packs the weight halves and allocates its scratch per call; the timers' kernel sum is
               recorded beside the call time.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.synth import make_meeting  # noqa: E402
from speaker_diarization_amd.ts_vad.embedding import ResNet34, extract_embed  # noqa: E402
from speaker_diarization_amd.weights import resnet34_embed_state_dict, sinusoid_pe, to_torch  # noqa: E402


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


def kernel_table(fn, calls=5):
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.sd_prof_reset()
    lib.sd_prof_enable(1)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    lib.sd_prof_enable(0)
    return {k: v["ms"] / calls for k, v in _lib.prof_stats().items() if v["launches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "resnet_emb_probe.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU only"
    dev = torch.device("cuda", 0)
    sd = to_torch(resnet34_embed_state_dict(777, 256, False))
    recs = []
    x = torch.randn(96, 598, 80, generator=torch.Generator().manual_seed(1)).to(dev)
    models = {}
    for prec in ("bf16", "fp32"):
        m = models[prec] = ResNet34(80, 256, two_emb_layer=False, device=dev, precision=prec).load_state_dict(sd)
        out = torch.empty(96, 256, device=dev)
        r = dict(record="forward", precision=prec, B=96, T=598, **event_times(lambda: m(x, out=out), a.warmup, a.reps))
        fams = kernel_table(lambda: m(x, out=out))
        total = sum(fams.values())
        r.update(kernel_ms_sum=total, tstp_pool_ms=fams.get("tstp_pool", 0.0), seg_linear_ms=fams.get("seg_linear", 0.0),
                 head_share=(fams.get("tstp_pool", 0.0) + fams.get("seg_linear", 0.0)) / total, families=fams)
        recs.append(r)
    wavs = [torch.from_numpy(make_meeting(150.0, n_spk=1, seed=900 + i).wav.astype(np.float32)).to(dev) for i in range(4)]
    frames = sum(w.numel() for w in wavs) // 160
    for prec in ("bf16", "fp32"):
        m = models[prec]

        def step():
            outs = [extract_embed(w, m, batch_size=96) for w in wavs]
            torch.cuda.synchronize()
            return outs

        for _ in range(a.warmup):
            step()
        secs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            step()
            secs.append(time.perf_counter() - t0)
        med = statistics.median(secs)
        recs.append(dict(record="extract", precision=prec, audio_s=600.0, frames=frames, chunks=4 * 144,
                         ms_median=med * 1e3, ms_min=min(secs) * 1e3, ms_max=max(secs) * 1e3, reps=a.reps,
                         warmup=a.warmup, frames_per_s=frames / med))
    del models
    B, NS, T, SE, E = 640, 4, 100, 256, 384
    g = torch.Generator(device=dev).manual_seed(2)
    ts = torch.randn(B, NS, SE, device=dev, generator=g)
    mix = torch.randn(B, T, SE, device=dev, generator=g)
    w = torch.randn(E, 2 * SE, device=dev, generator=g) / (2 * SE) ** 0.5
    bias, bn_a, bn_b = torch.zeros(E, device=dev), torch.ones(SE, device=dev), torch.zeros(SE, device=dev)
    pe = torch.from_numpy(np.ascontiguousarray(sinusoid_pe(T, E)[:, 0])).to(dev)
    out = torch.empty(B * NS * T, E, device=dev)
    xb = torch.empty(B * NS * T, E, device=dev, dtype=torch.bfloat16)
    p = _lib.ptr
    for prec, code in (("bf16", 1), ("fp32", 0)):
        def call():
            _lib.call("sd_op_speaker_input_proj", p(ts), p(mix), B, NS, T, T, SE, E, p(w), p(bias), p(pe), p(bn_a),
                      p(bn_b), None, B, p(out), p(xb) if code else None, code, _lib.stream_ptr(dev))
        r = dict(record="proj_stage", precision=prec, B=B, NS=NS, T=T, SE=SE, E=E, **event_times(call, a.warmup, a.reps))
        fams = kernel_table(call)
        r.update(kernel_ms_sum=sum(fams.values()), families=fams,
                 unsplit_gmac=B * NS * T * 2 * SE * E / 1e9, split_gmac=(B * NS + B * T) * SE * E / 1e9)
        recs.append(r)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        for r in recs:
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
