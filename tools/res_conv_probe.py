"""res_conv probe: sd_op_res_conv with use_generic 0 (res_conv.hip) and 1 (conv_gemm) on the ResNet34 trunk's layer
shapes of a B = 64, rs_len 4 batch (398 fbank frames).

    python tools/res_conv_probe.py [--batch 64] [--rounds 5] [--reps 5] [--out FILE] [--trunk resnet34|simam]
Per shape: the stride-1 convs carry the residual, the stride-2 block openers the fused 1x1 shortcut (the generic
arm runs it as a second conv_gemm).  Kernel time is the library's HIP-event timers (every family the call launched,
summed), after a warm-up call of both arms; the arms alternate round by round and each arm's spread over the rounds
(min .. max) is printed beside its mean, so a difference can be read against the same-binary noise.  One JSON line
per shape; FLOPs from the layer shape (2 * pixels * Cout * 9 Cin, + the shortcut's).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speaker_diarization_amd import _lib  # noqa: E402

# (H, W, Cin, Cout, stride): the distinct 3x3 convs of ResNet34 on an (80, 398) fbank map
SHAPES = [(80, 398, 32, 32, 1), (80, 398, 32, 64, 2), (40, 199, 64, 64, 1), (40, 199, 64, 128, 2),
          (20, 100, 128, 128, 1), (20, 100, 128, 256, 2), (10, 50, 256, 256, 1)]
# --trunk simam: the distinct 3x3 convs of SimAM-ResNet34 (base width 64) on an (80, 598) map, the extractor's 6 s chunk
SHAPES_SIMAM = [(80, 598, 64, 64, 1), (80, 598, 64, 128, 2), (40, 299, 128, 128, 1), (40, 299, 128, 256, 2),
                (20, 150, 256, 256, 1), (20, 150, 256, 512, 2), (10, 75, 512, 512, 1)]
BF16_PEAK_TFLOPS = 2500.0   # dense bf16 MFMA peak of an MI355X


def probe(B, H, W, Cin, Cout, s, rounds, reps):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(H * W + Cin + Cout)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x = torch.randn(B, H, W, Cin, device=dev, generator=g).bfloat16()
    w = torch.randn(Cout, Cin, 3, 3, device=dev, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    al = torch.rand(Cout, device=dev, generator=g) + 0.5
    be = torch.randn(Cout, device=dev, generator=g) * 0.1
    res = torch.randn(B, Ho, Wo, Cout, device=dev, generator=g).bfloat16() if s == 1 else None
    scw = torch.randn(Cout, Cin, 1, 1, device=dev, generator=g) / Cin ** 0.5 if s == 2 else None
    outs = [torch.empty(B, Ho, Wo, Cout, device=dev, dtype=torch.bfloat16) for _ in range(2)]
    scs = [torch.empty_like(outs[0]) if s == 2 else None for _ in range(2)]
    st = _lib.stream_ptr(dev)
    lib = _lib.load()
    p = _lib.ptr

    def call(arm):
        _lib.call("sd_op_res_conv", p(x), B, H, W, Cin, p(w), Cout, s, p(al), p(be), p(res), p(scw),
                  p(al) if s == 2 else None, p(be) if s == 2 else None, p(outs[arm]), p(scs[arm]), arm, st)

    for arm in (0, 1):
        call(arm)
    torch.cuda.synchronize()
    diff = float((outs[0].float() - outs[1].float()).abs().max())
    ms = {0: [], 1: []}
    fam = {0: set(), 1: set()}
    for _ in range(rounds):
        for arm in (0, 1):
            lib.sd_prof_reset()
            lib.sd_prof_enable(1)
            for _ in range(reps):
                call(arm)
            torch.cuda.synchronize()
            lib.sd_prof_enable(0)
            stats = {k: v for k, v in _lib.prof_stats().items() if v["launches"]}
            fam[arm] |= set(stats)
            ms[arm].append(sum(v["ms"] for v in stats.values()) / reps)
    px = B * Ho * Wo
    flops = 2.0 * px * Cout * 9 * Cin + (2.0 * px * Cout * Cin if s == 2 else 0.0)
    rec = dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, stride=s, gflop=flops / 1e9, max_abs_diff=diff)
    for arm, name in ((0, "res_conv"), (1, "generic")):
        v = ms[arm]
        mean = sum(v) / len(v)
        rec[name] = dict(ms_mean=mean, ms_min=min(v), ms_max=max(v), families=sorted(fam[arm]),
                         tflops=flops / (mean * 1e-3) / 1e12, mfma_roof_frac=flops / (mean * 1e-3) / 1e12 / BF16_PEAK_TFLOPS)
    spread = max(rec["res_conv"]["ms_max"] - rec["res_conv"]["ms_min"], rec["generic"]["ms_max"] - rec["generic"]["ms_min"])
    rec["spread_ms"] = spread
    rec["res_conv_wins"] = rec["generic"]["ms_mean"] - rec["res_conv"]["ms_mean"] > spread
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trunk", choices=("resnet34", "simam"), default="resnet34")
    a = ap.parse_args()
    fh = open(a.out, "w") if a.out else None
    for shape in (SHAPES if a.trunk == "resnet34" else SHAPES_SIMAM):
        r = probe(a.batch, *shape, rounds=a.rounds, reps=a.reps)
        line = json.dumps(r)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()
