"""Per-launch time of one CAM++ FCM residual block: the fused kernel (sd_op_fcm_block / sd_op_fcm_stem_block fused = 1)
against the trunk's two launches (fused = 0) at the C2 / C4 block shapes (GPU box), from the library's per-family
event timers (so the weight packing and the scratch maps of the test entry point are not in the figures).  layer1.0
is the stem + strided block from the fbank (F 80); its two launches are the stem-fused conv1 and conv2.
    python3 tools/fcm_block_bench.py [B]"""
import math
import sys

import torch

sys.path.insert(0, ".")
from speaker_diarization_amd import _lib

B = int(sys.argv[1]) if len(sys.argv) > 1 else 600
dev = torch.device("cuda", 0)
st = _lib.stream_ptr(dev)
lib = _lib.load()


def timed(fn, keys, reps=5):
    """Mean device time (us) per call of the kernel families `keys`, from the library's event timers."""
    fn()
    torch.cuda.synchronize()
    lib.sd_prof_enable(1)
    lib.sd_prof_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    stats = _lib.prof_stats()
    lib.sd_prof_enable(0)
    return sum(stats[k]["ms"] for k in keys) * 1e3 / reps


for W in (598, 398):
    g = torch.Generator().manual_seed(W)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    fb = 2.0 * r(B, W, 80)
    out = torch.empty(B, 40, W, 32, dtype=torch.bfloat16, device=dev)
    p = [r(32, 1, 3, 3) / 3, 1 + 0.1 * r(32), 0.1 * r(32), r(32, 32, 3, 3) / math.sqrt(288), 1 + 0.1 * r(32),
         0.1 * r(32), r(32, 32, 3, 3) / math.sqrt(288), 1 + 0.1 * r(32), 0.1 * r(32), r(32, 32, 1, 1) / math.sqrt(32),
         1 + 0.1 * r(32), 0.1 * r(32)]
    args = [_lib.ptr(t) for t in p]
    run = lambda fused: _lib.call("sd_op_fcm_stem_block", _lib.ptr(fb), B, W, 80, *args, _lib.ptr(out), fused, st)
    t1 = timed(lambda: run(1), ("fcm_stem_block",))
    ta, tb = timed(lambda: run(0), ("fcm_stem",)), timed(lambda: run(0), ("fcm_conv3x3_band",))
    gb = (fb.numel() * 4 + out.numel() * 2) / 1e9
    print(f"layer1.0 B {B} F 80 W {W} stem + stride 2: fused {t1:7.1f} us ({gb / t1 * 1e3:5.2f} TB/s of in + out)  "
          f"two launches {ta + tb:7.1f} us ({ta:.1f} + {tb:.1f})  ratio {(ta + tb) / t1:4.2f}", flush=True)
    for name, H, stride in (("layer1.1", 40, 1), ("layer2.0", 40, 2), ("layer2.1", 20, 1)):
        g = torch.Generator().manual_seed(H + stride)
        r = lambda *s: torch.randn(*s, generator=g).to(dev)
        Ho = (H - 1) // stride + 1
        x = r(B, H, W, 32).to(torch.bfloat16)
        out = torch.empty(B, Ho, W, 32, dtype=torch.bfloat16, device=dev)
        p = [r(32, 32, 3, 3) / math.sqrt(288), 1 + 0.1 * r(32), 0.1 * r(32), r(32, 32, 3, 3) / math.sqrt(288),
             1 + 0.1 * r(32), 0.1 * r(32)]
        sc = [r(32, 32, 1, 1) / math.sqrt(32), 1 + 0.1 * r(32), 0.1 * r(32)] if stride == 2 else [None] * 3
        args = [_lib.ptr(t) for t in p + sc]
        run = lambda fused: _lib.call("sd_op_fcm_block", _lib.ptr(x), B, H, W, stride, *args, _lib.ptr(out), fused, st)
        t1 = timed(lambda: run(1), ("fcm_block",))
        t0 = timed(lambda: run(0), ("fcm_conv3x3_band",))
        gb = (x.numel() + out.numel()) * 2 / 1e9
        print(f"{name} B {B} H {H} W {W} stride {stride}: fused {t1:7.1f} us ({gb / t1 * 1e3:5.2f} TB/s of in + out)  "
              f"two launches {t0:7.1f} us  ratio {t0 / t1:4.2f}", flush=True)
