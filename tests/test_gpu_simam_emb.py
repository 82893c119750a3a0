"""SimAM-ResNet34 (ASP) target-speaker embedding extractor on the GPU (libsdiar sd_simam_resnet34_* / sd_op_asp_pool)
against the reference goldens (tests/golden/make_golden_simam.py).  Tolerances: fp32 1e-3; bf16 trunk: cosine >= 0.999
per row (test_gpu_campp.py's bound) plus twice the measured absolute error, test_gpu_resnet_emb.py's scheme."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from make_golden import embed_wav  # noqa: E402
from make_golden_simam import CASES, EXTRACT, inputs  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.embedding import SimAM_ResNet34_ASP, extract_embed  # noqa: E402
from speaker_diarization_amd.weights import simam_resnet34_state_dict, to_torch  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_ATOL = 1e-3
# bf16 trunk (bf16 maps through 33 convs and 16 SimAM gates; ASP and the bottleneck fp32).  Measured max|x - golden|
# on MI355X (the kernels are deterministic); the bounds are twice the largest of each kind.
BF16_MEASURED = {
    "emb": {"t38": 1.82e-2, "t17": 2.03e-2, "t8": 1.63e-2, "t200": 1.42e-2, "extract": 2.49e-2},
    "stats": {"t38": 4.01e-2},
    "front": {"t38": 8.21e-2},        # map values up to ~7.2: a bf16 ulp there is 3.1e-2
}
BF16_ATOL = {k: 2 * max(v.values()) for k, v in BF16_MEASURED.items()}   # emb 5.0e-2 (std ~1.2), stats 8.0e-2, front 0.16

_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(gpu, wseed, precision, max_batch=3, max_frames=200):
    key = (wseed, precision, max_batch, max_frames)
    if key not in _models:
        m = SimAM_ResNet34_ASP(device=gpu, precision=precision, max_batch=max_batch, max_frames=max_frames)
        _models[key] = m.load_state_dict(to_torch(simam_resnet34_state_dict(wseed, 256)))
    return _models[key]


def _cos(a, b):
    a, b = a.reshape(len(a), -1).astype(np.float64), b.reshape(len(b), -1).astype(np.float64)
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


def asp_gpu(front, sd, gpu):
    """front (B, 5120, T') on the GPU -> ASP stats (B, 10240) numpy, with the model's own attention weights."""
    B, C, T = front.shape
    x = front.permute(0, 2, 1).contiguous()
    eps = 1e-5
    s = sd["pooling.attention.2.weight"] / torch.sqrt(sd["pooling.attention.2.running_var"] + eps)
    h = sd["pooling.attention.2.bias"] - sd["pooling.attention.2.running_mean"] * s
    args = [sd["pooling.attention.0.weight"].reshape(128, C), sd["pooling.attention.0.bias"], s, h,
            sd["pooling.attention.3.weight"].reshape(C, 128), sd["pooling.attention.3.bias"]]
    dev = [a.to(gpu).contiguous() for a in args]
    stats = torch.full((B, 2 * C), -7.0, device=gpu)
    _lib.call("sd_op_asp_pool", _lib.ptr(x), 0, B, T, C, *[_lib.ptr(a) for a in dev], _lib.ptr(stats),
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return stats.cpu().numpy()


def check(figs, precision):
    for kind, name, err, cos in figs:
        print(f"simam_emb {name} {precision} {kind}: max abs err {err:.3e}  min cos {cos:.6f}")
    for kind, name, err, cos in figs:
        if precision == "fp32":
            assert err <= FP32_ATOL
        else:
            assert cos >= 0.999
            assert err <= BF16_ATOL[kind]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_vs_reference_golden(gpu, name, precision):
    B, T, _, wseed, keep = CASES[name]
    g = gold("simam_emb")
    m = model(gpu, wseed, precision)
    x = torch.from_numpy(inputs(name)).to(gpu)
    emb = m(x).cpu().numpy()
    want = g[f"{name}.emb"]
    assert emb.shape == want.shape == (B, 256)
    assert np.isfinite(emb).all()                       # t8 included: one pooled frame is valid for ASP
    outs = [("emb", emb, want)]
    if keep:
        front = m.front(x)
        assert front.shape == (B, 5120, SimAM_ResNet34_ASP.out_frames(T))
        stats = asp_gpu(front, to_torch(simam_resnet34_state_dict(wseed, 256)), gpu)
        outs += [("front", front.cpu().numpy(), g[f"{name}.front"]), ("stats", stats, g[f"{name}.stats"])]
    check([(kind, name, float(np.abs(got - ref).max()), float(_cos(got, ref).min())) for kind, got, ref in outs],
          precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_extract_embed_matches_reference(gpu, precision):
    secs, bs, wav_seed, wseed = EXTRACT
    g = gold("simam_emb_extract")
    assert list(g["batches"]) == [2, 1]                 # the reference's device calls: 2 chunks, then the short file
    m = model(gpu, wseed, precision, max_batch=2, max_frames=598)
    figs = []
    for i, s in enumerate(secs):
        got = extract_embed(embed_wav(s, wav_seed + i), m, batch_size=bs).cpu().numpy()
        want = g[f"emb{i}"]
        assert got.shape == want.shape == (int(g["batches"][i]), 256)
        figs.append(("emb", f"extract{i}", float(np.abs(got - want).max()), float(_cos(got, want).min())))
    check(figs, precision)


def test_real_shape_rows_do_not_depend_on_the_batch(gpu):
    """One bf16 forward at the extractor's real shape, 96 chunks of 598 frames: rows 0 and 95 are bit-identical to
    the same two chunks run as a batch of 2 (each item's arithmetic, the SimAM statistics included, is independent of
    the batch), which an addressing error at large B * T would break."""
    m = model(gpu, 31, "bf16", max_batch=96, max_frames=598)
    g = torch.Generator().manual_seed(96)
    x = torch.randn(96, 598, 80, generator=g).to(gpu)
    full = m(x)
    two = m(torch.stack([x[0], x[95]]))
    torch.cuda.synchronize()
    assert torch.isfinite(full).all()
    assert torch.equal(full[[0, 95]].view(torch.int32), two.view(torch.int32))
    assert not torch.equal(full[0], full[95])


def test_batch_split_and_errors(gpu):
    sd = to_torch(simam_resnet34_state_dict(5, 256))
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((5, 60, 80)).astype(np.float32)).to(gpu)
    whole = SimAM_ResNet34_ASP(device=gpu, precision="fp32", max_batch=5, max_frames=64).load_state_dict(sd)
    split = SimAM_ResNet34_ASP(device=gpu, precision="fp32", max_batch=2, max_frames=64).load_state_dict(sd)
    a, b = whole(x), split(x)           # 5 > max_batch 2: three device calls
    assert a.shape == (5, 256) and torch.equal(a, b)
    out = torch.empty(5, 256, device=gpu)
    assert split(x, out=out) is out and torch.equal(out, a)
    assert split.device_bytes > 0 and split.eval() is split and split.to(gpu) is split
    with pytest.raises(ValueError, match="max_frames"):
        split(torch.zeros(1, 65, 80, device=gpu))
    with pytest.raises(ValueError, match="80-dim"):
        split(torch.zeros(1, 60, 40, device=gpu))           # feature dimension
    with pytest.raises(ValueError, match="at least 8"):
        split(torch.zeros(1, 7, 80, device=gpu))            # refused by the wrapper ...
    emb = torch.zeros(1, 256, device=gpu)
    with pytest.raises(AssertionError, match="at least 8"):  # ... and by the library (SD_ERR_SHAPE)
        _lib.call("sd_simam_resnet34_forward", split._h, _lib.ptr(torch.zeros(1, 7, 80, device=gpu)), 1, 7,
                  _lib.ptr(emb), None, _lib.stream_ptr(gpu))
    assert torch.isfinite(split(torch.randn(1, 8, 80, generator=torch.Generator().manual_seed(1)).to(gpu))).all()
    with pytest.raises(ValueError, match="NameError"):
        split(x[:1], get_time_out=True)
    bad = dict(sd)
    bad.pop("bottleneck.weight")
    with pytest.raises(RuntimeError, match="bottleneck.weight"):
        SimAM_ResNet34_ASP(device=gpu, max_batch=1).load_state_dict(bad)
    bad = dict(sd)
    bad.pop("front.layer2.0.downsample.0.weight")
    with pytest.raises(RuntimeError, match="front.layer2.0.downsample.0.weight"):
        SimAM_ResNet34_ASP(device=gpu, max_batch=1).load_state_dict(bad)
    extra = dict(sd)
    extra["front.layer1.0.shortcut.0.weight"] = torch.zeros(3)
    with pytest.raises(RuntimeError, match="front.layer1.0.shortcut.0.weight"):
        SimAM_ResNet34_ASP(device=gpu, max_batch=1).load_state_dict(extra)
