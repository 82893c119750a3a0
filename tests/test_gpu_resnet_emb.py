"""ResNet34 target-speaker embedding extractor on the GPU (libsdiar sd_resnet34_* / sd_op_tstp_pool) against the
reference goldens (tests/golden/make_golden_resnet_emb.py) and float64 statistics.  Tolerances: fp32 1e-3; bf16
trunk: cosine >= 0.999 per row (test_gpu_campp.py's bound) plus twice the measured absolute error."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import embed_wav  # noqa: E402
from make_golden_resnet_emb import EMB_CASES, EMB_EXTRACT, emb_inputs  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.embedding import ResNet34, extract_embed, load_ts_embed  # noqa: E402
from speaker_diarization_amd.weights import resnet34_embed_state_dict, to_torch  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_ATOL = 1e-3
# bf16 trunk (bf16 maps through 33 convs, activations up to ~9; TSTP and the seg layers fp32).  Measured
# max|x - golden| on MI355X (the kernels are deterministic); the bounds are twice the largest of each kind.
BF16_MEASURED = {
    "emb": {"t38": 2.78e-2, "t17": 1.88e-2, "t200": 1.24e-2, "t9": 1.84e-2, "two": 1.72e-2, "extract": 1.21e-2},
    "stats": {"t38": 2.64e-2},
    "time_out": {"t38": 6.62e-2},     # map values up to ~9: a bf16 ulp there is 3.1e-2
}
BF16_ATOL = {k: 2 * max(v.values()) for k, v in BF16_MEASURED.items()}   # emb 5.6e-2 (std ~0.9), stats 5.3e-2
TSTP_RTOL = 1e-5
CONST_STD = np.float32(np.sqrt(1e-7))

_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(gpu, wseed, two, precision, max_batch=3, max_frames=200):
    key = (wseed, two, precision, max_batch, max_frames)
    if key not in _models:
        m = ResNet34(80, 256, two_emb_layer=two, device=gpu, precision=precision, max_batch=max_batch,
                     max_frames=max_frames)
        _models[key] = m.load_state_dict(to_torch(resnet34_embed_state_dict(wseed, 256, two)))
    return _models[key]


def _cos(a, b):
    a, b = a.reshape(len(a), -1).astype(np.float64), b.reshape(len(b), -1).astype(np.float64)
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


def tstp_gpu(x, gpu):
    """x (B, T, C) torch fp32 or bf16 on the CPU -> stats (B, 2C) numpy."""
    B, T, C = x.shape
    xd = x.to(gpu).contiguous()
    stats = torch.full((B, 2 * C), -7.0, device=gpu)
    _lib.call("sd_op_tstp_pool", _lib.ptr(xd), int(x.dtype == torch.bfloat16), B, T, C, _lib.ptr(stats),
              _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return stats.cpu().numpy()


def crafted_map(T, seed, B=2, C=2560):
    """Random channels; constant ones (c % 7 == 0); offset ones (c % 11 == 3: mean 100 / std 0.1, c % 11 == 5: mean
    1000 / std 0.01); one NaN element."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    c = np.arange(C)
    const = c % 7 == 0
    x[:, :, const] = rng.standard_normal((B, 1, int(const.sum()))).astype(np.float32) * 3
    o1, o2 = (c % 11 == 3) & ~const, (c % 11 == 5) & ~const
    x[:, :, o1] = (100 + 0.1 * rng.standard_normal((B, T, int(o1.sum())))).astype(np.float32)
    x[:, :, o2] = (1000 + 0.01 * rng.standard_normal((B, T, int(o2.sum())))).astype(np.float32)
    nan_at = (1, min(1, T - 1), 78)
    x[nan_at] = np.nan
    return x, const, nan_at


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("T", [1, 2, 3, 25, 75])
def test_tstp_pool_vs_float64(gpu, T, dtype):
    x, const, nan_at = crafted_map(T, 40 + T)
    xt = torch.from_numpy(x)
    if dtype == "bf16":
        xt = xt.to(torch.bfloat16)
    x64 = xt.float().numpy().astype(np.float64)          # the (bf16-rounded) values the kernel reads
    C = x.shape[2]
    with np.errstate(all="ignore"):
        mean = x64.mean(1)
        var = ((x64 - mean[:, None, :]) ** 2).sum(1) / (T - 1) if T > 1 else np.full_like(mean, np.nan)
        want = np.concatenate([mean, np.sqrt(var + 1e-7)], 1)
    got = tstp_gpu(xt, gpu)
    assert got.shape == want.shape == (2, 2 * C)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN not where float64 puts it"
    nan_cols = np.isnan(want)
    assert nan_cols[nan_at[0], nan_at[2]] and (T == 1 or nan_cols[nan_at[0], C + nan_at[2]])
    if T == 1:
        assert nan_cols[:, C:].all() and nan_cols[:, :C].sum() == 1
    else:
        assert nan_cols.sum() == 2
        assert (got[:, C:][:, const] == CONST_STD).all()     # constant channels: variance exactly 0
    ok = ~nan_cols
    rel = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
    print(f"tstp T={T} {dtype}: max rel err {rel.max():.3e}")
    assert rel.max() <= TSTP_RTOL


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(EMB_CASES))
def test_forward_vs_reference_golden(gpu, name, precision):
    B, T, two, _, wseed, keep = EMB_CASES[name]
    g = gold("resnet_emb")
    m = model(gpu, wseed, two, precision)
    x = torch.from_numpy(emb_inputs(name)).to(gpu)
    first, emb = m(x)
    emb = emb.cpu().numpy()
    want = g[f"{name}.emb"]
    assert emb.shape == want.shape == (B, 256)
    if name == "t8":
        assert np.isnan(want).all() and np.isnan(emb).all()
        return
    assert np.isfinite(emb).all()
    outs = [("emb", emb, want)]
    if two:
        outs.append(("emb", first.cpu().numpy(), g[f"{name}.emb_a"]))
    else:
        assert first.shape == () and float(first) == 0.0
    if keep:
        tout = m(x, get_time_out=True)
        assert tout.shape == (B, 2560, ResNet34.out_frames(T))
        stats = tstp_gpu(tout.permute(0, 2, 1).contiguous().cpu(), gpu)
        outs += [("time_out", tout.cpu().numpy(), g[f"{name}.time_out"]), ("stats", stats, g[f"{name}.stats"])]
    figs = [(kind, float(np.abs(got - ref).max()), float(_cos(got, ref).min())) for kind, got, ref in outs]
    for kind, err, cos in figs:
        print(f"resnet_emb {name} {precision} {kind}: max abs err {err:.3e}  min cos {cos:.6f}")
    for kind, err, cos in figs:
        if precision == "fp32":
            assert err <= FP32_ATOL
        else:
            assert cos >= 0.999
            assert err <= BF16_ATOL[kind]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_extract_embed_matches_reference(gpu, precision):
    secs, bs, wav_seed, wseed = EMB_EXTRACT
    g = gold("resnet_emb_extract")
    m = model(gpu, wseed, False, precision, max_batch=2, max_frames=598)
    figs = []
    for i, s in enumerate(secs):
        got = extract_embed(embed_wav(s, wav_seed + i), m, batch_size=bs).cpu().numpy()
        want = g[f"emb{i}"]
        assert got.shape == want.shape
        figs.append((float(np.abs(got - want).max()), float(_cos(got, want).min())))
        print(f"resnet_emb extract {i} {precision}: max abs err {figs[-1][0]:.3e}  min cos {figs[-1][1]:.6f}")
    for err, cos in figs:
        if precision == "fp32":
            assert err <= FP32_ATOL
        else:
            assert cos >= 0.999
            assert err <= BF16_ATOL["emb"]


def test_pt_round_trip(gpu, tmp_path):
    secs, bs, wav_seed, wseed = EMB_EXTRACT
    m = model(gpu, wseed, False, "fp32", max_batch=2, max_frames=598)
    got = extract_embed(embed_wav(secs[0], wav_seed), m).cpu()
    assert got.shape == (2, 256)
    os.makedirs(tmp_path / "meet")
    torch.save(got, tmp_path / "meet" / "3.pt")
    ts = load_ts_embed(str(tmp_path), "meet", [3, -1, -2], 256)
    assert ts.shape == (3, 256) and (ts[1:] == 0).all()
    torch.testing.assert_close(ts[0], got.mean(0))


def test_real_shape_rows_do_not_depend_on_the_batch(gpu):
    """One bf16 forward at the extractor's real shape, 96 chunks of 598 frames: rows 0 and 95 are bit-identical to
    the same two chunks run as a batch of 2 (each item's arithmetic is independent of the batch), which an
    addressing error at large B * T would break."""
    m = model(gpu, 31, False, "bf16", max_batch=96, max_frames=598)
    g = torch.Generator().manual_seed(96)
    x = torch.randn(96, 598, 80, generator=g).to(gpu)
    _, full = m(x)
    pair = torch.stack([x[0], x[95]])
    _, two = m(pair)
    torch.cuda.synchronize()
    assert torch.isfinite(full).all()
    assert torch.equal(full[[0, 95]].view(torch.int32), two.view(torch.int32))
    assert not torch.equal(full[0], full[95])


def test_batch_split_and_errors(gpu):
    sd = to_torch(resnet34_embed_state_dict(5, 256, False))
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((5, 60, 80)).astype(np.float32)).to(gpu)
    whole = ResNet34(80, 256, two_emb_layer=False, device=gpu, precision="fp32", max_batch=5, max_frames=64)
    whole.load_state_dict(sd)
    split = ResNet34(80, 256, two_emb_layer=False, device=gpu, precision="fp32", max_batch=2, max_frames=64)
    split.load_state_dict(sd)
    a, b = whole(x)[1], split(x)[1]      # 5 > max_batch 2: three device calls
    assert torch.equal(a, b)
    assert split.device_bytes > 0 and split.eval() is split and split.to(gpu) is split
    with pytest.raises(ValueError):
        split(torch.zeros(1, 65, 80, device=gpu))           # exceeds max_frames
    with pytest.raises(ValueError, match="80-dim"):
        split(torch.zeros(1, 60, 40, device=gpu))           # feat_dim
    with pytest.raises(ValueError, match="feat_dim 80"):
        ResNet34(40, 256, device=gpu)
    with pytest.raises(ValueError, match="TSTP"):
        ResNet34(80, 256, pooling_func="ASTP", device=gpu)
    with pytest.raises(ValueError, match="speech_encoder"):
        ResNet34(80, 256, speech_encoder=True, device=gpu)
    bad = dict(sd)
    bad.pop("seg_1.weight")
    with pytest.raises(RuntimeError, match="seg_1.weight"):
        ResNet34(80, 256, two_emb_layer=False, device=gpu, max_batch=1).load_state_dict(bad)
    extra = dict(sd)
    extra["pool.weight"] = torch.zeros(3)
    with pytest.raises(RuntimeError, match="pool.weight"):
        ResNet34(80, 256, two_emb_layer=False, device=gpu, max_batch=1).load_state_dict(extra)
