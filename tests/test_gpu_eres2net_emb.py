"""ERes2NetV2 target-speaker embedding extractor on the GPU (libsdiar sd_eres2netv2_*) against the reference goldens
(tests/golden/make_golden_eres2net.py), for both size triples.  Tolerances: fp32 1e-3, the project's parity bar; bf16
trunk: cosine >= 0.999 per row plus twice the measured absolute error of each kind, test_gpu_simam_emb.py's scheme."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from make_golden import embed_wav  # noqa: E402
from make_golden_eres2net import CASES, EXTRACT, F100_T, F100_T25, FRAME_CASES, TRIPLES, inputs  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.embedding import ERes2NetV2, extract_embed  # noqa: E402
from speaker_diarization_amd.weights import eres2netv2_state_dict, to_torch  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_ATOL = 1e-3
# fp32 measured on MI355X, max |x - golden| over every case of both triples (frame maps hold values up to 40):
FP32_MEASURED = {"emb": 1.75e-5, "stats": 2.51e-4, "frame": 5.82e-4}
# bf16 trunk (bf16 maps through 49 / 81 convs and the AFF gates; fuse34's blend, TSTP and seg_1 fp32).  Measured
# max |x - golden| on MI355X (the kernels are deterministic), the largest case of each kind; the bounds are twice these.
BF16_MEASURED = {
    "emb": {"base.t38": 3.70e-2, "base.t17": 4.81e-2, "base.t9": 4.49e-2, "base.t200": 2.20e-2, "w24.t38": 8.68e-2,
            "w24.t17": 8.73e-2, "w24.t9": 8.54e-2, "w24.t200": 4.68e-2, "extract": 4.12e-2},
    "stats": {"base.t38": 5.18e-1, "w24.t38": 1.28},
    # map values up to 40 (a bf16 ulp there is 0.25) behind clamps at 20 that a rounding can switch on or off
    "frame": {"base.t38": 1.20, "base.t8": 5.60e-1, "w24.t38": 3.15, "w24.t8": 1.30, "f17.frame25": 5.36e-1,
              "f100.frame": 1.17, "f100.frame25": 6.44e-1},
}
BF16_ATOL = {k: 2 * max(v.values()) for k, v in BF16_MEASURED.items()}   # emb 0.17 (std ~1.5), stats 2.6, frame 6.3

_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def model(gpu, wseed, tag, precision, max_batch=3, max_frames=200):
    key = (wseed, tag, precision, max_batch, max_frames)
    if key not in _models:
        bw, sc, ex = TRIPLES[tag]
        m = ERes2NetV2(baseWidth=bw, scale=sc, expansion=ex, device=gpu, precision=precision, max_batch=max_batch,
                       max_frames=max_frames)
        _models[key] = m.load_state_dict(to_torch(eres2netv2_state_dict(wseed, bw, sc, ex, 192)))
    return _models[key]


def _cos(a, b):
    a, b = a.reshape(len(a), -1).astype(np.float64), b.reshape(len(b), -1).astype(np.float64)
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


def tstp_of_frames(frame, F=10):
    """(B, F C, T) in the frame-level order f * C + c -> TSTP statistics (B, 2 C F) in float64, flattened c * F + f."""
    B, D, T = frame.shape
    x = frame.astype(np.float64).reshape(B, F, D // F, T).transpose(0, 2, 1, 3).reshape(B, D, T)
    return np.concatenate((x.mean(-1), np.sqrt(x.var(-1, ddof=1) + 1e-8)), 1)


def check(figs, precision):
    for kind, name, err, cos in figs:
        print(f"eres2net {name} {precision} {kind}: max abs err {err:.3e}  min cos {cos:.6f}")
    for kind, name, err, cos in figs:
        if precision == "fp32":
            assert err <= FP32_ATOL
        else:
            assert cos >= 0.999
            assert err <= BF16_ATOL[kind]


def fig(kind, name, got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return kind, name, float(np.abs(got - ref).max()), float(_cos(got, ref).min())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("tag", list(TRIPLES))
def test_forward_vs_reference_golden(gpu, tag, name, precision):
    B, T, _, wseed = CASES[name]
    g, gf = gold(f"eres2net_{tag}_emb"), gold(f"eres2net_{tag}_frames")
    m = model(gpu, wseed, tag, precision)
    x = torch.from_numpy(inputs(name)).to(gpu)
    emb = m(x).cpu().numpy()
    assert emb.shape == (B, 192)
    D = 5120 * TRIPLES[tag][2]
    if name == "t8":                       # T' = 1: NaN standard deviations, an all-NaN embedding, a finite frame map
        assert np.array_equal(np.isnan(emb), g["t8.nan"]) and g["t8.nan"].all()
        frame = m.get_frame_level_feat(x).cpu().numpy()
        assert frame.shape == (1, D, 1)
        check([fig("frame", f"{tag}.{name}", frame, gf["t8.frame"])], precision)
        return
    figs = [fig("emb", f"{tag}.{name}", emb, g[f"{name}.emb"])]
    if name == "t38":
        frame = m.get_frame_level_feat(x).cpu().numpy()
        assert frame.shape == (B, D, ERes2NetV2.out_frames(T))
        figs.append(fig("frame", f"{tag}.{name}", frame[:1], gf["t38.frame"]))
        figs.append(fig("stats", f"{tag}.{name}", tstp_of_frames(frame[:1]).astype(np.float32), g["t38.stats"]))
    check(figs, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frame_level_outputs(gpu, precision):
    g = gold("eres2net_base_frames2")
    m = model(gpu, FRAME_CASES["f17"][3], "base", precision)
    x = torch.from_numpy(inputs("f17")).to(gpu)
    f25 = m.get_frame_level_feat_frame_rate25(x).cpu().numpy()
    figs = [fig("frame", "f17.frame25", f25, g["f17.frame25"])]
    m = model(gpu, FRAME_CASES["f100"][3], "base", precision)
    x = torch.from_numpy(inputs("f100")).to(gpu)
    f, f25 = m.get_frame_level_feat(x).cpu().numpy(), m.get_frame_level_feat_frame_rate25(x).cpu().numpy()
    assert f.shape == (1, 10240, 13) and f25.shape == (1, 10240, 25)
    figs.append(fig("frame", "f100.frame", f[:, :, list(F100_T)], g["f100.frame"]))
    figs.append(fig("frame", "f100.frame25", f25[:, :, list(F100_T25)], g["f100.frame25"]))
    check(figs, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_extract_embed_matches_reference(gpu, precision):
    secs, bs, wav_seed, wseed = EXTRACT
    g = gold("eres2net_extract")
    assert list(g["batches"]) == [2, 1]                 # the reference's device calls: 2 chunks, then the short file
    m = model(gpu, wseed, "w24", precision, max_batch=2, max_frames=598)
    figs = []
    for i, s in enumerate(secs):
        got = extract_embed(embed_wav(s, wav_seed + i), m, batch_size=bs).cpu().numpy()
        assert got.shape == (int(g["batches"][i]), 192)
        figs.append(fig("emb", f"extract{i}", got, g[f"emb{i}"]))
    check(figs, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", list(TRIPLES))
def test_rows_do_not_depend_on_the_batch(gpu, tag, precision):
    """Every output of a row is bit-identical whether the row runs alone or in a batch of 3."""
    m = model(gpu, CASES["t17"][3], tag, precision)
    x = torch.from_numpy(inputs("t17")).to(gpu)
    full, fr, fr25 = m(x), m.get_frame_level_feat(x), m.get_frame_level_feat_frame_rate25(x)
    for b in range(3):
        one = x[b:b + 1]
        for whole, alone in ((full, m(one)), (fr, m.get_frame_level_feat(one)),
                             (fr25, m.get_frame_level_feat_frame_rate25(one))):
            assert torch.equal(whole[b:b + 1].contiguous().view(torch.int32), alone.contiguous().view(torch.int32))
    assert not torch.equal(full[0], full[1])


def test_batch_split_and_errors(gpu):
    sd = to_torch(eres2netv2_state_dict(5, 26, 2, 2, 192))
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((5, 60, 80)).astype(np.float32)).to(gpu)
    whole = ERes2NetV2(device=gpu, precision="fp32", max_batch=5, max_frames=64).load_state_dict(sd)
    split = ERes2NetV2(device=gpu, precision="fp32", max_batch=2, max_frames=64).load_state_dict(sd)
    a, b = whole(x), split(x)           # 5 > max_batch 2: three device calls
    assert a.shape == (5, 192) and torch.equal(a, b)
    out = torch.empty(5, 192, device=gpu)
    assert split(x, out=out) is out and torch.equal(out, a)
    assert torch.equal(whole.get_frame_level_feat(x), split.get_frame_level_feat(x))
    assert split.device_bytes > 0 and split.eval() is split and split.to(gpu) is split
    with pytest.raises(ValueError, match="max_frames"):
        split(torch.zeros(1, 65, 80, device=gpu))
    with pytest.raises(ValueError, match="80-dim"):
        split(torch.zeros(1, 60, 40, device=gpu))           # feature dimension
    with pytest.raises(ValueError, match="at least 8"):
        split(torch.zeros(1, 7, 80, device=gpu))            # refused by the wrapper ...
    emb = torch.zeros(1, 192, device=gpu)
    with pytest.raises(AssertionError, match="at least 8"):  # ... and by the library (SD_ERR_SHAPE)
        _lib.call("sd_eres2netv2_forward", split._h, _lib.ptr(torch.zeros(1, 7, 80, device=gpu)), 1, 7,
                  _lib.ptr(emb), None, None, _lib.stream_ptr(gpu))
    with pytest.raises(ValueError, match="max_batch"):      # the library's own bound, past the wrapper's split
        _lib.call("sd_eres2netv2_forward", split._h, _lib.ptr(torch.zeros(3, 8, 80, device=gpu)), 3, 8,
                  _lib.ptr(torch.zeros(3, 192, device=gpu)), None, None, _lib.stream_ptr(gpu))
    bad = dict(sd)
    bad.pop("seg_1.weight")
    with pytest.raises(RuntimeError, match="seg_1.weight"):
        ERes2NetV2(device=gpu, max_batch=1).load_state_dict(bad)
    bad = dict(sd)
    bad.pop("layer3.0.fuse_models.0.local_att.3.bias")
    with pytest.raises(RuntimeError, match="layer3.0.fuse_models.0.local_att.3.bias"):
        ERes2NetV2(device=gpu, max_batch=1).load_state_dict(bad)
    extra = dict(sd)
    extra["layer1.1.shortcut.0.weight"] = torch.zeros(3)
    with pytest.raises(RuntimeError, match="layer1.1.shortcut.0.weight"):
        ERes2NetV2(device=gpu, max_batch=1).load_state_dict(extra)
    with pytest.raises(RuntimeError, match="conv1.weight"):     # the base triple's weights in the w24 model
        ERes2NetV2(baseWidth=24, scale=4, expansion=4, device=gpu, max_batch=1).load_state_dict(sd)
