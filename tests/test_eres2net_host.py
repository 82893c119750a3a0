"""ERes2NetV2 embedding extractor: the torch-functional restatement against the reference goldens, the key layout, the
new kind's lifecycle argument checks, the wrapper's refusals and the library's exports.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ts_vad.embedding import ERes2NetV2  # noqa: E402
from speaker_diarization_amd.weights import (TSVADConfig, eres2netv2_layout, eres2netv2_state_dict,  # noqa: E402
                                             to_torch)
import eres2net_ref as er  # noqa: E402
from make_golden import embed_wav  # noqa: E402
from make_golden_eres2net import (CASES, EXTRACT, F100_T, F100_T25, FRAME_CASES, TRIPLES, inputs)  # noqa: E402

GOLD = os.path.join(HERE, "golden")
# fp32 CPU round-off between the restatement and the reference module (two orderings of the same fp32 arithmetic:
# torch's BatchNorm against the scale / shift form of oracle.tsvad_ref._bn, through 16 blocks of values up to 40).
# Measured maxima over every case of both triples, and the bound = 4 x the measurement:
MEASURED_MAX = {"emb": 7.2e-6, "stats": 1.03e-4, "frame": 2.12e-4, "extract": 4.5e-6}
ATOL = {k: 4.0 * v for k, v in MEASURED_MAX.items()}
KIND = "eres2netv2"
GOOD = dict(feat_dim=80, embedding_size=192, m_channels=64, base_width=26, scale=2, expansion=2, max_batch=1,
            max_frames=200, precision=0)
MEASURED = {}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def max_err(got, ref, kind=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    e = float(np.abs(got - ref).max())
    if kind:
        MEASURED[kind] = max(MEASURED.get(kind, 0.0), e)
    return e


def state(tag, wseed):
    return to_torch(eres2netv2_state_dict(wseed, *TRIPLES[tag], 192))


@pytest.mark.parametrize("tag", list(TRIPLES))
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_reference(tag, name):
    g, gf = gold(f"eres2net_{tag}_emb"), gold(f"eres2net_{tag}_frames")
    bw, sc, _ = TRIPLES[tag]
    r = er.forward(state(tag, CASES[name][3]), torch.from_numpy(inputs(name)), bw, sc)
    if name == "t8":                       # T' = 1: the unbiased variance of one frame is NaN, and so is every output
        assert g["t8.nan"].all() and np.isnan(r["emb"].numpy()).all()
        assert np.array_equal(np.isnan(r["emb"].numpy()), g["t8.nan"])
        err = max_err(r["frame"].numpy(), gf["t8.frame"], "frame")
        print(tag, name, "frame max err", err)
        assert err <= ATOL["frame"]
        return
    err = max_err(r["emb"].numpy(), g[f"{name}.emb"], "emb")
    print(tag, name, "emb max err", err)
    assert err <= ATOL["emb"]
    if name == "t38":
        e1 = max_err(r["stats"][:1].numpy(), g["t38.stats"], "stats")
        e2 = max_err(r["frame"][:1].numpy(), gf["t38.frame"], "frame")
        print(tag, name, "stats max err", e1, "frame max err", e2)
        assert e1 <= ATOL["stats"] and e2 <= ATOL["frame"]


def test_frame_level_restatement_matches_reference():
    g = gold("eres2net_base_frames2")
    bw, sc, _ = TRIPLES["base"]
    r = er.forward(state("base", FRAME_CASES["f17"][3]), torch.from_numpy(inputs("f17")), bw, sc)
    assert max_err(r["frame25"].numpy(), g["f17.frame25"], "frame") <= ATOL["frame"]
    r = er.forward(state("base", FRAME_CASES["f100"][3]), torch.from_numpy(inputs("f100")), bw, sc)
    assert list(g["f100.frame_t"]) == list(F100_T) and list(g["f100.frame25_t"]) == list(F100_T25)
    assert tuple(r["frame"].shape) == (1, 10240, 13) and tuple(r["frame25"].shape) == (1, 10240, 25)
    assert max_err(r["frame"][:, :, list(F100_T)].numpy(), g["f100.frame"], "frame") <= ATOL["frame"]
    assert max_err(r["frame25"][:, :, list(F100_T25)].numpy(), g["f100.frame25"], "frame") <= ATOL["frame"]
    print("measured", MEASURED)


def test_goldens_are_alive():
    for tag in TRIPLES:
        g, gf = gold(f"eres2net_{tag}_emb"), gold(f"eres2net_{tag}_frames")
        assert 0.3 <= g["t200.emb"].std() <= 5.0
        fr = gf["t38.frame"]
        assert 0.01 < (fr > 20).mean() + (fr == 0).mean() < 0.9     # the blend leaves [0, 20]; zeros are not everything
        assert fr.max() > 20.0                                      # x (1 + tanh) exceeds the clamp's 20: out4 reached it


def test_hardtanh_semantics():
    x = torch.tensor([float("nan"), -1.0, 5.0, 25.0, float("inf")])
    y = er.clamp20(x)
    assert torch.isnan(y[0]) and y[1:].tolist() == [0.0, 5.0, 20.0, 20.0]


def test_extract_restatement_matches_reference():
    g = gold("eres2net_extract")
    secs, bs, wav_seed, wseed = EXTRACT
    bw, sc, _ = TRIPLES["w24"]
    sd = state("w24", wseed)
    assert list(g["batches"]) == [2, 1]
    for i, s in enumerate(secs):
        wav = np.round(embed_wav(s, wav_seed + i) * 32768).astype(np.int16).astype(np.float64) / 32768.0
        got = er.extract_embed(sd, wav, bw, sc, batch_size=bs).numpy()
        err = max_err(got, g[f"emb{i}"])
        print("extract", i, got.shape, "max err", err)
        assert err <= ATOL["extract"]


@pytest.mark.parametrize("tag", list(TRIPLES))
def test_layout_matches_reference_keys(tag):
    g = gold("eres2net_keys")
    ref = {str(n): tuple(int(d) for d in str(s).split(",") if d) for n, s in zip(g[f"{tag}.names"], g[f"{tag}.shapes"])}
    lay = eres2netv2_layout(*TRIPLES[tag], 192)
    ours = {n: tuple(s) for n, s, _ in lay}
    assert len(ours) == len(lay), "duplicate key in the layout"
    assert set(ours) == set(ref), (sorted(set(ours) - set(ref))[:5], sorted(set(ref) - set(ours))[:5])
    assert ours == ref
    assert "layer1.0.shortcut.0.weight" in ours and "layer1.1.shortcut.0.weight" not in ours
    assert "layer2.0.fuse_models.0.local_att.0.weight" not in ours
    assert f"layer3.0.fuse_models.{TRIPLES[tag][1] - 2}.local_att.4.running_var" in ours


# ---- the lifecycle argument checks of tests/test_capi_lifecycle.py, for the new kind
def _create(conf, out):
    _lib.call(f"sd_{KIND}_create", None if conf is None else ctypes.byref(conf),
              None if out is None else ctypes.byref(out))


def test_kind_is_registered():
    assert _lib.KINDS[KIND] is _lib.Eres2netv2Config
    names = [f"sd_{KIND}_{f}" for f in ("create", "set_param", "finalize", "forward", "device_bytes", "destroy")]
    names += ["sd_op_res2_conv3x3", "sd_op_aff_gate"]
    assert set(names) <= set(_lib.EXPORTED)
    lib = _lib.load()
    assert not [s for s in names if not hasattr(lib, s)]


def test_create_null_arguments():
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: null argument$"):
        _create(None, ctypes.c_void_p())
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: null argument$"):
        _create(_lib.Eres2netv2Config(**GOOD), None)


TRIPLE_MSG = "ERes2NetV2 (MI355X backend) builds (baseWidth, scale, expansion) = (26, 2, 2) or (24, 4, 4) only"
SIZE_MSG = "ERes2NetV2 (MI355X backend) supports feat_dim 80 and m_channels 64 only"


@pytest.mark.parametrize("fields,msg", [
    (dict(precision=3), "precision must be 0 or 1"),
    (dict(precision=2), "precision must be 0 or 1"),
    (dict(embedding_size=12), "embedding_size must be a positive multiple of 8"),
    (dict(embedding_size=0), "embedding_size must be a positive multiple of 8"),
    (dict(feat_dim=40), SIZE_MSG),
    (dict(m_channels=32), SIZE_MSG),
    (dict(base_width=24), TRIPLE_MSG),
    (dict(scale=4), TRIPLE_MSG),
    (dict(expansion=4), TRIPLE_MSG),
    (dict(base_width=26, scale=4, expansion=4), TRIPLE_MSG),
    (dict(max_batch=0), "bad workspace sizes"),
    (dict(max_frames=7), "bad workspace sizes"),
])
def test_create_rejects_bad_fields(fields, msg):
    h = ctypes.c_void_p()
    with pytest.raises(ValueError) as e:
        _create(_lib.Eres2netv2Config(**dict(GOOD, **fields)), h)
    assert str(e.value) == f"sd_{KIND}_create: {msg}"
    assert h.value is None      # a refused create writes no handle


def test_null_handle():
    lib = _lib.load()
    data = (ctypes.c_float * 1)(1.0)
    shape = (ctypes.c_int64 * 1)(1)
    with pytest.raises(ValueError, match=f"^sd_{KIND}_set_param: null argument$"):
        _lib.call(f"sd_{KIND}_set_param", None, b"w", data, shape, 1)
    with pytest.raises(ValueError, match=f"^sd_{KIND}_finalize: null handle$"):
        _lib.call(f"sd_{KIND}_finalize", None)
    with pytest.raises(ValueError, match=f"^sd_{KIND}_forward: null argument$"):
        _lib.call(f"sd_{KIND}_forward", None, None, 1, 8, None, None, None, None)
    assert getattr(lib, f"sd_{KIND}_destroy")(None) == _lib.SD_OK
    assert getattr(lib, f"sd_{KIND}_device_bytes")(None) == 0


# ---- the wrapper's refusals come before it touches a device
def test_wrapper_refusals():
    with pytest.raises(ValueError, match="two_emb_layer=False only"):
        ERes2NetV2(two_emb_layer=True)
    with pytest.raises(ValueError, match="TSTP pooling only"):
        ERes2NetV2(pooling_func="TAP")
    with pytest.raises(ValueError, match=r"\(26, 2, 2\) or \(24, 4, 4\) only"):
        ERes2NetV2(baseWidth=24)
    with pytest.raises(ValueError, match=r"\(26, 2, 2\) or \(24, 4, 4\) only"):
        ERes2NetV2(baseWidth=26, scale=4, expansion=4)
    with pytest.raises(ValueError, match="feat_dim 80"):
        ERes2NetV2(feat_dim=40)
    with pytest.raises(ValueError, match="m_channels 64"):
        ERes2NetV2(m_channels=32)
    with pytest.raises(ValueError, match="precision"):
        ERes2NetV2(precision="bf16x3")
    m = ERes2NetV2.__new__(ERes2NetV2)
    m.feat_dim = 80
    with pytest.raises(ValueError, match="at least 8 fbank frames"):
        m.forward(torch.zeros(1, 7, 80))
    with pytest.raises(ValueError, match="80-dim fbank"):
        m.get_frame_level_feat(torch.zeros(1, 8, 40))


@pytest.mark.parametrize("name", ["ERes2NetV2_COMMON", "ERes2NetV2_w24s4ep4_COMMON"])
def test_tsvad_speech_encoder_stays_unsupported(name):
    with pytest.raises(ValueError, match="unsupported TS-VAD configuration"):
        TSVADConfig(speech_encoder_type=name).variant
