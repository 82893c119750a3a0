"""SimAM-ResNet34 (ASP) embedding extractor: the torch-functional restatement against the reference goldens, the key
layout, the new kind's lifecycle argument checks, the wrapper's refusals and the library's exports.  No GPU."""
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
from speaker_diarization_amd.ts_vad.embedding import SimAM_ResNet34_ASP  # noqa: E402
from speaker_diarization_amd.weights import (TSVADConfig, simam_resnet34_layout, simam_resnet34_state_dict,  # noqa: E402
                                             to_torch)
import simam_ref as sr  # noqa: E402
from make_golden import embed_wav  # noqa: E402
from make_golden_simam import CASES, EXTRACT, inputs  # noqa: E402

GOLD = os.path.join(HERE, "golden")
ATOL = 2e-5
KIND = "simam_resnet34"
GOOD = dict(in_planes=64, embed_dim=256, acoustic_dim=80, max_batch=1, max_frames=200, precision=0)


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def max_err(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    return float(np.abs(got - ref).max())


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_reference(name):
    g = gold("simam_emb")
    B, T, _, wseed, keep = CASES[name]
    sd = to_torch(simam_resnet34_state_dict(wseed, 256))
    r = sr.simam_resnet34_embedding(sd, torch.from_numpy(inputs(name)))
    err = max_err(r["emb"].numpy(), g[f"{name}.emb"])
    print(name, "emb max err", err)
    assert err <= ATOL
    if keep:
        for k in ("front", "stats"):
            err = max_err(r[k].numpy(), g[f"{name}.{k}"])
            print(name, k, "max err", err)
            assert err <= ATOL


def test_goldens_are_alive_and_one_frame_is_finite():
    g = gold("simam_emb")
    assert np.isfinite(g["t8.emb"]).all()                       # T' = 1 is valid for ASP (NaN for ResNet34's TSTP)
    assert 0.3 <= g["t200.emb"].std() <= 5.0
    front, stats = g["t38.front"], g["t38.stats"]
    const = front.std(-1) == 0
    assert 0.0 < const.mean() < 0.05                           # the goldens exercise constant channels, under 5 % ...
    assert (stats[:, 5120:][const] == np.float32(np.sqrt(np.float32(1e-5)))).all()   # ... whose sg is the clamp
    sd = to_torch(simam_resnet34_state_dict(CASES["t8"][3], 256))
    one = sr.simam_resnet34_embedding(sd, torch.from_numpy(inputs("t8")))
    assert one["front"].shape == (1, 5120, 1)
    assert (one["stats"][:, 5120:] == torch.sqrt(torch.tensor(1e-5))).all()
    assert torch.equal(one["stats"][:, :5120], one["front"][:, :, 0])


def test_extract_restatement_matches_reference():
    g = gold("simam_emb_extract")
    secs, bs, wav_seed, wseed = EXTRACT
    sd = to_torch(simam_resnet34_state_dict(wseed, 256))
    assert list(g["batches"]) == [2, 1]
    for i, s in enumerate(secs):
        wav = np.round(embed_wav(s, wav_seed + i) * 32768).astype(np.int16).astype(np.float64) / 32768.0
        got = sr.extract_embed(sd, wav, batch_size=bs).numpy()
        err = max_err(got, g[f"emb{i}"])
        print("extract", i, got.shape, "max err", err)
        assert err <= ATOL


def test_layout_matches_reference_keys():
    g = gold("simam_emb_keys")
    ref = {str(n): tuple(int(d) for d in str(s).split(",") if d)
           for n, s in zip(g["simam_resnet34.names"], g["simam_resnet34.shapes"])}
    lay = simam_resnet34_layout(256)
    ours = {n: tuple(s) for n, s, _ in lay}
    assert len(ours) == len(lay), "duplicate key in the layout"
    assert set(ours) == set(ref), (sorted(set(ours) - set(ref))[:5], sorted(set(ref) - set(ours))[:5])
    assert ours == ref
    assert "front.layer1.0.downsample.0.weight" not in ours and "front.layer2.0.downsample.0.weight" in ours
    assert not [n for n in ours if "shortcut" in n]


# ---- the lifecycle argument checks of tests/test_capi_lifecycle.py, for the new kind
def _create(conf, out):
    _lib.call(f"sd_{KIND}_create", None if conf is None else ctypes.byref(conf),
              None if out is None else ctypes.byref(out))


def test_kind_is_registered():
    assert _lib.KINDS[KIND] is _lib.SimamResnet34Config
    names = [f"sd_{KIND}_{f}" for f in ("create", "set_param", "finalize", "forward", "device_bytes", "destroy")]
    names += ["sd_op_simam", "sd_op_asp_pool", "sd_op_stem_conv"]
    assert set(names) <= set(_lib.EXPORTED)
    lib = _lib.load()
    assert not [s for s in names if not hasattr(lib, s)]


def test_create_null_arguments():
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: null argument$"):
        _create(None, ctypes.c_void_p())
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: null argument$"):
        _create(_lib.SimamResnet34Config(**GOOD), None)


@pytest.mark.parametrize("field,value,msg", [
    ("precision", 3, "precision must be 0 or 1"),
    ("precision", 2, "precision must be 0 or 1"),
    ("embed_dim", 12, "embed_dim must be a positive multiple of 8"),
    ("embed_dim", 0, "embed_dim must be a positive multiple of 8"),
    ("in_planes", 32, "SimAM_ResNet34_ASP (MI355X backend) supports in_planes 64 and acoustic_dim 80 only"),
    ("acoustic_dim", 40, "SimAM_ResNet34_ASP (MI355X backend) supports in_planes 64 and acoustic_dim 80 only"),
    ("max_batch", 0, "bad workspace sizes"),
    ("max_frames", 7, "bad workspace sizes"),
])
def test_create_rejects_one_bad_field(field, value, msg):
    h = ctypes.c_void_p()
    with pytest.raises(ValueError) as e:
        _create(_lib.SimamResnet34Config(**dict(GOOD, **{field: value})), h)
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
        _lib.call(f"sd_{KIND}_forward", None, None, 1, 8, None, None, None)
    assert getattr(lib, f"sd_{KIND}_destroy")(None) == _lib.SD_OK
    assert getattr(lib, f"sd_{KIND}_device_bytes")(None) == 0


# ---- the wrapper's refusals come before it touches a device
def test_wrapper_refusals():
    with pytest.raises(ValueError, match="NameError"):
        SimAM_ResNet34_ASP(speech_encoder=True)
    with pytest.raises(ValueError, match="in_planes 64"):
        SimAM_ResNet34_ASP(in_planes=32)
    with pytest.raises(ValueError, match="acoustic_dim 80"):
        SimAM_ResNet34_ASP(acoustic_dim=40)
    with pytest.raises(ValueError, match="NameError"):
        SimAM_ResNet34_ASP.__new__(SimAM_ResNet34_ASP).forward(torch.zeros(1, 8, 80), get_time_out=True)


def test_tsvad_speech_encoder_stays_unsupported():
    with pytest.raises(ValueError, match="unsupported TS-VAD configuration"):
        TSVADConfig(speech_encoder_type="simam_resnet34_wespeaker").variant
