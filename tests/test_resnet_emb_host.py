"""ResNet34 embedding extractor and TS-VAD proj_layer: key layouts, the torch-functional restatement against the
reference goldens, the split of proj_layer, seeded-weight stability and the library's exports.  No GPU."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.weights import (TSVADConfig, campplus_state_dict, resnet34_embed_layout,  # noqa: E402
                                             resnet34_embed_state_dict, resnet34_layout, to_torch, tsvad_layout,
                                             tsvad_state_dict)
import resnet_emb_ref as er  # noqa: E402
from make_golden import embed_wav  # noqa: E402
from make_golden_resnet_emb import (EMB_CASES, EMB_EXTRACT, PROJ_CASES, emb_inputs, proj_config,  # noqa: E402
                                    proj_inputs)

GOLD = os.path.join(HERE, "golden")
ATOL = 1e-5

# sha256 over (key, dtype, shape, bytes) of the seeded state dicts, recorded on the parent commit: the new layouts
# must not move any existing seed
PARENT_HASHES = {
    "v0": "f02d9ea21f06adc7ce8fbd673728e606afdf109871b3919a822de6f85066c86e",
    "rn34": "0ef90debc092a01dea124136275283658d9914d3c5301cb671e47af1dc83ebc6",
    "v1": "2f668bfa2063302aea4011552fb6b8aa8acbb1e56395c93fd8c57e4d66e3d21a",
    "campp": "151eb4397216f9a5eae3b107e363113eb88732a2634c1bba2fc8c42fb465d70d",
}


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def close(got, ref, atol=ATOL):
    """max abs error over the finite entries; NaN positions must be equal."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN positions differ"
    ok = ~np.isnan(ref)
    err = float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0
    return err, err <= atol


def sd_hash(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        a = np.ascontiguousarray(v)
        h.update(k.encode())
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name", list(EMB_CASES))
def test_embedding_restatement_matches_reference(name):
    g = gold("resnet_emb")
    B, T, two, _, wseed, keep = EMB_CASES[name]
    sd = to_torch(resnet34_embed_state_dict(wseed, 256, two))
    r = er.resnet34_embedding(sd, torch.from_numpy(emb_inputs(name)), two)
    last = r["embed_b"] if two else r["embed_a"]
    err, ok = close(last.numpy(), g[f"{name}.emb"])
    print(name, "emb max err", err)
    assert ok
    if two:
        err, ok = close(r["embed_a"].numpy(), g[f"{name}.emb_a"])
        assert ok, err
    if keep:
        for k in ("stats", "time_out"):
            err, ok = close(r[k].numpy(), g[f"{name}.{k}"])
            print(name, k, "max err", err)
            assert ok


def test_short_inputs_are_nan_then_finite():
    g = gold("resnet_emb")
    assert np.isnan(g["t8.emb"]).all() and np.isfinite(g["t9.emb"]).all()
    dead = (g["t38.time_out"].std(-1) == 0).mean()
    assert 0.01 < dead < 0.2, dead           # the goldens exercise constant (dead ReLU) channels
    std = g["t38.stats"][:, 2560:]
    assert (std[g["t38.time_out"].std(-1) == 0] == np.float32(np.sqrt(np.float32(1e-7)))).all()
    assert 0.3 <= g["t200.emb"].std() <= 5.0   # the seeded model is alive


def test_extract_restatement_matches_reference():
    g = gold("resnet_emb_extract")
    secs, bs, wav_seed, wseed = EMB_EXTRACT
    sd = to_torch(resnet34_embed_state_dict(wseed, 256, False))
    assert list(g["batches"]) == [2, 1]
    for i, s in enumerate(secs):
        wav = np.round(embed_wav(s, wav_seed + i) * 32768).astype(np.int16).astype(np.float64) / 32768.0
        got = er.extract_embed(sd, wav, batch_size=bs).numpy()
        err, ok = close(got, g[f"emb{i}"])
        print("extract", i, got.shape, "max err", err)
        assert ok


@pytest.mark.parametrize("name", list(PROJ_CASES))
def test_tsvad_proj_restatement_matches_reference(name):
    g = gold("tsvad_proj")
    _, B, T_fb, n_lab, _, wseed, nan_at = PROJ_CASES[name]
    cfg = proj_config(name)
    sd = to_torch(tsvad_state_dict(cfg, seed=wseed))
    ref_speech, ts = proj_inputs(name)
    got = er.tsvad_forward(sd, cfg, torch.from_numpy(ref_speech), torch.from_numpy(ts), n_lab).numpy()
    err, ok = close(got, g[f"{name}.logits"])
    print(name, "logits max err", err)
    assert ok
    if nan_at is not None:
        assert np.isnan(got[nan_at[0]]).all() and np.isfinite(np.delete(got, nan_at[0], 0)).all()
        base = g["rn34_tiny.logits"]
        assert np.abs(np.delete(got, nan_at[0], 0) - np.delete(base, nan_at[0], 0)).max() > 1e-3   # BN bypassed


def test_proj_split_equals_linear():
    rng = np.random.default_rng(5)
    se, e, B, T = 256, 384, 2, 7
    w = torch.from_numpy(rng.uniform(-1, 1, (e, 2 * se)).astype(np.float32) / np.float32(np.sqrt(2 * se)))
    b = torch.from_numpy(rng.standard_normal(e).astype(np.float32) * 0.05)
    ts = torch.from_numpy(rng.standard_normal((B, 1, se)).astype(np.float32))
    mix = torch.from_numpy(np.abs(rng.standard_normal((B, T, se))).astype(np.float32))
    ref = F.linear(torch.cat((ts.expand(B, T, se), mix), 2), w, b)
    wt, wm = er.proj_split(w, se)
    got = F.linear(ts, wt, b) + F.linear(mix, wm)
    assert float((got - ref).abs().max()) < 2e-6


def _keys(model):
    g = gold("resnet_emb_keys")
    return {str(n): tuple(int(d) for d in str(s).split(",") if d)
            for n, s in zip(g[f"{model}.names"], g[f"{model}.shapes"])}


@pytest.mark.parametrize("model,layout", [
    ("resnet34_one", lambda: resnet34_embed_layout(256, False)),
    ("resnet34_two", lambda: resnet34_embed_layout(256, True)),
    ("tsvad_campp_se256", lambda: tsvad_layout(TSVADConfig(speaker_embed_dim=256))),
    ("tsvad_rn34_se256", lambda: tsvad_layout(TSVADConfig(speech_encoder_type="resnet34_wespeaker",
                                                          speaker_embed_dim=256))),
])
def test_layout_matches_reference_keys(model, layout):
    ref = _keys(model)
    lay = layout()
    ours = {n: tuple(s) for n, s, _ in lay}
    assert len(ours) == len(lay), "duplicate key in the layout"
    assert set(ours) == set(ref), (sorted(set(ours) - set(ref))[:5], sorted(set(ref) - set(ours))[:5])
    assert ours == ref


def test_embed_layout_extends_the_trunk_unchanged():
    trunk = resnet34_layout("")
    for two in (False, True):
        lay = resnet34_embed_layout(256, two)
        assert lay[:len(trunk)] == trunk
        extra = [n for n, _, _ in lay[len(trunk):]]
        assert not [n for n in extra if n.startswith("pool")]
        assert ("seg_2.weight" in extra) == two and ("seg_bn_1.running_mean" in extra) == two
        assert "seg_bn_1.weight" not in extra   # BatchNorm1d(affine=False)


def test_proj_keys_only_when_needed():
    for cfg in (TSVADConfig(), TSVADConfig(speech_encoder_type="resnet34_wespeaker"), TSVADConfig.ots_vad_v1()):
        assert not [n for n, _, _ in tsvad_layout(cfg) if n.startswith("proj_layer")]
    for se in (256, 512):
        lay = dict((n, s) for n, s, _ in tsvad_layout(TSVADConfig(speaker_embed_dim=se)))
        assert lay["proj_layer.weight"] == (384, 2 * se) and lay["proj_layer.bias"] == (384,)


def test_existing_seeded_weights_unchanged():
    got = {
        "v0": sd_hash(tsvad_state_dict(TSVADConfig())),
        "rn34": sd_hash(tsvad_state_dict(TSVADConfig(speech_encoder_type="resnet34_wespeaker"))),
        "v1": sd_hash(tsvad_state_dict(TSVADConfig.ots_vad_v1())),
        "campp": sd_hash(campplus_state_dict()),
    }
    assert got == PARENT_HASHES


NEW_SYMBOLS = ("sd_resnet34_create", "sd_resnet34_set_param", "sd_resnet34_finalize", "sd_resnet34_forward",
               "sd_resnet34_device_bytes", "sd_resnet34_destroy", "sd_op_tstp_pool", "sd_op_speaker_input_proj")


def test_library_exports_new_symbols():
    assert set(NEW_SYMBOLS) <= set(_lib.EXPORTED)
    lib = _lib.load()
    missing = [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing


def _tsvad_conf(variant, se, e=384):
    return _lib.TsvadConfig(variant=variant, max_num_speaker=4, rs_len=4, max_batch=1, max_fbank_frames=398,
                            precision=0, num_transformer_layer=2, num_attention_head=4, transformer_embed_dim=e,
                            transformer_ffn_embed_dim=1536, speaker_embed_dim=se)


def test_create_rejects_proj_for_ots_vad_and_odd_widths_without_gpu():
    h = ctypes.c_void_p()
    with pytest.raises(ValueError, match="proj_layer"):
        _lib.call("sd_tsvad_create", ctypes.byref(_tsvad_conf(1, 256)), ctypes.byref(h))
    with pytest.raises(ValueError, match="multiples of 8"):
        _lib.call("sd_tsvad_create", ctypes.byref(_tsvad_conf(0, 250)), ctypes.byref(h))
    conf = _lib.Resnet34Config(feat_dim=40, embed_dim=256, two_emb_layer=0, max_batch=1, max_frames=598, precision=0)
    with pytest.raises(ValueError, match="feat_dim 80"):
        _lib.call("sd_resnet34_create", ctypes.byref(conf), ctypes.byref(h))
