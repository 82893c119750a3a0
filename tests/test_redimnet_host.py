"""ReDimNetB2 embedding extractor and TS-VAD variant 4: the torch-functional restatement against the reference goldens,
the key layouts, the byte stability of the seeded weights, the exactness of the head padding, the new kind's lifecycle
argument checks, the wrapper's refusals and the library's exports.  No GPU."""
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
from speaker_diarization_amd.ts_vad.embedding import ReDimNetB2  # noqa: E402
from speaker_diarization_amd.weights import (TSVADConfig, redimnet_embed_state_dict, redimnet_layout,  # noqa: E402
                                             to_torch, tsvad_layout, tsvad_state_dict)
import redimnet_ref as rr  # noqa: E402
from make_golden_redimnet import (DIGEST_SEED, EMB_CASES, FRAME_CASE, KEEP_FRAMES, T1_CASE, TSVAD_CASES,  # noqa: E402
                                  TSVAD_NAN, TSVAD_RAISES, emb_inputs, state_digest, tsvad_inputs72)

GOLD = os.path.join(HERE, "golden")
KIND = "redimnet"
GOOD = dict(feat_dim=72, embed_dim=192, max_batch=1, max_frames=200, precision=0)
ATOL = 1e-5    # restatement against the reference module, frame-level map and embedding: the ECAPA host test's bound


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def err(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    return float(np.abs(got - ref).max())


@pytest.mark.parametrize("name", list(EMB_CASES) + [FRAME_CASE[0]])
def test_restatement_matches_reference(name):
    g = gold("redimnet_b2_emb")
    B, T, iseed, wseed = dict(EMB_CASES, **{FRAME_CASE[0]: FRAME_CASE[1]})[name]
    emb, frames = rr.embed(to_torch(redimnet_embed_state_dict(wseed)), torch.from_numpy(emb_inputs(B, T, iseed)))
    frames = frames.permute(0, 2, 1)
    if name in KEEP_FRAMES:
        frames = frames[:, list(KEEP_FRAMES[name])]
    e1, e2 = err(emb.numpy(), g[f"{name}.emb"]), err(frames.numpy(), g[f"{name}.frames"])
    print(name, "emb err", e1, "frames err", e2)
    assert e1 < ATOL and e2 < ATOL


def test_one_frame_map_is_finite_and_embedding_is_not():
    g = gold("redimnet_b2_emb")
    name, (B, T, iseed, wseed) = T1_CASE
    emb, frames = rr.embed(to_torch(redimnet_embed_state_dict(wseed)), torch.from_numpy(emb_inputs(B, T, iseed)))
    assert not np.isfinite(emb.numpy()).any()        # ASTP's unbiased variance of one frame
    assert err(frames.permute(0, 2, 1).numpy(), g[f"{name}.frames"]) < ATOL


def test_head_padding_is_exact():
    """Zero rows in q / k / v and zero columns in out_proj add exact zeros: the padded restatement equals the plain one
    to the last bit of every sum that does not change its length, and to fp32 round-off where torch's matmul blocks
    the longer dot product differently."""
    B, T, iseed, wseed = EMB_CASES["t8"]
    sd = to_torch(redimnet_embed_state_dict(wseed))
    x = torch.from_numpy(emb_inputs(B, T, iseed))
    plain, padded = rr.frame_level(sd, x), rr.frame_level(sd, x, padded=True)
    e = err(padded.numpy(), plain.numpy())
    print("padded heads against plain heads: max err", e)
    assert e < ATOL
    assert [rr.padded_width(h) for h in (24, 36, 72)] == [32, 48, 96]
    # one attention call, where the padding is the only difference: outputs of magnitude <= 3 from dot products of up to
    # 288 terms that torch blocks differently at the two widths, i.e. a few 1e-6 of fp32 round-off at the most
    p = "backbone.stage5.6.tcm.4.attention."
    h = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 9, 288)).astype(np.float32))
    assert err(rr.mha(sd, p, h, 96).numpy(), rr.mha(sd, p, h).numpy()) < ATOL


def test_layout_matches_reference_keys():
    g = gold("redimnet_b2_keys")
    ref = {str(n): tuple(int(d) for d in str(s).split(",") if d) for n, s in zip(g["names"], g["shapes"])}
    lay = redimnet_layout()
    ours = {n: tuple(s) for n, s, _ in lay}
    assert len(ref) == 548 and int(g["n_params"]) == 4888241
    assert len(ours) == len(lay), "duplicate key in the layout"
    assert set(ours) == set(ref), (sorted(set(ours) - set(ref))[:5], sorted(set(ref) - set(ours))[:5])
    assert ours == ref
    assert [n for n, _, _ in lay] == [str(n) for n in g["names"]]      # the reference's order too
    assert "backbone.stage0.4.tcm.4.attention.q_proj.weight" in ours and "backbone.stage5.6.exp_dim_conv.bias" in ours


def test_seeded_weights_are_byte_stable_and_not_trivial():
    g = gold("redimnet_b2_keys")
    assert int(g["digest_seed"]) == DIGEST_SEED
    sd = redimnet_embed_state_dict(DIGEST_SEED)
    assert state_digest(sd) == str(g["digest"])
    assert state_digest(redimnet_embed_state_dict(DIGEST_SEED + 1)) != str(g["digest"])
    w = sd["backbone.inputs_weights.3"]
    assert w.shape == (1, 4, 1152, 1) and 0.3 < w.std() < 0.8            # a swapped stage order shows
    assert sd["backbone.stage2.1.conv_block.norm.running_mean"].std() > 0.15
    v = sd["backbone.stage2.1.conv_block.norm.running_var"]
    assert v.min() < 0.7 and v.max() > 1.3                               # a wrong-side BatchNorm shows
    for k in ("backbone.stem.1.weight", "backbone.stage0.4.red_dim_conv.1.weight",
              "backbone.stage0.4.tcm.4.final_layer_norm.weight"):
        assert np.abs(sd[k] - 1.0).max() > 0.1, k                        # a dropped LayerNorm gain shows


# ---- the lifecycle argument checks of tests/test_capi_lifecycle.py, for the new kind
def _create(conf, out):
    _lib.call(f"sd_{KIND}_create", None if conf is None else ctypes.byref(conf),
              None if out is None else ctypes.byref(out))


def test_kind_is_registered():
    assert _lib.KINDS[KIND] is _lib.RedimnetConfig
    names = [f"sd_{KIND}_{f}" for f in ("create", "set_param", "finalize", "forward", "device_bytes", "destroy",
                                         "debug_generic")]
    names += ["sd_op_redim_block2d", "sd_op_redim_dwconv1d", "sd_op_redim_stage_mix", "sd_op_redim_stem",
              "sd_op_astp_pool_c"]
    assert set(names) <= set(_lib.EXPORTED)
    lib = _lib.load()
    assert not [s for s in names if not hasattr(lib, s)]


def test_create_null_arguments():
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: null argument$"):
        _create(None, ctypes.c_void_p())
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: null argument$"):
        _create(_lib.RedimnetConfig(**GOOD), None)


@pytest.mark.parametrize("fields,msg", [
    (dict(precision=3), "precision must be 0, 1 or 2"),
    (dict(precision=-1), "precision must be 0, 1 or 2"),
    (dict(feat_dim=80), "ReDimNetB2 (MI355X backend) supports feat_dim 72 only"),
    (dict(embed_dim=0), "embed_dim must be a positive multiple of 4"),
    (dict(embed_dim=190), "embed_dim must be a positive multiple of 4"),
    (dict(max_batch=0), "bad workspace sizes"),
    (dict(max_frames=1), "bad workspace sizes"),
])
def test_create_rejects_bad_fields(fields, msg):
    h = ctypes.c_void_p()
    with pytest.raises(ValueError) as e:
        _create(_lib.RedimnetConfig(**dict(GOOD, **fields)), h)
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
    with pytest.raises(ValueError, match=f"^sd_{KIND}_debug_generic: null handle$"):
        _lib.call(f"sd_{KIND}_debug_generic", None, 1)
    assert getattr(lib, f"sd_{KIND}_destroy")(None) == _lib.SD_OK
    assert getattr(lib, f"sd_{KIND}_device_bytes")(None) == 0


def test_op_argument_checks_need_no_device():
    with pytest.raises(ValueError, match="redim_block2d: bad argument"):
        _lib.call("sd_op_redim_block2d", None, 1, 1, 16, None, None, None, None, None, None, None, 1, 0, None)
    with pytest.raises(ValueError, match="redim_stage_mix: 2 to 7 inputs"):
        _lib.call("sd_op_redim_stage_mix", None, 2, 1, None, None, 0, None)
    with pytest.raises(ValueError, match="redim_stem: bad argument"):
        _lib.call("sd_op_redim_stem", None, 1, 1, None, None, None, None, None, 0, None)
    with pytest.raises(ValueError, match="redim_dwconv1d: bad argument"):
        _lib.call("sd_op_redim_dwconv1d", None, 1, 1, 96, 7, None, None, None, None, None, 0, None)
    with pytest.raises(ValueError, match="astp_pool: bad argument"):
        _lib.call("sd_op_astp_pool_c", None, 0, 1, 2, 1152, None, None, None, None, None, None)


# ---- the wrapper's refusals come before it touches a device
def test_wrapper_refusals():
    with pytest.raises(ValueError, match="feat_dim 72 only"):
        ReDimNetB2(feat_dim=80)
    with pytest.raises(ValueError, match="ASTP pooling only"):
        ReDimNetB2(pooling_func="TSTP")
    with pytest.raises(ValueError, match="two_emb_layer=False only"):
        ReDimNetB2(two_emb_layer=True)
    with pytest.raises(ValueError, match="precision"):
        ReDimNetB2(precision="fp16")
    m = ReDimNetB2.__new__(ReDimNetB2)
    m.feat_dim = 72
    with pytest.raises(AssertionError, match="at least 2 fbank frames"):
        m.forward(torch.zeros(1, 1, 72))
    with pytest.raises(ValueError, match=r"expected \(B, T, 72\) fbank"):
        m.get_frame_level_feat(torch.zeros(1, 8, 80))


# ---- TS-VAD variant 4
def test_tsvad_config_resolves_to_variant_4():
    cfg = TSVADConfig(speech_encoder_type="ReDimNetB2")
    assert cfg.variant == 4 and cfg.n_mels == 72
    assert TSVADConfig().variant == 0 and TSVADConfig().n_mels == 80 and TSVADConfig.ots_vad_v1().variant == 1
    assert TSVADConfig(speech_encoder_type="resnet34_wespeaker").variant == 2
    assert TSVADConfig(speech_encoder_type="ecapa_channel_1024_wespeaker").variant == 3


@pytest.mark.parametrize("name", ["ReDimNetB2_layernorm", "ReDimNetB2_offical", "ReDimNetB0", "ReDimNetB3", "ReDimNetM"])
def test_other_redimnet_encoders_stay_unsupported(name):
    with pytest.raises(ValueError, match="unsupported TS-VAD configuration"):
        TSVADConfig(speech_encoder_type=name).variant


def test_rejected_combinations_raise_as_ecapas_do():
    """ots_vad_style v1 and the lstm / conformer back ends: the same error as with ECAPA, up to the encoder's name at
    the head of the message."""
    def message(enc, kw):
        with pytest.raises(ValueError) as e:
            TSVADConfig(speech_encoder_type=enc, **kw).variant
        return str(e.value).replace(f"configuration {enc}/", "configuration <enc>/")

    for kw in (dict(ots_vad_style="v1"), dict(multi_backend_type="lstm_ots_vad"),
               dict(single_backend_type="conformer_ots_vad")):
        assert message("ReDimNetB2", kw) == message("ecapa_channel_1024_wespeaker", kw)


def test_tsvad_layout_matches_reference_keys():
    g = gold("tsvad_redimnet_keys")
    ref = {str(n): tuple(int(d) for d in str(s).split(",") if d) for n, s in zip(g["names"], g["shapes"])}
    ours = {n: tuple(s) for n, s, _ in tsvad_layout(TSVADConfig(speech_encoder_type="ReDimNetB2"))}
    assert set(ours) == set(ref), (sorted(set(ours) - set(ref))[:5], sorted(set(ref) - set(ours))[:5])
    assert ours == ref
    assert ours["speech_down_or_up.0.weight"] == (192, 1152, 5) and "speech_encoder.seg_1.weight" in ours


@pytest.mark.parametrize("name", list(TSVAD_CASES))
def test_tsvad_restatement_matches_reference(name):
    (B, T, nl, _, wseed), x, ts = tsvad_inputs72(name)
    g = gold(name)
    cfg = TSVADConfig(speech_encoder_type="ReDimNetB2")
    sd = to_torch(tsvad_state_dict(cfg, seed=wseed))
    enc = rr.speech_encoder_out(sd, torch.from_numpy(x)).numpy()
    logits = rr.tsvad_forward(sd, cfg, torch.from_numpy(x), torch.from_numpy(ts), nl).numpy()
    e1, e2 = err(enc, g["speech_enc"]), err(logits, g["logits"])
    print(name, "speech_enc err", e1, "logits err", e2)
    assert e1 < ATOL and e2 < 1e-4


def test_tsvad_restatement_length_rule_and_nan_window():
    cfg = TSVADConfig(speech_encoder_type="ReDimNetB2")
    for base, nl in TSVAD_RAISES:
        (B, T, _, _, wseed), x, ts = tsvad_inputs72(base)
        with pytest.raises(AssertionError, match="label and ref_speech"):
            rr.tsvad_forward(to_torch(tsvad_state_dict(cfg, seed=wseed)), cfg, torch.from_numpy(x), torch.from_numpy(ts), nl)
    name = "tsvad_redimnet_nan"
    (B, T, nl, _, wseed), x, ts = tsvad_inputs72(name)
    g, bad = gold(name)["logits"], TSVAD_NAN[name][1]
    keep = [i for i in range(B) if i != bad]
    got = rr.tsvad_forward(to_torch(tsvad_state_dict(cfg, seed=wseed)), cfg, torch.from_numpy(x), torch.from_numpy(ts),
                           nl).numpy()
    assert np.isnan(got[bad]).all() and np.abs(got[keep] - g[keep]).max() < 1e-4
