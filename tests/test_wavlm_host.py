"""WavLM feature extractor: the torch-functional restatement against the reference goldens, the key names and byte
stability of the seeded weights, the relative-position buckets and the folded positional-conv weight of the library
against the reference's, the new kind's lifecycle argument checks, the wrapper's refusals and the library's exports.
No GPU."""
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
from speaker_diarization_amd.ssl.wavlm import WavLM, WavLMConfig, check_config, num_frames  # noqa: E402
from speaker_diarization_amd.weights import TSVADConfig, to_torch, wavlm_state_dict  # noqa: E402
import wavlm_ref as wr  # noqa: E402
from make_golden_wavlm import BUCKET_SPAN, CASES, DIGEST_SEED, case_config, case_input, keep_frames, tag  # noqa: E402
from make_golden_redimnet import state_digest  # noqa: E402

GOLD = os.path.join(HERE, "golden")
KIND = "wavlm"
GOOD = dict(embed_dim=768, ffn_dim=3072, heads=12, encoder_layers=2, extractor_mode=0, layer_norm_first=0, max_batch=1,
            max_samples=16000, precision=0)


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def test_frame_counts():
    assert [num_frames(n) for n in (400, 719, 720, 16000, 35000, 64000, 96000)] == [1, 1, 2, 49, 109, 199, 299]
    assert [wr.frames(n) for n in (400, 719, 16000, 64000)] == [1, 1, 49, 199]
    lib = _lib.load()
    for n in (0, 9, 399, 400, 719, 720, 16000, 35000, 64000, 96000):
        assert lib.sd_wavlm_frames(n) == (num_frames(n) if n >= 400 else 0), n


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_reference(name):
    """wavlm_ref reproduces every golden within 1e-4 max(1, max |golden|)."""
    g = gold(f"wavlm_{name}")
    cfg = case_config(name)
    _, _, B, n, settings, _, wseed = CASES[name]
    sd = to_torch(wavlm_state_dict(cfg, wseed))
    wav = torch.from_numpy(case_input(name))
    frames = [int(f) for f in g["frames"]]
    assert int(g["T"]) == num_frames(n) and frames == keep_frames(int(g["T"]))
    with torch.no_grad():
        for ol in settings:
            out = wr.extract_features(sd, cfg, wav, output_layer=ol)
            got = {f"x_{tag(ol)}": out["x"], "features": out["features"]}
            got.update({f"layer_{i}": h for i, h in enumerate(out["layers"])})
            assert len(out["layers"]) == (0 if ol is None else ol + 1)
            for k, v in got.items():
                ref = g[k]
                e = float(np.abs(v[:, frames].numpy() - ref).max())
                bar = 1e-4 * max(1.0, float(np.abs(ref).max()))
                print(name, k, "err", e, "bar", bar)
                assert e <= bar, (name, k, e, bar)


def test_final_layer_norm_only_without_output_layer():
    """Large (pre-LN): extract_features(x) and extract_features(x, output_layer=L) differ with the same weights."""
    g = gold("wavlm_lg_t49")
    assert np.abs(g["x_none"] - g["x_2"]).max() > 1.0
    assert np.array_equal(g["x_2"], g["layer_2"])
    b = gold("wavlm_bp_t199")
    assert np.abs(b["x_none"] - b["x_2"]).max() > 0.1      # three layers against two


@pytest.mark.parametrize("geom,case", [("bp", "bp_t49"), ("lg", "lg_t49")])
def test_seeded_keys_shapes_and_digest(geom, case):
    g = gold("wavlm_keys")
    cfg = case_config(case)
    ref = {str(n): tuple(int(d) for d in str(s).split(",") if d) for n, s in zip(g[f"{geom}.names"], g[f"{geom}.shapes"])}
    sd = wavlm_state_dict(cfg, DIGEST_SEED)
    ours = {k: tuple(v.shape) for k, v in sd.items()}
    assert set(ours) == set(ref), (sorted(set(ours) - set(ref))[:5], sorted(set(ref) - set(ours))[:5])
    assert ours == ref
    assert int(g["digest_seed"]) == DIGEST_SEED
    assert state_digest(sd) == str(g[f"{geom}.digest"])
    assert state_digest(wavlm_state_dict(cfg, DIGEST_SEED + 1)) != str(g[f"{geom}.digest"])
    # the terms a default initialisation leaves inert are wide here (weights.wavlm_state_dict)
    a = "encoder.layers.0.self_attn."
    assert sd[a + "relative_attention_bias.weight"].std() > 1.0 and sd[a + "grep_linear.weight"].std() > 0.3
    assert np.abs(sd[a + "grep_a"] - 1.0).max() > 0.2 and sd[a + "q_proj.weight"].std() > 0.1


def test_buckets_equal_the_reference_row():
    """sd_probe_wavlm_buckets(3000) equals the reference's row exactly; distance 713 lies 3.7e-5 below a bucket edge,
    so the evaluation order of the logarithm is pinned here."""
    ref = gold("wavlm_keys")["buckets"]
    n = BUCKET_SPAN
    assert ref.shape == (2 * n - 1,)
    out = np.full(2 * n - 1, -1, dtype=np.int32)
    _lib.call("sd_probe_wavlm_buckets", n, out.ctypes.data_as(ctypes.c_void_p))
    assert np.array_equal(out, ref), np.nonzero(out != ref)[0][:10] - (n - 1)
    mid = n - 1
    assert out[mid] == 0 and out[mid + 1] == 161 and out[mid - 1] == 1 and out[mid + 79] == 239 and out[mid - 79] == 79
    assert out[mid + 713] == 160 + 155 and out[mid - 713] == 155        # 80 + int(75.99996)
    assert out[mid + 800] == 319 and out[mid + 2999] == 319 and out[0] == 159
    assert np.array_equal(wr.buckets(torch.arange(-(n - 1), n)).numpy().astype(np.int32), ref)
    with pytest.raises(ValueError, match="^sd_probe_wavlm_buckets: null argument$"):
        _lib.call("sd_probe_wavlm_buckets", 4, None)
    with pytest.raises(ValueError, match="n must be at least 1"):
        _lib.call("sd_probe_wavlm_buckets", 0, out.ctypes.data_as(ctypes.c_void_p))


@pytest.mark.parametrize("case", ["bp_t49", "lg_t49"])
def test_folded_pos_conv_weight(case):
    """The library's fold equals g v / |v| (the norm over output and input channels of each tap), and the restatement
    reads the same weight from both key spellings."""
    cfg = case_config(case)
    sd = to_torch(wavlm_state_dict(cfg, 5))
    p = "encoder.pos_conv.0."
    g, v = sd[p + "parametrizations.weight.original0"], sd[p + "parametrizations.weight.original1"]
    D = cfg.encoder_embed_dim
    assert tuple(g.shape) == (1, 1, 128) and tuple(v.shape) == (D, D // 16, 128)
    want = (g.double() * v.double() / v.double().pow(2).sum(dim=(0, 1), keepdim=True).sqrt()).float().numpy()
    out = np.zeros_like(want)
    _lib.call("sd_probe_wavlm_pos_weight", g.numpy().ctypes.data_as(ctypes.c_void_p),
              v.numpy().ctypes.data_as(ctypes.c_void_p), D, out.ctypes.data_as(ctypes.c_void_p))
    assert np.abs(out - want).max() <= 1e-7 * np.abs(want).max()
    assert np.abs(out - v.numpy()).max() > 1e-3          # the seeded gains are not |v|: a dropped fold shows
    old = {k: t for k, t in sd.items() if "parametrizations" not in k}
    old[p + "weight_g"], old[p + "weight_v"] = g, v
    assert torch.equal(wr.pos_conv_weight(sd), wr.pos_conv_weight(old))
    assert np.abs(wr.pos_conv_weight(sd).numpy() - want).max() <= 1e-6 * np.abs(want).max()
    with pytest.raises(ValueError, match="^sd_probe_wavlm_pos_weight: null argument$"):
        _lib.call("sd_probe_wavlm_pos_weight", None, None, D, None)
    with pytest.raises(ValueError, match="D must be 768 or 1024"):
        _lib.call("sd_probe_wavlm_pos_weight", g.numpy().ctypes.data_as(ctypes.c_void_p),
                  v.numpy().ctypes.data_as(ctypes.c_void_p), 512, out.ctypes.data_as(ctypes.c_void_p))


# ---- the lifecycle argument checks of tests/test_capi_lifecycle.py, for the new kind
def _create(conf, out):
    _lib.call(f"sd_{KIND}_create", None if conf is None else ctypes.byref(conf),
              None if out is None else ctypes.byref(out))


def test_kind_is_registered():
    assert _lib.KINDS[KIND] is _lib.WavlmConfig
    names = [f"sd_{KIND}_{f}" for f in ("create", "set_param", "finalize", "forward", "device_bytes", "destroy")]
    names += ["sd_probe_wavlm_buckets", "sd_probe_wavlm_pos_weight", "sd_op_wavlm_layer0", "sd_op_wavlm_conv",
              "sd_op_wavlm_pos_conv", "sd_op_wavlm_bias_table", "sd_op_wavlm_attention"]
    assert set(names) <= set(_lib.EXPORTED)
    lib = _lib.load()
    assert not [s for s in names if not hasattr(lib, s)]


def test_create_null_arguments():
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: null argument$"):
        _create(None, ctypes.c_void_p())
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: null argument$"):
        _create(_lib.WavlmConfig(**GOOD), None)


GEOMETRY = "WavLM (MI355X backend) builds (embed_dim, ffn_dim, heads) = (768, 3072, 12) or (1024, 4096, 16) only"
MODES = ("WavLM (MI355X backend) builds (extractor_mode, layer_norm_first) = (0 default, 0) or (1 layer_norm, 1) only")


@pytest.mark.parametrize("fields,msg", [
    (dict(precision=2), "precision must be 0 or 1"),          # bf16x3 is refused, as for ECAPA
    (dict(precision=-1), "precision must be 0 or 1"),
    (dict(embed_dim=512), GEOMETRY),
    (dict(ffn_dim=4096), GEOMETRY),
    (dict(heads=16), GEOMETRY),
    (dict(embed_dim=1024, ffn_dim=4096, heads=12), GEOMETRY),
    (dict(encoder_layers=0), "encoder_layers must be 1..24"),
    (dict(encoder_layers=25), "encoder_layers must be 1..24"),
    (dict(extractor_mode=1), MODES),
    (dict(layer_norm_first=1), MODES),
    (dict(extractor_mode=2, layer_norm_first=1), MODES),
    (dict(max_batch=0), "max_batch must be positive"),
    (dict(max_samples=399), "max_samples must be at least 400"),
    (dict(max_batch=4096, max_samples=960000), "max_batch * frames(max_samples) * ffn_dim must be below 2^31"),
])
def test_create_rejects_bad_fields(fields, msg):
    h = ctypes.c_void_p()
    with pytest.raises(ValueError) as e:
        _create(_lib.WavlmConfig(**dict(GOOD, **fields)), h)
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
        _lib.call(f"sd_{KIND}_forward", None, None, 1, 400, 0, None, None, None, None)
    assert getattr(lib, f"sd_{KIND}_destroy")(None) == _lib.SD_OK
    assert getattr(lib, f"sd_{KIND}_device_bytes")(None) == 0


def test_op_argument_checks_need_no_device():
    with pytest.raises(ValueError, match="wavlm_layer0: null argument"):
        _lib.call("sd_op_wavlm_layer0", None, 1, 400, None, None, None, 0, None, 0, None)
    with pytest.raises(ValueError, match="wavlm_conv: bad argument"):
        _lib.call("sd_op_wavlm_conv", None, 1, 4, None, 2, None, None, None, 0, None)
    with pytest.raises(ValueError, match="wavlm_pos_conv: null argument"):
        _lib.call("sd_op_wavlm_pos_conv", None, 1, 1, 768, None, None, None, 0, None)
    with pytest.raises(ValueError, match="wavlm_bias_table: bad argument"):
        _lib.call("sd_op_wavlm_bias_table", None, 1, 12, None, None)
    with pytest.raises(ValueError, match="wavlm_attention: null argument"):
        _lib.call("sd_op_wavlm_attention", None, None, 1, 1, 12, None, None, None, None, None, 0, None)


# ---- the wrapper's refusals come before it touches a device
@pytest.mark.parametrize("fields,field", [
    (dict(encoder_embed_dim=512), "encoder_embed_dim"),
    (dict(encoder_ffn_embed_dim=2048), "encoder_ffn_embed_dim"),
    (dict(encoder_attention_heads=8), "encoder_attention_heads"),
    (dict(encoder_layers=0), "encoder_layers"),
    (dict(encoder_layers=25), "encoder_layers"),
    (dict(conv_feature_layers="[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)]"), "conv_feature_layers"),
    (dict(conv_bias=True), "conv_bias"),
    (dict(conv_pos=64), "conv_pos"),
    (dict(conv_pos_groups=8), "conv_pos_groups"),
    (dict(relative_position_embedding=False), "relative_position_embedding"),
    (dict(gru_rel_pos=False), "gru_rel_pos"),
    (dict(num_buckets=160), "num_buckets"),
    (dict(max_distance=1280), "max_distance"),
    (dict(activation_fn="relu"), "activation_fn"),
    (dict(extractor_mode="layer_norm"), "extractor_mode"),
    (dict(layer_norm_first=True), "layer_norm_first"),
])
def test_wrapper_refuses_unsupported_configurations(fields, field):
    with pytest.raises(ValueError, match=field):
        WavLM(WavLMConfig(fields))


def test_wrapper_refusals():
    check_config(WavLMConfig())
    check_config(WavLMConfig.large())
    check_config(WavLMConfig.large(encoder_layers=6))
    check_config(WavLMConfig(dict(conv_feature_layers="[(512,10,5)]+[(512,3,2)]*4+[(512,2,2)]*2")))      # spaces aside
    check_config(WavLMConfig(dict(conv_feature_layers=[[512, 10, 5]] + [[512, 3, 2]] * 4 + [[512, 2, 2]] * 2)))
    with pytest.raises(ValueError, match="conv_feature_layers"):       # compared, never evaluated
        check_config(WavLMConfig(dict(conv_feature_layers="__import__('os').getcwd()")))
    with pytest.raises(ValueError, match="precision must be 0 or 1"):
        WavLM(WavLMConfig(), precision="bf16x3")
    with pytest.raises(ValueError, match="max_samples"):
        WavLM(WavLMConfig(), max_samples=399)
    with pytest.raises(ValueError, match="'cfg' and 'model'"):
        WavLM.from_checkpoint({"model": {}})
    m = WavLM.__new__(WavLM)
    m.cfg, m.max_batch, m.max_samples = WavLMConfig(dict(encoder_layers=2)), 2, 16000
    x = torch.zeros(2, 16000)
    with pytest.raises(ValueError, match="padding_mask"):
        m.extract_features(x, padding_mask=torch.zeros(2, 16000, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask=True"):
        m.extract_features(x, mask=True)
    with pytest.raises(ValueError, match="n_samples must be at least 400"):
        m.extract_features(torch.zeros(2, 399))
    with pytest.raises(ValueError, match="exceeds max_samples"):
        m.extract_features(torch.zeros(2, 16001))
    with pytest.raises(ValueError, match="exceeds max_batch"):
        m.extract_features(torch.zeros(3, 16000))
    with pytest.raises(ValueError, match="output_layer must be 1..2"):
        m.extract_features(x, output_layer=3)
    with pytest.raises(ValueError, match="output_layer must be 1..2"):
        m.extract_features(x, output_layer=0)
    with pytest.raises(ValueError, match="strict=True"):
        m.load_state_dict({}, strict=False)


@pytest.mark.parametrize("name", ["WavLM", "WavLM_weight_sum"])
def test_tsvad_wavlm_variants_stay_unsupported(name):
    with pytest.raises(ValueError, match="unsupported TS-VAD configuration"):
        TSVADConfig(speech_encoder_type=name).variant
