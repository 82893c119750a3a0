"""The w2v-BERT 2.0 speech encoder, host side: the torch restatement (tests/w2vbert_ref.py) against the goldens of
transformers' Wav2Vec2BertModel at the fp32 bar, the state_dict layout against the module's stored key list, the
configuration check, and the C ABI: exported symbols, one create refusal per field, NULL arguments of every entry point
(all of which return before the library's first HIP call)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import w2vbert_ref as ref  # noqa: E402
from w2vbert_cases import TRUNK, keep_frames, trunk_config, trunk_input  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.ssl.w2vbert import W2vBert, W2vBertConfig, check_config  # noqa: E402
from speaker_diarization_amd.weights import to_torch, w2vbert_layout, w2vbert_state_dict  # noqa: E402

GOLD = os.path.join(HERE, "golden")
FP32_RTOL = 1e-3
KIND = "w2vbert"
GOOD = dict(hidden=1024, heads=16, ffn=4096, layers=6, conv_kernel=31, left=64, right=8, in_dim=160, precision=0,
            max_batch=1, max_frames=200, position_embeddings=0, add_adapter=0)
SYMBOLS = ["sd_w2vbert_create", "sd_w2vbert_set_param", "sd_w2vbert_finalize", "sd_w2vbert_forward",
           "sd_w2vbert_device_bytes", "sd_w2vbert_destroy", "sd_op_w2vbert_attention", "sd_op_w2vbert_conv_mix"]


def gold(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(TRUNK))
def test_restatement_vs_reference_golden(name):
    layers, B, T2, _, wseed, every = TRUNK[name]
    g = gold(name)
    frames = keep_frames(T2)
    assert list(g["frames"]) == frames
    hs = ref.trunk(to_torch(w2vbert_state_dict(trunk_config(layers), wseed)), layers, torch.from_numpy(trunk_input(name)))
    assert len(hs) == layers + 1
    pairs = [("x", hs[-1])] + ([(f"layer_{i}", h) for i, h in enumerate(hs)] if every else [])
    for key, h in pairs:
        want = g[key]
        err = float(np.abs(h[:, frames].numpy() - want).max())
        print(f"{name} {key}: max|diff| = {err:.3e}")
        assert err <= FP32_RTOL * max(1.0, float(np.abs(want).max())), (name, key, err)


def test_layout_matches_the_module_keys():
    keys = gold("tsvad_w2vbert_keys")
    want = [(n, tuple(int(d) for d in s.split(",") if d)) for n, s in zip(keys["trunk_l2.names"], keys["trunk_l2.shapes"])]
    lay = [(n, tuple(s)) for n, s, _ in w2vbert_layout(trunk_config(2))]
    assert lay == want                                   # names, shapes and the module's registration order
    assert lay[0] == ("masked_spec_embed", (1024,))
    sd = w2vbert_state_dict(trunk_config(2), 5)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    # a deeper model's first layers are the shallower one's: the golden generator's "one layer more" relies on it
    sd3 = w2vbert_state_dict(trunk_config(3), 5)
    assert all(np.array_equal(sd3[k], v) for k, v in sd.items())


def test_seeded_distance_term_is_comparable_to_q_dot_k():
    """The seeds make q . E as large as q . k, so the goldens are sensitive to the distance embedding."""
    sd = to_torch(w2vbert_state_dict(trunk_config(1), 7))
    y = torch.from_numpy(np.random.default_rng(1).standard_normal((1, 40, 1024)).astype(np.float32))
    a = "encoder.layers.0.self_attn."
    q, k = (torch.nn.functional.linear(y, sd[a + n + ".weight"], sd[a + n + ".bias"]).view(1, 40, 16, 64).transpose(1, 2)
            for n in ("linear_q", "linear_k"))
    qk = (q @ k.transpose(-1, -2) / 8).std()
    qe = (q @ sd[a + "distance_embedding.weight"].t() / 8).std()
    assert 1.5 <= float(qk) <= 3.5 and 0.5 <= float(qe / qk) <= 2.0, (float(qk), float(qe))


def test_distance_index_clamps():
    idx = ref.distance_index(80)
    assert idx[0, 0] == 64 and idx[0, 8] == 72 and idx[0, 9] == 72 and idx[0, 79] == 72     # right clamp at +8
    assert idx[64, 0] == 0 and idx[65, 0] == 0 and idx[63, 0] == 1 and idx[79, 0] == 0     # left clamp at -64
    assert idx.min() == 0 and idx.max() == 72


def test_check_config_names_the_field():
    check_config(W2vBertConfig())
    assert W2vBertConfig().num_hidden_layers == 24
    for field, bad in (("hidden_size", 768), ("num_attention_heads", 8), ("intermediate_size", 2048),
                       ("feature_projection_input_dim", 80), ("hidden_act", "gelu"),
                       ("position_embeddings_type", "relative"), ("left_max_position_embeddings", 8),
                       ("right_max_position_embeddings", 64), ("conv_depthwise_kernel_size", 15),
                       ("add_adapter", True), ("use_intermediate_ffn_before_adapter", True),
                       ("output_hidden_size", 768), ("layer_norm_eps", 1e-6)):
        with pytest.raises(ValueError, match=field):
            check_config(W2vBertConfig(**{field: bad}))
    for bad in (0, 25, 2.0):
        with pytest.raises(ValueError, match="num_hidden_layers must be 1..24"):
            check_config(W2vBertConfig(num_hidden_layers=bad))
    with pytest.raises(ValueError, match="precision"):
        W2vBert(W2vBertConfig(), precision="bf16x3")


def test_abi_symbols_exported():
    lib = _lib.load()
    assert _lib.KINDS[KIND] is _lib.W2vbertConfig
    assert [n for n, _ in _lib.W2vbertConfig._fields_][:11] == [
        "hidden", "heads", "ffn", "layers", "conv_kernel", "left", "right", "in_dim", "precision", "max_batch",
        "max_frames"]
    for s in SYMBOLS:
        assert s in _lib.EXPORTED and hasattr(lib, s), s


def _create(conf, out):
    _lib.call(f"sd_{KIND}_create", None if conf is None else ctypes.byref(conf), None if out is None else ctypes.byref(out))


@pytest.mark.parametrize("field,value,msg", [
    ("hidden", 768, "hidden 1024"), ("heads", 8, "heads 16"), ("ffn", 3072, "ffn 4096"), ("layers", 0, "layers must be 1..24"),
    ("layers", 25, "layers must be 1..24"), ("conv_kernel", 15, "conv_kernel 31"), ("left", 8, "left 64"),
    ("right", 64, "right 8"), ("in_dim", 80, "in_dim 160"), ("precision", 2, "precision must be 0 or 1"),
    ("max_batch", 0, "max_batch must be positive"), ("max_frames", 0, "max_frames must be positive"),
    ("max_batch", 4096, r"max_batch \* max_frames \* ffn must be below 2\^31"),
    ("position_embeddings", 1, "position_embeddings 0"), ("add_adapter", 1, "add_adapter 0")])
def test_create_refuses_one_bad_field(field, value, msg):
    h = ctypes.c_void_p()
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: .*{msg}"):
        _create(_lib.W2vbertConfig(**dict(GOOD, **{field: value})), h)
    assert h.value is None      # a refused create writes no handle


def test_null_arguments_of_every_entry_point():
    lib = _lib.load()
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: null argument$"):
        _create(None, ctypes.c_void_p())
    with pytest.raises(ValueError, match=f"^sd_{KIND}_create: null argument$"):
        _create(_lib.W2vbertConfig(**GOOD), None)
    data, shape = (ctypes.c_float * 1)(1.0), (ctypes.c_int64 * 1)(1)
    with pytest.raises(ValueError, match=f"^sd_{KIND}_set_param: null argument$"):
        _lib.call(f"sd_{KIND}_set_param", None, b"w", data, shape, 1)
    with pytest.raises(ValueError, match=f"^sd_{KIND}_finalize: null handle$"):
        _lib.call(f"sd_{KIND}_finalize", None)
    with pytest.raises(ValueError, match=f"^sd_{KIND}_forward: null argument$"):
        _lib.call(f"sd_{KIND}_forward", None, None, 1, 1, None, None, None)
    assert getattr(lib, f"sd_{KIND}_destroy")(None) == _lib.SD_OK
    assert getattr(lib, f"sd_{KIND}_device_bytes")(None) == 0
    with pytest.raises(ValueError, match="^sd_op_w2vbert_attention: w2vbert_attention: null argument$"):
        _lib.call("sd_op_w2vbert_attention", None, 1, 1, 16, None, None, 0, None)
    with pytest.raises(ValueError, match="^sd_op_w2vbert_conv_mix: w2vbert_conv_mix: null argument$"):
        _lib.call("sd_op_w2vbert_conv_mix", None, 1, 1, None, None, None, None, 0, None)
