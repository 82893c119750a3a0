"""The handle lifecycle's argument checks, the same for every model kind of include/sdiar.h: what sd_<kind>_create,
set_param, finalize, device_bytes and destroy answer to NULL arguments and to a bad configuration.  Every check here
runs before the library's first HIP call, so none needs a device.  Plus the host conversion every wrapper's
load_state_dict hands to set_param."""
import ctypes

import numpy as np
import pytest
import torch

from speaker_diarization_amd import _lib

# kind: (config struct, a configuration create accepts, the field of one bad size with its value, the message)
KINDS = {
    "tsvad": (_lib.TsvadConfig,
              dict(variant=0, max_num_speaker=4, rs_len=4, max_batch=1, max_fbank_frames=398, precision=0,
                   num_transformer_layer=2, num_attention_head=4, transformer_embed_dim=384,
                   transformer_ffn_embed_dim=1536, speaker_embed_dim=192),
              ("max_batch", 0), "bad workspace sizes"),
    "tsvad_stream": (_lib.TsvadStreamConfig,
                     dict(max_num_speaker=4, max_labels=64, precision=0, num_transformer_layer=2,
                          num_attention_head=4, transformer_embed_dim=384, transformer_ffn_embed_dim=1536,
                          speaker_embed_dim=192, max_windows=1),
                     ("max_labels", 0), "bad workspace sizes"),
    "eda": (_lib.EdaConfig,
            dict(variant=0, in_size=345, n_units=256, n_heads=4, n_layers=2, dim_feedforward=2048, max_seqs=1,
                 max_frames=128, max_n_speakers=15, precision=0, n_speakers=2),
            ("max_n_speakers", 1), "bad workspace sizes"),
    "fseend": (_lib.FseendConfig,
               dict(in_size=345, n_units=256, n_heads=4, enc_n_layers=4, enc_dim_feedforward=2048, dec_n_layers=2,
                    dec_dim_feedforward=2048, conv_delay=9, mask_delay=0, has_mask=1, max_seqs=1, max_frames=128,
                    max_nspks=6, precision=0),
               ("max_nspks", 0), "bad workspace sizes"),
    "campp": (_lib.CamppConfig, dict(feat_dim=80, embedding_size=192, max_batch=1, max_frames=200, precision=0),
              ("max_frames", 7), "bad workspace sizes"),
    "resnet34": (_lib.Resnet34Config,
                 dict(feat_dim=80, embed_dim=256, two_emb_layer=0, max_batch=1, max_frames=200, precision=0),
                 ("embed_dim", 12), "embed_dim must be a positive multiple of 8"),
    "ssnd": (_lib.SsndConfig,
             dict(max_batch=1, max_fbank_frames=800, max_speakers=4, feat_dim=80, emb_dim=256, q_det_aux_dim=256,
                  q_rep_aux_dim=256, d_model=256, nhead=8, d_ff=512, num_layers=4, vad_out_len=200, pos_emb_dim=256,
                  max_seq_len=1000, n_all_speakers=1000, conformer_kernel=15, precision=0),
             ("max_fbank_frames", 7), "bad workspace sizes"),
}
# the precisions each kind takes: 2 (bf16x3) only where conv_gemm's exact path is wired through the handle
PRECISION_MSG = {k: "precision must be 0, 1 or 2" if k in ("tsvad", "eda", "fseend") else "precision must be 0 or 1"
                 for k in KINDS}


def _create(kind, conf, out):
    _lib.call(f"sd_{kind}_create", None if conf is None else ctypes.byref(conf),
              None if out is None else ctypes.byref(out))


@pytest.mark.parametrize("kind", list(KINDS))
def test_create_null_arguments(kind):
    struct, good, _, _ = KINDS[kind]
    with pytest.raises(ValueError, match=f"^sd_{kind}_create: null argument$"):
        _create(kind, None, ctypes.c_void_p())
    with pytest.raises(ValueError, match=f"^sd_{kind}_create: null argument$"):
        _create(kind, struct(**good), None)


@pytest.mark.parametrize("kind", list(KINDS))
def test_create_rejects_one_bad_field(kind):
    struct, good, (field, value), msg = KINDS[kind]
    h = ctypes.c_void_p()
    with pytest.raises(ValueError) as e:
        _create(kind, struct(**dict(good, precision=3)), h)
    assert str(e.value) == f"sd_{kind}_create: {PRECISION_MSG[kind]}"
    with pytest.raises(ValueError) as e:
        _create(kind, struct(**dict(good, **{field: value})), h)
    assert str(e.value) == f"sd_{kind}_create: {msg}"
    assert h.value is None      # a refused create writes no handle


@pytest.mark.parametrize("kind", list(KINDS))
def test_null_handle(kind):
    lib = _lib.load()
    data = (ctypes.c_float * 1)(1.0)
    shape = (ctypes.c_int64 * 1)(1)
    with pytest.raises(ValueError, match=f"^sd_{kind}_set_param: null argument$"):
        _lib.call(f"sd_{kind}_set_param", None, b"w", data, shape, 1)
    with pytest.raises(ValueError, match=f"^sd_{kind}_finalize: null handle$"):
        _lib.call(f"sd_{kind}_finalize", None)
    assert getattr(lib, f"sd_{kind}_destroy")(None) == _lib.SD_OK
    assert getattr(lib, f"sd_{kind}_device_bytes")(None) == 0


def test_fseend_stream_null_handle():
    lib = _lib.load()
    with pytest.raises(ValueError, match="^sd_fseend_stream_create: null argument$"):
        _lib.call("sd_fseend_stream_create", None, 1, 64, 6, 0, ctypes.byref(ctypes.c_void_p()))
    assert lib.sd_fseend_stream_destroy(None) == _lib.SD_OK
    assert lib.sd_fseend_stream_device_bytes(None) == 0


HOST_TENSORS = {
    "float32": lambda: torch.randn(3, 5, generator=torch.Generator().manual_seed(1)),
    "float64": lambda: torch.randn(4, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 1e3 + 1 / 3,
    "float16": lambda: torch.randn(2, 3, 4, generator=torch.Generator().manual_seed(3)).to(torch.float16),
    "int64": lambda: torch.tensor([0, -1, 7, 2 ** 24 + 1, 2 ** 40 + 12345, -(2 ** 53) - 1]),
    "float32_0d": lambda: torch.tensor(0.1),
    "float64_0d": lambda: torch.tensor(1 / 3, dtype=torch.float64),
    "float16_0d": lambda: torch.tensor(0.1, dtype=torch.float16),
    "int64_0d": lambda: torch.tensor(16777217),           # num_batches_tracked-like; not a float32 integer
    "float32_strided": lambda: torch.arange(24, dtype=torch.float32).reshape(4, 6).t(),
}


@pytest.mark.parametrize("name", list(HOST_TENSORS))
def test_host_state_matches_the_torch_conversion(name):
    v = HOST_TENSORS[name]()
    want = torch.as_tensor(np.asarray(v.cpu())).to(torch.float32).contiguous()
    got = _lib.host_state({"k": v})["k"]
    assert got.dtype == np.float32 and got.shape == tuple(want.shape)
    assert got.tobytes() == want.numpy().tobytes()      # tobytes() reads in C order whatever the strides
