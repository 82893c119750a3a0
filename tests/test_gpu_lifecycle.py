"""The handle lifecycle on the GPU, the same contract for every model kind of include/sdiar.h: create -> set_param*
-> finalize -> forward* -> destroy, with kErrState for a call out of order and strict loading.  Pinned through the raw
C API for the seven kinds and through every Python class that owns a handle; one forward per class is compared bit for
bit with the same forward on a handle this file builds with raw sd_<kind>_create / set_param / finalize calls.

Each case is its kind's smallest configuration of the suite (TS-VAD: the shortest golden geometry, 38 fbank frames ->
10 labels, batch 1; the others: the smallest shape of their own test_gpu_* file), fp32, seeded weights.

What differs between the classes today and is kept as it is:
  * eager classes (TSVADModel, TSVADStreamingModel, CAMPPlus, ResNet34, SSNDModel) create the handle in the
    constructor, refuse strict=False with "the MI355X backend only supports strict=True loading" and have device_bytes
    as a property; lazy ones (TransformerEdaModel, EendEdaModel, eend TransformerModel, OnlineTransformerDADiarization)
    create it in load_state_dict, refuse with "strict=False is not supported by the MI355X backend" and have
    device_bytes() as a method (0 before the load) -- except eend's TransformerModel, which has none;
  * SSNDModel maps device="cpu" to the current HIP device, every other class raises ValueError.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from make_golden import campp_inputs, eda_inputs, tsvad_inputs, tsvad_stream_inputs
from make_golden_resnet_emb import emb_inputs
from make_ssnd_golden import ssnd_cfg, ssnd_inputs
from speaker_diarization_amd import _lib, weights as W
from speaker_diarization_amd.eend.models import TransformerModel
from speaker_diarization_amd.eend_eda.models import EendEdaModel, TransformerEdaModel
from speaker_diarization_amd.fs_eend.model import OnlineTransformerDADiarization
from speaker_diarization_amd.ssnd.model import SSNDModel
from speaker_diarization_amd.ts_vad.embedding import CAMPPlus, ResNet34
from speaker_diarization_amd.ts_vad.model import TSVADModel
from speaker_diarization_amd.ts_vad.streaming import TSVADStreamingModel

pytestmark = pytest.mark.gpu

EAGER_STRICT = "the MI355X backend only supports strict=True loading"
LAZY_STRICT = "strict=False is not supported by the MI355X backend"
P3 = "precision must be bf16, fp32 or bf16x3, got int8"
P2 = "precision must be bf16 or fp32, got int8"


def _dev(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _empty(gpu, *shape):
    return torch.empty(*shape, device=gpu, dtype=torch.float32)


def _eda_feats(x, in_ld, gpu):
    """pad_sequence(-1) of one (T, 345) sequence into in_ld-wide rows, zero pad columns."""
    buf = torch.full((1, x.shape[0], in_ld), -1.0, device=gpu, dtype=torch.float32)
    buf[0, :, :345] = _dev(x, gpu)
    buf[:, :, 345:] = 0.0
    return buf


# ---------------------------------------------------------------------------------------------- TS-VAD (variant 2)
TSVAD_CFG = W.TSVADConfig(speech_encoder_type="resnet34_wespeaker")
TSVAD_B, TSVAD_T, TSVAD_NL = 1, 38, 10


def tsvad_conf():
    c = TSVAD_CFG
    return _lib.TsvadConfig(variant=c.variant, max_num_speaker=c.max_num_speaker, rs_len=c.rs_len, max_batch=TSVAD_B,
                            max_fbank_frames=398, precision=0, num_transformer_layer=c.num_transformer_layer,
                            num_attention_head=c.num_attention_head, transformer_embed_dim=c.transformer_embed_dim,
                            transformer_ffn_embed_dim=c.transformer_ffn_embed_dim,
                            speaker_embed_dim=c.speaker_embed_dim)


def tsvad_in(gpu):
    x, ts = tsvad_inputs(TSVAD_B, TSVAD_T, TSVAD_NL, seed=77)
    return _dev(x, gpu), _dev(ts, gpu)


def tsvad_raw(h, inp, gpu, call):
    x, ts = inp
    out = _empty(gpu, TSVAD_B, 4, TSVAD_NL)
    call("sd_tsvad_forward_batched", h, _lib.ptr(x), _lib.ptr(ts), TSVAD_B, TSVAD_T, TSVAD_NL, 0, 0, _lib.ptr(out),
         _lib.stream_ptr(gpu))
    return (out,)


# ---------------------------------------------------------------------------------------------- streaming TS-VAD
STREAM_TLAB, STREAM_CHUNK, STREAM_LEFT = 60, 10, 2      # tsvad_stream_c10_l2


def stream_conf():
    c = W.TSVADStreamingConfig()
    return _lib.TsvadStreamConfig(max_num_speaker=c.max_num_speaker, max_labels=64, precision=0,
                                  num_transformer_layer=c.num_transformer_layer,
                                  num_attention_head=c.num_attention_head,
                                  transformer_embed_dim=c.transformer_embed_dim,
                                  transformer_ffn_embed_dim=c.transformer_ffn_embed_dim,
                                  speaker_embed_dim=c.speaker_embed_dim, max_windows=1)


def stream_in(gpu):
    xs, ts = tsvad_stream_inputs(4 * STREAM_TLAB, 62)
    return _dev(xs, gpu), _dev(ts, gpu)


def stream_raw(h, inp, gpu, call):
    xs, ts = inp
    out = _empty(gpu, 1, 4, STREAM_TLAB)
    call("sd_tsvad_stream_forward", h, _lib.ptr(xs), _lib.ptr(ts), 1, STREAM_TLAB, STREAM_CHUNK, STREAM_LEFT,
         _lib.ptr(out), _lib.stream_ptr(gpu))
    return (out,)


# ---------------------------------------------------------------------------------------------- EEND-EDA / EEND
EDA_T = 99


def eda_conf(variant, n_att=15, n_speakers=0):
    return _lib.EdaConfig(variant=variant, in_size=345, n_units=256, n_heads=4, n_layers=2, dim_feedforward=2048,
                          max_seqs=1, max_frames=128, max_n_speakers=n_att, precision=0, n_speakers=n_speakers)


def eda_in(gpu):
    x = eda_inputs([EDA_T], seed=14)[0]
    perm = np.random.default_rng(5).permutation(EDA_T).astype(np.int32)
    return x, perm


def eda_raw(h, inp, gpu, call):
    x, perm = inp
    in_ld = _lib.load().sd_eda_input_stride(h) or 352      # 0 before finalize
    feats = _eda_feats(x, in_ld, gpu)
    lens = torch.tensor([EDA_T], dtype=torch.int32, device=gpu)
    perm_d = _dev(perm[None], gpu)
    probs, act = _empty(gpu, 1, 15), _empty(gpu, 1, EDA_T, 14)
    call("sd_eda_forward", h, _lib.ptr(feats), in_ld, 1, EDA_T, _lib.ptr(lens), None, _lib.ptr(perm_d),
         _lib.ptr(probs), _lib.ptr(act), _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return act, probs


def eda_cls(m, inp, gpu):
    x, perm = inp
    feats, ilens = m._pad_src([torch.from_numpy(x)])
    return m.forward_infer(feats, ilens, [torch.from_numpy(perm)], 15)


def eend_raw(h, inp, gpu, call):
    x, _ = inp
    in_ld = _lib.load().sd_eda_input_stride(h) or 352
    feats = _eda_feats(x, in_ld, gpu)
    out = _empty(gpu, 1, EDA_T, 2)
    call("sd_eda_forward", h, _lib.ptr(feats), in_ld, 1, EDA_T, None, None, None, None, _lib.ptr(out),
         _lib.stream_ptr(gpu))
    return (out,)


# ---------------------------------------------------------------------------------------------- FS-EEND
FSEEND_T = 97


def fseend_conf():
    c = W.FSEENDConfig()
    return _lib.FseendConfig(in_size=c.in_size, n_units=c.n_units, n_heads=c.n_heads, enc_n_layers=c.enc_n_layers,
                             enc_dim_feedforward=c.enc_dim_feedforward, dec_n_layers=c.dec_n_layers,
                             dec_dim_feedforward=c.dec_dim_feedforward, conv_delay=c.conv_delay,
                             mask_delay=c.mask_delay, has_mask=int(bool(c.has_mask)), max_seqs=1, max_frames=128,
                             max_nspks=6, precision=0)


def fseend_make(gpu, **kw):
    c = W.FSEENDConfig()
    return OnlineTransformerDADiarization(None, c.in_size, c.n_units, c.n_heads, c.enc_n_layers, c.dec_n_layers,
                                          c.dropout, c.has_mask, c.max_seqlen, c.dec_dim_feedforward,
                                          **dict(dict(device=gpu, max_seqs=1, max_frames=128, max_nspks=6), **kw))


def fseend_raw(h, inp, gpu, call):
    in_ld = _lib.load().sd_fseend_input_stride(h) or 352
    feats = _eda_feats(inp, in_ld, gpu)
    preds, emb, att = _empty(gpu, 1, FSEEND_T, 6), _empty(gpu, 1, FSEEND_T, 256), _empty(gpu, 1, FSEEND_T, 6, 256)
    lens = (ctypes.c_int * 1)(FSEEND_T)
    call("sd_fseend_test", h, _lib.ptr(feats), in_ld, 1, FSEEND_T, lens, 6, _lib.ptr(preds), _lib.ptr(emb),
         _lib.ptr(att), _lib.stream_ptr(gpu))
    return preds, emb, att


def fseend_cls(m, inp, gpu):
    out, emb, att = m.test([torch.from_numpy(inp)], [FSEEND_T], max_nspks=6)
    return out[0][None], emb[0][None], att[0][None]


# ---------------------------------------------------------------------------------------------- CAM++ / ResNet34
CAMPP_B, CAMPP_T = 2, 150


def campp_raw(h, inp, gpu, call):
    out = _empty(gpu, CAMPP_B, 192)
    call("sd_campp_forward", h, _lib.ptr(inp), CAMPP_B, CAMPP_T, _lib.ptr(out), None, _lib.stream_ptr(gpu))
    return (out,)


RES_T = 9      # case t9: T' = 2, the shortest finite case


def resnet_raw(h, inp, gpu, call):
    out = _empty(gpu, 1, 256)
    call("sd_resnet34_forward", h, _lib.ptr(inp), 1, RES_T, _lib.ptr(out), None, None, _lib.stream_ptr(gpu))
    return (out,)


# ---------------------------------------------------------------------------------------------- SSND (decoders)
SSND_B, SSND_T, SSND_N = 2, 200, 4


def ssnd_conf():
    c = ssnd_cfg(SSND_N)
    return _lib.SsndConfig(max_batch=SSND_B, max_fbank_frames=4 * c.vad_out_len, max_speakers=SSND_N,
                           feat_dim=c.feat_dim, emb_dim=c.emb_dim, q_det_aux_dim=c.q_det_aux_dim,
                           q_rep_aux_dim=c.q_rep_aux_dim, d_model=c.d_model, nhead=c.nhead, d_ff=c.d_ff,
                           num_layers=c.num_layers, vad_out_len=c.vad_out_len, pos_emb_dim=c.pos_emb_dim,
                           max_seq_len=c.max_seq_len, n_all_speakers=c.n_all_speakers,
                           conformer_kernel=c.conformer_kernel, precision=0)


def ssnd_make(gpu, **kw):
    return SSNDModel(None, max_speakers=SSND_N, vad_out_len=200, **dict(dict(device=gpu, max_batch=SSND_B), **kw))


def ssnd_raw(h, inp, gpu, call):
    enc, x, spk = inp
    vad, emb = _empty(gpu, SSND_B, SSND_N, SSND_T), _empty(gpu, SSND_B, SSND_N, 256)
    call("sd_ssnd_decode", h, _lib.ptr(enc), _lib.ptr(x), _lib.ptr(spk), SSND_B, SSND_T, _lib.ptr(vad), _lib.ptr(emb),
         _lib.stream_ptr(gpu))
    return vad, emb


def _eda_kw(gpu, **kw):
    return dict(dict(n_speakers=2, in_size=345, n_heads=4, n_units=256, n_layers=2, device=gpu, max_seqs=1,
                     max_frames=128), **kw)


@functools.lru_cache(maxsize=None)
def _state(name):
    return {
        "tsvad": lambda: W.tsvad_state_dict(TSVAD_CFG, seed=780),
        "tsvad_stream": lambda: W.tsvad_streaming_state_dict(W.TSVADStreamingConfig(), seed=812),
        "eda": lambda: W.eda_state_dict(W.EDAConfig(model_type="TransformerEda", n_layers=2), seed=784),
        "eend_eda": lambda: W.eda_state_dict(W.EDAConfig(model_type="EendEda", n_layers=2), seed=782),
        "eend": lambda: W.synthetic_state_dict(W.eend_layout(W.EDAConfig(n_speakers=2, n_layers=2)), 795),
        "fseend": lambda: W.fseend_state_dict(W.FSEENDConfig(), seed=792),
        "campp": lambda: W.campplus_state_dict(4, 192),
        "resnet34": lambda: W.resnet34_embed_state_dict(904, 256, False),
        "ssnd": lambda: W.ssnd_state_dict(ssnd_cfg(SSND_N), seed=901),
    }[name]()


# name: kind, raw config, inputs(gpu), raw forward, constructor(gpu, **kw), class forward -> tuple of tensors,
#       lazy, a key of the state_dict, precision text, what device="cpu" does (the ValueError's subject, or None)
CASES = {
    "tsvad": ("tsvad", tsvad_conf, tsvad_in, tsvad_raw,
              lambda gpu, **kw: TSVADModel(TSVAD_CFG, **dict(dict(device=gpu, precision="fp32", max_batch=TSVAD_B), **kw)),
              lambda m, inp, gpu: (m.forward(inp[0], inp[1], TSVAD_NL),), False, "fc.bias", P3, "TSVADModel"),
    "tsvad_stream": ("tsvad_stream", stream_conf, stream_in, stream_raw,
                     lambda gpu, **kw: TSVADStreamingModel(**dict(dict(device=gpu, precision="fp32", max_labels=64), **kw)),
                     lambda m, inp, gpu: (m.forward_chunk_by_chunk(inp[0], inp[1], STREAM_TLAB, STREAM_CHUNK,
                                                                    STREAM_LEFT),),
                     False, "fc.bias", P2, "TSVADStreamingModel"),
    "eda": ("eda", lambda: eda_conf(0), eda_in, eda_raw, lambda gpu, **kw: TransformerEdaModel(**_eda_kw(gpu, **kw)),
            eda_cls, True, "eda.linear.bias", P3, "EEND-EDA"),
    "eend_eda": ("eda", lambda: eda_conf(1), eda_in, eda_raw, lambda gpu, **kw: EendEdaModel(**_eda_kw(gpu, **kw)),
                 eda_cls, True, "eda.linear.bias", P3, "EEND-EDA"),
    "eend": ("eda", lambda: eda_conf(3, 2, 2), eda_in, eend_raw,
             lambda gpu, **kw: TransformerModel(**_eda_kw(gpu, **kw)),
             lambda m, inp, gpu: (torch.stack(m([torch.from_numpy(inp[0])], activation=torch.sigmoid)),),
             True, "decoder.bias", P3, "EEND"),
    "fseend": ("fseend", fseend_conf, lambda gpu: eda_inputs([FSEEND_T], seed=32)[0], fseend_raw, fseend_make,
               fseend_cls, True, "cnn.weight", P3, "FS-EEND"),
    "campp": ("campp", lambda: _lib.CamppConfig(feat_dim=80, embedding_size=192, max_batch=CAMPP_B, max_frames=200,
                                                precision=0),
              lambda gpu: _dev(campp_inputs(CAMPP_B, CAMPP_T, 8), gpu), campp_raw,
              lambda gpu, **kw: CAMPPlus(**dict(dict(device=gpu, precision="fp32", max_batch=CAMPP_B, max_frames=200),
                                                **kw)),
              lambda m, inp, gpu: (m(inp),), False, "xvector.dense.linear.weight", P2, "CAMPPlus"),
    "resnet34": ("resnet34", lambda: _lib.Resnet34Config(feat_dim=80, embed_dim=256, two_emb_layer=0, max_batch=1,
                                                         max_frames=16, precision=0),
                 lambda gpu: _dev(emb_inputs("t9"), gpu), resnet_raw,
                 lambda gpu, **kw: ResNet34(80, 256, two_emb_layer=False,
                                            **dict(dict(device=gpu, precision="fp32", max_batch=1, max_frames=16), **kw)),
                 lambda m, inp, gpu: (m(inp)[1],), False, "seg_1.bias", P2, "ResNet34"),
    "ssnd": ("ssnd", ssnd_conf,
             lambda gpu: tuple(_dev(a, gpu) for a in ssnd_inputs("decode", SSND_B, SSND_T, SSND_N, 31, ssnd_cfg(SSND_N))),
             ssnd_raw, ssnd_make, lambda m, inp, gpu: m.decode(*inp), False, "det_decoder.out_proj.bias", P2, None),
}
KINDS = ["tsvad", "tsvad_stream", "eda", "fseend", "campp", "resnet34", "ssnd"]      # one case per C-API kind
LAZY = [n for n, c in CASES.items() if c[6]]
# the device-level entry point of each lazy class (infer() / test() need in_ld, which only a load sets)
BEFORE_LOAD = {
    "eda": lambda m, gpu: m.forward_infer(torch.zeros(1, 8, 352, device=gpu), [8], [torch.arange(8)]),
    "eend_eda": lambda m, gpu: m.forward_infer(torch.zeros(1, 8, 352, device=gpu), [8], [torch.arange(8)]),
    "eend": lambda m, gpu: m([torch.zeros(8, 345)], activation=torch.sigmoid),
    "fseend": lambda m, gpu: m.test_device(torch.zeros(1, 8, 352, device=gpu), [8]),
}


def _set_params(kind, h, state, call=_lib.call):
    for k, v in state.items():
        a = np.ascontiguousarray(v, dtype=np.float32)
        shape = (ctypes.c_int64 * max(v.ndim, 1))(*v.shape)
        call(f"sd_{kind}_set_param", h, k.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, v.ndim)


def _raw_handle(name):
    kind, conf = CASES[name][:2]
    c = conf()
    h = ctypes.c_void_p()
    _lib.call(f"sd_{kind}_create", ctypes.byref(c), ctypes.byref(h))
    return kind, h


def _status_call(codes):
    lib = _lib.load()
    return lambda name, *args: codes.append(getattr(lib, name)(*args))


@pytest.mark.parametrize("name", KINDS)
def test_raw_lifecycle_order(gpu, name):
    lib = _lib.load()
    kind, h = _raw_handle(name)
    inputs, raw = CASES[name][2:4]
    inp = inputs(gpu)
    try:
        assert getattr(lib, f"sd_{kind}_device_bytes")(h) == 0
        codes = []
        raw(h, inp, gpu, _status_call(codes))                    # forward before finalize
        assert codes == [_lib.SD_ERR_STATE]
        with pytest.raises(_lib.SdiarError, match="model not finalized"):
            raw(h, inp, gpu, _lib.call)
        _set_params(kind, h, _state(name))
        _lib.call(f"sd_{kind}_finalize", h)
        assert getattr(lib, f"sd_{kind}_device_bytes")(h) > 0
        one = np.ones(1, np.float32)
        args = (h, b"late.weight", one.ctypes.data_as(ctypes.c_void_p), (ctypes.c_int64 * 1)(1), 1)
        assert getattr(lib, f"sd_{kind}_set_param")(*args) == _lib.SD_ERR_STATE
        with pytest.raises(_lib.SdiarError, match=f"^sd_{kind}_set_param: set_param after finalize$"):
            _lib.call(f"sd_{kind}_set_param", *args)
        assert getattr(lib, f"sd_{kind}_finalize")(h) == _lib.SD_ERR_STATE
        with pytest.raises(_lib.SdiarError, match=f"^sd_{kind}_finalize: finalize called twice$"):
            _lib.call(f"sd_{kind}_finalize", h)
    finally:
        assert getattr(lib, f"sd_{kind}_destroy")(h) == _lib.SD_OK


@pytest.mark.parametrize("name", KINDS)
def test_raw_strict_keys(gpu, name):
    lib = _lib.load()
    key = CASES[name][7]
    state = _state(name)
    assert key in state
    missing = {k: v for k, v in state.items() if k != key}
    extra = dict(state, **{"not.a.key": np.zeros(3, np.float32)})
    for bad, what, k in ((missing, "Missing key", key), (extra, "Unexpected key", "not.a.key")):
        kind, h = _raw_handle(name)
        try:
            _set_params(kind, h, bad)
            with pytest.raises(RuntimeError) as e:
                _lib.call(f"sd_{kind}_finalize", h)
            assert str(e.value).startswith("Error(s) in loading state_dict") and what in str(e.value) and k in str(e.value)
            assert not isinstance(e.value, _lib.SdiarError)
            assert getattr(lib, f"sd_{kind}_finalize")(h) == _lib.SD_ERR_PARAM      # a failed finalize does not latch
        finally:
            assert getattr(lib, f"sd_{kind}_destroy")(h) == _lib.SD_OK


@pytest.mark.parametrize("name", list(CASES))
def test_class_argument_errors(gpu, name):
    make, lazy, ptext, cpu_subject = CASES[name][4], CASES[name][6], CASES[name][8], CASES[name][9]
    with pytest.raises(ValueError) as e:
        make(gpu, precision="int8")
    assert str(e.value) == ptext
    if cpu_subject is None:
        assert make(gpu, device="cpu").device == torch.device("cuda", torch.cuda.current_device())
    else:
        with pytest.raises(ValueError) as e:
            make(gpu, device="cpu")
        assert str(e.value) == f"{cpu_subject} (MI355X backend) runs on a HIP device only"
    m = make(gpu)
    with pytest.raises(ValueError) as e:
        m.load_state_dict({}, strict=False)
    assert str(e.value) == (LAZY_STRICT if lazy else EAGER_STRICT)
    assert (m._h is None) == lazy        # eager: the constructor made the handle; it is a raw c_void_p
    assert lazy or isinstance(m._h, ctypes.c_void_p)


@pytest.mark.parametrize("name", list(CASES))
def test_class_forward_equals_raw_handle(gpu, name):
    lib = _lib.load()
    _, _, inputs, raw, make, fwd, lazy = CASES[name][:7]
    inp = inputs(gpu)
    kind, h = _raw_handle(name)
    try:
        _set_params(kind, h, _state(name))
        _lib.call(f"sd_{kind}_finalize", h)
        want = [t.clone() for t in raw(h, inp, gpu, _lib.call)]
        torch.cuda.synchronize()
        raw_bytes = getattr(lib, f"sd_{kind}_device_bytes")(h)
    finally:
        assert getattr(lib, f"sd_{kind}_destroy")(h) == _lib.SD_OK
    m = make(gpu)
    assert m.load_state_dict(W.to_torch(_state(name))) is m
    assert isinstance(m._h, ctypes.c_void_p)
    got = fwd(m, inp, gpu)
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(g.view(torch.int32), w.view(torch.int32))
    assert getattr(lib, f"sd_{kind}_device_bytes")(m._h) == raw_bytes > 0
    if name != "eend":       # eend's TransformerModel has no device_bytes
        assert callable(m.device_bytes) == lazy
        assert (m.device_bytes() if lazy else m.device_bytes) == raw_bytes


@pytest.mark.parametrize("name", LAZY)
def test_lazy_class_reload(gpu, name):
    lib = _lib.load()
    kind, _, inputs, _, make, fwd = CASES[name][:6]
    inp = inputs(gpu)
    m = make(gpu)
    if name != "eend":
        assert m.device_bytes() == 0
    with pytest.raises(RuntimeError, match="load_state_dict\\(\\) must be called before"):
        BEFORE_LOAD[name](m, gpu)
    sd = W.to_torch(_state(name))
    m.load_state_dict(sd)
    first, nbytes = m._h.value, getattr(lib, f"sd_{kind}_device_bytes")(m._h)
    a = [t.clone() for t in fwd(m, inp, gpu)]
    m.load_state_dict(sd)
    assert m._h.value is not None and m._h.value != first      # the new handle exists before the old one is destroyed
    assert getattr(lib, f"sd_{kind}_device_bytes")(m._h) == nbytes
    b = fwd(m, inp, gpu)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    bad = dict(sd)
    bad.pop(CASES[name][7])
    kept = m._h.value
    with pytest.raises(RuntimeError, match="^Error\\(s\\) in loading state_dict"):
        m.load_state_dict(bad)
    assert m._h.value == kept      # a failed reload keeps the loaded handle
