"""TS-VAD speech encoder "CAM++_frame_level_gsp_fc" (egs/magicdata-ramc/ts_vad2/model.py:543-563, 1275-1287), host side:
the configuration mapping, the state-dict layout against the reference's stored key lists, the CPU restatement
(tests/gsp_ref.py, swapped into the existing whole-model restatements) against the reference-run goldens
tests/golden/tsvad_gsp*.npz, the fold of gsp_fc into the conv in float64, and the C ABI without a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import gsp_ref  # noqa: E402
import resnet_emb_ref  # noqa: E402
from make_golden_tsvad_gsp import CASES, ENCODER, case_cfg, case_inputs  # noqa: E402
from oracle import tsvad_ref  # noqa: E402
from speaker_diarization_amd import _lib  # noqa: E402
from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_layout, tsvad_state_dict  # noqa: E402

_cache = {}


def golden(name):
    if name not in _cache:
        with np.load(os.path.join(HERE, "golden", f"{name}.npz")) as z:
            _cache[name] = {k: z[k] for k in z.files}
    return _cache[name]


def state(name):
    return to_torch(tsvad_state_dict(case_cfg(name), seed=int(golden(name)["weight_seed"])))


def test_variant_and_backend_mapping():
    pairs = {("transformer", "transformer"): 0, ("mamba2", "transformer"): 1, ("mamba2", "mamba2"): 2,
             ("conformer", "transformer"): 4, ("conformer", "conformer"): 5}
    for (single, multi), backend in pairs.items():
        c = TSVADConfig(speech_encoder_type=ENCODER, single_backend_type=single, multi_backend_type=multi)
        assert (c.variant, c.backend, c.frame_level_gsp) == (0, backend, True)
        plain = TSVADConfig(single_backend_type=single, multi_backend_type=multi)
        assert (plain.variant, plain.backend, plain.frame_level_gsp) == (0, backend, False)   # CAM++ is unchanged
    assert c.mamba2_backend is False and TSVADConfig(speech_encoder_type=ENCODER,
                                                     single_backend_type="mamba2").mamba2_backend is True
    assert TSVADConfig.ots_vad_v1().frame_level_gsp is False
    unsupported = "unsupported TS-VAD configuration"
    for kw in (dict(ots_vad_style="v0"), dict(multi_backend_type="conformer"),
               dict(single_backend_type="conformer", multi_backend_type="mamba2"),
               dict(single_backend_type="mamba2_unidirectional")):
        for prop in ("variant", "backend", "frame_level_gsp"):
            with pytest.raises(ValueError, match=unsupported):
                getattr(TSVADConfig(speech_encoder_type=ENCODER, **kw), prop)
    with pytest.raises(ValueError, match="ots_vad_style v1 is built for"):
        TSVADConfig(speech_encoder_type=ENCODER, ots_vad_style="v1").variant
    with pytest.raises(ValueError, match=unsupported + ".*CAM\\+\\+_frame_level_gsp_fc with the same five"):
        TSVADConfig(speech_encoder_type="hubert").variant


@pytest.mark.parametrize("name", list(CASES))
def test_layout_matches_the_reference_keys(name):
    g = golden(name)
    want = dict(zip(g["names"].tolist(), g["shapes"].tolist()))
    got = {k: ",".join(str(d) for d in shape) for k, shape, _ in tsvad_layout(case_cfg(name))}
    assert got == want
    assert list(got) == g["names"].tolist()       # the reference's own order too
    se = CASES[name][0]
    assert len(got) == (1004 if se == 192 else 1006)
    assert got["gsp_fc.weight"] == "256,2" and got["gsp_fc.bias"] == "256"
    assert got["speech_down_or_up.0.weight"] == f"{se},256,5"
    assert ("proj_layer.weight" in got) == (se != 192)
    sd = tsvad_state_dict(case_cfg(name), seed=int(g["weight_seed"]))
    assert {k: ",".join(str(d) for d in v.shape) for k, v in sd.items()} == want
    # the CAM++ layout keeps its 512-channel conv and has no gsp_fc
    plain = {k: shape for k, shape, _ in tsvad_layout(TSVADConfig(speaker_embed_dim=se))}
    assert plain["speech_down_or_up.0.weight"] == (se, 512, 5) and "gsp_fc.weight" not in plain


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_vs_reference_golden(name):
    """The bounds tests/test_oracle.py applies to variant 0 against its golden: logits atol 2e-5 / rtol 1e-5, the
    speech encoder's output atol 1e-5 / rtol 1e-5."""
    g = golden(name)
    x, ts = case_inputs(name)
    assert np.array_equal(x, g["ref_speech"]) and np.array_equal(ts, g["ts"])    # the inputs follow from the seed
    sd, cfg = state(name), case_cfg(name)
    stage = gsp_ref.speech_encoder_out(sd, torch.from_numpy(x)).numpy()
    print(f"{name}: max|stage - golden| = {float(np.abs(stage - g['speech_down_or_up']).max()):.3e}")
    np.testing.assert_allclose(stage, g["speech_down_or_up"], atol=1e-5, rtol=1e-5)
    # oracle.tsvad_ref.tsvad_forward has no proj_layer; tests/resnet_emb_ref.py restates the same forward with it
    fwd = tsvad_ref.tsvad_forward if CASES[name][0] == 192 else resnet_emb_ref.tsvad_forward
    with gsp_ref.swapped():
        out = fwd(sd, cfg, torch.from_numpy(x), torch.from_numpy(ts), int(g["n_label"])).numpy()
    print(f"{name}: max|logits - golden| = {float(np.abs(out - g['logits']).max()):.3e}")
    np.testing.assert_allclose(out, g["logits"], atol=2e-5, rtol=1e-5)
    # the swap is what made it match: the CAM++ encoder cannot even read this state dict's (SE, 256, 5) conv
    with pytest.raises(RuntimeError):
        fwd(sd, cfg, torch.from_numpy(x), torch.from_numpy(ts), int(g["n_label"]))


def test_golden_sees_the_padding_rule():
    """A stage that adds every tap's C term unconditionally (the trap: the reference zero-pads gsp_fc's OUTPUT) is
    wrong at the first and last output frames only, and the golden stage output sees it."""
    name = "tsvad_gsp"
    g, sd = golden(name), state(name)
    x = tsvad_ref.campplus_time_out(sd, torch.from_numpy(g["ref_speech"])).permute(0, 2, 1).double().numpy()
    mean, std = x.mean(-1), x.std(-1, ddof=1)
    gw, gb, w, cb = (sd[k].numpy() for k in ("gsp_fc.weight", "gsp_fc.bias", "speech_down_or_up.0.weight",
                                             "speech_down_or_up.0.bias"))
    A, S, C = gsp_ref.fold_f64(gw, gb, w)
    right = gsp_ref.folded_f64(mean, std, A, S, C, cb)
    T2 = mean.shape[1]
    pad = lambda a: np.pad(a, ((0, 0), (2, 2)))  # noqa: E731
    # zero statistics in the padding, but its C terms stay
    wrong = np.stack([sum(pad(mean)[:, 2 * j + k, None] * A[:, k] + pad(std)[:, 2 * j + k, None] * S[:, k] + C[:, k]
                          for k in range(5)) + cb for j in range((T2 - 1) // 2 + 1)], 1)
    diff = np.abs(wrong - right).max(axis=(0, 2))
    assert diff[0] > 1e-3 and diff[-1] > 1e-3 and diff[1:-1].max() < 1e-12

    def finish(y):   # speech_down_or_up.1 + ReLU in eval, (B, T3, SE) -> (B, SE, T3)
        return torch.relu(tsvad_ref._bn(torch.from_numpy(y).float().permute(0, 2, 1), sd, "speech_down_or_up.1.bn")).numpy()
    assert np.abs(finish(right) - g["speech_down_or_up"]).max() < 1e-5
    assert np.abs(finish(wrong) - g["speech_down_or_up"]).max() > 1e-3


@pytest.mark.parametrize("T2", [1, 2, 5, 19, 20])
def test_fold_equals_the_unfolded_form_in_float64(T2):
    """A / S / C as the runtime folds them against Linear + zero-padded conv, both float64: each output sums about
    5 * 256 = 1300 products of O(1) terms, so the two orders differ by ~1300 * 2^-53 * O(1) ~ 1e-13; 1e-9 is four
    orders above that and nine below the O(1) outputs."""
    rng = np.random.default_rng(6000 + T2)
    SE, B = 192, 2
    mean, std = rng.uniform(0.2, 1.0, (B, T2)), rng.uniform(0.1, 1.0, (B, T2))
    gw, gb = rng.standard_normal((256, 2)), rng.standard_normal(256)
    w, cb = rng.standard_normal((SE, 256, 5)) / np.sqrt(1280), rng.standard_normal(SE)
    want = gsp_ref.unfolded_f64(mean, std, gw, gb, w, cb)
    A, S, C = gsp_ref.fold_f64(gw, gb, w)
    assert A.shape == S.shape == C.shape == (SE, 5)
    got = gsp_ref.folded_f64(mean, std, A, S, C, cb)
    assert got.shape == want.shape == (B, (T2 - 1) // 2 + 1, SE)
    err = float(np.abs(got - want).max())
    print(f"T2 {T2}: max|folded - unfolded| = {err:.3e} at |y| max {float(np.abs(want).max()):.2f}")
    assert err <= 1e-9
    # the unfolded form agrees with torch's conv1d over F.linear
    t = torch.from_numpy
    ref = torch.nn.functional.conv1d(
        torch.nn.functional.linear(torch.stack([t(mean), t(std)], -1), t(gw), t(gb)).permute(0, 2, 1), t(w), t(cb),
        stride=2, padding=2).permute(0, 2, 1).numpy()
    assert np.abs(ref - want).max() <= 1e-9


GOOD = dict(variant=0, max_num_speaker=4, rs_len=4, max_batch=1, max_fbank_frames=398, precision=0,
            num_transformer_layer=2, num_attention_head=4, transformer_embed_dim=384, transformer_ffn_embed_dim=1536,
            speaker_embed_dim=192)


def create_ex(**kw):
    """sd_tsvad_create_ex on GOOD + kw.  A configuration the library accepts then allocates the handle's pinned flags
    on the device: without one that step (and only that one) fails, with SD_ERR_HIP -> SdiarError; with one the handle
    is destroyed again.  A refused configuration is SD_ERR_INVALID -> ValueError before anything is allocated."""
    h = ctypes.c_void_p()
    try:
        _lib.call("sd_tsvad_create_ex", ctypes.byref(_lib.TsvadConfigEx(**dict(GOOD, **kw))), ctypes.byref(h))
    except _lib.SdiarError as e:
        assert not torch.cuda.is_available() and "frame_level_gsp" not in str(e), e
        assert h.value is None
        return
    assert h.value is not None
    _lib.call("sd_tsvad_destroy", h)


def test_abi_without_a_device():
    assert {"sd_tsvad_create_ex", "sd_op_gsp_down", "sd_gsp_down_frame_tile"} <= set(_lib.EXPORTED)
    lib = _lib.load()
    for n in ("sd_tsvad_create_ex", "sd_op_gsp_down", "sd_gsp_down_frame_tile"):
        assert hasattr(lib, n)
    # sd_tsvad_config_ex = sd_tsvad_config + the new field, last
    assert ctypes.sizeof(_lib.TsvadConfigEx) == ctypes.sizeof(_lib.TsvadConfig) + ctypes.sizeof(ctypes.c_int)
    assert _lib.TsvadConfigEx.frame_level_gsp.offset == ctypes.sizeof(_lib.TsvadConfig)
    assert _lib.TsvadConfigEx._fields_[-1][0] == "frame_level_gsp"
    create_ex(frame_level_gsp=1)                                       # back end 0
    create_ex(frame_level_gsp=1, backend=1, d_state=128, expand=4)     # back end 1
    h = ctypes.c_void_p()
    for kw, msg in ((dict(variant=2), "frame_level_gsp"), (dict(variant=1), "frame_level_gsp"),
                    (dict(frame_level_gsp=2), "frame_level_gsp"), (dict(speaker_embed_dim=200), "multiple of 32"),
                    (dict(backend=3), "backend must be")):
        with pytest.raises(ValueError, match=msg):
            _lib.call("sd_tsvad_create_ex", ctypes.byref(_lib.TsvadConfigEx(**{**GOOD, "frame_level_gsp": 1, **kw})),
                      ctypes.byref(h))
        assert h.value is None
    assert lib.sd_tsvad_create_ex(None, ctypes.byref(h)) == _lib.SD_ERR_INVALID
    assert lib.sd_gsp_down_frame_tile() == 32
