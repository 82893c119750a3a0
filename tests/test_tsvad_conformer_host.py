"""TS-VAD conformer back ends (single_backend_type "conformer", multi_backend_type "transformer" / "conformer" behind
CAM++), host side: the configuration mapping, the state-dict layout and the CPU restatement
(tests/tsvad_conformer_ref.py) against the reference-run goldens tests/golden/tsvad_conf_*.npz.

The goldens were written by the reference TSVADModel with oracle.torchaudio_conformer.Conformer installed as
torchaudio.models.Conformer (torchaudio is absent): they pin the wiring around the conformer, the key set and the
BatchNorm form; the conformer arithmetic itself stays parity unpinned."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import tsvad_conformer_ref as cfr  # noqa: E402
from make_golden_tsvad_conformer import CASES, case_cfg, case_inputs  # noqa: E402
from speaker_diarization_amd.weights import TSVADConfig, to_torch, tsvad_layout, tsvad_state_dict  # noqa: E402

ORACLE_ATOL = 1e-5     # the project's oracle bar: restatement vs reference run
VISIBLE = 1e-3         # a perturbation the golden must see moves the logits by more than this

_cache = {}


def golden(name):
    if name not in _cache:
        with np.load(os.path.join(HERE, "golden", f"{name}.npz")) as z:
            _cache[name] = {k: z[k] for k in z.files}
    return _cache[name]


def state(name):
    return to_torch(tsvad_state_dict(case_cfg(name), seed=int(golden(name)["weight_seed"])))


def restate(name, sd=None, **kw):
    g = golden(name)
    return cfr.tsvad_forward(sd if sd is not None else state(name), case_cfg(name), torch.from_numpy(g["ref_speech"]),
                             torch.from_numpy(g["ts"]), int(g["n_label"]), **kw).numpy()


def test_variant_and_backend_mapping():
    c = TSVADConfig(single_backend_type="conformer")
    assert (c.variant, c.backend) == (0, 4)
    c = TSVADConfig(single_backend_type="conformer", multi_backend_type="conformer")
    assert (c.variant, c.backend) == (0, 5)
    # unchanged
    assert TSVADConfig().backend == 0 and TSVADConfig.ots_vad_v1().backend == 0
    assert TSVADConfig(single_backend_type="mamba2", d_state=128).backend == 1
    assert TSVADConfig(single_backend_type="mamba2", multi_backend_type="mamba2").backend == 2
    only_tfm = "transformer single and multi back ends only"
    unsupported = "unsupported TS-VAD configuration"
    from speaker_diarization_amd.ssl.wavlm import WavLMConfig
    refused = [
        (dict(multi_backend_type="conformer"), unsupported),                      # transformer + conformer: no recipe
        (dict(single_backend_type="conformer", ots_vad_style="v0"), unsupported),
        (dict(single_backend_type="conformer", multi_backend_type="mamba2"), unsupported),
        (dict(single_backend_type="mamba2", multi_backend_type="conformer"), unsupported),
        (dict(single_backend_type="conformer", speech_encoder_type="ReDimNetB2"), unsupported),
        (dict(single_backend_type="conformer", speech_encoder_type="resnet34_wespeaker"), unsupported),
        (dict(single_backend_type="conformer", multi_backend_type="conformer",
              speech_encoder_type="ecapa_channel_1024_wespeaker"), unsupported),
        (dict(single_backend_type="conformer", speech_encoder_type="hubert"), unsupported),
        (dict(single_backend_type="conformer", speech_encoder_type="whisper"), only_tfm),
        (dict(single_backend_type="conformer", multi_backend_type="conformer", speech_encoder_type="w2v-bert2"), only_tfm),
        (dict(single_backend_type="conformer", speech_encoder_type="WavLM", wavlm_cfg=WavLMConfig()), only_tfm),
        (dict(single_backend_type="conformer", speech_encoder_type="WavLM_weight_sum", wavlm_cfg=WavLMConfig(),
              wavlm_fuse_feat_post_norm=True), only_tfm),
    ]
    for kw, msg in refused:
        with pytest.raises(ValueError, match=msg):
            TSVADConfig(**kw).variant
        with pytest.raises(ValueError, match=msg):
            TSVADConfig(**kw).backend
    with pytest.raises(ValueError, match="ots_vad_style v1 is built for"):
        TSVADConfig(single_backend_type="conformer", ots_vad_style="v1").variant


@pytest.mark.parametrize("name", list(CASES))
def test_layout_matches_the_reference_keys(name):
    g = golden(name)
    want = dict(zip(g["names"].tolist(), g["shapes"].tolist()))
    got = {k: ",".join(str(d) for d in shape) for k, shape, _ in tsvad_layout(case_cfg(name))}
    assert list(got) == g["names"].tolist()       # the reference's own order too
    assert got == want
    bn = [k for k in got if ".conv_module.sequential.3." in k]
    n_stacks = 2 if CASES[name][0] == "conformer" else 1
    assert len(bn) == 5 * 2 * n_stacks            # weight, bias, running_mean, running_var, num_batches_tracked
    assert ("proj_layer.weight" in got) == (CASES[name][1] != 192)
    assert not any(k.startswith("single_backend.layers.") for k in got)


def test_seeded_batchnorm_statistics_are_not_the_identity():
    sd = state("tsvad_conf_c")
    for stack in ("single_backend", "multi_backend"):
        for i in range(2):
            p = f"{stack}.conformer_layers.{i}.conv_module.sequential.3."
            assert float((sd[p + "running_var"] - 1).abs().max()) > 0.2
            assert float(sd[p + "running_mean"].abs().max()) > 0.1
            assert float((sd[p + "weight"] - 1).abs().max()) > 0.1


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_vs_reference_golden(name):
    g = golden(name)
    x, ts = case_inputs(name)
    assert np.array_equal(x, g["ref_speech"]) and np.array_equal(ts, g["ts"])    # the inputs follow from the seed
    for fp64 in (False, True):
        err = float(np.abs(restate(name, fp64=fp64) - g["logits"]).max())
        print(f"{name} fp64={fp64}: max|restatement - golden| = {err:.3e}")
        assert err <= ORACLE_ATOL


@pytest.mark.parametrize("name", list(CASES))
def test_golden_sees_a_dropped_fold_and_a_wrong_head_count(name):
    g = golden(name)
    no_bn = float(np.abs(restate(name, sd=cfr.drop_bn_fold(state(name))) - g["logits"]).max())
    nh8 = float(np.abs(restate(name, nh=8) - g["logits"]).max())
    print(f"{name}: BatchNorm fold dropped moves the logits by {no_bn:.3e}, 8 heads instead of 4 by {nh8:.3e}")
    assert no_bn > VISIBLE and nh8 > VISIBLE
