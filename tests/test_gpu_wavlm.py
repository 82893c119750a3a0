"""WavLM.extract_features on the HIP path (sd_wavlm_*) against the reference goldens
(tests/golden/make_golden_wavlm.py): Base+ and Large, fp32 and bf16, every output the reference returns.

Tolerances.  fp32: the project's fp32 bar, max |got - golden| <= 1e-3 max(1, max |golden|), for x, the projected conv
features and every layer_results entry.  bf16: nobody had measured this trunk, so the maxima of one run per case and the
smallest per-frame cosine are recorded in BF16_MEASURED and every case of a geometry is bounded at twice the largest of
them (the convention of tests/test_gpu_redimnet_emb.py).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from speaker_diarization_amd.ssl.wavlm import WavLM, num_frames  # noqa: E402
from speaker_diarization_amd.weights import to_torch, wavlm_state_dict  # noqa: E402
from make_golden_wavlm import CASES, case_config, case_input, tag  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_RTOL = 1e-3
# bf16 against the fp32 goldens, one run on an MI355X: per case the largest max |diff| over x, the features and the
# layer entries, and the smallest cosine of a stored frame of any of them.  Base+ outputs (post-LN) reach |x| 4.1 .. 4.7,
# Large ones (pre-LN, an unnormalised residual stream) 13 .. 16.
# The seeded weights make the attention sharp on purpose (q / k projections 6x the usual scale, scores of standard
# deviation ~11: weights.wavlm_state_dict), so the 2^-9 rounding of q and k moves a score by a few 1e-2 and a softmax
# weight by percents: these figures are the trunk's sensitivity at those weights, not the kernels' error, which
# tests/test_gpu_wavlm_ops.py bounds per op.  Cosines per case: bp_t1 0.999943, bp_t2 0.999474, bp_t49 0.999295,
# bp_t109 0.996637, bp_t199 0.997541, lg_t49 0.997515, lg_t1 0.999936.
BF16_MEASURED = {
    "bp": {"max_diff": {"bp_t1": 3.558e-2, "bp_t2": 1.081e-1, "bp_t49": 1.791e-1, "bp_t109": 2.854e-1,
                        "bp_t199": 2.648e-1},
           "min_cosine": 0.996637},
    "lg": {"max_diff": {"lg_t49": 9.178e-1, "lg_t1": 1.335e-1}, "min_cosine": 0.997515},
}
_models = {}


def gold(name):
    with np.load(os.path.join(GOLD, f"wavlm_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def model(name, precision, gpu, max_batch=None, max_samples=None):
    _, _, B, n, _, _, wseed = CASES[name]
    key = (name, precision, max_batch, max_samples)
    if key not in _models:
        _models.clear()          # one model's workspace at a time
        cfg = case_config(name)
        m = WavLM(cfg, device=gpu, precision=precision, max_batch=max_batch or B, max_samples=max_samples or n)
        m.load_state_dict(to_torch(wavlm_state_dict(cfg, wseed)))
        _models[key] = m.eval()
    return _models[key]


def outputs(m, name, gpu):
    """{golden key: array at the stored frames} of one case, through the wrapper's reference-shaped returns."""
    g = gold(name)
    frames = [int(f) for f in g["frames"]]
    wav = torch.from_numpy(case_input(name)).to(gpu)
    B, T, D = wav.shape[0], int(g["T"]), m.embed_dim
    out = {}
    for ol in CASES[name][4]:
        (x, results), pm = m.extract_features(wav, output_layer=ol, ret_layer_results=True)
        assert pm is None and tuple(x.shape) == (B, T, D)
        out[f"x_{tag(ol)}"] = x[:, frames].cpu().numpy()
        assert len(results) == (0 if ol is None else ol + 1)
        for i, (h, z) in enumerate(results):
            assert z is None and tuple(h.shape) == (T, B, D)
            out[f"layer_{i}"] = h.transpose(0, 1)[:, frames].cpu().numpy()
    feats, pm = m.extract_features(wav, ret_conv=True)
    assert pm is None and tuple(feats.shape) == (B, T, D)
    out["features"] = feats[:, frames].cpu().numpy()
    assert set(out) == {k for k in g if k.startswith(("x_", "layer_", "features"))}
    return out, g


def cosine(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_matches_reference(gpu, name):
    got, g = outputs(model(name, "fp32", gpu), name, gpu)
    for k, v in got.items():
        e, bar = float(np.abs(v - g[k]).max()), FP32_RTOL * max(1.0, float(np.abs(g[k]).max()))
        print(f"{name} fp32 {k}: max|diff| {e:.3e}  bar {bar:.3e}")
        assert np.isfinite(v).all() and e <= bar, (name, k, e, bar)


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_matches_reference(gpu, name):
    got, g = outputs(model(name, "bf16", gpu), name, gpu)
    e = max(float(np.abs(v - g[k]).max()) for k, v in got.items())
    cos = min(float(cosine(v, g[k]).min()) for k, v in got.items())
    peak = max(float(np.abs(g[k]).max()) for k in got)
    print(f"{name} bf16: max|diff| {e:.3e}  min cosine {cos:.6f}  (max|golden| {peak:.2f})")
    assert all(np.isfinite(v).all() for v in got.values())
    table = BF16_MEASURED[name[:2]]
    assert e <= 2 * max(table["max_diff"].values())
    assert 1.0 - cos <= 2 * (1.0 - table["min_cosine"])


def test_old_weight_norm_keys_load_to_the_same_model(gpu):
    """weight_g / weight_v instead of parametrizations.weight.original0 / original1."""
    name = "bp_t49"
    cfg = case_config(name)
    sd = to_torch(wavlm_state_dict(cfg, CASES[name][6]))
    p = "encoder.pos_conv.0."
    old = {k: v for k, v in sd.items() if "parametrizations" not in k}
    old[p + "weight_g"] = sd[p + "parametrizations.weight.original0"]
    old[p + "weight_v"] = sd[p + "parametrizations.weight.original1"]
    wav = torch.from_numpy(case_input(name)).to(gpu)
    want = model(name, "fp32", gpu).extract_features(wav)[0].cpu()
    m = WavLM(cfg, device=gpu, precision="fp32", max_batch=2, max_samples=16000).load_state_dict(old)
    assert torch.equal(m.extract_features(wav)[0].cpu(), want)
    both = dict(old, **{p + "parametrizations.weight.original0": old[p + "weight_g"]})
    with pytest.raises(RuntimeError, match="parametrizations.weight.original0"):     # strict: an unexpected key
        WavLM(cfg, device=gpu, precision="fp32", max_batch=2, max_samples=16000).load_state_dict(both)


@pytest.mark.parametrize("name", ["bp_t49", "lg_t49"])
def test_return_nesting_of_the_four_flag_combinations(gpu, name):
    m = model(name, "fp32", gpu)
    wav = torch.from_numpy(case_input(name)).to(gpu)
    B, T, D = wav.shape[0], num_frames(wav.shape[1]), m.embed_dim
    x, pm = m.extract_features(wav)
    assert pm is None and torch.is_tensor(x) and tuple(x.shape) == (B, T, D)
    f, pm = m.extract_features(wav, ret_conv=True)
    assert pm is None and torch.is_tensor(f) and tuple(f.shape) == (B, T, D) and not torch.equal(f, x)
    (x2, res), pm = m.extract_features(wav, ret_layer_results=True)
    assert pm is None and res == [] and torch.equal(x2, x)
    (f2, res), pm = m.extract_features(wav, ret_conv=True, ret_layer_results=True, output_layer=1)
    assert pm is None and torch.equal(f2, f) and len(res) == 2
    assert all(z is None and tuple(h.shape) == (T, B, D) for h, z in res)
    (x1, res1), _ = m.extract_features(wav, output_layer=1, ret_layer_results=True)
    assert torch.equal(res1[1][0].transpose(0, 1), x1) and torch.equal(res1[1][0], res[1][0])
    (xl, _), _ = m.extract_features(wav, output_layer=2, ret_layer_results=True)
    # two layers either way: equal for Base+, and apart by the final LayerNorm for Large (wavlm.py:623-624)
    assert torch.equal(xl, x) == (name == "bp_t49")


def test_refused_arguments(gpu):
    m = model("bp_t49", "fp32", gpu)
    wav = torch.zeros(2, 16000, device=gpu)
    with pytest.raises(ValueError, match="output_layer must be 1..2"):
        m.extract_features(wav, output_layer=3)
    with pytest.raises(ValueError, match="n_samples must be at least 400"):
        m.extract_features(wav[:, :399])
    with pytest.raises(ValueError, match="exceeds max_batch"):
        m.extract_features(torch.zeros(3, 16000, device=gpu))
    from speaker_diarization_amd import _lib
    out = torch.empty(2, 49, 768, device=gpu)
    for args, msg in (((2, 16000, 3), "output_layer must be 0"), ((2, 399, 0), "n_samples must be at least 400"),
                      ((3, 16000, 0), "batch exceeds max_batch"), ((2, 16001, 0), "n_samples exceeds max_samples")):
        with pytest.raises(ValueError, match=msg):
            _lib.call("sd_wavlm_forward", m._h, _lib.ptr(wav), *args, _lib.ptr(out), None, None, _lib.stream_ptr(gpu))
    with pytest.raises(ValueError, match="layers_out needs output_layer >= 1"):
        _lib.call("sd_wavlm_forward", m._h, _lib.ptr(wav), 2, 16000, 0, None, None, _lib.ptr(out), _lib.stream_ptr(gpu))
    assert m.device_bytes > 0


def test_two_lengths_on_one_handle(gpu):
    """199 frames, then 49, then 199 again on one handle: the workspace and the per-T bias table are rebuilt for each."""
    name = "bp_t199"
    g = gold(name)
    m = model(name, "fp32", gpu, max_batch=2, max_samples=64000)
    frames = [int(f) for f in g["frames"]]
    long = torch.from_numpy(case_input(name)).to(gpu)
    short = long[:, 3000:19000].contiguous()
    first = m.extract_features(long, output_layer=2)[0]
    bar = FP32_RTOL * max(1.0, float(np.abs(g["x_2"]).max()))
    assert float(np.abs(first[:, frames].cpu().numpy() - g["x_2"]).max()) <= bar
    got_short = m.extract_features(short, output_layer=2)[0].cpu()
    assert tuple(got_short.shape) == (1, 49, 768)
    assert torch.equal(m.extract_features(long, output_layer=2)[0], first)
    fresh = WavLM(case_config(name), device=gpu, precision="fp32", max_batch=1, max_samples=16000)
    fresh.load_state_dict(to_torch(wavlm_state_dict(case_config(name), CASES[name][6])))
    want_short = fresh.extract_features(short, output_layer=2)[0].cpu()
    e = float((got_short - want_short).abs().max())
    print(f"49 frames after 199 on one handle against a fresh handle: max|diff| {e:.3e}")
    assert e <= FP32_RTOL * max(1.0, float(want_short.abs().max()))
    # and against the CPU restatement, which test_wavlm_host.py holds to the reference
    import wavlm_ref as wr
    sd = to_torch(wavlm_state_dict(case_config(name), CASES[name][6]))
    with torch.no_grad():
        ref = wr.extract_features(sd, case_config(name), short.cpu(), output_layer=2)["x"]
    assert float((got_short - ref).abs().max()) <= FP32_RTOL * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("name,B,n", [("bp_t49", 10, 16000), ("lg_t1", 9, 720)])
def test_batch_past_one_front_end_slice(gpu, name, B, n):
    """More windows than one pass of the conv front end takes (8): the second slice reads its own waveforms, reuses the
    ping-pong maps and the statistics scratch, and writes its own rows of the feature map.  Against the CPU
    restatement (which tests/test_wavlm_host.py holds to the reference), every window and frame, fp32 bar."""
    import wavlm_ref as wr
    cfg = case_config(name)
    sd = to_torch(wavlm_state_dict(cfg, CASES[name][6]))
    wav = torch.from_numpy((np.random.default_rng(B + n).standard_normal((B, n)) * 0.5).astype(np.float32))
    with torch.no_grad():
        ref = wr.extract_features(sd, cfg, wav, output_layer=2)
    m = WavLM(cfg, device=gpu, precision="fp32", max_batch=B, max_samples=n).load_state_dict(sd)
    (x, results), _ = m.extract_features(wav.to(gpu), output_layer=2, ret_layer_results=True)
    feats, _ = m.extract_features(wav.to(gpu), ret_conv=True)
    for what, got, want in (("x", x, ref["x"]), ("features", feats, ref["features"]),
                            ("layer_0", results[0][0].transpose(0, 1), ref["layers"][0])):
        per_window = (got.cpu() - want).abs().amax(dim=(1, 2))
        bar = FP32_RTOL * max(1.0, float(want.abs().max()))
        print(f"{name} B={B} n={n} {what}: max|diff| per window {[f'{float(e):.1e}' for e in per_window]}  bar {bar:.3e}")
        assert float(per_window.max()) <= bar, (what, per_window)
    assert not torch.equal(x[0], x[8])          # the windows differ, so a slice reading the wrong rows shows
