"""Golden outputs of the w2v-BERT 2.0 trunk (w2vbert_*) and of TS-VAD with speech_encoder_type "w2v-bert2"
(tsvad_w2vbert_*) by running transformers' Wav2Vec2BertModel and the REFERENCE MagicData TSVADModel (build container
only: it imports `transformers` and the reference).

    HF_HUB_OFFLINE=1 PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_w2vbert.py

Same method as make_golden_tsvad_wavlm.py.  The reference builds its encoder with from_pretrained(cfg.speech_encoder_path),
so seeded weights are written with save_pretrained into a temporary directory that speech_encoder_path and
speech_encoder_config point at; then tsvad_state_dict's seeded weights are loaded strict=True and the model runs in eval
on seeded inputs.  Only seeds, outputs, key names / shapes and recorded messages are stored.

Asserted here: every golden is finite (outside a NaN window) with a standard deviation in [0.1, 10]; each perturbation of
`perturbed_runs` moves the (1, 400, 100) logits by at least ten fp32 bars (the observed factors are stored in
tsvad_w2vbert_keys.npz); an odd T raises in the reference (its message is stored); the label-length rule's accept /
raise cases.
"""
from __future__ import annotations

import contextlib
import math
import os
import sys
import tempfile

import numpy as np

os.environ.setdefault("HF_HUB_OFFLINE", "1")
import transformers  # noqa: E402,F401  (before install_stubs: the torchaudio stub has no __spec__ and trips its lazy import)
from transformers import Wav2Vec2BertConfig, Wav2Vec2BertModel  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, install_stubs  # noqa: E402
from w2vbert_cases import (NAN, PERTURB_CASE, RAISES, TRUNK, TSVAD, keep_frames, trunk_config, trunk_input,  # noqa: E402
                           tsvad_cfg, tsvad_inputs)

LIMIT = 650_000
FP32_RTOL = 1e-3


def hf_config(layers):
    conf = Wav2Vec2BertConfig(hidden_act="swish", num_hidden_layers=layers)
    from speaker_diarization_amd.ssl.w2vbert import W2vBertConfig
    for k, v in W2vBertConfig().__dict__.items():      # the published geometry is the class's default
        if k != "num_hidden_layers":
            assert getattr(conf, k) == v, (k, getattr(conf, k), v)
    return conf


def hf_model(layers):
    import torch
    torch.manual_seed(0)
    m = Wav2Vec2BertModel(hf_config(layers))
    m.eval()
    return m


def reference_tsvad(cfg):
    """The reference TSVADModel of a project TSVADConfig (imports under the stubs of SURVEY Appendix A)."""
    import torch
    from oracle.torchaudio_conformer import Conformer
    from speaker_diarization_amd.weights import to_torch, w2vbert_state_dict
    install_stubs(Conformer)
    d = os.path.join(REF, "egs/magicdata-ramc/ts_vad2")
    for q in (os.path.dirname(d), d):
        if q not in sys.path:
            sys.path.insert(0, q)
    import model as ref_model
    assert os.path.dirname(os.path.abspath(ref_model.__file__)) == os.path.abspath(d), ref_model.__file__
    mcfg = ref_model.TSVADConfig()
    mcfg.speech_encoder_type = cfg.speech_encoder_type
    mcfg.select_encoder_layer_nums = cfg.select_encoder_layer_nums
    mcfg.speaker_embed_dim = cfg.speaker_embed_dim
    dcfg = ref_model.TSVADDataConfig()
    dcfg.rs_len = 4
    depth = cfg.w2vbert_cfg.num_hidden_layers
    with tempfile.TemporaryDirectory() as tmp:
        m0 = hf_model(depth)
        m0.load_state_dict(to_torch(w2vbert_state_dict(trunk_config(depth), 1)), strict=True)
        m0.save_pretrained(tmp)
        mcfg.speech_encoder_path = tmp
        mcfg.speech_encoder_config = tmp
        torch.manual_seed(0)
        m = ref_model.TSVADModel(cfg=mcfg, task_cfg=dcfg)
    m.eval()
    assert len(m.speech_encoder.encoder.layers) == cfg.select_encoder_layer_nums
    return m


def run(m, ref, ts, n_lab):
    import torch
    with torch.no_grad():
        return m(torch.from_numpy(ref), torch.from_numpy(ts), torch.zeros(ref.shape[0], 4, n_lab),
                 num_updates=0).numpy().astype(np.float32)


def flipped_attention(attn):
    """Wav2Vec2BertSelfAttention.forward restated with the distance's sign flipped: E[clamp(l - r, -64, 8) + 64]."""
    import torch

    def forward(hidden_states, attention_mask=None, relative_position_embeddings=None, output_attentions=False):
        B, T, _ = hidden_states.shape
        q, k, v = (f(hidden_states).view(B, T, attn.num_heads, attn.head_size).transpose(1, 2)
                   for f in (attn.linear_q, attn.linear_k, attn.linear_v))
        pos = torch.arange(T)
        d = torch.clamp(pos[:, None] - pos[None, :], -attn.left_max_position_embeddings,
                        attn.right_max_position_embeddings) + attn.left_max_position_embeddings
        rel = torch.einsum("bhld,lrd->bhlr", q, attn.distance_embedding(d))
        p = torch.softmax((q @ k.transpose(-1, -2) + rel) / math.sqrt(attn.head_size), -1)
        return attn.linear_out((p @ v).transpose(1, 2).reshape(B, T, -1)), None
    return forward


def perturbed_runs(m, sd, ref, ts, n_lab, deeper):
    """name -> logits of the reference with one thing wrong."""
    import torch
    import torch.nn.functional as F
    layers = m.speech_encoder.encoder.layers
    out = {}

    def with_sd(edit):
        psd = {k: (edit(k, v) if edit(k, v) is not None else v) for k, v in sd.items()}
        m.load_state_dict(psd, strict=True)
        try:
            return run(m, ref, ts, n_lab)
        finally:
            m.load_state_dict(sd, strict=True)

    @contextlib.contextmanager
    def attrs(pairs):
        old = [(o, n, getattr(o, n)) for o, n, _ in pairs]
        for o, n, v in pairs:
            setattr(o, n, v)
        try:
            yield
        finally:
            for o, n, v in old:
                setattr(o, n, v)

    out["zeroed distance_embedding"] = with_sd(
        lambda k, v: torch.zeros_like(v) if k.endswith("distance_embedding.weight") else None)
    with attrs([(l.self_attn, "forward", flipped_attention(l.self_attn)) for l in layers]):
        out["sign of the distance flipped"] = run(m, ref, ts, n_lab)
    with attrs([(l.self_attn, n, v) for l in layers
                for n, v in (("left_max_position_embeddings", 8), ("right_max_position_embeddings", 64))]):
        out["clamp bounds swapped to (8, 64)"] = run(m, ref, ts, n_lab)
    real_pad = F.pad
    with attrs([(F, "pad", lambda x, pad, *a, **k: real_pad(x, (15, 15) if tuple(pad) == (30, 0) else pad, *a, **k))]):
        out["symmetric instead of causal padding"] = run(m, ref, ts, n_lab)
    out["0.5 of the FFN half-steps dropped"] = with_sd(lambda k, v: 2 * v if ".output_dense." in k else None)
    with attrs([(l, "final_layer_norm", torch.nn.Identity()) for l in layers]):
        out["final_layer_norm skipped"] = run(m, ref, ts, n_lab)
    with attrs([(o, n, torch.nn.GELU()) for l in layers for o, n in ((l.ffn1, "intermediate_act_fn"),
                                                           (l.ffn2, "intermediate_act_fn"),
                                                           (l.conv_module, "activation"))]):
        out["gelu instead of swish"] = run(m, ref, ts, n_lab)
    T = ref.shape[1]
    halves = np.stack([ref[:, :T // 2], ref[:, T // 2:]], 2).reshape(ref.shape)   # reshape pairs [t, t + T/2]
    out["frame pairing [t, t + T/2]"] = run(m, halves, ts, n_lab)
    out["one layer more"] = deeper(ref, ts, n_lab)
    return out


def save(name, out):
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.shape}, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < LIMIT, "golden larger than the largest one committed"


def main():
    import torch
    from speaker_diarization_amd.weights import to_torch, tsvad_state_dict, w2vbert_state_dict
    keys, factors = {}, {}
    # ---- trunk
    m = hf_model(2)
    sd0 = m.state_dict()
    keys["trunk_l2.names"] = np.array(list(sd0), dtype="U")
    keys["trunk_l2.shapes"] = np.array([",".join(str(d) for d in t.shape) for t in sd0.values()], dtype="U")
    for name, (layers, B, T2, iseed, wseed, every) in TRUNK.items():
        assert layers == 2
        m.load_state_dict(to_torch(w2vbert_state_dict(trunk_config(layers), wseed)), strict=True)
        x = trunk_input(name)
        with torch.no_grad():
            o = m(torch.from_numpy(x), output_hidden_states=True)
        assert len(o.hidden_states) == layers + 1 and torch.equal(o.hidden_states[-1], o.last_hidden_state)
        frames = keep_frames(T2)
        last = o.last_hidden_state.numpy().astype(np.float32)
        std, peak = float(last.std()), float(np.abs(last).max())
        print(f"{name}: last_hidden_state std {std:.3f}  max |.| {peak:.3f}")
        assert np.isfinite(last).all() and 0.1 <= std <= 10.0, (name, std)
        out = dict(x=last[:, frames], B=np.int64(B), T2=np.int64(T2), frames=np.array(frames, np.int64),
                   input_seed=np.int64(iseed), weight_seed=np.int64(wseed))
        if every:
            for i, h in enumerate(o.hidden_states):
                out[f"layer_{i}"] = h.numpy().astype(np.float32)[:, frames]
        save(name, out)
    # ---- TS-VAD
    models = {}
    for name in list(TSVAD) + list(NAN):
        base = NAN[name][0] if name in NAN else name
        _, _, _, se, depth, select, _, _ = TSVAD[base]
        cfg = tsvad_cfg(name)
        mk = (se, depth, select)
        if mk not in models:
            models[mk] = reference_tsvad(cfg)
            sd0 = models[mk].state_dict()
            tag = f"se{se}_d{depth}_l{select}"
            keys[tag + ".names"] = np.array(list(sd0), dtype="U")
            keys[tag + ".shapes"] = np.array([",".join(str(d) for d in t.shape) for t in sd0.values()], dtype="U")
        m = models[mk]
        (B, T, n_lab, wseed), ref, ts = tsvad_inputs(name)
        sd = to_torch(tsvad_state_dict(cfg, seed=wseed))
        m.load_state_dict(sd, strict=True)
        logits = run(m, ref, ts, n_lab)
        assert logits.shape == (B, 4, n_lab), logits.shape
        good = logits if name not in NAN else np.delete(logits, NAN[name][1], 0)
        if name in NAN:
            assert np.isnan(logits[NAN[name][1]]).all()
        std = float(good.std())
        print(f"{name}: logit std {std:.3f}  max |logit| {float(np.abs(good).max()):.3f}")
        assert np.isfinite(good).all() and 0.1 <= std <= 10.0, (name, std)
        save(name, dict(logits=logits, B=np.int64(B), T=np.int64(T), n_label=np.int64(n_lab),
                        weight_seed=np.int64(wseed)))
        if name == PERTURB_CASE:
            from speaker_diarization_amd.weights import TSVADConfig
            cfg3 = TSVADConfig(speech_encoder_type="w2v-bert2", w2vbert_cfg=trunk_config(3), select_encoder_layer_nums=3,
                               speaker_embed_dim=se)
            sd3 = to_torch(tsvad_state_dict(cfg3, seed=wseed))
            assert all(torch.equal(sd3[k], v) for k, v in sd.items())   # the first two layers and the rest are the same

            def deeper(ref, ts, n_lab):
                m3 = reference_tsvad(cfg3)
                m3.load_state_dict(sd3, strict=True)
                return run(m3, ref, ts, n_lab)

            bar = FP32_RTOL * max(1.0, float(np.abs(logits).max()))
            for what, got in perturbed_runs(m, sd, ref, ts, n_lab, deeper).items():
                moved = float(np.abs(got - logits).max())
                print(f"  {name}: {what}: moves the logits by {moved:.3e} = {moved / bar:.0f} fp32 bars")
                assert moved >= 10 * bar, (name, what, moved, bar)
                factors[what] = moved / bar
            assert float(np.abs(run(m, ref, ts, n_lab) - logits).max()) == 0.0     # everything was put back
    # ---- the label-length rule and the odd-T refusal
    accept, refuse = [], []
    for base, n_lab in RAISES:
        cfg = tsvad_cfg(base)
        _, _, _, se, depth, select, _, _ = TSVAD[base]
        m = models[(se, depth, select)]
        (B, T, _, wseed), ref, ts = tsvad_inputs(base)
        m.load_state_dict(to_torch(tsvad_state_dict(cfg, seed=wseed)), strict=True)
        try:
            run(m, ref, ts, n_lab)
        except AssertionError as e:
            print(f"labels {n_lab} at T {T}: reference raises: {str(e)[:70]}")
            refuse.append((T, n_lab))
        else:
            raise SystemExit(f"the reference accepted labels {n_lab} at T {T}")
    for name in ("tsvad_w2vbert_t22_l5", "tsvad_w2vbert_t22_l6"):
        accept.append((TSVAD[name][1], TSVAD[name][2]))
    keys["label_rule.accept"] = np.array(accept, np.int64)
    keys["label_rule.raise"] = np.array(refuse, np.int64)
    (B, T, n_lab, _), ref, ts = tsvad_inputs("tsvad_w2vbert_t22_l5")
    try:
        run(m, ref[:, :21], ts, n_lab)
    except RuntimeError as e:
        raised = str(e)
        print("odd T: reference raises:", raised[:90])
        assert "is invalid for input of size" in raised, raised
    else:
        raise SystemExit("the reference ran an odd number of fbank frames")
    keys["odd_T_raises"] = np.array(raised[:200])
    keys["perturbation.names"] = np.array(list(factors), dtype="U")
    keys["perturbation.fp32_bars"] = np.array(list(factors.values()), np.float64)
    save("tsvad_w2vbert_keys", keys)


if __name__ == "__main__":
    main()
