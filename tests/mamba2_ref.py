"""CPU restatement of the TS-VAD Mamba2 back ends (plain torch, fp64 by default).

Mamba2BlockV2 (egs/*/ts_vad2/mamba.py:149-213) over mamba_ssm's Mamba2 mixer at the defaults the reference leaves
untouched (headdim 64, ngroups 1, d_conv 4, rmsnorm, norm_before_gate False, no projection biases, dt_limit (0, inf)),
and forward_common with those back ends (egs/magicdata-ramc/ts_vad2/model.py:1330-1400).  mamba_ssm is CUDA-only and
not installed where this was written, so nothing here is pinned by a reference run (parity unpinned, like
oracle.tsvad_ref.conformer): the mixer is written in two independent forms that must agree, and the GPU path is held to
them.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import tsvad_ref as tr  # noqa: E402
from speaker_diarization_amd.weights import mamba2_block_v2_layout, synthetic_state_dict, to_torch  # noqa: E402

HEADDIM = 64
EPS = 1e-5
BLOCK_KEYS = ("norm.weight", "mixer.in_proj.weight", "mixer.conv1d.weight", "mixer.conv1d.bias", "mixer.dt_bias",
              "mixer.A_log", "mixer.D", "mixer.norm.weight", "mixer.out_proj.weight")


def rmsnorm(x, w, eps=EPS):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def causal_conv(x, w, b):
    """Depthwise causal conv over dim 1 of x (Bt, L, C): y[l] = b + sum_k w[c, 0, k] x[l - 3 + k], zeros before the
    sequence's start (nn.Conv1d(groups=C, kernel 4, padding 3)[..., :L])."""
    L, k = x.shape[1], w.shape[-1]
    xp = F.pad(x, (0, 0, k - 1, 0))
    y = b.expand_as(x).clone()
    for j in range(k):
        y = y + xp[:, j:j + L] * w[:, 0, j]
    return y


def _scan_recurrent(xs, Bm, Cm, dt, A):
    """S_l = exp(dt_l A) S_{l-1} + dt_l x_l (x) Bm_l, y_l = S_l Cm_l.  xs (Bt, L, H, P), Bm / Cm (Bt, L, N), dt (Bt, L, H)."""
    Bt, L, H, P = xs.shape
    S = xs.new_zeros(Bt, H, P, Bm.shape[-1])
    ys = []
    for l in range(L):
        da = torch.exp(dt[:, l] * A)                                       # (Bt, H)
        S = da[:, :, None, None] * S + (dt[:, l, :, None] * xs[:, l])[..., None] * Bm[:, l, None, None, :]
        ys.append((S * Cm[:, l, None, None, :]).sum(-1))
    return torch.stack(ys, 1)


def _scan_chunked(xs, Bm, Cm, dt, A, chunk):
    """The same map in the quadratic (SSD) form over chunks of `chunk` steps, the state carried between chunks."""
    Bt, L, H, P = xs.shape
    S = xs.new_zeros(Bt, H, P, Bm.shape[-1])
    out = []
    for c0 in range(0, L, chunk):
        x, b, c, d = xs[:, c0:c0 + chunk], Bm[:, c0:c0 + chunk], Cm[:, c0:c0 + chunk], dt[:, c0:c0 + chunk]
        q = x.shape[1]
        cum = torch.cumsum(d * A, dim=1)                                   # (Bt, q, H)
        seg = cum[:, :, None, :] - cum[:, None, :, :]                      # (Bt, l, m, H)
        mask = torch.tril(torch.ones(q, q, dtype=torch.bool))[None, :, :, None]
        decay = torch.exp(seg.masked_fill(~mask, float("-inf")))           # exp(cum_l - cum_m) for m <= l, else 0
        gm = torch.einsum("bln,bmn->blm", c, b)                            # shared by the heads
        y = torch.einsum("blm,blmh,bmh,bmhp->blhp", gm, decay, d, x)
        y = y + torch.einsum("bln,blh,bhpn->blhp", c, torch.exp(cum), S)   # the carried state's share
        tail = torch.exp(cum[:, -1:, :] - cum)                             # (Bt, q, H)
        S = torch.exp(cum[:, -1])[:, :, None, None] * S + torch.einsum("bmh,bmh,bmhp,bmn->bhpn", tail, d, x, b)
        out.append(y)
    return torch.cat(out, 1)


def mamba2_mixer(sd, p, x, form="recurrent", chunk=64, probe=None):
    """Mamba2.forward of the block at key prefix p (`...forward_blocks.0.mixer.`) on x (Bt, L, E).  form: "recurrent"
    (step by step) or "chunked" (SSD, chunk length `chunk`).  probe (dict): receives decay, y_state and y."""
    d_inner = sd[p + "norm.weight"].shape[0]
    H = sd[p + "A_log"].shape[0]
    N = (sd[p + "conv1d.weight"].shape[0] - d_inner) // 2
    assert H * HEADDIM == d_inner
    zxbcdt = F.linear(x, sd[p + "in_proj.weight"])
    z, xBC, dt_raw = torch.split(zxbcdt, [d_inner, d_inner + 2 * N, H], dim=-1)
    xBC = F.silu(causal_conv(xBC, sd[p + "conv1d.weight"], sd[p + "conv1d.bias"]))
    xs, Bm, Cm = torch.split(xBC, [d_inner, N, N], dim=-1)
    xs = xs.reshape(*xs.shape[:2], H, HEADDIM)
    dt = F.softplus(dt_raw + sd[p + "dt_bias"])
    A = -torch.exp(sd[p + "A_log"])
    if form == "recurrent":
        ys = _scan_recurrent(xs, Bm, Cm, dt, A)
    else:
        ys = _scan_chunked(xs, Bm, Cm, dt, A, chunk)
    y = ys + sd[p + "D"][:, None] * xs
    if probe is not None:
        probe.setdefault("decay", []).append(torch.exp(dt * A))
        probe.setdefault("y_state", []).append(ys)
        probe.setdefault("y", []).append(y)
    g = y.reshape(*y.shape[:2], d_inner) * F.silu(z)
    return F.linear(rmsnorm(g, sd[p + "norm.weight"]), sd[p + "out_proj.weight"])


def n_layers(sd, prefix):
    n = 0
    while f"{prefix}forward_blocks.{n}.norm.weight" in sd:
        n += 1
    return n


def mamba2_block_v2(sd, prefix, x, form="recurrent", chunk=64, probe=None):
    """Mamba2BlockV2(bidirectional=True).forward on x (Bt, L, E) -> (Bt, L, 2 E): batch on dim 0, sequence on dim 1,
    whatever the caller meant those axes to be."""
    def chain(name, u):
        hidden, residual = u, None
        for i in range(n_layers(sd, prefix)):
            p = f"{prefix}{name}.{i}."
            residual = hidden + residual if residual is not None else hidden       # Block.forward, fused_add_norm=False
            hidden = mamba2_mixer(sd, p + "mixer.", rmsnorm(residual, sd[p + "norm.weight"]), form, chunk, probe)
        return hidden + residual
    fwd = chain("forward_blocks", x)
    bwd = torch.flip(chain("backward_blocks", torch.flip(x, [1])), [1])
    return torch.cat([fwd, bwd], -1)


def to_double(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@torch.no_grad()
def tsvad_forward(sd, cfg, ref_speech, target_speech, max_len, probe=None, form="recurrent"):
    """TSVADModel.forward in eval with single_backend_type "mamba2" and multi_backend_type "transformer" or "mamba2"
    (magicdata model.py:1330-1400; alimeeting model.py:869-897): ONE reference forward call over the B windows given.
    The speech encoder runs in fp32 (oracle.tsvad_ref), the back end in fp64; form: the mixer form (the chunked one is
    the cheaper of the two on long label axes).  -> logits (B, NS, max_len) fp32."""
    ns, nh = cfg.max_num_speaker, cfg.num_attention_head
    x = tr.speech_encoder_out(sd, ref_speech)
    gap = x.size(-1) - max_len
    assert -1 <= gap <= 2, f"label and ref_speech(mix speech) diff: {gap}"
    if gap == -1:
        x = F.pad(x, (0, 1))
    mix = x[:, :, :max_len].transpose(1, 2).double()
    sd = to_double(sd)
    ts = target_speech.double()
    B, T, _ = mix.shape
    outs = []
    for i in range(ns):
        cat = torch.cat((ts[:, i, None, :].expand(B, T, -1), mix), 2)
        if "proj_layer.weight" in sd:
            cat = F.linear(cat, sd["proj_layer.weight"], sd["proj_layer.bias"])
        cat = cat.transpose(0, 1)                         # (T, B, E)
        cat = tr.positional_encoding(cat, sd)
        # the seq-first tensor goes to a batch-first module: T is its batch, the B windows are its sequence
        cat = mamba2_block_v2(sd, "single_backend.", cat, form, probe=probe)
        outs.append(cat.transpose(0, 1))                  # (B, T, 2 E)
    cat = torch.stack(outs).permute(1, 0, 3, 2).reshape(B, -1, T)
    cat = F.relu(tr._bn1d_nan_bypass(F.conv1d(cat, sd["backend_down.0.weight"], sd["backend_down.0.bias"], padding=2),
                                     sd, "backend_down.1.bn"))
    cat = tr.positional_encoding(cat.permute(2, 0, 1), sd)   # (T, B, E)
    if cfg.multi_backend_type == "mamba2":
        cat = mamba2_block_v2(sd, "multi_backend.", cat, form, probe=probe)
        cat = F.linear(cat.transpose(0, 1), sd["multi_backend_proj.weight"], sd["multi_backend_proj.bias"])
    else:
        for l in range(cfg.num_transformer_layer):
            cat = tr.transformer_layer(cat, sd, f"multi_backend.layers.{l}.", nh)
        cat = cat.transpose(0, 1)
    return F.linear(cat, sd["fc.weight"], sd["fc.bias"]).transpose(1, 2).float()


def tsvad_forward_grouped(sd, cfg, ref_speech, target_speech, max_len, forward_batch=0):
    """The reference loop over forward calls of `forward_batch` consecutive windows (0: one call)."""
    B = ref_speech.shape[0]
    G = forward_batch if forward_batch > 0 else B
    return torch.cat([tsvad_forward(sd, cfg, ref_speech[g:g + G], target_speech[g:g + G], max_len)
                      for g in range(0, B, G)])


# ----------------------------------------------------------------------------- seeded cases of the operator tests
def stack_state_dict(E, d_state, expand, n_layer, seed):
    """Seeded weights of one Mamba2BlockV2 under the keys forward_blocks.{i}. / backward_blocks.{i}. (torch, fp32)."""
    k = []
    mamba2_block_v2_layout(k, "", E, n_layer, d_state, expand)
    return to_torch(synthetic_state_dict(k, seed))


def flat_weights(sd, n_layer):
    """The weight array sd_op_mamba2_stack takes: direction-major, then layer, then BLOCK_KEYS order."""
    return torch.cat([sd[f"{d}.{i}.{k}"].reshape(-1).float() for d in ("forward_blocks", "backward_blocks")
                      for i in range(n_layer) for k in BLOCK_KEYS])


def stack_input(R, L, E, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((R, L, E)).astype(np.float32))


# (E, expand, d_state, R, n_layer) x L of the operator tests: two heads, the smallest and the recipe's state size, every
# length around the kernel's 16-step staging chunk and the 64-window tile of a reference batch, plus the model's widths
OP_LENGTHS = (1, 2, 5, 64, 65, 130)
OP_CASES = [(64, 2, ds, 3, nl, L) for ds in (16, 128) for nl in (1, 2) for L in OP_LENGTHS] + [(384, 4, 128, 5, 2, 7)]


def op_case(case):
    E, expand, ds, R, nl, L = case
    sd = stack_state_dict(E, ds, expand, nl, seed=1000 + ds + nl)
    return sd, stack_input(R, L, E, seed=2000 + L)
