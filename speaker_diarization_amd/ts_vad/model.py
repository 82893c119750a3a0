"""TSVADModel — drop-in for egs/alimeeting/ts_vad2/model.py:179 (inference).

Same constructor inputs (TSVADConfig + data config), same state_dict keys,
same forward(ref_speech, target_speech, labels, num_updates) -> logits
(B, max_num_speaker, T_label) and infer(...) -> (result, res_dict) surface.
The forward runs entirely in libsdiar (HIP, gfx950); this class only moves
state_dict tensors across the C ABI and wraps device pointers.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np

from .. import _lib
from ..weights import TSVADConfig, unwrap_checkpoint


def fbank_frames(rs_len: int, sample_rate: int = 16000) -> int:
    n = rs_len * sample_rate
    return 1 + (n - 400) // 160


class TSVADModel(_lib.Handle):
    kind = "tsvad"

    def __init__(self, cfg: TSVADConfig = None, task_cfg=None, device=None, precision: str = "bf16",
                 max_batch: int = 64):
        self.cfg = cfg or TSVADConfig()
        if task_cfg is not None:   # mirror of TSVADDataConfig fields the model reads
            for k in ("rs_len", "max_num_speaker", "label_rate", "sample_rate"):
                if hasattr(task_cfg, k):
                    setattr(self.cfg, k, getattr(task_cfg, k))
        assert self.cfg.label_rate == 25, f"self.label_rate is {self.cfg.label_rate} not support!"
        _lib.precision_code(precision)
        self.precision = precision
        self.device = _lib.hip_device(device, "TSVADModel")
        self.max_batch = max_batch
        self.max_num_speaker = self.cfg.max_num_speaker
        self.max_fbank = fbank_frames(self.cfg.rs_len, self.cfg.sample_rate)
        c = self.cfg
        wav = {}
        if c.variant in (5, 6):
            # the WavLM speech encoders read the raw waveform: the geometry of wavlm_cfg and the longest window
            if precision == "bf16x3":
                raise ValueError("the WavLM speech encoders do not build bf16x3 (the WavLM trunk runs in fp32 or bf16)")
            w = c.effective_wavlm_cfg()
            self.max_samples = c.rs_len * c.sample_rate
            wav = dict(wavlm_embed_dim=w.encoder_embed_dim, wavlm_layers=w.encoder_layers,
                       wavlm_layer_norm_mode=int(w.extractor_mode == "layer_norm"),
                       wavlm_pre_ln=int(bool(w.layer_norm_first)), max_samples=self.max_samples)
        if c.variant == 7:
            # w2v-bert2 reads variant 0's fbank windows; only the encoder depth is its own
            if precision == "bf16x3":
                raise ValueError("the w2v-bert2 speech encoder does not build bf16x3 (the w2v-BERT trunk runs in fp32 "
                                 "or bf16)")
            wav = dict(w2vbert_layers=c.effective_w2vbert_cfg().num_hidden_layers)
            # the reference takes any even frame count; rs_len seconds at 100 frames / s is the longest a window gives
            self.max_fbank = max(self.max_fbank, c.rs_len * 100)
        wcfg = None
        if c.variant == 8:
            # whisper reads the raw waveform too; the trunk's geometry travels in its own struct
            # (sd_tsvad_create_whisper: sd_tsvad_config keeps its fields)
            if precision == "bf16x3":
                raise ValueError("the whisper speech encoder does not build bf16x3 (the Whisper trunk runs in fp32 or "
                                 "bf16)")
            w = c.effective_whisper_cfg()
            self.max_samples = c.rs_len * c.sample_rate
            wav = dict(max_samples=self.max_samples)
            wcfg = _lib.WhisperConfig(
                n_mels=w.n_mels, n_audio_ctx=w.n_audio_ctx, n_audio_state=w.n_audio_state,
                n_audio_head=w.n_audio_head, n_audio_layer=w.n_audio_layer, layer_st=w.layer_st, layer_ed=w.layer_ed,
                precision=_lib.PRECISION[precision], max_batch=self.max_batch, max_samples=self.max_samples)
        conf = (_lib.TsvadConfigEx if c.frame_level_gsp else _lib.TsvadConfig)(
            variant=c.variant, max_num_speaker=c.max_num_speaker, rs_len=c.rs_len, max_batch=self.max_batch,
            max_fbank_frames=self.max_fbank, precision=_lib.PRECISION[precision],
            num_transformer_layer=c.num_transformer_layer, num_attention_head=c.num_attention_head,
            transformer_embed_dim=c.transformer_embed_dim,
            transformer_ffn_embed_dim=c.transformer_ffn_embed_dim, speaker_embed_dim=c.speaker_embed_dim,
            backend=c.backend, d_state=c.d_state if c.mamba2_backend else 0,
            expand=c.expand if c.mamba2_backend else 0, **wav)
        if c.frame_level_gsp:
            # "CAM++_frame_level_gsp_fc": variant 0 with the gsp_fc stage, a field past sd_tsvad_config's own
            import ctypes
            conf.frame_level_gsp = 1
            h = ctypes.c_void_p()
            _lib.call("sd_tsvad_create_ex", ctypes.byref(conf), ctypes.byref(h))
            self._h = h
        elif wcfg is None:
            self._create(conf)
        else:
            import ctypes
            h = ctypes.c_void_p()
            _lib.call("sd_tsvad_create_whisper", ctypes.byref(conf), ctypes.byref(wcfg), ctypes.byref(h))
            self._h = h

    def load_state_dict(self, state_dict, strict: bool = True):
        """Strict load (missing/unexpected keys raise RuntimeError like torch)."""
        if not strict:
            raise ValueError("the MI355X backend only supports strict=True loading")
        state = unwrap_checkpoint(state_dict)
        if self.cfg.variant == 8:
            # the Whisper front end's mel matrix: a constant computed on the host, not a reference key
            from ..feature import whisper_mel_filters
            state = dict(state)
            if "speech_encoder.mel_filters" in state:
                raise RuntimeError('Error(s) in loading state_dict: Unexpected key(s) in state_dict: '
                                   '"speech_encoder.mel_filters"')
            state["speech_encoder.mel_filters"] = whisper_mel_filters(self.cfg.whisper_n_mels)
        self._load(state)
        return self

    def eval(self):
        return self

    def to(self, device):
        import torch
        if torch.device(device) != self.device:
            raise ValueError("re-create the model on the target device")
        return self

    @property
    def device_bytes(self) -> int:
        return self._device_bytes()

    # ------------------------------------------------------------------ forward
    def forward(self, ref_speech, target_speech, labels, num_updates: int = 0, out=None, check: bool = True,
                forward_batch: int = 0, _force: int = 0):
        """ref_speech (B, T_fb, 80) ((B, T_fb, 72) with the ReDimNetB2 speech encoder; the raw waveform (B, n_samples),
        400 <= n_samples <= rs_len * sample_rate and a multiple of 4, with the WavLM ones), target_speech (B, NS, speaker_embed_dim), labels (B, NS, T) (only
        labels.size(-1) is read, model.py:681/770) -> logits (B, NS, T).  check: wait for the
        stream and raise RuntimeError in this call if the BiLSTM's persistent recurrence lost
        co-residency (its logits are NaN); check=False defers that to status().
        forward_batch: windows per reference forward call when this call covers several of them (the
        pipeline's fused device batches): the scope of BatchNorm1D's NaN bypass (model.py:161-171).  0: this
        call is one batch.  A call of more than max_batch windows runs as several device forwards cut at
        reference-batch boundaries; a reference batch wider than max_batch is cut into device forwards that
        each learn (`_force`) whether a non-finite input sits anywhere in that batch, so the bypass keeps the
        reference's scope.
        With a Mamba2 back end (single_backend_type "mamba2") forward_batch is part of the model's function: the
        reference scans along the windows of each forward call (sdiar.h, sd_tsvad_config.backend), so the logits
        depend on which windows share a group and in which order; a group wider than max_batch is refused."""
        import torch
        T_lab = labels if isinstance(labels, int) else labels.size(-1)
        if self.cfg.waveform_input:
            # the WavLM speech encoders: ref_speech (B, n_samples) raw waveform, n_samples goes where T_fb does
            if ref_speech.dim() != 2:
                raise ValueError(f"{self.cfg.speech_encoder_type} expects the raw waveform (B, n_samples), got "
                                 f"{tuple(ref_speech.shape)}")
            B, T_fb = ref_speech.shape
            if self.cfg.variant == 8:
                from ..ssl.whisper import check_samples
                check_samples(self.cfg.effective_whisper_cfg(), T_fb)
        else:
            B, T_fb, F = ref_speech.shape
            assert F == self.cfg.n_mels, f"{self.cfg.speech_encoder_type} expects {self.cfg.n_mels}-dim fbank"
            if self.cfg.variant == 7 and T_fb % 2:
                # torch.reshape(ref_speech, (B, T // 2, 160)) of the reference (magicdata model.py:1228-1231)
                raise ValueError(f"w2v-bert2 needs an even number of fbank frames, got {T_fb}: the reference reshapes "
                                 f"(B, T, 80) to (B, T // 2, 160) and raises (shape '[{B}, {T_fb // 2}, 160]' is "
                                 f"invalid for input of size {B * T_fb * 80})")
        ref = ref_speech.to(self.device, torch.float32).contiguous()
        ts = target_speech.to(self.device, torch.float32).contiguous()
        assert ts.shape == (B, self.max_num_speaker, self.cfg.speaker_embed_dim)
        if out is None:
            out = torch.empty(B, self.max_num_speaker, T_lab, device=self.device, dtype=torch.float32)
        G = forward_batch if forward_batch > 0 else B
        if B > self.max_batch:
            if G <= self.max_batch:      # whole reference batches per device forward
                step = self.max_batch // G * G
                for s in range(0, B, step):
                    e = min(B, s + step)
                    self.forward(ref[s:e], ts[s:e], T_lab, out=out[s:e], check=False, forward_batch=G)
            elif self.cfg.mamba2_backend:
                raise ValueError(f"a Mamba2 back end scans over the {G} windows of a reference forward call: "
                                 f"create the model with max_batch >= {G} (it is {self.max_batch})")
            else:                        # a reference batch spans device forwards: its non-finite flags up front
                for g0 in range(0, B, G):
                    g1 = min(B, g0 + G)
                    force = 3 if not bool(torch.isfinite(ref[g0:g1]).all()) else 0
                    if self.cfg.variant != 1 and not bool(torch.isfinite(ts[g0:g1]).all()):
                        force |= 2
                    for s in range(g0, g1, self.max_batch):
                        e = min(g1, s + self.max_batch)
                        self.forward(ref[s:e], ts[s:e], T_lab, out=out[s:e], check=False, _force=force)
            if check:
                self.status()
            return out
        _lib.call("sd_tsvad_forward_batched", self._h, _lib.ptr(ref), _lib.ptr(ts), B, T_fb, T_lab,
                  int(forward_batch), int(_force), _lib.ptr(out), _lib.stream_ptr(self.device))
        if check:
            self.status()
        return out

    def status(self):
        """sd_tsvad_status: wait for the device stream, raise RuntimeError if a persistent LSTM
        recurrence of the forwards enqueued so far timed out."""
        _lib.call("sd_tsvad_status", self._h, _lib.stream_ptr(self.device))

    __call__ = forward

    # ------------------------------------------------------------------ infer (model.py:923-970)
    def infer(self, ref_speech, target_speech, labels, labels_len, num_updates: int = 0, file_path=None,
              speaker_ids=None, start=None):
        import torch
        outs = self.forward(ref_speech, target_speech, labels, num_updates)
        outs_prob = torch.sigmoid(outs).cpu().numpy()
        logits = outs.cpu().numpy().astype(np.float64)
        lab = labels.cpu().numpy().astype(np.float64)
        lens = np.asarray(labels_len.cpu() if hasattr(labels_len, "cpu") else labels_len)
        loss = 0.0
        for i in range(len(lens)):
            x, y = logits[i, :, : lens[i]], lab[i, :, : lens[i]]
            loss += np.mean(np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x))))
        result = {"losses": {"diar": loss / len(lens)}}
        mi, fa, cf, acc, der = calc_diarization_result(outs_prob.transpose((0, 2, 1)),
                                                        lab.transpose(0, 2, 1), lens)
        result.update(labels_len=labels_len, DER=der, ACC=acc, MI=mi, FA=fa, CF=cf)
        res_dict = defaultdict(lambda: defaultdict(list))
        B = outs_prob.shape[0]
        for b in range(B):
            n = max(speaker_ids[b])
            for t in range(int(lens[b])):
                for i in range(n):
                    res_dict[str(file_path[b]) + "-" + str(speaker_ids[b][i])][start[b] + t].append(outs_prob[b, i, t])
        return result, res_dict


def calc_diarization_error(pred, label, length):
    """model.py:973-1015 (EEND-style frame error counts), numpy."""
    batch_size, max_len, num_output = label.shape
    mask = np.zeros((batch_size, max_len, num_output))
    for i in range(batch_size):
        mask[i, : length[i], :] = 1
    label_np = label.astype(int) * mask
    pred_np = (pred > 0.5).astype(int) * mask
    n_ref = np.sum(label_np, axis=2)
    n_sys = np.sum(pred_np, axis=2)
    speech_scored = float(np.sum(n_ref > 0))
    speech_miss = float(np.sum(np.logical_and(n_ref > 0, n_sys == 0)))
    speech_falarm = float(np.sum(np.logical_and(n_ref == 0, n_sys > 0)))
    speaker_scored = float(np.sum(n_ref))
    speaker_miss = float(np.sum(np.maximum(n_ref - n_sys, 0)))
    speaker_falarm = float(np.sum(np.maximum(n_sys - n_ref, 0)))
    n_map = np.sum(np.logical_and(label_np == 1, pred_np == 1), axis=2)
    speaker_error = float(np.sum(np.minimum(n_ref, n_sys) - n_map))
    correct = float(1.0 * np.sum((label_np == pred_np) * mask) / num_output)
    num_frames = np.sum(length)
    return (correct, num_frames, speech_scored, speech_miss, speech_falarm, speaker_scored, speaker_miss,
            speaker_falarm, speaker_error)


def calc_diarization_result(outs_prob, labels, labels_len):
    """model.py:1018-1048."""
    (correct, num_frames, speech_scored, speech_miss, speech_falarm, speaker_scored, speaker_miss,
     speaker_falarm, speaker_error) = calc_diarization_error(outs_prob, labels, labels_len)
    if speech_scored == 0 or speaker_scored == 0:
        return 0, 0, 0, 0, 0
    return (speaker_miss / speaker_scored, speaker_falarm / speaker_scored, speaker_error / speaker_scored,
            correct / num_frames, (speaker_miss + speaker_falarm + speaker_error) / speaker_scored)
