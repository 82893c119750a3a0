"""Target-speaker embedding extraction on the MI355X path.

Drop-in for the step before TS-VAD inference:
  * `CAMPPlus` — egs/alimeeting/ts_vad2/cam_pplus_wespeaker.py:311-399 (same constructor
    arguments, same standalone state_dict keys, forward(x) -> (B, E) and
    forward(x, get_time_out=True) -> (B, 512, T')), run by libsdiar (`sd_campp_*`).
  * `ResNet34` — egs/alimeeting/ts_vad2/resnet_wespeaker.py:108-208 (speech_encoder=False): the WeSpeaker
    ResNet34 extractor of generate_chunk_speaker_embedding_from_wespeaker_for_diarization.py:116-133 (256-d
    embeddings, TSTP pooling + seg_1), run by libsdiar (`sd_resnet34_*`).
  * `ECAPA_TDNN_GLOB_c1024` — egs/alimeeting/ts_vad2/ecapa_tdnn_wespeaker.py:161-271: the WeSpeaker ECAPA-TDNN
    extractor of generate_chunk_speaker_embedding_from_ecapa_tdnn_for_diarization.py:95-172 (192-d embeddings,
    attentive statistics pooling with the global context), run by libsdiar (`sd_ecapa_*`); `extract_embed` drives
    any of the models.
  * `ERes2NetV2` — egs/alimeeting/ts_vad2/ERes2NetV2.py:162-255: the 3D-Speaker extractor of
    generate_chunk_speaker_embedding_from_modelscope_for_diarization.py:110-136 (192-d embeddings), run by libsdiar
    (`sd_eres2netv2_*`).
  * `FBank` — the extractor's FBank (generate_chunk_speaker_embedding_from_modelscope_for_
    diarization.py:307-331): kaldi fbank with the povey window, dither 0, no 2^15 scale,
    mean_nor over the chunk.
  * `extract_embed` — :271-304: 6 s chunks every 1 s (starts range(0, N - L, step)), or the
    whole file when it is not longer than one chunk; returns the (n_chunks, E) tensor the
    script `torch.save`s (:351).  The fbank is computed once per file and each chunk is a
    slice of it (chunk starts are whole frames: 16000 samples = 100 frames), then the
    per-chunk mean is subtracted on the device (`sd_window_cmn`).
  * `load_ts_embed` — TSVADDataset.load_alimeeting_ts_embed at inference
    (ts_vad_dataset.py:494-537): mean over chunks, zeros for speaker ids -1 / -2.
"""
from __future__ import annotations

import os

import numpy as np

from .. import _lib
from ..frontend import FRAME_LEN, FRAME_SHIFT, _mel_device, num_frames
from ..weights import unwrap_checkpoint

POVEY = 1


class CAMPPlus(_lib.Handle):
    kind = "campp"

    def __init__(self, feat_dim: int = 80, embedding_size: int = 192, growth_rate: int = 32, bn_size: int = 4,
                 init_channels: int = 128, config_str: str = "batchnorm-relu", memory_efficient: bool = True,
                 *, device=None, precision: str = "bf16", max_batch: int = 96, max_frames: int = 598):
        if (growth_rate, bn_size, init_channels, config_str) != (32, 4, 128, "batchnorm-relu"):
            raise ValueError("the MI355X CAM++ supports the shipped CAMPPlus topology only")
        code = _lib.precision_code(precision, ("bf16", "fp32"))
        self.device = _lib.hip_device(device, "CAMPPlus")
        self.feat_dim, self.embedding_size = feat_dim, embedding_size
        self.precision, self.max_batch, self.max_frames = precision, max_batch, max_frames
        self._create(_lib.CamppConfig(feat_dim=feat_dim, embedding_size=embedding_size, max_batch=max_batch,
                                      max_frames=max_frames, precision=code))

    def load_state_dict(self, state_dict, strict: bool = True):
        if not strict:
            raise ValueError("the MI355X backend only supports strict=True loading")
        self._load(unwrap_checkpoint(state_dict, kind="campp"))
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

    def forward(self, x, get_time_out: bool = False, out=None):
        """x (B, T, 80) -> (B, E), or (B, 512, (T-1)//2+1) with get_time_out (cam_pplus_wespeaker.py:388-399)."""
        import torch
        B, T, F = x.shape
        if F != self.feat_dim:
            raise ValueError(f"expected {self.feat_dim}-dim fbank, got {F}")
        x = x.to(self.device, torch.float32).contiguous()
        if B > self.max_batch:
            return torch.cat([self.forward(x[s:s + self.max_batch], get_time_out)
                              for s in range(0, B, self.max_batch)])
        st = _lib.stream_ptr(self.device)
        if get_time_out:
            t2 = (T - 1) // 2 + 1
            tout = torch.empty(B, t2, 512, device=self.device, dtype=torch.float32)
            _lib.call("sd_campp_forward", self._h, _lib.ptr(x), B, T, None, _lib.ptr(tout), st)
            return tout.permute(0, 2, 1)
        if out is None:
            out = torch.empty(B, self.embedding_size, device=self.device, dtype=torch.float32)
        _lib.call("sd_campp_forward", self._h, _lib.ptr(x), B, T, _lib.ptr(out), None, st)
        return out

    __call__ = forward


class ResNet34(_lib.Handle):
    """egs/alimeeting/ts_vad2/resnet_wespeaker.py:108-183, 198-208 with speech_encoder=False: the WeSpeaker
    ResNet34 embedding extractor (TSTP pooling + seg_1 [+ seg_bn_1 + seg_2]) run by libsdiar (`sd_resnet34_*`).
    Same constructor arguments and standalone state_dict keys; forward(x) -> (embed_a, embed_b), or
    (tensor(0.0), embed_a) without two_emb_layer; forward(x, get_time_out=True) -> (B, 2560, T').  The encoder-only
    form (speech_encoder=True) is TSVADModel's speech encoder, not this class."""
    kind = "resnet34"

    def __init__(self, feat_dim: int, embed_dim: int, pooling_func: str = "TSTP", two_emb_layer: bool = True,
                 speech_encoder: bool = False, *, device=None, precision: str = "bf16", max_batch: int = 96,
                 max_frames: int = 598):
        if pooling_func != "TSTP":
            raise ValueError(f"the MI355X ResNet34 builds TSTP pooling only, got {pooling_func}")
        if speech_encoder:
            raise ValueError("speech_encoder=True (no pooling head) is TSVADModel's resnet34_wespeaker speech encoder")
        code = _lib.precision_code(precision, ("bf16", "fp32"))
        self.device = _lib.hip_device(device, "ResNet34")
        self.feat_dim, self.embed_dim, self.two_emb_layer = feat_dim, embed_dim, bool(two_emb_layer)
        self.embedding_size = embed_dim      # what extract_embed sizes its output with
        self.precision, self.max_batch, self.max_frames = precision, max_batch, max_frames
        self._create(_lib.Resnet34Config(feat_dim=feat_dim, embed_dim=embed_dim,
                                         two_emb_layer=int(self.two_emb_layer), max_batch=max_batch,
                                         max_frames=max_frames, precision=code))

    def load_state_dict(self, state_dict, strict: bool = True):
        if not strict:
            raise ValueError("the MI355X backend only supports strict=True loading")
        self._load(unwrap_checkpoint(state_dict, kind="resnet34"))
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

    @staticmethod
    def out_frames(T: int) -> int:
        for _ in range(3):
            T = (T - 1) // 2 + 1
        return T

    def forward(self, x, get_time_out: bool = False, out=None):
        """x (B, T, 80) -> (embed_a, embed_b) / (tensor(0.0), embed_a) (resnet_wespeaker.py:176-183), or
        (B, 2560, T') with get_time_out (:165-171).  out: (B, embed_dim) destination of the last tuple element."""
        import torch
        B, T, F = x.shape
        if F != self.feat_dim:
            raise ValueError(f"expected {self.feat_dim}-dim fbank, got {F}")
        x = x.to(self.device, torch.float32).contiguous()
        if B > self.max_batch:
            parts = [self.forward(x[s:s + self.max_batch], get_time_out,
                                  None if out is None else out[s:s + self.max_batch])
                     for s in range(0, B, self.max_batch)]
            if get_time_out:
                return torch.cat(parts)
            first = torch.cat([p[0] for p in parts]) if self.two_emb_layer else parts[0][0]
            return first, (out if out is not None else torch.cat([p[1] for p in parts]))
        st = _lib.stream_ptr(self.device)
        if get_time_out:
            tout = torch.empty(B, self.out_frames(T), 2560, device=self.device, dtype=torch.float32)
            _lib.call("sd_resnet34_forward", self._h, _lib.ptr(x), B, T, None, None, _lib.ptr(tout), st)
            return tout.permute(0, 2, 1)
        if out is None:
            out = torch.empty(B, self.embed_dim, device=self.device, dtype=torch.float32)
        if not self.two_emb_layer:
            _lib.call("sd_resnet34_forward", self._h, _lib.ptr(x), B, T, _lib.ptr(out), None, None, st)
            return torch.tensor(0.0), out
        emb_a = torch.empty(B, self.embed_dim, device=self.device, dtype=torch.float32)
        _lib.call("sd_resnet34_forward", self._h, _lib.ptr(x), B, T, _lib.ptr(out), _lib.ptr(emb_a), None, st)
        return emb_a, out

    __call__ = forward


class SimAM_ResNet34_ASP(_lib.Handle):
    """egs/alimeeting/ts_vad2/samresnet_wespeaker.py:134-160 with speech_encoder=False: the WeSpeaker SimAM-ResNet34
    embedding extractor (SimAM BasicBlocks at 64/128/256/512 channels, ASP pooling, bottleneck) run by libsdiar
    (`sd_simam_resnet34_*`).  Same constructor arguments and standalone state_dict keys; forward(x) -> (B, embed_dim).
    The encoder-only form is not built: the reference's forward(x, get_time_out=True) raises NameError (:150 reads an
    undefined `out`), so there is no behaviour to reproduce."""
    kind = "simam_resnet34"
    _NO_TIME_OUT = ("the reference's SimAM_ResNet34_ASP.forward(x, get_time_out=True) raises NameError "
                    "(samresnet_wespeaker.py:150 reads an undefined `out`): the encoder-only form is not built")

    def __init__(self, in_planes: int = 64, embed_dim: int = 256, acoustic_dim: int = 80, dropout: float = 0,
                 speech_encoder: bool = False, *, device=None, precision: str = "bf16", max_batch: int = 96,
                 max_frames: int = 598):
        if speech_encoder:
            raise ValueError("speech_encoder=True builds no pooling head, and " + self._NO_TIME_OUT)
        if in_planes != 64:
            raise ValueError(f"the MI355X SimAM_ResNet34_ASP supports in_planes 64 only, got {in_planes}")
        if acoustic_dim != 80:
            raise ValueError(f"the MI355X SimAM_ResNet34_ASP supports acoustic_dim 80 only, got {acoustic_dim}")
        if dropout:
            raise ValueError("the MI355X SimAM_ResNet34_ASP is inference only (dropout 0, the extractor script's setting)")
        code = _lib.precision_code(precision, ("bf16", "fp32"))
        self.device = _lib.hip_device(device, "SimAM_ResNet34_ASP")
        self.in_planes, self.embed_dim, self.acoustic_dim = in_planes, embed_dim, acoustic_dim
        self.feat_dim = acoustic_dim
        self.embedding_size = embed_dim      # what extract_embed sizes its output with
        self.precision, self.max_batch, self.max_frames = precision, max_batch, max_frames
        self._create(_lib.SimamResnet34Config(in_planes=in_planes, embed_dim=embed_dim, acoustic_dim=acoustic_dim,
                                              max_batch=max_batch, max_frames=max_frames, precision=code))

    def load_state_dict(self, state_dict, strict: bool = True):
        if not strict:
            raise ValueError("the MI355X backend only supports strict=True loading")
        self._load(unwrap_checkpoint(state_dict, kind="simam_resnet34"))
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

    out_frames = staticmethod(ResNet34.out_frames)

    def forward(self, x, get_time_out: bool = False, out=None):
        """x (B, T, 80) -> (B, embed_dim) (samresnet_wespeaker.py:156-160).  T >= 8 (ValueError below: the trunk's
        kernels are exercised from 8 frames on); T == 8 gives one pooled frame and finite embeddings."""
        import torch
        if get_time_out:
            raise ValueError(self._NO_TIME_OUT)
        B, T, F = x.shape
        if F != self.feat_dim:
            raise ValueError(f"expected {self.feat_dim}-dim fbank, got {F}")
        if T < 8:
            raise ValueError(f"SimAM_ResNet34_ASP needs at least 8 fbank frames, got {T}")
        x = x.to(self.device, torch.float32).contiguous()
        if B > self.max_batch:
            parts = [self.forward(x[s:s + self.max_batch], out=None if out is None else out[s:s + self.max_batch])
                     for s in range(0, B, self.max_batch)]
            return out if out is not None else torch.cat(parts)
        if out is None:
            out = torch.empty(B, self.embed_dim, device=self.device, dtype=torch.float32)
        _lib.call("sd_simam_resnet34_forward", self._h, _lib.ptr(x), B, T, _lib.ptr(out), None,
                  _lib.stream_ptr(self.device))
        return out

    __call__ = forward

    def front(self, x):
        """x (B, T, 80) -> the front's map (B, 5120, T') as ASP.forward flattens it (pooling_layers_wespeaker.py:162),
        channel c * 10 + f: what the pooling head reads (tests and diagnostics)."""
        import torch
        B, T, F = x.shape
        if F != self.feat_dim or T < 8 or B > self.max_batch:
            raise ValueError("front: (B <= max_batch, T >= 8, 80) fbank expected")
        x = x.to(self.device, torch.float32).contiguous()
        fo = torch.empty(B, self.out_frames(T), 5120, device=self.device, dtype=torch.float32)
        _lib.call("sd_simam_resnet34_forward", self._h, _lib.ptr(x), B, T, None, _lib.ptr(fo),
                  _lib.stream_ptr(self.device))
        return fo.permute(0, 2, 1)


class ERes2NetV2(_lib.Handle):
    """egs/alimeeting/ts_vad2/ERes2NetV2.py:162-255: the 3D-Speaker ERes2NetV2 embedding extractor (Res2Net blocks with
    Hardtanh(0, 20), AFF gates in layers 3-4, layer3_ds + fuse34, TSTP with eps 1e-8, seg_1) run by libsdiar
    (`sd_eres2netv2_*`).  Same constructor arguments and state_dict keys; forward(x) -> (B, embedding_size), and the two
    frame-level outputs of egs/magicdata-ramc/ots_vad/ERes2NetV2.py.  Built at (baseWidth, scale, expansion) = (26, 2, 2)
    (the class default) and (24, 4, 4) (iic/speech_eres2netv2w24s4ep4_sv_zh-cn_16k-common,
    generate_chunk_speaker_embedding_from_modelscope_for_diarization.py:110-136)."""
    kind = "eres2netv2"
    TRIPLES = ((26, 2, 2), (24, 4, 4))

    def __init__(self, feat_dim: int = 80, embedding_size: int = 192, m_channels: int = 64, baseWidth: int = 26,
                 scale: int = 2, expansion: int = 2, pooling_func: str = "TSTP", two_emb_layer: bool = False,
                 *, device=None, precision: str = "bf16", max_batch: int = 96, max_frames: int = 598):
        if two_emb_layer:
            raise ValueError("the MI355X ERes2NetV2 builds two_emb_layer=False only (the extractor's setting)")
        if pooling_func != "TSTP":
            raise ValueError(f"the MI355X ERes2NetV2 builds TSTP pooling only, got {pooling_func}")
        if (baseWidth, scale, expansion) not in self.TRIPLES:
            raise ValueError("the MI355X ERes2NetV2 builds (baseWidth, scale, expansion) = (26, 2, 2) or (24, 4, 4) only, "
                             f"got {(baseWidth, scale, expansion)}")
        if feat_dim != 80:
            raise ValueError(f"the MI355X ERes2NetV2 supports feat_dim 80 only, got {feat_dim}")
        if m_channels != 64:
            raise ValueError(f"the MI355X ERes2NetV2 supports m_channels 64 only, got {m_channels}")
        code = _lib.precision_code(precision, ("bf16", "fp32"))
        self.device = _lib.hip_device(device, "ERes2NetV2")
        self.feat_dim, self.embedding_size, self.m_channels = feat_dim, embedding_size, m_channels
        self.baseWidth, self.scale, self.expansion = baseWidth, scale, expansion
        self.frame_channels = 5120 * expansion     # 512 e x 10 rows, and 256 e x 20 rows
        self.precision, self.max_batch, self.max_frames = precision, max_batch, max_frames
        self._create(_lib.Eres2netv2Config(feat_dim=feat_dim, embedding_size=embedding_size, m_channels=m_channels,
                                           base_width=baseWidth, scale=scale, expansion=expansion,
                                           max_batch=max_batch, max_frames=max_frames, precision=code))

    def load_state_dict(self, state_dict, strict: bool = True):
        if not strict:
            raise ValueError("the MI355X backend only supports strict=True loading")
        self._load(unwrap_checkpoint(state_dict, kind="eres2netv2"))
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

    out_frames = staticmethod(ResNet34.out_frames)

    @staticmethod
    def frames25(T: int) -> int:
        for _ in range(2):
            T = (T - 1) // 2 + 1
        return T

    def _input(self, x):
        import torch
        B, T, F = x.shape
        if F != self.feat_dim:
            raise ValueError(f"expected {self.feat_dim}-dim fbank, got {F}")
        if T < 8:
            raise ValueError(f"ERes2NetV2 needs at least 8 fbank frames, got {T}")
        return x.to(self.device, torch.float32).contiguous()

    def forward(self, x, out=None):
        """x (B, T, 80) -> (B, embedding_size) (ERes2NetV2.py:236-255).  T >= 8; T == 8 pools one frame and gives the
        reference's all-NaN embedding (the unbiased variance of one frame)."""
        import torch
        x = self._input(x)
        B, T, _ = x.shape
        if B > self.max_batch:
            parts = [self.forward(x[s:s + self.max_batch], out=None if out is None else out[s:s + self.max_batch])
                     for s in range(0, B, self.max_batch)]
            return out if out is not None else torch.cat(parts)
        if out is None:
            out = torch.empty(B, self.embedding_size, device=self.device, dtype=torch.float32)
        _lib.call("sd_eres2netv2_forward", self._h, _lib.ptr(x), B, T, _lib.ptr(out), None, None,
                  _lib.stream_ptr(self.device))
        return out

    __call__ = forward

    def _frames(self, x, which: int):
        import torch
        x = self._input(x)
        B, T, _ = x.shape
        if B > self.max_batch:
            return torch.cat([self._frames(x[s:s + self.max_batch], which) for s in range(0, B, self.max_batch)])
        Tn = self.out_frames(T) if which == 0 else self.frames25(T)
        fo = torch.empty(B, Tn, self.frame_channels, device=self.device, dtype=torch.float32)
        _lib.call("sd_eres2netv2_forward", self._h, _lib.ptr(x), B, T, None, _lib.ptr(fo) if which == 0 else None,
                  _lib.ptr(fo) if which == 1 else None, _lib.stream_ptr(self.device))
        return fo.permute(0, 2, 1)

    def get_frame_level_feat(self, x):
        """x (B, T, 80) -> the fuse34 map (B, 5120 e, T'), channel f * C + c (ots_vad/ERes2NetV2.py:253-258)."""
        return self._frames(x, 0)

    def get_frame_level_feat_frame_rate25(self, x):
        """x (B, T, 80) -> out3 (B, 5120 e, T3), channel f * C + c (ots_vad/ERes2NetV2.py:259-272)."""
        return self._frames(x, 1)


class ECAPA_TDNN_GLOB_c1024(_lib.Handle):
    """egs/alimeeting/ts_vad2/ecapa_tdnn_wespeaker.py:161-254, 264-271 with speech_encoder=False: ECAPA-TDNN at 1024
    channels with global-context ASTP, bn and linear, run by libsdiar (`sd_ecapa_*`).  Same constructor arguments and
    standalone state_dict keys; forward(x) -> (B, embed_dim), forward(x, get_time_out=True) -> (B, 1536, T).  The
    encoder-only form (speech_encoder=True) is TSVADModel's speech encoder, not this class."""
    kind = "ecapa"

    def __init__(self, feat_dim: int = 80, embed_dim: int = 192, pooling_func: str = "ASTP", emb_bn: bool = False,
                 speech_encoder: bool = False, *, device=None, precision: str = "bf16", max_batch: int = 96,
                 max_frames: int = 598):
        if pooling_func != "ASTP":
            raise ValueError(f"the MI355X ECAPA-TDNN builds ASTP pooling only, got {pooling_func}")
        if emb_bn:
            raise ValueError("the MI355X ECAPA-TDNN builds emb_bn=False only (the extractor script's setting)")
        if speech_encoder:
            raise ValueError("speech_encoder=True (no pooling head) is TSVADModel's ecapa_channel_1024_wespeaker "
                             "speech encoder")
        if feat_dim != 80:
            raise ValueError(f"the MI355X ECAPA-TDNN supports feat_dim 80 only, got {feat_dim}")
        code = _lib.precision_code(precision, ("bf16", "fp32"))
        self.device = _lib.hip_device(device, "ECAPA_TDNN_GLOB_c1024")
        self.feat_dim, self.embed_dim = feat_dim, embed_dim
        self.embedding_size = embed_dim      # what extract_embed sizes its output with
        self.precision, self.max_batch, self.max_frames = precision, max_batch, max_frames
        self._create(_lib.EcapaConfig(channels=1024, embed_dim=embed_dim, max_batch=max_batch, max_frames=max_frames,
                                      precision=code))

    def load_state_dict(self, state_dict, strict: bool = True):
        if not strict:
            raise ValueError("the MI355X backend only supports strict=True loading")
        self._load(unwrap_checkpoint(state_dict, kind="ecapa"))
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

    def forward(self, x, get_time_out: bool = False, out=None):
        """x (B, T, 80) -> (B, embed_dim) (ecapa_tdnn_wespeaker.py:250-254), or (B, 1536, T) with get_time_out
        (:247-249).  Embeddings need T >= 2 (AssertionError otherwise: the reference's are NaN there)."""
        import torch
        B, T, F = x.shape
        if F != self.feat_dim:
            raise ValueError(f"expected {self.feat_dim}-dim fbank, got {F}")
        x = x.to(self.device, torch.float32).contiguous()
        if B > self.max_batch:
            parts = [self.forward(x[s:s + self.max_batch], get_time_out,
                                  None if out is None else out[s:s + self.max_batch])
                     for s in range(0, B, self.max_batch)]
            return out if (out is not None and not get_time_out) else torch.cat(parts)
        st = _lib.stream_ptr(self.device)
        if get_time_out:
            tout = torch.empty(B, T, 1536, device=self.device, dtype=torch.float32)
            _lib.call("sd_ecapa_forward", self._h, _lib.ptr(x), B, T, None, _lib.ptr(tout), st)
            return tout.permute(0, 2, 1)
        if out is None:
            out = torch.empty(B, self.embed_dim, device=self.device, dtype=torch.float32)
        _lib.call("sd_ecapa_forward", self._h, _lib.ptr(x), B, T, _lib.ptr(out), None, st)
        return out

    __call__ = forward

    def pooled_stats(self, B: int):
        """The pre-bn ASTP statistics (B, 3072) [mean | std] of the last forward that returned embeddings."""
        import ctypes
        import torch
        p = ctypes.c_void_p()
        _lib.call("sd_ecapa_debug_stats", self._h, ctypes.byref(p))
        out = torch.empty(B, 3072, device=self.device, dtype=torch.float32)
        torch.cuda.current_stream(self.device).synchronize()
        rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(out.data_ptr()), p, ctypes.c_size_t(out.numel() * 4), 3)
        if rc != 0:
            raise _lib.SdiarError("copy of the ASTP statistics failed")
        return out


class ReDimNetB2(_lib.Handle):
    """egs/magicdata-ramc/ts_vad2/redimnet_wespeaker.py:925-948 (ReDimNet :793-872): the WeSpeaker ReDimNetB2 embedding
    extractor (stem, six stages of ConvNeXt-like 2-D blocks and a conv + attention time-context block on a (B, T, 1152)
    map that is never subsampled, ASTP with the global context, seg_1) run by libsdiar (`sd_redimnet_*`).  Same
    constructor arguments and state_dict keys; forward(x) -> (tensor(0.0), embed_a), the reference's pair;
    get_frame_level_feat(x) -> (B, T, 1152).  Use with extract_embed(..., n_mels=72).  Deviation: forward with T < 2
    raises (AssertionError) where the reference returns a non-finite embedding; get_frame_level_feat works from T = 1."""
    kind = "redimnet"

    def __init__(self, feat_dim: int = 72, embed_dim: int = 192, pooling_func: str = "ASTP", two_emb_layer: bool = False,
                 *, device=None, precision: str = "bf16", max_batch: int = 96, max_frames: int = 598):
        if feat_dim != 72:
            raise ValueError(f"the MI355X ReDimNetB2 supports feat_dim 72 only, got {feat_dim}")
        if pooling_func != "ASTP":
            raise ValueError(f"the MI355X ReDimNetB2 builds ASTP pooling only, got {pooling_func}")
        if two_emb_layer:
            raise ValueError("the MI355X ReDimNetB2 builds two_emb_layer=False only (the extractor's setting)")
        code = _lib.precision_code(precision)
        self.device = _lib.hip_device(device, "ReDimNetB2")
        self.feat_dim, self.embed_dim, self.two_emb_layer = feat_dim, embed_dim, False
        self.embedding_size = embed_dim      # what extract_embed sizes its output with
        self.precision, self.max_batch, self.max_frames = precision, max_batch, max_frames
        self._create(_lib.RedimnetConfig(feat_dim=feat_dim, embed_dim=embed_dim, max_batch=max_batch,
                                         max_frames=max_frames, precision=code))

    def load_state_dict(self, state_dict, strict: bool = True):
        if not strict:
            raise ValueError("the MI355X backend only supports strict=True loading")
        self._load(unwrap_checkpoint(state_dict, kind="redimnet"))
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

    def _input(self, x):
        import torch
        if x.dim() != 3 or x.shape[2] != self.feat_dim:
            raise ValueError(f"expected (B, T, {self.feat_dim}) fbank, got {tuple(x.shape)}")
        return x.to(self.device, torch.float32).contiguous()

    def forward(self, x, out=None):
        """x (B, T, 72) -> (tensor(0.0), embed_a (B, embed_dim)) (redimnet_wespeaker.py:861-872).  T >= 2."""
        import torch
        if x.dim() == 3 and x.shape[1] < 2:
            raise AssertionError("ReDimNetB2 embeddings need at least 2 fbank frames (ASTP's unbiased variance of one "
                                 "frame is NaN)")
        x = self._input(x)
        B, T, _ = x.shape
        if B > self.max_batch:
            parts = [self.forward(x[s:s + self.max_batch], None if out is None else out[s:s + self.max_batch])[1]
                     for s in range(0, B, self.max_batch)]
            return torch.tensor(0.0), (out if out is not None else torch.cat(parts))
        if out is None:
            out = torch.empty(B, self.embed_dim, device=self.device, dtype=torch.float32)
        _lib.call("sd_redimnet_forward", self._h, _lib.ptr(x), B, T, _lib.ptr(out), None, _lib.stream_ptr(self.device))
        return torch.tensor(0.0), out

    __call__ = forward

    def get_frame_level_feat(self, x):
        """x (B, T, 72) -> (B, T, 1152), channel f * c + ch (redimnet_wespeaker.py:855-859)."""
        import torch
        x = self._input(x)
        B, T, _ = x.shape
        if B > self.max_batch:
            return torch.cat([self.get_frame_level_feat(x[s:s + self.max_batch]) for s in range(0, B, self.max_batch)])
        fo = torch.empty(B, T, 1152, device=self.device, dtype=torch.float32)
        _lib.call("sd_redimnet_forward", self._h, _lib.ptr(x), B, T, None, _lib.ptr(fo), _lib.stream_ptr(self.device))
        return fo

    def use_generic_blocks(self, on: bool):
        """Tests and tools/redimnet_probe.py: run the 2-D blocks of a bf16 model as the generic arm."""
        _lib.call("sd_redimnet_debug_generic", self._h, int(bool(on)))
        return self


def kaldi_fbank_povey(wav, n_mels: int = 80, out=None):
    """Kaldi.fbank(wav, num_mel_bins, sample_frequency=16000, dither=0) (povey window,
    samples as read, no 2^15 scale): 1-D float32 CUDA tensor -> (n_frames, n_mels)."""
    import torch
    assert wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 1
    n = num_frames(wav.numel())
    if out is None:
        out = torch.empty(n, n_mels, device=wav.device, dtype=torch.float32)
    fb = _mel_device(n_mels, wav.device)
    _lib.call("sd_fbank_kaldi_ex", _lib.ptr(wav.contiguous()), wav.numel(), 1.0, n, _lib.ptr(fb), n_mels, POVEY,
              _lib.ptr(out), _lib.stream_ptr(wav.device))
    return out


class FBank:
    """generate_chunk_..._for_diarization.py:307-331 (16 kHz only, as the reference asserts)."""

    def __init__(self, n_mels: int, sample_rate: int, mean_nor: bool = False):
        self.n_mels, self.sample_rate, self.mean_nor = n_mels, sample_rate, mean_nor

    def __call__(self, wav, dither=0):
        import torch
        assert self.sample_rate == 16000
        if dither != 0:
            raise ValueError("the MI355X fbank is deterministic (dither 0, the extractor's default)")
        if wav.dim() == 2:
            wav = wav[0]
        feat = kaldi_fbank_povey(wav.to(torch.float32).contiguous(), self.n_mels)
        if self.mean_nor:
            feat = feat - feat.mean(0, keepdim=True)
        return feat


def embedding_chunks(n_samples: int, length_embedding: float = 6.0, step_embedding: float = 1.0,
                     sample_rate: int = 16000):
    """[(start, stop)] of extract_embed (:274-299)."""
    L, S = int(length_embedding * sample_rate), int(step_embedding * sample_rate)
    if n_samples > L:
        return [(s, s + L) for s in range(0, n_samples - L, S)]
    return [(0, n_samples)]


def extract_embed(wav, model, length_embedding: float = 6.0, step_embedding: float = 1.0,
                  batch_size: int = 96, n_mels: int = 80):
    """wav: 1-D float samples in [-1, 1) (numpy or tensor; soundfile values cast to float32
    like torch.FloatTensor at :283) -> (n_chunks, E) float32 embeddings on the model device.
    model: CAMPPlus, ResNet34 (generate_chunk_speaker_embedding_from_wespeaker_for_diarization.py:143-176, the
    same chunk loop; the last element of the model's tuple is kept, :132-133), ECAPA_TDNN_GLOB_c1024
    (generate_chunk_speaker_embedding_from_ecapa_tdnn_for_diarization.py:142-172, the same loop again) or ERes2NetV2 (the
    modelscope script's own entry, :110-136, through the loop at :271-304).  A file too short for ResNet34's
    three stride-2 stages (at most 8 fbank frames) yields the reference's all-NaN embedding."""
    import torch
    dev = model.device
    w = torch.as_tensor(np.asarray(wav) if not isinstance(wav, torch.Tensor) else wav)
    w = w.to(dev, torch.float32).contiguous()
    chunks = embedding_chunks(w.numel(), length_embedding, step_embedding)
    if any(a % FRAME_SHIFT for a, _ in chunks):
        raise ValueError("chunk starts must be whole fbank frames (step_embedding * 16000 % 160 == 0)")
    if isinstance(model, CAMPPlus) and num_frames(chunks[0][1] - chunks[0][0]) < 8:
        raise ValueError("audio shorter than CAM++'s minimum of 8 fbank frames")
    feats = kaldi_fbank_povey(w, n_mels)
    nf = num_frames(chunks[0][1] - chunks[0][0])           # every chunk has the same length
    starts = torch.tensor([a // FRAME_SHIFT for a, _ in chunks], dtype=torch.int32, device=dev)
    lens = torch.full((len(chunks),), nf, dtype=torch.int32, device=dev)
    win = torch.empty(len(chunks), nf, n_mels, device=dev, dtype=torch.float32)
    _lib.call("sd_window_cmn", _lib.ptr(feats), n_mels, _lib.ptr(starts), _lib.ptr(lens), len(chunks), nf,
              _lib.ptr(win), _lib.stream_ptr(dev))
    out = torch.empty(len(chunks), model.embedding_size, device=dev, dtype=torch.float32)
    step = min(batch_size, model.max_batch)
    for s in range(0, len(chunks), step):
        model.forward(win[s:s + step], out=out[s:s + step])
    return out


def load_ts_embed(spk_path: str, file: str, speaker_ids, speaker_embed_dim: int = 192):
    """TSVADDataset.load_alimeeting_ts_embed at inference (ts_vad_dataset.py:494-537, is_train
    False): <spk_path>/<file>/<id>.pt, (n_chunks, E) averaged over chunks; -1 / -2 -> zeros.
    Loads with weights_only=True (the files hold one tensor)."""
    import torch
    feats = []
    for sid in speaker_ids:
        if sid in (-1, -2):
            feats.append(torch.zeros(speaker_embed_dim))
            continue
        f = torch.load(os.path.join(spk_path, file, f"{sid}.pt"), map_location="cpu", weights_only=True)
        feats.append(f.mean(dim=0) if f.dim() == 2 else f)
    return torch.stack(feats)
