"""Whisper-PMFA speech encoder on the HIP path.

Mirrors the reference's `WhisperEncoder` / `ModelDimensions` (egs/magicdata-ramc/ts_vad2/whisper_encoder.py:19-27,
150-244) in eval mode behind libsdiar's `sd_whisper_*` handle: the same config fields, the class's own state_dict keys
(not Hugging Face's), the same output.  The log-mel front end is restated from the published formula
(`whisper.log_mel_spectrogram` as torch.stft + the slaney mel matrix), not taken from the `whisper` package.
"""
from __future__ import annotations

from dataclasses import dataclass

from .. import _lib
from ..feature import whisper_mel_filters
from ..weights import unwrap_checkpoint

HOP = 160
MIN_SAMPLES = 400
MAX_WIDE = 16384


@dataclass
class WhisperConfig:
    """ModelDimensions (whisper_encoder.py:19-27) at the reference's defaults: the first 24 blocks of a whisper-large
    encoder, blocks 16..23 concatenated."""
    n_mels: int = 80
    n_audio_ctx: int = 1500
    n_audio_state: int = 1280
    n_audio_head: int = 20
    n_audio_layer: int = 24
    layer_st: int = 16
    layer_ed: int = 23

    @property
    def n_cat(self) -> int:
        return self.layer_ed - self.layer_st + 1

    @property
    def out_dim(self) -> int:
        return self.n_audio_state * self.n_cat


def check_config(cfg: WhisperConfig):
    """ValueError naming the field for anything the HIP model does not build."""
    for name in ("n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer", "layer_st", "layer_ed"):
        if not isinstance(getattr(cfg, name), int):
            raise ValueError(f"{name} must be an int, got {getattr(cfg, name)!r}")
    if cfg.n_mels not in (80, 128):
        raise ValueError(f"n_mels must be 80 or 128, got {cfg.n_mels}")
    if cfg.n_audio_ctx < 1:
        raise ValueError(f"n_audio_ctx must be positive, got {cfg.n_audio_ctx}")
    if cfg.n_audio_head < 1 or cfg.n_audio_state != 64 * cfg.n_audio_head:
        raise ValueError(f"n_audio_state must be 64 * n_audio_head (head size 64 only), got {cfg.n_audio_state} with "
                         f"n_audio_head {cfg.n_audio_head}")
    if cfg.n_audio_state % 32:
        raise ValueError(f"n_audio_state must be a multiple of 32, got {cfg.n_audio_state}")
    if not 1 <= cfg.n_audio_layer <= 32:
        raise ValueError(f"n_audio_layer must be 1..32, got {cfg.n_audio_layer}")
    if not 0 <= cfg.layer_st <= cfg.layer_ed:
        raise ValueError(f"layer_st must be 0..layer_ed, got {cfg.layer_st} with layer_ed {cfg.layer_ed}")
    if cfg.layer_ed >= cfg.n_audio_layer:
        raise ValueError(f"layer_ed must be below n_audio_layer, got {cfg.layer_ed}")
    if cfg.out_dim > MAX_WIDE:
        raise ValueError(f"n_audio_state * (layer_ed - layer_st + 1) must be at most {MAX_WIDE} (ln_post2's row), got "
                         f"{cfg.out_dim}")


def frames(n_samples: int) -> int:
    """T' of a window: F = n_samples // 160 mel frames through the stride-2 conv."""
    return (n_samples // HOP - 1) // 2 + 1


def check_samples(cfg: WhisperConfig, n_samples: int):
    """The input-length rules of the encoder (and of TS-VAD on it)."""
    if n_samples < MIN_SAMPLES:
        raise ValueError(f"n_samples must be at least {MIN_SAMPLES}, got {n_samples}")
    if frames(n_samples) > cfg.n_audio_ctx:
        raise ValueError(f"{n_samples} samples give {frames(n_samples)} frames, more than n_audio_ctx "
                         f"{cfg.n_audio_ctx}: the reference truncates there (whisper_encoder.py:225-227) and TS-VAD's "
                         "label-length assertion then fails")


class WhisperEncoder(_lib.Handle):
    """WhisperEncoder (whisper_encoder.py:150-244) run by libsdiar (`sd_whisper_*`)."""
    kind = "whisper"

    def __init__(self, cfg: WhisperConfig = None, *, device=None, precision: str = "bf16", max_batch: int = 64,
                 max_samples: int = 64000):
        cfg = cfg or WhisperConfig()
        check_config(cfg)
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision must be bf16 or fp32 (the Whisper encoder does not build bf16x3), got {precision}")
        if max_batch < 1 or max_samples < MIN_SAMPLES:
            raise ValueError(f"max_batch must be >= 1 and max_samples >= {MIN_SAMPLES}")
        self.cfg = cfg
        self.device = _lib.hip_device(device, "WhisperEncoder")
        self.precision, self.max_batch, self.max_samples = precision, max_batch, max_samples
        self._create(_lib.WhisperConfig(
            n_mels=cfg.n_mels, n_audio_ctx=cfg.n_audio_ctx, n_audio_state=cfg.n_audio_state,
            n_audio_head=cfg.n_audio_head, n_audio_layer=cfg.n_audio_layer, layer_st=cfg.layer_st,
            layer_ed=cfg.layer_ed, precision=_lib.PRECISION[precision], max_batch=max_batch, max_samples=max_samples))

    def load_state_dict(self, state_dict, strict: bool = True):
        if not strict:
            raise ValueError("the MI355X backend only supports strict=True loading")
        state = dict(unwrap_checkpoint(state_dict, kind="whisper"))
        if "mel_filters" in state:
            raise RuntimeError('Error(s) in loading state_dict: Unexpected key(s) in state_dict: "mel_filters"')
        state["mel_filters"] = whisper_mel_filters(self.cfg.n_mels)   # the front end's constant, not a reference key
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

    def forward(self, wavs):
        """wavs (B, n_samples) -> (B, T', n_audio_state * (layer_ed - layer_st + 1)) fp32."""
        import torch
        if wavs.dim() != 2:
            raise ValueError(f"expected (B, n_samples) wavs, got {tuple(wavs.shape)}")
        B, n = wavs.shape
        check_samples(self.cfg, n)
        if n > self.max_samples:
            raise ValueError(f"n_samples {n} exceeds max_samples {self.max_samples}")
        if B < 1 or B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        src = wavs.to(self.device, torch.float32).contiguous()
        out = torch.empty(B, frames(n), self.cfg.out_dim, device=self.device, dtype=torch.float32)
        _lib.call("sd_whisper_forward", self._h, _lib.ptr(src), B, n, _lib.ptr(out), _lib.stream_ptr(self.device))
        return out

    __call__ = forward
