"""WavLM (Base+ / Large) waveform feature extractor on the HIP path.

Mirrors `WavLM.extract_features` of the reference (egs/magicdata-ramc/ts_vad2/wavlm.py:359-414, with
ConvFeatureExtractionModel :434-556, TransformerEncoder :559-675, TransformerSentenceEncoderLayer :678-805 and
MultiheadAttention of modules.py:463-579) behind libsdiar's `sd_wavlm_*` handle: same config fields, same state_dict
keys (both weight-norm spellings of pos_conv), same return nesting.  Inference only: `mask=True` and `padding_mask`
are refused, and so is every configuration outside the two published geometries.
"""
from __future__ import annotations

from .. import _lib
from ..weights import unwrap_checkpoint

CONV_FEATURE_LAYERS = "[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2"
_CONV_LAYERS = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2
MIN_SAMPLES = 400


def num_frames(n_samples: int) -> int:
    """Output frames of the conv front end: 400..719 samples -> 1, 16000 -> 49, 64000 -> 199, 96000 -> 299."""
    n = int(n_samples)
    for _, k, s in _CONV_LAYERS:
        n = (n - k) // s + 1
    return n


class WavLMConfig:
    """wavlm.py:162-253: the fields the inference path reads, at the released checkpoints' values (Base+); `update`
    takes a checkpoint's `cfg` dict (fields of training-time masking and dropout are kept but not used)."""

    def __init__(self, cfg=None):
        self.extractor_mode = "default"
        self.encoder_layers = 12
        self.encoder_embed_dim = 768
        self.encoder_ffn_embed_dim = 3072
        self.encoder_attention_heads = 12
        self.activation_fn = "gelu"
        self.layer_norm_first = False
        self.conv_feature_layers = CONV_FEATURE_LAYERS
        self.conv_bias = False
        self.normalize = False
        self.conv_pos = 128
        self.conv_pos_groups = 16
        self.relative_position_embedding = True
        self.num_buckets = 320
        self.max_distance = 800
        self.gru_rel_pos = True
        if cfg is not None:
            self.update(cfg)

    def update(self, cfg: dict):
        self.__dict__.update(cfg)

    @staticmethod
    def large(**kw) -> "WavLMConfig":
        c = WavLMConfig(dict(extractor_mode="layer_norm", layer_norm_first=True, encoder_layers=24,
                             encoder_embed_dim=1024, encoder_ffn_embed_dim=4096, encoder_attention_heads=16,
                             normalize=True))
        c.update(kw)
        return c


def check_config(cfg: WavLMConfig):
    """ValueError naming the field for anything the HIP model does not build."""
    geom = (cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_attention_heads)
    if geom not in ((768, 3072, 12), (1024, 4096, 16)):
        raise ValueError("the MI355X WavLM builds (encoder_embed_dim, encoder_ffn_embed_dim, encoder_attention_heads) = "
                         f"(768, 3072, 12) or (1024, 4096, 16) only, got {geom}")
    if not (isinstance(cfg.encoder_layers, int) and 1 <= cfg.encoder_layers <= 24):
        raise ValueError(f"encoder_layers must be 1..24, got {cfg.encoder_layers}")
    # a checkpoint supplies this string: compared with the one accepted spelling (spaces aside), never evaluated
    layers = cfg.conv_feature_layers
    same = ("".join(layers.split()) == "".join(CONV_FEATURE_LAYERS.split()) if isinstance(layers, str)
            else [tuple(x) for x in layers] == _CONV_LAYERS)
    if not same:
        raise ValueError(f"conv_feature_layers must be {CONV_FEATURE_LAYERS}, got {layers}")
    for name, want in (("conv_bias", False), ("conv_pos", 128), ("conv_pos_groups", 16),
                       ("relative_position_embedding", True), ("gru_rel_pos", True), ("num_buckets", 320),
                       ("max_distance", 800), ("activation_fn", "gelu")):
        if getattr(cfg, name) != want:
            raise ValueError(f"the MI355X WavLM builds {name}={want!r} only, got {getattr(cfg, name)!r}")
    if (cfg.extractor_mode, bool(cfg.layer_norm_first)) not in (("default", False), ("layer_norm", True)):
        raise ValueError("the MI355X WavLM builds (extractor_mode, layer_norm_first) = ('default', False) or "
                         f"('layer_norm', True) only, got ({cfg.extractor_mode!r}, {cfg.layer_norm_first!r})")


class WavLM(_lib.Handle):
    """wavlm.py:256-305 run by libsdiar (`sd_wavlm_*`).  No waveform normalisation is applied (nor does the reference
    class apply one): a checkpoint with cfg.normalize expects the caller's layer-normed waveform."""
    kind = "wavlm"

    def __init__(self, cfg: WavLMConfig, *, device=None, precision: str = "bf16", max_batch: int = 64,
                 max_samples: int = 64000):
        check_config(cfg)
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision must be 0 or 1 (fp32 or bf16), got {precision}")
        if max_batch < 1 or max_samples < MIN_SAMPLES:
            raise ValueError(f"max_batch must be >= 1 and max_samples >= {MIN_SAMPLES}")
        self.cfg = cfg
        self.device = _lib.hip_device(device, "WavLM")
        self.precision, self.max_batch, self.max_samples = precision, max_batch, max_samples
        self.embed_dim = cfg.encoder_embed_dim
        self._create(_lib.WavlmConfig(
            embed_dim=cfg.encoder_embed_dim, ffn_dim=cfg.encoder_ffn_embed_dim, heads=cfg.encoder_attention_heads,
            encoder_layers=cfg.encoder_layers, extractor_mode=int(cfg.extractor_mode == "layer_norm"),
            layer_norm_first=int(bool(cfg.layer_norm_first)), max_batch=max_batch, max_samples=max_samples,
            precision=_lib.PRECISION[precision]))

    @classmethod
    def from_checkpoint(cls, checkpoint, **kw) -> "WavLM":
        """A released checkpoint's {"cfg": ..., "model": ...} (wavlm.py's loading recipe) -> a loaded model."""
        if not (isinstance(checkpoint, dict) and "cfg" in checkpoint and "model" in checkpoint):
            raise ValueError("expected a checkpoint dict with 'cfg' and 'model'")
        m = cls(WavLMConfig(checkpoint["cfg"]), **kw)
        return m.load_state_dict(checkpoint["model"])

    def load_state_dict(self, state_dict, strict: bool = True):
        if not strict:
            raise ValueError("the MI355X backend only supports strict=True loading")
        self._load(unwrap_checkpoint(state_dict, kind="wavlm"))
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

    def extract_features(self, source, padding_mask=None, mask: bool = False, ret_conv: bool = False,
                         output_layer=None, ret_layer_results: bool = False):
        """source (B, n_samples) -> (feature, None) (wavlm.py:359-414): feature is x (B, T, D), or the projected conv
        features with ret_conv, or (that, [(h, None), ...]) with ret_layer_results, h the (T, B, D) views of the input
        to layer 0 and of every layer's output up to output_layer (an empty list without output_layer)."""
        import torch
        if padding_mask is not None:
            raise ValueError("the MI355X WavLM does not build padding_mask (TS-VAD passes whole windows)")
        if mask:
            raise ValueError("the MI355X WavLM does not build mask=True (training-time masking)")
        if source.dim() != 2:
            raise ValueError(f"expected (B, n_samples) waveforms, got {tuple(source.shape)}")
        B, n = source.shape
        if n < MIN_SAMPLES:
            raise ValueError(f"n_samples must be at least {MIN_SAMPLES}, got {n}")
        if n > self.max_samples:
            raise ValueError(f"n_samples {n} exceeds max_samples {self.max_samples}")
        if B < 1 or B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        L = self.cfg.encoder_layers
        if output_layer is not None and not 1 <= int(output_layer) <= L:
            raise ValueError(f"output_layer must be 1..{L} (encoder_layers) or None, got {output_layer}")
        k = 0 if output_layer is None else int(output_layer)
        T, D = num_frames(n), self.embed_dim
        src = source.to(self.device, torch.float32).contiguous()
        want_x = not ret_conv
        x = torch.empty(B, T, D, device=self.device, dtype=torch.float32) if want_x else None
        feats = torch.empty(B, T, D, device=self.device, dtype=torch.float32) if ret_conv else None
        layers = (torch.empty(k + 1, B, T, D, device=self.device, dtype=torch.float32)
                  if ret_layer_results and k else None)
        _lib.call("sd_wavlm_forward", self._h, _lib.ptr(src), B, n, k, _lib.ptr(x), _lib.ptr(feats), _lib.ptr(layers),
                  _lib.stream_ptr(self.device))
        feature = feats if ret_conv else x
        if ret_layer_results:
            results = [] if layers is None else [(layers[i].transpose(0, 1), None) for i in range(k + 1)]
            feature = (feature, results)
        return feature, None
