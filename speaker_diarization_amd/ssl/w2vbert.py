"""w2v-BERT 2.0 speech encoder (the relative-key Conformer) on the HIP path.

Mirrors transformers' `Wav2Vec2BertModel` in eval mode as the reference builds it for TS-VAD
(egs/magicdata-ramc/ts_vad2/model.py:805-840: `Wav2Vec2BertConfig.from_pretrained(..., hidden_act="swish")` with
`num_hidden_layers` cut to `select_encoder_layer_nums`) behind libsdiar's `sd_w2vbert_*` handle: the same config
fields, the same state_dict keys, the same outputs.  Inference only: `attention_mask`, masking, the adapter and the
rotary / `relative` position types are refused, and so is every geometry but the published one.
"""
from __future__ import annotations

from collections import namedtuple

from .. import _lib
from ..weights import unwrap_checkpoint

IN_DIM = 160

W2vBertOutput = namedtuple("W2vBertOutput", ["last_hidden_state", "hidden_states"])


class W2vBertConfig:
    """The fields of transformers' Wav2Vec2BertConfig that the inference path reads, at the published values of
    w2v-BERT 2.0 (facebook/w2v-bert-2.0's config.json; hidden_act as the reference overrides it); `update` takes a
    config.json's dict (training-time fields are kept but not used)."""

    def __init__(self, cfg=None, **kw):
        self.hidden_size = 1024
        self.num_hidden_layers = 24
        self.num_attention_heads = 16
        self.intermediate_size = 4096
        self.feature_projection_input_dim = IN_DIM
        self.hidden_act = "swish"
        self.position_embeddings_type = "relative_key"
        self.left_max_position_embeddings = 64
        self.right_max_position_embeddings = 8
        self.conv_depthwise_kernel_size = 31
        self.layer_norm_eps = 1e-5
        self.add_adapter = False
        self.use_intermediate_ffn_before_adapter = False
        self.output_hidden_size = 1024
        if cfg is not None:
            self.update(cfg)
        self.update(kw)

    def update(self, cfg: dict):
        self.__dict__.update(cfg)


def check_config(cfg: W2vBertConfig):
    """ValueError naming the field for anything the HIP model does not build."""
    for name, want in (("hidden_size", 1024), ("num_attention_heads", 16), ("intermediate_size", 4096),
                       ("feature_projection_input_dim", IN_DIM), ("hidden_act", "swish"),
                       ("position_embeddings_type", "relative_key"), ("left_max_position_embeddings", 64),
                       ("right_max_position_embeddings", 8), ("conv_depthwise_kernel_size", 31),
                       ("layer_norm_eps", 1e-5), ("add_adapter", False),
                       ("use_intermediate_ffn_before_adapter", False), ("output_hidden_size", 1024)):
        if getattr(cfg, name) != want:
            raise ValueError(f"the MI355X w2v-BERT 2.0 builds {name}={want!r} only, got {getattr(cfg, name)!r}")
    if not (isinstance(cfg.num_hidden_layers, int) and 1 <= cfg.num_hidden_layers <= 24):
        raise ValueError(f"num_hidden_layers must be 1..24, got {cfg.num_hidden_layers}")


class W2vBert(_lib.Handle):
    """Wav2Vec2BertModel (modeling_wav2vec2_bert.py:923-1050) run by libsdiar (`sd_w2vbert_*`)."""
    kind = "w2vbert"

    def __init__(self, cfg: W2vBertConfig = None, *, device=None, precision: str = "bf16", max_batch: int = 64,
                 max_frames: int = 200):
        cfg = cfg or W2vBertConfig()
        check_config(cfg)
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision must be 0 or 1 (fp32 or bf16), got {precision}")
        if max_batch < 1 or max_frames < 1:
            raise ValueError("max_batch and max_frames must be >= 1")
        self.cfg = cfg
        self.device = _lib.hip_device(device, "W2vBert")
        self.precision, self.max_batch, self.max_frames = precision, max_batch, max_frames
        self.hidden_size = cfg.hidden_size
        self._create(_lib.W2vbertConfig(
            hidden=cfg.hidden_size, heads=cfg.num_attention_heads, ffn=cfg.intermediate_size,
            layers=cfg.num_hidden_layers, conv_kernel=cfg.conv_depthwise_kernel_size,
            left=cfg.left_max_position_embeddings, right=cfg.right_max_position_embeddings,
            in_dim=cfg.feature_projection_input_dim, precision=_lib.PRECISION[precision], max_batch=max_batch,
            max_frames=max_frames, position_embeddings=0, add_adapter=0))

    def load_state_dict(self, state_dict, strict: bool = True):
        if not strict:
            raise ValueError("the MI355X backend only supports strict=True loading")
        self._load(unwrap_checkpoint(state_dict, kind="w2vbert"))
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

    def forward(self, input_features, attention_mask=None, mask_time_indices=None, output_hidden_states: bool = False):
        """input_features (B, T2, 160) -> last_hidden_state (B, T2, 1024); with output_hidden_states the HF model's
        pair (last_hidden_state, hidden_states), hidden_states the tuple of the input to layer 0 and every layer's
        output."""
        import torch
        if attention_mask is not None:
            raise ValueError("the MI355X w2v-BERT 2.0 does not build attention_mask (TS-VAD passes whole windows)")
        if mask_time_indices is not None:
            raise ValueError("the MI355X w2v-BERT 2.0 does not build mask_time_indices (training-time masking)")
        if input_features.dim() != 3 or input_features.shape[2] != IN_DIM:
            raise ValueError(f"expected (B, T2, {IN_DIM}) input_features, got {tuple(input_features.shape)}")
        B, T2, _ = input_features.shape
        if T2 < 1 or T2 > self.max_frames:
            raise ValueError(f"frames {T2} exceed max_frames {self.max_frames}")
        if B < 1 or B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        L, D = self.cfg.num_hidden_layers, self.hidden_size
        src = input_features.to(self.device, torch.float32).contiguous()
        x = torch.empty(B, T2, D, device=self.device, dtype=torch.float32)
        layers = torch.empty(L + 1, B, T2, D, device=self.device, dtype=torch.float32) if output_hidden_states else None
        _lib.call("sd_w2vbert_forward", self._h, _lib.ptr(src), B, T2, _lib.ptr(x), _lib.ptr(layers),
                  _lib.stream_ptr(self.device))
        if output_hidden_states:
            return W2vBertOutput(x, tuple(layers[i] for i in range(L + 1)))
        return x

    __call__ = forward
