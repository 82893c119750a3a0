"""State-dict layouts of the reference models and seeded synthetic weights.

No trained checkpoints exist offline, so benchmarks and parity tests use
seeded random weights laid out under the reference's exact key names (the
golden-vector script loads them into the reference modules with strict=True,
which pins the key set).  Checkpoint loading mirrors the reference loaders:
TS-VAD `{"model": state_dict}` (ts_vad2/infer.py:184), EEND bare state_dict
(eend_eda/infer_eda.py:88), FS-EEND Lightning `state_dict` with a `model.`
prefix (fs_eend/train.py:183-191).
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

Shape = Tuple[int, ...]


# ----------------------------------------------------------------------------- TS-VAD
# (speech_encoder_type, single_backend_type, multi_backend_type) -> sd_tsvad_config.backend of the Mamba2 back ends.
# Mamba v1 ("mamba", "mamba_v2"), "mamba2_unidirectional" and mamba2 behind another speech encoder are not built.
_MAMBA2_BACKENDS = {("CAM++", "mamba2", "transformer"): 1, ("CAM++", "mamba2", "mamba2"): 2,
                    ("CAM++_frame_level_gsp_fc", "mamba2", "transformer"): 1,
                    ("CAM++_frame_level_gsp_fc", "mamba2", "mamba2"): 2}
MAMBA2_HEADDIM = 64   # mamba_ssm Mamba2's headdim default
# The conformer back ends (egs/magicdata-ramc/ts_vad2/model.py:290-313, 451-463): torchaudio.models.Conformer with a
# BatchNorm conv module, along time.  The reference's recipes pair them with CAM++ only and never run a transformer
# single back end in front of a conformer multi one.
_CONFORMER_BACKENDS = {("CAM++", "conformer", "transformer"): 4, ("CAM++", "conformer", "conformer"): 5,
                       ("CAM++_frame_level_gsp_fc", "conformer", "transformer"): 4,
                       ("CAM++_frame_level_gsp_fc", "conformer", "conformer"): 5}
# "CAM++_frame_level_gsp_fc" (egs/magicdata-ramc/ts_vad2/model.py:543-563, 1275-1287): the CAM++ trunk and every back end
# built behind it, with frame-level statistics + gsp_fc = Linear(2, GSP_FC_DIM) in front of speech_down_or_up's conv
FRAME_LEVEL_GSP = "CAM++_frame_level_gsp_fc"
GSP_FC_DIM = 256
CONFORMER_BACKEND_KERNEL = 31   # depthwise_conv_kernel_size the reference passes


@dataclass
class TSVADConfig:
    """Mirror of ts_vad2/model.py:40-110 (TSVADConfig) restricted to the fields
    the inference path reads, plus TSVADDataConfig (build_datasets.py:10-82)
    fields the model consumes."""
    speech_encoder_type: str = "CAM++"
    num_attention_head: int = 4
    num_transformer_layer: int = 2
    transformer_embed_dim: int = 384
    transformer_ffn_embed_dim: int = 1536
    speaker_embed_dim: int = 192
    dropout: float = 0.1
    single_backend_type: str = "transformer"
    multi_backend_type: str = "transformer"
    ots_vad_style: str = ""
    # Mamba2 back ends (egs/magicdata-ramc/ts_vad2/model.py:377-403): the reference defaults; the MagicData recipe
    # (run_ts_vad2_based_on_system_sad.sh:58-68) sets d_state 128
    d_state: int = 64
    expand: int = 4
    # data config
    rs_len: int = 4
    segment_shift: int = 1
    max_num_speaker: int = 4
    label_rate: int = 25
    sample_rate: int = 16000
    # WavLM speech encoders (egs/magicdata-ramc/ts_vad2/model.py:867-927).  wavlm_cfg stands in for checkpoint["cfg"] of
    # cfg.speech_encoder_path, which the reference reads to build the encoder: a WavLMConfig of
    # speaker_diarization_amd.ssl.wavlm.  Without it the two configurations cannot be built, here as there.
    wavlm_cfg: Optional[Any] = None
    select_encoder_layer_nums: int = 6         # "WavLM": encoder layers kept (model.py:870)
    wavlm_fuse_feat_post_norm: bool = False    # "WavLM_weight_sum": weights -> wavlmproj -> wavlmlnorm (:904-909)
    # "w2v-bert2" (egs/magicdata-ramc/ts_vad2/model.py:805-840): w2vbert_cfg stands in for the config.json of
    # cfg.speech_encoder_config, a W2vBertConfig of speaker_diarization_amd.ssl.w2vbert; None: the published geometry.
    # select_encoder_layer_nums overrides its depth (model.py:816).
    w2vbert_cfg: Optional[Any] = None
    # "whisper" (egs/magicdata-ramc/ts_vad2/model.py:928-955): whisper_cfg is a WhisperConfig of
    # speaker_diarization_amd.ssl.whisper; None: the published ModelDimensions() with n_mels = whisper_n_mels, the only
    # geometry the reference can build (its ModelDimensions() takes no argument there).
    whisper_n_mels: int = 80
    whisper_cfg: Optional[Any] = None

    @property
    def waveform_input(self) -> bool:
        """ref_speech is the raw waveform (B, n_samples), not fbank: the WavLM and Whisper speech encoders."""
        return self.speech_encoder_type in ("WavLM", "WavLM_weight_sum", "whisper")

    def effective_whisper_cfg(self):
        """whisper_cfg, or the published ModelDimensions() with n_mels = whisper_n_mels."""
        from .ssl.whisper import WhisperConfig
        return self.whisper_cfg if self.whisper_cfg is not None else WhisperConfig(n_mels=self.whisper_n_mels)

    def _whisper_variant(self) -> int:
        se = self.speech_encoder_type
        if self.ots_vad_style or (self.single_backend_type, self.multi_backend_type) != ("transformer", "transformer"):
            raise ValueError(
                f"unsupported TS-VAD configuration {se}/{self.single_backend_type}/{self.multi_backend_type}"
                f"{' ots_vad_style ' + self.ots_vad_style if self.ots_vad_style else ''}: the whisper speech encoder "
                "is built with the transformer single and multi back ends only (no Mamba2, no ots_vad)")
        from .ssl.whisper import check_config
        w = self.effective_whisper_cfg()
        check_config(w)
        if w.n_mels != self.whisper_n_mels:
            raise ValueError(f"whisper_cfg.n_mels {w.n_mels} differs from whisper_n_mels {self.whisper_n_mels}")
        return 8

    @property
    def wavlm_encoder_layers(self) -> int:
        """Encoder layers of speech_encoder.*: select_encoder_layer_nums for "WavLM" (model.py:870), the checkpoint's
        for "WavLM_weight_sum"."""
        return (self.select_encoder_layer_nums if self.speech_encoder_type == "WavLM"
                else self.wavlm_cfg.encoder_layers)

    def effective_wavlm_cfg(self):
        """wavlm_cfg with the encoder-layer override of "WavLM" applied (a copy)."""
        import copy
        c = copy.copy(self.wavlm_cfg)
        c.encoder_layers = self.wavlm_encoder_layers
        return c

    def effective_w2vbert_cfg(self):
        """w2vbert_cfg (None: the published geometry) with num_hidden_layers = select_encoder_layer_nums (a copy)."""
        import copy
        from .ssl.w2vbert import W2vBertConfig
        c = copy.copy(self.w2vbert_cfg) if self.w2vbert_cfg is not None else W2vBertConfig()
        c.num_hidden_layers = self.select_encoder_layer_nums
        return c

    def _w2vbert_variant(self) -> int:
        se = self.speech_encoder_type
        if self.ots_vad_style or (self.single_backend_type, self.multi_backend_type) != ("transformer", "transformer"):
            raise ValueError(
                f"unsupported TS-VAD configuration {se}/{self.single_backend_type}/{self.multi_backend_type}"
                f"{' ots_vad_style ' + self.ots_vad_style if self.ots_vad_style else ''}: the w2v-bert2 speech encoder "
                "is built with the transformer single and multi back ends only (no Mamba2, no ots_vad)")
        from .ssl.w2vbert import check_config
        check_config(self.effective_w2vbert_cfg())
        return 7

    def _wavlm_variant(self) -> int:
        se = self.speech_encoder_type
        if self.wavlm_cfg is None:
            raise ValueError(
                f"unsupported TS-VAD configuration {se}/{self.single_backend_type}/{self.multi_backend_type}: "
                "wavlm_cfg is missing (the WavLM checkpoint's cfg, which the reference reads from speech_encoder_path "
                "to build the encoder)")
        if self.ots_vad_style or (self.single_backend_type, self.multi_backend_type) != ("transformer", "transformer"):
            raise ValueError(
                f"unsupported TS-VAD configuration {se}/{self.single_backend_type}/{self.multi_backend_type}"
                f"{' ots_vad_style ' + self.ots_vad_style if self.ots_vad_style else ''}: the WavLM speech encoders "
                "are built with the transformer single and multi back ends only (no Mamba2, no ots_vad)")
        if se == "WavLM_weight_sum" and not self.wavlm_fuse_feat_post_norm:
            raise ValueError(
                "WavLM_weight_sum with wavlm_fuse_feat_post_norm=False is not built: the reference's forward "
                "(egs/magicdata-ramc/ts_vad2/model.py:1206-1213) unpacks the stacked (T, B, D, L) layer outputs as "
                "(_, T, B, D) and its view(B, T, D) raises (RuntimeError: shape ... is invalid for input of size ...) "
                "for every input whose frame count differs from the layer count; set wavlm_fuse_feat_post_norm=True")
        from .ssl.wavlm import check_config
        check_config(self.effective_wavlm_cfg())
        return 5 if se == "WavLM" else 6

    @property
    def n_mels(self) -> int:
        """Mel bins of ref_speech: ReDimNetB2 reads 72-bin fbank (egs/magicdata-ramc/ts_vad2/model.py:694-697), every
        other speech encoder built here 80."""
        return 72 if self.speech_encoder_type == "ReDimNetB2" else 80

    @property
    def variant(self) -> int:
        if self.speech_encoder_type == "whisper":
            return self._whisper_variant()   # 8
        if self.waveform_input:
            return self._wavlm_variant()   # 5 "WavLM", 6 "WavLM_weight_sum" with wavlm_fuse_feat_post_norm
        if self.speech_encoder_type == "w2v-bert2":
            return self._w2vbert_variant()   # 7
        if self.ots_vad_style == "v1":
            if (self.speech_encoder_type, self.single_backend_type, self.multi_backend_type) != (
                    "CAM++_ots_vad", "conformer_ots_vad", "lstm_ots_vad"):
                raise ValueError("ots_vad_style v1 is built for CAM++_ots_vad + conformer_ots_vad + lstm_ots_vad")
            return 1
        if (self.speech_encoder_type, self.single_backend_type, self.multi_backend_type) == (
                "resnet34_wespeaker", "transformer", "transformer"):
            return 2
        if (self.speech_encoder_type, self.single_backend_type, self.multi_backend_type) == (
                "ecapa_channel_1024_wespeaker", "transformer", "transformer"):
            return 3
        if (self.speech_encoder_type, self.single_backend_type, self.multi_backend_type) == (
                "ReDimNetB2", "transformer", "transformer"):
            return 4
        if not self.ots_vad_style and (self.speech_encoder_type, self.single_backend_type,
                                       self.multi_backend_type) in _MAMBA2_BACKENDS:
            return 0   # CAM++ with Mamba2 back ends: variant 0 plus `backend`
        if not self.ots_vad_style and (self.speech_encoder_type, self.single_backend_type,
                                       self.multi_backend_type) in _CONFORMER_BACKENDS:
            return 0   # CAM++ with conformer back ends: variant 0 plus `backend`
        if not self.ots_vad_style and (self.speech_encoder_type, self.single_backend_type,
                                       self.multi_backend_type) == (FRAME_LEVEL_GSP, "transformer", "transformer"):
            return 0   # variant 0's trunk and back end around the gsp_fc stage (`frame_level_gsp`)
        if (self.speech_encoder_type, self.single_backend_type, self.multi_backend_type) != (
                "CAM++", "transformer", "transformer"):
            raise ValueError(
                f"unsupported TS-VAD configuration {self.speech_encoder_type}/"
                f"{self.single_backend_type}/{self.multi_backend_type} (MI355X backend builds CAM++ "
"with transformer, mamba2 + transformer, mamba2 + mamba2, conformer + transformer, conformer + conformer or "
                "conformer_ots_vad/lstm_ots_vad, CAM++_frame_level_gsp_fc with the same five back-end pairs, "
                "resnet34_wespeaker, ecapa_channel_1024_wespeaker and ReDimNetB2 with transformer, WavLM / "
                "WavLM_weight_sum with transformer given wavlm_cfg, w2v-bert2 with transformer, whisper with transformer)")
        return 0

    @property
    def backend(self) -> int:
        """sd_tsvad_config.backend: 0 the variant's own back end, 1 single_backend "mamba2" + multi_backend
        "transformer", 2 "mamba2" for both (bidirectional Mamba2BlockV2 stacks, CAM++ only), 4 single_backend
        "conformer" + multi_backend "transformer", 5 "conformer" for both (torchaudio Conformers, CAM++ only).  Raises
        like `variant`."""
        self.variant
        key = (self.speech_encoder_type, self.single_backend_type, self.multi_backend_type)
        return _MAMBA2_BACKENDS.get(key, _CONFORMER_BACKENDS.get(key, 0))

    @property
    def frame_level_gsp(self) -> bool:
        """speech_encoder_type "CAM++_frame_level_gsp_fc": variant 0 with per-frame (mean, std) + gsp_fc in front of
        speech_down_or_up (sd_tsvad_config_ex.frame_level_gsp).  Raises like `variant`."""
        self.variant
        return self.speech_encoder_type == FRAME_LEVEL_GSP

    @property
    def mamba2_backend(self) -> bool:
        """A Mamba2 back end: the scan runs along the windows of a reference forward call."""
        return self.backend in (1, 2)

    @staticmethod
    def ots_vad_v1(**kw) -> "TSVADConfig":
        """The C2 configuration (egs/alimeeting/run_ts_vad2.sh:8298-8356)."""
        d = dict(speech_encoder_type="CAM++_ots_vad", single_backend_type="conformer_ots_vad",
                 multi_backend_type="lstm_ots_vad", ots_vad_style="v1", rs_len=6)
        d.update(kw)
        return TSVADConfig(**d)


def _bn(keys: list, prefix: str, c: int, affine: bool = True, kind: str = "bn"):
    if affine:
        keys.append((prefix + ".weight", (c,), kind + "_w"))
        keys.append((prefix + ".bias", (c,), kind + "_b"))
    keys.append((prefix + ".running_mean", (c,), kind + "_m"))
    keys.append((prefix + ".running_var", (c,), kind + "_v"))
    keys.append((prefix + ".num_batches_tracked", (), "nbt"))


def campplus_layout(prefix: str = "speech_encoder.", embedding_size: int = 192) -> list:
    """Key layout of CAMPPlus(feat_dim=80, embedding_size=192)
    (cam_pplus_wespeaker.py:311-386).  prefix "" is the standalone embedding
    extractor (generate_chunk_speaker_embedding_from_modelscope_for_diarization.py:60-66)."""
    k: list = []
    p = prefix + "head."
    k.append((p + "conv1.weight", (32, 1, 3, 3), "conv2d"))
    _bn(k, p + "bn1", 32)
    for layer in (1, 2):
        for blk in (0, 1):
            q = f"{p}layer{layer}.{blk}."
            k.append((q + "conv1.weight", (32, 32, 3, 3), "conv2d"))
            _bn(k, q + "bn1", 32)
            k.append((q + "conv2.weight", (32, 32, 3, 3), "conv2d"))
            _bn(k, q + "bn2", 32)
            if blk == 0:
                k.append((q + "shortcut.0.weight", (32, 32, 1, 1), "conv2d"))
                _bn(k, q + "shortcut.1", 32)
    k.append((p + "conv2.weight", (32, 32, 3, 3), "conv2d"))
    _bn(k, p + "bn2", 32)
    x = prefix + "xvector."
    k.append((x + "tdnn.linear.weight", (128, 320, 5), "kaiming"))
    _bn(k, x + "tdnn.nonlinear.batchnorm", 128)
    ch = 128
    for b, n in enumerate((12, 24, 16)):
        for i in range(n):
            q = f"{x}block{b + 1}.tdnnd{i + 1}."
            cin = ch + i * 32
            _bn(k, q + "nonlinear1.batchnorm", cin)
            k.append((q + "linear1.weight", (128, cin, 1), "kaiming"))
            _bn(k, q + "nonlinear2.batchnorm", 128)
            k.append((q + "cam_layer.linear_local.weight", (32, 128, 3), "kaiming"))
            k.append((q + "cam_layer.linear1.weight", (64, 128, 1), "kaiming"))
            k.append((q + "cam_layer.linear1.bias", (64,), "zero"))
            k.append((q + "cam_layer.linear2.weight", (32, 64, 1), "kaiming"))
            k.append((q + "cam_layer.linear2.bias", (32,), "zero"))
        ch += n * 32
        _bn(k, f"{x}transit{b + 1}.nonlinear.batchnorm", ch)
        k.append((f"{x}transit{b + 1}.linear.weight", (ch // 2, ch, 1), "kaiming"))
        ch //= 2
    _bn(k, x + "out_nonlinear.batchnorm", ch)
    k.append((x + "dense.linear.weight", (embedding_size, ch * 2, 1), "kaiming"))
    _bn(k, x + "dense.nonlinear.batchnorm", embedding_size, affine=False)
    return k


def resnet34_layout(prefix: str = "speech_encoder.") -> list:
    """Key layout of ResNet34(feat_dim=80, embed_dim=256, speech_encoder=True) (resnet_wespeaker.py:108-154,
    198-208): BasicBlocks [3, 4, 6, 3] at 32/64/128/256 channels, no pool / seg_1 (the TS-VAD speech encoder,
    model.py:584-606).  The conv / BN init kinds keep the seeded activations O(1) through the 16 residual blocks."""
    k: list = []
    k.append((prefix + "conv1.weight", (32, 1, 3, 3), "rn_conv"))
    _bn(k, prefix + "bn1", 32)
    cin = 32
    for layer, (planes, n) in enumerate(((32, 3), (64, 4), (128, 6), (256, 3)), start=1):
        for blk in range(n):
            q = f"{prefix}layer{layer}.{blk}."
            k.append((q + "conv1.weight", (planes, cin, 3, 3), "rn_conv"))
            _bn(k, q + "bn1", planes)
            k.append((q + "conv2.weight", (planes, planes, 3, 3), "rn_conv2"))
            _bn(k, q + "bn2", planes)
            if blk == 0 and layer > 1:
                k.append((q + "shortcut.0.weight", (planes, cin, 1, 1), "rn_sc"))
                _bn(k, q + "shortcut.1", planes)
            cin = planes
    return k


def resnet34_embed_layout(embed_dim: int = 256, two_emb_layer: bool = False) -> list:
    """Key layout of the standalone embedding extractor ResNet34(feat_dim=80, embed_dim, pooling_func="TSTP",
    two_emb_layer, speech_encoder=False) (resnet_wespeaker.py:108-147; the extractor script builds it with
    embed_dim 256 and two_emb_layer=False, generate_chunk_speaker_embedding_from_wespeaker_for_diarization.py:
    116-117): the trunk of resnet34_layout("") + seg_1 on the 5120 TSTP statistics (TSTP has no parameters)
    [+ seg_bn_1 (affine=False) + seg_2]."""
    k = resnet34_layout("")
    k.append(("seg_1.weight", (embed_dim, 5120), "kaiming"))
    k.append(("seg_1.bias", (embed_dim,), "small"))
    if two_emb_layer:
        _bn(k, "seg_bn_1", embed_dim, affine=False)
        k.append(("seg_2.weight", (embed_dim, embed_dim), "kaiming"))
        k.append(("seg_2.bias", (embed_dim,), "small"))
    return k


def simam_resnet34_layout(embed_dim: int = 256) -> list:
    """Key layout of the standalone extractor SimAM_ResNet34_ASP(in_planes=64, embed_dim, acoustic_dim=80, dropout=0,
    speech_encoder=False) (samresnet_wespeaker.py:134-141; generate_chunk_speaker_embedding_from_wespeaker_for_
    diarization.py:119-120): front = SimAM BasicBlocks [3, 4, 6, 3] at 64/128/256/512 channels with a downsample.{0,1}
    pair in the first block of layers 2-4 (:44-55, 126-127), pooling = ASP on the 5120-channel map
    (pooling_layers_wespeaker.py:146-159: attention = Conv1d, ReLU, BatchNorm1d, Conv1d, Softmax), bottleneck =
    Linear(10240, embed_dim)."""
    k: list = []
    p = "front."
    k.append((p + "conv1.weight", (64, 1, 3, 3), "rn_conv"))
    _bn(k, p + "bn1", 64)
    cin = 64
    for layer, (planes, n) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3)), start=1):
        for blk in range(n):
            q = f"{p}layer{layer}.{blk}."
            k.append((q + "conv1.weight", (planes, cin, 3, 3), "rn_conv"))
            _bn(k, q + "bn1", planes)
            k.append((q + "conv2.weight", (planes, planes, 3, 3), "sam_conv2"))
            _bn(k, q + "bn2", planes, kind="sam")
            if blk == 0 and layer > 1:
                k.append((q + "downsample.0.weight", (planes, cin, 1, 1), "rn_sc"))
                _bn(k, q + "downsample.1", planes)
            cin = planes
    k.append(("pooling.attention.0.weight", (128, 5120, 1), "sam_att1"))
    k.append(("pooling.attention.0.bias", (128,), "small"))
    _bn(k, "pooling.attention.2", 128, kind="ec")
    k.append(("pooling.attention.3.weight", (5120, 128, 1), "sam_att2"))
    k.append(("pooling.attention.3.bias", (5120,), "small"))
    k.append(("bottleneck.weight", (embed_dim, 10240), "kaiming"))
    k.append(("bottleneck.bias", (embed_dim,), "small"))
    return k


def eres2netv2_layout(base_width: int = 26, scale: int = 2, expansion: int = 2, embedding_size: int = 192) -> list:
    """Key layout of ERes2NetV2(feat_dim=80, embedding_size, m_channels=64, baseWidth, scale, expansion,
    pooling_func="TSTP", two_emb_layer=False) (ERes2NetV2.py:162-226; the modelscope extractor script builds it at (24, 4,
    4), generate_chunk_speaker_embedding_from_modelscope_for_diarization.py:110-136): Res2Net blocks [3, 4, 6, 3] at
    planes 64 .. 512 with `scale` slice convs of width floor(planes baseWidth / 64), AFF gates between the slices in
    layers 3-4 (fusion.py:10-22: Conv2d with bias, BatchNorm2d, SiLU, Conv2d with bias, BatchNorm2d), a shortcut pair in
    every block whose input differs from planes * expansion, layer3_ds, fuse34 and seg_1 on the TSTP statistics."""
    k: list = []

    def aff(p: str, c: int):
        k.append((p + "local_att.0.weight", (c // 4, 2 * c, 1, 1), "er_att1"))
        k.append((p + "local_att.0.bias", (c // 4,), "small"))
        _bn(k, p + "local_att.1", c // 4)
        k.append((p + "local_att.3.weight", (c, c // 4, 1, 1), "er_att2"))
        k.append((p + "local_att.3.bias", (c,), "small"))
        _bn(k, p + "local_att.4", c)

    k.append(("conv1.weight", (64, 1, 3, 3), "rn_conv"))
    _bn(k, "bn1", 64)
    cin = 64
    for layer, (planes, n) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3)), start=1):
        width = planes * base_width // 64
        for blk in range(n):
            q = f"layer{layer}.{blk}."
            k.append((q + "conv1.weight", (width * scale, cin, 1, 1), "er_conv1"))
            _bn(k, q + "bn1", width * scale, kind="er")
            for i in range(scale):
                k.append((f"{q}convs.{i}.weight", (width, width, 3, 3), "er_conv"))
            for i in range(scale):
                _bn(k, f"{q}bns.{i}", width, kind="er")
            if layer >= 3:
                for j in range(scale - 1):
                    aff(f"{q}fuse_models.{j}.", width)
            k.append((q + "conv3.weight", (planes * expansion, width * scale, 1, 1), "er_conv3"))
            _bn(k, q + "bn3", planes * expansion)
            if (blk == 0 and layer > 1) or cin != planes * expansion:
                k.append((q + "shortcut.0.weight", (planes * expansion, cin, 1, 1), "er_sc"))
                _bn(k, q + "shortcut.1", planes * expansion)
            cin = planes * expansion
    k.append(("layer3_ds.weight", (512 * expansion, 256 * expansion, 3, 3), "er_ds"))
    aff("fuse34.", 512 * expansion)
    k.append(("seg_1.weight", (embedding_size, 10240 * expansion), "er_seg"))
    k.append(("seg_1.bias", (embedding_size,), "small"))
    return k


def _conv_relu_bn(k: list, p: str, cout: int, cin: int, taps: int, kind: str):
    """Conv1dReluBn (ecapa_tdnn_wespeaker.py:85-108): conv with bias, ReLU, then BatchNorm."""
    k.append((p + "conv.weight", (cout, cin, taps), kind))
    k.append((p + "conv.bias", (cout,), "small"))
    _bn(k, p + "bn", cout, kind="ec")


def ecapa_layout(prefix: str = "speech_encoder.") -> list:
    """Key layout of ECAPA_TDNN_GLOB_c1024(feat_dim=80, speech_encoder=True) (ecapa_tdnn_wespeaker.py:161-209): layer1
    (k5), three SE_Res2Blocks (1x1, Res2 chain of 7 k3 128 -> 128 convs, 1x1, SE 1024 -> 128 -> 1024) and the
    3072 -> 1536 conv; no pool / bn / linear (the TS-VAD speech encoder, model.py:631-640)."""
    k: list = []
    _conv_relu_bn(k, prefix + "layer1.", 1024, 80, 5, "ec_conv")
    for layer in (2, 3, 4):
        q = f"{prefix}layer{layer}.se_res2block."
        _conv_relu_bn(k, q + "0.", 1024, 1024, 1, "ec_conv")
        for i in range(7):
            k.append((f"{q}1.convs.{i}.weight", (128, 128, 3), "ec_conv"))
            k.append((f"{q}1.convs.{i}.bias", (128,), "small"))
        for i in range(7):
            _bn(k, f"{q}1.bns.{i}", 128, kind="ec")
        _conv_relu_bn(k, q + "2.", 1024, 1024, 1, "ec_conv2")
        k.append((q + "3.linear1.weight", (128, 1024), "ec_se1"))
        k.append((q + "3.linear1.bias", (128,), "small"))
        k.append((q + "3.linear2.weight", (1024, 128), "ec_se2"))
        k.append((q + "3.linear2.bias", (1024,), "small"))
    k.append((prefix + "conv.weight", (1536, 3072, 1), "ec_out"))
    k.append((prefix + "conv.bias", (1536,), "small"))
    return k


def ecapa_embed_layout(embed_dim: int = 192) -> list:
    """Key layout of the standalone extractor ECAPA_TDNN_GLOB_c1024(feat_dim=80, embed_dim, pooling_func="ASTP")
    (ecapa_tdnn_wespeaker.py:161-225): the trunk of ecapa_layout("") + ASTP with global context
    (pooling_layers_wespeaker.py:91-144: linear1 4608 -> 128, linear2 128 -> 1536) + bn(3072) + linear(3072 -> E)."""
    k = ecapa_layout("")
    k.append(("pool.linear1.weight", (128, 4608, 1), "ec_att1"))
    k.append(("pool.linear1.bias", (128,), "small"))
    k.append(("pool.linear2.weight", (1536, 128, 1), "ec_att2"))
    k.append(("pool.linear2.bias", (1536,), "small"))
    _bn(k, "bn", 3072, kind="ec")
    k.append(("linear.weight", (embed_dim, 3072), "kaiming"))
    k.append(("linear.bias", (embed_dim,), "small"))
    return k


# ReDimNetB2 stages_setup (redimnet_wespeaker.py:934-941): (stride, 2-D blocks, 1-D reduction), and the depthwise kernel
# sizes of TimeContextBlock1d's "conv+att" form (:586-607).
REDIM_STAGES = ((1, 2, 12), (2, 2, 12), (1, 3, 12), (2, 4, 8), (1, 4, 8), (2, 4, 4))
REDIM_KERNELS = (7, 19, 31, 59)
REDIM_CF = 1152


def redimnet_layout(prefix: str = "", embed_dim: int = 192) -> list:
    """Key layout of ReDimNetB2(feat_dim=72, embed_dim, pooling_func="ASTP", two_emb_layer=False)
    (redimnet_wespeaker.py:925-948; ReDimNet :793-845, ReDimNetBone.build :654-756): the per-stage input weights, the
    stem, six stages of (entry conv, ConvNeXt-like 2-D blocks, to1d, TimeContextBlock1d) — to1d has no parameters, so
    the 1-D block sits at index blocks + 2 — then ASTP with the global context and seg_1.  548 keys."""
    k: list = []
    bb, cf = prefix + "backbone.", REDIM_CF

    def conv(p: str, shape, kind: str):
        k.append((p + ".weight", shape, kind))
        k.append((p + ".bias", (shape[0],), "small"))

    k.append((bb + "inputs_weights.0", (1, 1, 1, 1), "ones"))
    for i in range(1, len(REDIM_STAGES) + 1):
        k.append((bb + f"inputs_weights.{i}", (1, i + 1, cf, 1), "rd_mix"))
    conv(bb + "stem.0", (16, 1, 3, 3), "rd_conv")
    k.append((bb + "stem.1.weight", (16,), "rd_ln_w"))
    k.append((bb + "stem.1.bias", (16,), "small"))
    c = 16
    for i, (stride, blocks, red) in enumerate(REDIM_STAGES):
        sp = f"{bb}stage{i}."
        conv(sp + "0", (c * stride, c, stride, 1), "rd_conv")
        c *= stride
        for b in range(1, blocks + 1):
            q = f"{sp}{b}.conv_block."
            conv(q + "dwconvs.0", (c, 4, 3, 3), "rd_conv")
            _bn(k, q + "norm", c, kind="rd")
            conv(q + "pwconv1", (c, c, 1, 1), "rd_out")
        t, hc = f"{sp}{blocks + 2}.", cf // red
        conv(t + "red_dim_conv.0", (hc, cf, 1), "rd_conv")
        k.append((t + "red_dim_conv.1.weight", (hc,), "rd_ln_w"))
        k.append((t + "red_dim_conv.1.bias", (hc,), "small"))
        for j, ks in enumerate(REDIM_KERNELS):
            q = f"{t}tcm.{j}."
            conv(q + "dwconvs.0", (hc, 1, ks), "rd_conv")
            _bn(k, q + "norm", hc, kind="rd")
            conv(q + "pwconv1", (hc, hc, 1), "rd_out")
        a = t + "tcm.4."
        for n in ("k_proj", "v_proj", "q_proj"):
            conv(a + "attention." + n, (hc, hc), "rd_conv")
        conv(a + "attention.out_proj", (hc, hc), "rd_out")
        k.append((a + "layer_norm.weight", (hc,), "rd_ln_w"))
        k.append((a + "layer_norm.bias", (hc,), "small"))
        conv(a + "feed_forward.intermediate_dense", (hc, hc), "rd_conv")
        conv(a + "feed_forward.output_dense", (hc, hc), "rd_out")
        k.append((a + "final_layer_norm.weight", (hc,), "rd_ln_w"))
        k.append((a + "final_layer_norm.bias", (hc,), "small"))
        conv(t + "exp_dim_conv", (cf, hc, 1), "rd_out")
    conv(prefix + "pool.linear1", (128, 3 * cf, 1), "ec_att1")
    conv(prefix + "pool.linear2", (cf, 128, 1), "ec_att2")
    conv(prefix + "seg_1", (embed_dim, 2 * cf), "kaiming")
    return k


def _mha(k: list, p: str, e: int):
    k.append((p + "in_proj_weight", (3 * e, e), "xavier"))
    k.append((p + "in_proj_bias", (3 * e,), "small"))
    k.append((p + "out_proj.weight", (e, e), "linear"))
    k.append((p + "out_proj.bias", (e,), "small"))


def _ln(k: list, p: str, e: int):
    k.append((p + ".weight", (e,), "ln_w"))
    k.append((p + ".bias", (e,), "small"))


def tsvad_layout(cfg: TSVADConfig) -> list:
    """Key layout of TSVADModel(cfg) (ts_vad2/model.py:179-367)."""
    e, se, ns = cfg.transformer_embed_dim, cfg.speaker_embed_dim, cfg.max_num_speaker
    if cfg.variant == 2:
        # ResNet34 + SpeechFeatUpsample2 (model.py:114-134, 584-606); the back end is variant 0's
        k = resnet34_layout()
        k.append(("speech_down_or_up.up.weight", (2560, se, 5), "convT"))
        k.append(("speech_down_or_up.up.bias", (se,), "small"))
        _bn(k, "speech_down_or_up.batchnorm.bn", se)
    elif cfg.variant == 3:
        # ECAPA-TDNN c1024 + Conv1d(1536 -> D, k5, stride 4, pad 2) (model.py:631-654); the back end is variant 0's
        k = ecapa_layout()
        k.append(("speech_down_or_up.0.weight", (se, 1536, 5), "ec_down"))
        k.append(("speech_down_or_up.0.bias", (se,), "small"))
        _bn(k, "speech_down_or_up.1.bn", se)
    elif cfg.variant == 4:
        # ReDimNetB2 (with its pool / seg_1, which the reference builds and never runs here) + Conv1d(1152 -> D, k5,
        # stride 4, pad 2) (egs/magicdata-ramc/ts_vad2/model.py:694-715); the back end is variant 0's
        k = redimnet_layout("speech_encoder.")
        k.append(("speech_down_or_up.0.weight", (se, REDIM_CF, 5), "ec_down"))
        k.append(("speech_down_or_up.0.bias", (se,), "small"))
        _bn(k, "speech_down_or_up.1.bn", se)
    elif cfg.variant in (5, 6):
        # WavLM on the waveform (egs/magicdata-ramc/ts_vad2/model.py:867-927); the back end is variant 0's
        w = cfg.effective_wavlm_cfg()
        d = w.encoder_embed_dim
        k = wavlm_layout(w, "speech_encoder.")
        if cfg.variant == 6:
            k.append(("weights.weight", (1, w.encoder_layers), "wavlm_mix"))
            k.append(("wavlmproj.weight", (se, d), "linear"))
            k.append(("wavlmproj.bias", (se,), "wavlm_b"))
            k.append(("wavlmlnorm.weight", (se,), "rd_ln_w"))
            k.append(("wavlmlnorm.bias", (se,), "rd_b"))
        k.append(("speech_down_or_up.0.weight", (se, se if cfg.variant == 6 else d, 5), "conv1d"))
        k.append(("speech_down_or_up.0.bias", (se,), "small"))
        _bn(k, "speech_down_or_up.1.bn", se)
    elif cfg.variant == 7:
        # the first select_encoder_layer_nums layers of w2v-BERT 2.0 + Conv1d(1024 -> D, k5, stride 2, pad 2)
        # (egs/magicdata-ramc/ts_vad2/model.py:805-840); the back end is variant 0's
        w = cfg.effective_w2vbert_cfg()
        k = w2vbert_layout(w, "speech_encoder.")
        k.append(("speech_down_or_up.0.weight", (se, w.output_hidden_size, 5), "conv1d"))
        k.append(("speech_down_or_up.0.bias", (se,), "small"))
        _bn(k, "speech_down_or_up.1.bn", se)
    elif cfg.variant == 8:
        # the Whisper-PMFA encoder + Conv1d(n_audio_state * n_cat -> D, k5, stride 2, pad 2)
        # (egs/magicdata-ramc/ts_vad2/model.py:928-955); the back end is variant 0's
        w = cfg.effective_whisper_cfg()
        k = whisper_layout(w, "speech_encoder.")
        k.append(("speech_down_or_up.0.weight", (se, w.out_dim, 5), "conv1d"))
        k.append(("speech_down_or_up.0.bias", (se,), "small"))
        _bn(k, "speech_down_or_up.1.bn", se)
    else:
        k = campplus_layout()
        if cfg.variant == 1:
            k.append(("gsp_fc.weight", (se, 2), "linear"))
            k.append(("gsp_fc.bias", (se,), "small"))
        if cfg.frame_level_gsp:   # Linear(2, 256) on the frame statistics, then the conv on its 256 features
            k.append(("gsp_fc.weight", (GSP_FC_DIM, 2), "linear"))
            k.append(("gsp_fc.bias", (GSP_FC_DIM,), "small"))
        k.append(("speech_down_or_up.0.weight", (se, GSP_FC_DIM if cfg.frame_level_gsp else 512, 5), "conv1d"))
        k.append(("speech_down_or_up.0.bias", (se,), "small"))
        _bn(k, "speech_down_or_up.1.bn", se)
    if se * 2 != e:
        # nn.Linear(2 * speaker_embed_dim, transformer_embed_dim) on cat(ts_embed, mix_embeds) (model.py:212-217,
        # 873-874); the reference registers it for every variant, its ots_vad forward never applies it
        k.append(("proj_layer.weight", (e, 2 * se), "linear"))
        k.append(("proj_layer.bias", (e,), "small"))
    if cfg.variant in (0, 2, 3, 4, 5, 6, 7, 8):
        k.append(("pos_encoder.pe", (cfg.rs_len * cfg.label_rate, 1, e), "pe"))
        backend = cfg.backend
        m2 = cfg.mamba2_backend
        ffn = cfg.transformer_ffn_embed_dim
        if m2:
            # Mamba2BlockV2(e, n_layer, d_state, d_conv=4, expand, bidirectional=True): the two directions are
            # concatenated, so backend_down reads 2 e ns channels (magicdata model.py:377-403)
            mamba2_block_v2_layout(k, "single_backend.", e, cfg.num_transformer_layer, cfg.d_state, cfg.expand)
        elif backend in (4, 5):
            # torchaudio.models.Conformer(e, num_attention_head, ffn, num_transformer_layer, 31): use_group_norm False,
            # so conv_module.sequential.3 is a BatchNorm1d (magicdata model.py:290-313)
            for i in range(cfg.num_transformer_layer):
                _conformer_layer(k, f"single_backend.conformer_layers.{i}.", e, ffn, CONFORMER_BACKEND_KERNEL,
                                 group_norm=False)
        else:
            for i in range(cfg.num_transformer_layer):
                _tfm(k, f"single_backend.layers.{i}.", e, ffn)
        k.append(("backend_down.0.weight", (e, (2 if m2 else 1) * e * ns, 5), "conv1d"))
        k.append(("backend_down.0.bias", (e,), "small"))
        _bn(k, "backend_down.1.bn", e)
        if backend == 2:
            mamba2_block_v2_layout(k, "multi_backend.", e, cfg.num_transformer_layer, cfg.d_state, cfg.expand)
            k.append(("multi_backend_proj.weight", (e, 2 * e), "linear"))   # magicdata model.py:488-504
            k.append(("multi_backend_proj.bias", (e,), "small"))
        elif backend == 5:
            for i in range(cfg.num_transformer_layer):   # magicdata model.py:451-463
                _conformer_layer(k, f"multi_backend.conformer_layers.{i}.", e, ffn, CONFORMER_BACKEND_KERNEL,
                                 group_norm=False)
        else:
            for i in range(cfg.num_transformer_layer):
                _tfm(k, f"multi_backend.layers.{i}.", e, ffn)
        k.append(("fc.weight", (ns, e), "linear"))
        k.append(("fc.bias", (ns,), "small"))
    else:
        for i in range(6):
            p = f"single_backend.conformer_layers.{i}."
            for f in ("ffn1", "ffn2"):
                _ln(k, p + f + ".sequential.0", e)
                k.append((p + f + ".sequential.1.weight", (512, e), "linear"))
                k.append((p + f + ".sequential.1.bias", (512,), "small"))
                k.append((p + f + ".sequential.4.weight", (e, 512), "linear"))
                k.append((p + f + ".sequential.4.bias", (e,), "small"))
                if f == "ffn1":
                    _ln(k, p + "self_attn_layer_norm", e)
                    _mha(k, p + "self_attn.", e)
                    _ln(k, p + "conv_module.layer_norm", e)
                    k.append((p + "conv_module.sequential.0.weight", (2 * e, e, 1), "conv1d"))
                    k.append((p + "conv_module.sequential.0.bias", (2 * e,), "small"))
                    k.append((p + "conv_module.sequential.2.weight", (e, 1, 31), "conv1d"))
                    k.append((p + "conv_module.sequential.2.bias", (e,), "small"))
                    k.append((p + "conv_module.sequential.3.weight", (e,), "ln_w"))
                    k.append((p + "conv_module.sequential.3.bias", (e,), "small"))
                    k.append((p + "conv_module.sequential.5.weight", (e, e, 1), "conv1d"))
                    k.append((p + "conv_module.sequential.5.bias", (e,), "small"))
            _ln(k, p + "final_layer_norm", e)
        h = 256
        for sfx in ("", "_reverse"):
            k.append((f"multi_backend.weight_ih_l0{sfx}", (4 * h, ns * e), "lstm"))
            k.append((f"multi_backend.weight_hh_l0{sfx}", (4 * h, h), "lstm"))
            k.append((f"multi_backend.bias_ih_l0{sfx}", (4 * h,), "lstm"))
            k.append((f"multi_backend.bias_hh_l0{sfx}", (4 * h,), "lstm"))
        k.append(("fc.weight", (ns, 2 * h), "linear"))
        k.append(("fc.bias", (ns,), "small"))
    return k


def mamba2_sizes(e: int, d_state: int, expand: int):
    """(d_inner, heads, conv_dim, d_in_proj) of mamba_ssm's Mamba2(d_model=e, d_state, expand) at its defaults
    (headdim 64, ngroups 1)."""
    d_inner = expand * e
    if d_inner % MAMBA2_HEADDIM:
        raise ValueError(f"expand * transformer_embed_dim = {d_inner} is not a multiple of {MAMBA2_HEADDIM}")
    heads = d_inner // MAMBA2_HEADDIM
    return d_inner, heads, d_inner + 2 * d_state, 2 * d_inner + 2 * d_state + heads


def mamba2_block_v2_layout(k: list, prefix: str, e: int, n_layer: int, d_state: int, expand: int):
    """Keys of Mamba2BlockV2(bidirectional=True) (ts_vad2/mamba.py:149-213): Block(norm = RMSNorm, mixer = Mamba2,
    mlp = Identity) per layer and direction.  mamba_ssm is CUDA-only, so no reference run pins this key set."""
    d_inner, heads, conv_dim, d_in_proj = mamba2_sizes(e, d_state, expand)
    for d in ("forward_blocks", "backward_blocks"):
        for i in range(n_layer):
            p = f"{prefix}{d}.{i}."
            k.append((p + "norm.weight", (e,), "m2_w"))
            k.append((p + "mixer.in_proj.weight", (d_in_proj, e), f"m2_in{heads}"))
            k.append((p + "mixer.conv1d.weight", (conv_dim, 1, 4), "m2_conv"))
            k.append((p + "mixer.conv1d.bias", (conv_dim,), "m2_conv"))
            k.append((p + "mixer.dt_bias", (heads,), "m2_dtb"))
            k.append((p + "mixer.A_log", (heads,), "m2_alog"))
            k.append((p + "mixer.D", (heads,), "ones"))
            k.append((p + "mixer.norm.weight", (d_inner,), "m2_w"))
            k.append((p + "mixer.out_proj.weight", (e, d_inner), "linear"))


def _tfm(k: list, p: str, e: int, ffn: int):
    _mha(k, p + "self_attn.", e)
    k.append((p + "linear1.weight", (ffn, e), "linear"))
    k.append((p + "linear1.bias", (ffn,), "small"))
    k.append((p + "linear2.weight", (e, ffn), "linear"))
    k.append((p + "linear2.bias", (e,), "small"))
    _ln(k, p + "norm1", e)
    _ln(k, p + "norm2", e)


def sinusoid_pe(max_len: int, d: int) -> np.ndarray:
    """PositionalEncoding.pe buffer (ts_vad2/model.py:137-150), shape (max_len, 1, d)."""
    pos = np.arange(max_len, dtype=np.float32)[:, None]
    div = np.exp(np.arange(0, d, 2, dtype=np.float32) * np.float32(-np.log(10000.0) / d)).astype(np.float32)
    pe = np.zeros((max_len, 1, d), np.float32)
    pe[:, 0, 0::2] = np.sin(pos * div)
    pe[:, 0, 1::2] = np.cos(pos * div)
    return pe


# Seeded ResNet34 init (resnet34_layout): He-normal keeps the ReLU branch at its input's scale; the block's second
# conv is damped so the residual sum grows by ~(1 + g^2) in variance per block instead of doubling over 16 blocks
# (trunk maximum ~9 on the golden inputs), and the transposed conv is scaled so the mix embeddings it feeds the back
# end are O(1) like the CAM++ variants' (mean ~0.5, maximum ~5): tests/golden/make_golden_resnet.py asserts the
# reference run of the seeded model is alive.
RN_GAIN = {"rn_conv": 1.0, "rn_conv2": 0.3, "rn_sc": 0.7}
CONVT_GAIN = 0.5


# Seeded ECAPA init (ecapa_layout).  Every conv is followed by ReLU and THEN BatchNorm, so the BatchNorm's running
# mean sits near the mean of a rectified unit-variance signal (0.4 +- 0.2) and its running variance varies by 3x:
# a BatchNorm applied on the wrong side of the ReLU moves every activation by O(1).  The block's closing 1x1 conv
# is damped so the three residual sums stay O(1); the SE and attention gains are tuned until
# tests/golden/make_golden_ecapa.py's assertions on the reference run hold (gates on both sides of 0.4 .. 0.6,
# attention weights neither uniform nor one-hot).
EC_GAIN = {"ec_conv": 1.0, "ec_conv2": 0.5, "ec_out": 1.0, "ec_down": 0.5, "ec_se1": 1.0, "ec_se2": 2.0,
           "ec_att1": 1.0, "ec_att2": 2.0}


# Seeded SimAM-ResNet34 init (simam_resnet34_layout): the ResNet34 roles, with the block's second conv at its own gain
# (the SimAM gate scales the branch by sigmoid(>= 0.5), 0.62 .. 1), a positive bn2 shift and the two ASP attention
# convs tuned until tests/golden/make_golden_simam.py's assertions on the reference run hold for every case
# (last-block gates spread, attention weights neither uniform nor one-hot, under 5 % of the front channels constant
# over time, embedding std in [0.3, 5]).  With bn2's shift centred on 0 a channel-row that the block's ReLU has
# zeroed stays zero through the identity shortcuts whenever its small gated branch is negative, and 7 % of the rows
# were constant over t38's 5 frames at every conv gain; centred on 0.1 it is 3.7 % (t17 2.8 %, t200 2.1 %).
SAM_BN2_BIAS = 0.1
SAM_GAIN = {"sam_conv2": 0.3, "sam_att1": 1.0, "sam_att2": 1.0}


# Seeded ERes2NetV2 init (eres2netv2_layout): He-normal times a per-role gain, and a positive shift on the BatchNorms
# in front of a Hardtanh(0, 20) (kinds er_*), chosen so that tests/golden/make_golden_eres2net.py's assertions on the
# reference run hold for every case: the clamp at 20 fires on a share of the elements but not everywhere, and the AFF
# gates' tanh neither vanishes nor saturates.
ER_GAIN = {"er_conv1": 0.8, "er_conv": 1.0, "er_conv3": 0.6, "er_sc": 0.6, "er_att1": 0.15, "er_att2": 0.5,
           "er_ds": 0.5, "er_seg": 0.1}
ER_BN_BIAS = 0.3


# Seeded ReDimNetB2 init (redimnet_layout): He-normal times a per-role gain, the convs that close a residual branch
# (pwconv1, out_proj, output_dense, exp_dim_conv) damped so that 22 + 24 skip sums stay O(1); BatchNorm running
# statistics spread (mean +- 0.3, variance 0.5 .. 1.5), LayerNorm gains 0.7 .. 1.3 and inputs_weights of +- 0.5, so a
# BatchNorm on the wrong side, a unit LayerNorm gain or a swapped stage order each move the outputs by O(1).
# tests/golden/make_golden_redimnet.py asserts the reference's frame-level maps have a standard deviation in [0.1, 10].
RD_GAIN = {"rd_conv": 1.0, "rd_out": 0.5}


# Seeded Mamba2 init (mamba2_block_v2_layout), in the spirit of mamba_ssm's: A = U[1, 16], dt_bias the inverse softplus
# of a log-uniform dt in [1e-3, 1e-1], D = 1.  in_proj's z / x / Bm / Cm rows give outputs of standard deviation
# M2_IN_GAIN on the normalised rows; its dt rows are drawn wider (M2_DT_GAIN) so that dt_raw moves dt over its whole
# range from step to step: tests/test_mamba2_host.py asserts that the per-step decay exp(dt A) falls both below 0.5 and
# above 0.9 and that the state term carries at least a tenth of rms(y), so a test cannot pass on a scan that forgets
# everything or never decays.  At d_state 16 with two heads, the smallest operator case, the state term's share is
# 0.06 at gains (1.0, 3.0) and (1.5, 2.5) and 0.12 at these.
M2_IN_GAIN = 1.25
M2_DT_GAIN = 3.5


def _init(rng: np.random.Generator, shape: Shape, kind: str) -> np.ndarray:
    if kind == "nbt":
        return np.array(0, dtype=np.int64)
    n = int(np.prod(shape)) if shape else 1
    fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else max(shape[0], 1)
    if kind == "conv2d":
        b = 1.0 / np.sqrt(fan_in)
        v = rng.uniform(-b, b, n)
    elif kind in ("kaiming", "conv1d"):
        v = rng.standard_normal(n) * np.sqrt(2.0 / fan_in)
        if kind == "conv1d":
            v *= 0.5
    elif kind == "linear":
        b = 1.0 / np.sqrt(fan_in)
        v = rng.uniform(-b, b, n)
    elif kind in RN_GAIN:                 # ResNet34 convs: He-normal times a per-role gain
        v = rng.standard_normal(n) * (RN_GAIN[kind] * np.sqrt(2.0 / fan_in))
    elif kind in EC_GAIN:                 # ECAPA convs / linears: He-normal times a per-role gain
        v = rng.standard_normal(n) * (EC_GAIN[kind] * np.sqrt(2.0 / fan_in))
    elif kind in SAM_GAIN:                # SimAM-ResNet34 conv2 / ASP attention: He-normal times a per-role gain
        v = rng.standard_normal(n) * (SAM_GAIN[kind] * np.sqrt(2.0 / fan_in))
    elif kind in ER_GAIN:                 # ERes2NetV2 convs: He-normal times a per-role gain
        v = rng.standard_normal(n) * (ER_GAIN[kind] * np.sqrt(2.0 / fan_in))
    elif kind in RD_GAIN:                 # ReDimNetB2 convs / linears: He-normal times a per-role gain
        v = rng.standard_normal(n) * (RD_GAIN[kind] * np.sqrt(2.0 / fan_in))
    elif kind == "wavlm_mix":             # weights.weight: clearly non-uniform, signs mixed, so a wrong layer order or an
        v = rng.permutation(np.linspace(-0.9, 1.3, n)) + rng.standard_normal(n) * 0.05   # off-by-one on hss[1:] shows
    elif kind == "wavlm_b":               # wavlmproj.bias: at "small" (0.05 N) zeroing it moves the Large goldens by 9 fp32 bars
        v = rng.standard_normal(n) * 0.2
    elif kind == "rd_mix":                # inputs_weights: far from the all-zero init, so the stage order matters
        v = rng.standard_normal(n) * 0.5
    elif kind in ("rd_w", "rd_ln_w"):
        v = rng.uniform(0.7, 1.3, n)
    elif kind == "rd_b":
        v = rng.standard_normal(n) * 0.1
    elif kind == "rd_m":
        v = rng.standard_normal(n) * 0.3
    elif kind == "rd_v":
        v = rng.uniform(0.5, 1.5, n)
    elif kind == "ones":
        v = np.ones(n)
    elif kind == "m2_w":                  # RMSNorm weights: far enough from 1 that a dropped weight shows
        v = rng.uniform(0.7, 1.3, n)
    elif kind.startswith("m2_in"):        # in_proj, kind "m2_in<heads>": its last <heads> rows are dt's (gains above)
        v = rng.standard_normal(n).reshape(shape) * (M2_IN_GAIN / np.sqrt(fan_in))
        v[shape[0] - int(kind[5:]):] *= M2_DT_GAIN / M2_IN_GAIN
    elif kind == "m2_conv":               # nn.Conv1d(groups = channels, k 4): U(+-1 / sqrt(4)), weight and bias
        v = rng.uniform(-0.5, 0.5, n)
    elif kind == "m2_dtb":                # inverse softplus of dt ~ log-uniform [1e-3, 1e-1] (mamba_ssm's dt_min / dt_max)
        dt = np.exp(rng.uniform(np.log(1e-3), np.log(1e-1), n))
        v = dt + np.log(-np.expm1(-dt))
    elif kind == "m2_alog":               # A ~ U[1, 16] (mamba_ssm's A_init_range)
        v = np.log(rng.uniform(1.0, 16.0, n))
    elif kind in ("er_w", "er_m", "er_v"):
        return _init(rng, shape, "bn" + kind[2:])
    elif kind == "er_b":
        v = ER_BN_BIAS + rng.standard_normal(n) * 0.05
    elif kind in ("sam_w", "sam_m", "sam_v"):   # SimAM-ResNet34 bn2: the generic BatchNorm statistics ...
        return _init(rng, shape, "bn" + kind[3:])
    elif kind == "sam_b":                 # ... with a positive shift (SAM_BN2_BIAS)
        v = SAM_BN2_BIAS + rng.standard_normal(n) * 0.05
    elif kind == "ec_w":
        v = rng.uniform(0.7, 1.3, n)
    elif kind == "ec_b":
        v = rng.standard_normal(n) * 0.1
    elif kind == "ec_m":
        v = rng.uniform(0.2, 0.6, n)
    elif kind == "ec_v":
        v = rng.uniform(0.5, 1.5, n)
    elif kind == "convT":                 # ConvTranspose1d (Cin, Cout, k), stride 2: Cin * k / 2 taps per output
        v = rng.standard_normal(n) * (CONVT_GAIN * np.sqrt(2.0 / (shape[0] * shape[2] / 2.0)))
    elif kind == "xavier":
        b = np.sqrt(6.0 / (shape[0] / 3 + shape[1]))
        v = rng.uniform(-b, b, n)
    elif kind == "lstm":
        b = 1.0 / np.sqrt(256)
        v = rng.uniform(-b, b, n)
    elif kind == "bn_w":
        v = rng.uniform(0.8, 1.2, n)
    elif kind in ("bn_b", "small"):
        v = rng.standard_normal(n) * 0.05
    elif kind == "bn_m":
        v = rng.standard_normal(n) * 0.1
    elif kind == "bn_v":
        v = rng.uniform(0.6, 1.4, n)
    elif kind == "ln_w":
        v = 1.0 + rng.standard_normal(n) * 0.05
    elif kind == "zero":
        v = np.zeros(n)
    elif kind == "randn":                 # nn.Parameter(torch.randn(...)) (ssnd_model.py:415-431)
        v = rng.standard_normal(n)
    else:
        raise ValueError(kind)
    return v.astype(np.float32).reshape(shape)


def synthetic_state_dict(layout: list, seed: int = 777, extras: Dict[str, np.ndarray] | None = None
                         ) -> "OrderedDict[str, np.ndarray]":
    """Seeded random weights (numpy PCG64: identical on every host)."""
    rng = np.random.default_rng(seed)
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for name, shape, kind in layout:
        if kind == "pe":
            sd[name] = sinusoid_pe(shape[0], shape[2])
        elif kind == "pe1":   # (1, max_len, d) buffer of the wenet-style PositionalEncoding
            sd[name] = np.ascontiguousarray(sinusoid_pe(shape[1], shape[2]).transpose(1, 0, 2))
        else:
            sd[name] = _init(rng, shape, kind)
    if extras:
        sd.update(extras)
    return sd


def tsvad_state_dict(cfg: TSVADConfig, seed: int = 777, spread: bool = False, dynamic: bool = False):
    """Seeded weights of the reference layout.  spread: the 'spread' variant (tests/golden/calibrate_spread.py) whose
    final Linear is rescaled per track so the posteriors of the bench meeting cover the recipe thresholds
    (a DER comparison that can fail) instead of sitting on a near-constant plateau.  dynamic: the 'dynamic'
    variant (tests/golden/calibrate_dynamic.py): two upstream layers centred and scaled so the activations vary with
    the frame, fc at a gain of DYN_FC_GAIN."""
    layout = tsvad_layout(cfg)
    if cfg.variant in (5, 6):
        # the encoder part: wavlm_state_dict's sharp weights (the terms the extractor goldens are sensitive to); the
        # rest seeded as for every other variant, with weights.weight non-uniform and wavlmlnorm's affine perturbed
        if spread or dynamic:
            raise ValueError("no spread / dynamic calibration for the WavLM speech encoders")
        enc = wavlm_state_dict(cfg.effective_wavlm_cfg(), seed)
        rest = synthetic_state_dict([e for e in layout if not e[0].startswith("speech_encoder.")], seed + 1)
        return OrderedDict([("speech_encoder." + k, v) for k, v in enc.items()] + list(rest.items()))
    if cfg.variant == 7:
        # the encoder part: w2vbert_state_dict's sharp weights; the rest seeded as for every other variant
        if spread or dynamic:
            raise ValueError("no spread / dynamic calibration for the w2v-bert2 speech encoder")
        enc = w2vbert_state_dict(cfg.effective_w2vbert_cfg(), seed)
        rest = synthetic_state_dict([e for e in layout if not e[0].startswith("speech_encoder.")], seed + 1)
        return OrderedDict([("speech_encoder." + k, v) for k, v in enc.items()] + list(rest.items()))
    if cfg.variant == 8:
        # the encoder part: whisper_state_dict's sharp weights; the rest seeded as for every other variant
        if spread or dynamic:
            raise ValueError("no spread / dynamic calibration for the whisper speech encoder")
        enc = whisper_state_dict(cfg.effective_whisper_cfg(), seed)
        rest = synthetic_state_dict([e for e in layout if not e[0].startswith("speech_encoder.")], seed + 1)
        return OrderedDict([("speech_encoder." + k, v) for k, v in enc.items()] + list(rest.items()))
    sd = synthetic_state_dict(layout, seed)
    if spread and dynamic:
        raise ValueError("spread and dynamic are two different variants")
    if dynamic:
        if seed != 777:
            raise ValueError("the dynamic variant is calibrated for seed 777")
        return dynamic_weights(sd, cfg, dynamic_calibration())
    return spread_fc(sd, cfg, seed) if spread else sd


# 'dynamic' variant gains (tests/golden/calibrate_dynamic.py): the GSP statistic enters the conformer at unit variance
# (G_GSP), the BiLSTM gates swing G_IH times further around their operating point, fc is scaled by <= 4.
DYN_G_GSP = 1.0
DYN_G_IH = 8.0
DYN_FC_GAIN = 4.0
_DYN_CACHE: dict = {}


def dynamic_calibration() -> Dict[str, np.ndarray]:
    """The oracle statistics tests/golden/calibrate_dynamic.py measured on the bench meeting (seed 777, first 48
    windows): weights_dynamic.npz next to this file (data, no code)."""
    if not _DYN_CACHE:
        import os
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "weights_dynamic.npz")) as z:
            _DYN_CACHE.update({k: np.asarray(z[k], np.float64) for k in z.files})
    return _DYN_CACHE


def dynamic_weights(sd, cfg: TSVADConfig, c: Dict[str, np.ndarray], stage: int = 3):
    """Apply the dynamic variant's gains (stage < 3: the partial variants the calibration measures on)."""
    out = OrderedDict(sd)
    f64 = lambda k: np.asarray(sd[k], np.float64)   # noqa: E731
    if cfg.variant == 1:
        if cfg.rs_len != 6:
            raise ValueError("the dynamic variant is calibrated for ots_vad v1 at rs_len 6")
        mu, sg = c["v1_stat_mean"], c["v1_stat_std"]
        w = f64("gsp_fc.weight")
        out["gsp_fc.weight"] = (w * (DYN_G_GSP / sg)[None, :]).astype(np.float32)
        out["gsp_fc.bias"] = (f64("gsp_fc.bias") - w @ (DYN_G_GSP * mu / sg)).astype(np.float32)
        if stage >= 2:
            xbar = c["v1_conformer_mean"]
            for sfx in ("", "_reverse"):
                wih = f64(f"multi_backend.weight_ih_l0{sfx}")
                out[f"multi_backend.weight_ih_l0{sfx}"] = (wih * DYN_G_IH).astype(np.float32)
                out[f"multi_backend.bias_ih_l0{sfx}"] = (f64(f"multi_backend.bias_ih_l0{sfx}")
                                                        - (DYN_G_IH - 1.0) * (wih @ xbar)).astype(np.float32)
        if stage < 3:
            return out
        mean = c["v1_logit_mean"]
    else:
        if cfg.rs_len != 4 or cfg.variant != 0:
            raise ValueError("the dynamic variant is calibrated for the CAM++/transformer model at rs_len 4")
        mean = c["v0_logit_mean"]
    out["fc.weight"] = (f64("fc.weight") * DYN_FC_GAIN).astype(np.float32)
    out["fc.bias"] = (DYN_FC_GAIN * (f64("fc.bias") - mean)).astype(np.float32)
    return out


# Per-track logit mean / std of the seed-777 weights on the first 48 windows of the bench meeting (synth.py seed
# 777), measured by tests/golden/calibrate_spread.py with the fp32 CPU oracle.
SPREAD_FC = {
    (1, 6): {"mean": [0.258351, 0.142728, -0.231329, 0.047318], "std": [0.033554, 0.035482, 0.052413, 0.064769]},
    (0, 4): {"mean": [0.779544, -0.063408, 0.516351, -0.875209], "std": [0.287668, 0.215942, 0.231649, 0.308424]},
}
# target logit std per track and centre (window logits; the overlap mean of 4-6 windows narrows them): chosen so
# a 90-window DER span of the bench meeting has no threshold at DER 100 (measured with the fp32 oracle)
SPREAD = {(1, 6): (8.0, 0.0), (0, 4): (16.0, 2.0)}


def spread_fc(sd, cfg: TSVADConfig, seed: int = 777):
    """logit'_s = k_s (logit_s - mean_s) + c, k_s = std / std_s: only fc.weight / fc.bias change."""
    key = (cfg.variant, cfg.rs_len)
    if seed != 777 or key not in SPREAD_FC:
        raise ValueError(f"no spread calibration for variant/rs_len {key} seed {seed}")
    c = SPREAD_FC[key]
    std, centre = SPREAD[key]
    k = std / np.asarray(c["std"], np.float64)
    out = OrderedDict(sd)
    w = np.asarray(sd["fc.weight"], np.float64)
    b = np.asarray(sd["fc.bias"], np.float64)
    out["fc.weight"] = (w * k[:, None]).astype(np.float32)
    out["fc.bias"] = (k * (b - np.asarray(c["mean"], np.float64)) + centre).astype(np.float32)
    return out


@dataclass
class TSVADStreamingConfig:
    """egs/alimeeting/ts_vad2_streaming/model.py:38-79 (TSVADConfig) fields the chunk-streaming
    inference path reads (CAM++ Subsampling4 + wenet pre-LN transformers)."""
    num_attention_head: int = 4
    num_transformer_layer: int = 2
    transformer_embed_dim: int = 384
    transformer_ffn_embed_dim: int = 1536
    speaker_embed_dim: int = 192
    max_num_speaker: int = 4
    pe_max_len: int = 5000           # PositionalEncoding default max_len (model.py:1189-1212)


def _wenet_layer(k: list, p: str, e: int, ffn: int):
    """transformer_chunk_streaming.TransformerEncoderLayer (MultiHeadedAttention with separate
    linear_q/k/v/out, PositionwiseFeedForward w_1/w_2, norm1/norm2)."""
    for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
        k.append((f"{p}self_attn.{n}.weight", (e, e), "linear"))
        k.append((f"{p}self_attn.{n}.bias", (e,), "small"))
    k.append((p + "feed_forward.w_1.weight", (ffn, e), "linear"))
    k.append((p + "feed_forward.w_1.bias", (ffn,), "small"))
    k.append((p + "feed_forward.w_2.weight", (e, ffn), "linear"))
    k.append((p + "feed_forward.w_2.bias", (e,), "small"))
    _ln(k, p + "norm1", e)
    _ln(k, p + "norm2", e)


def tsvad_streaming_layout(cfg: TSVADStreamingConfig) -> list:
    """Key layout of ts_vad2_streaming/model.py TSVADModel (:96-171)."""
    e, se, ns = cfg.transformer_embed_dim, cfg.speaker_embed_dim, cfg.max_num_speaker
    k = campplus_layout("embed.speech_encoder.")
    k.append(("embed.speech_down_or_up.0.weight", (se, 512, 5), "conv1d"))
    k.append(("embed.speech_down_or_up.0.bias", (se,), "small"))
    _bn(k, "embed.speech_down_or_up.1.bn", se)
    for i in range(cfg.num_transformer_layer):
        _wenet_layer(k, f"single_backend.{i}.", e, cfg.transformer_ffn_embed_dim)
    k.append(("backend_down.0.weight", (e, e * ns, 5), "conv1d"))
    k.append(("backend_down.0.bias", (e,), "small"))
    _bn(k, "backend_down.1.bn", e)
    k.append(("pos_encoder.pe", (1, cfg.pe_max_len, e), "pe1"))
    for i in range(cfg.num_transformer_layer):
        _wenet_layer(k, f"multi_backend.{i}.", e, cfg.transformer_ffn_embed_dim)
    k.append(("fc.weight", (ns, e), "linear"))
    k.append(("fc.bias", (ns,), "small"))
    return k


def tsvad_streaming_state_dict(cfg: TSVADStreamingConfig, seed: int = 777):
    return synthetic_state_dict(tsvad_streaming_layout(cfg), seed)


def campplus_state_dict(seed: int = 777, embedding_size: int = 192):
    """Seeded weights for a standalone CAMPPlus (keys head.*, xvector.*)."""
    return synthetic_state_dict(campplus_layout("", embedding_size), seed)


def resnet34_embed_state_dict(seed: int = 777, embed_dim: int = 256, two_emb_layer: bool = False):
    """Seeded weights for a standalone ResNet34 embedding extractor (keys conv1.*, layer*.*, seg_*)."""
    return synthetic_state_dict(resnet34_embed_layout(embed_dim, two_emb_layer), seed)


def simam_resnet34_state_dict(seed: int = 777, embed_dim: int = 256):
    """Seeded weights for a standalone SimAM_ResNet34_ASP extractor (keys front.*, pooling.attention.*, bottleneck.*)."""
    return synthetic_state_dict(simam_resnet34_layout(embed_dim), seed)


def eres2netv2_state_dict(seed: int = 777, base_width: int = 26, scale: int = 2, expansion: int = 2,
                          embedding_size: int = 192):
    """Seeded ERes2NetV2 weights under the reference key names (eres2netv2_layout)."""
    return synthetic_state_dict(eres2netv2_layout(base_width, scale, expansion, embedding_size), seed)


def ecapa_embed_state_dict(seed: int = 777, embed_dim: int = 192):
    """Seeded weights for a standalone ECAPA_TDNN_GLOB_c1024 extractor (keys layer*.*, conv.*, pool.*, bn.*, linear.*)."""
    return synthetic_state_dict(ecapa_embed_layout(embed_dim), seed)


def redimnet_embed_state_dict(seed: int = 777, embed_dim: int = 192):
    """Seeded weights for a standalone ReDimNetB2 extractor (keys backbone.*, pool.*, seg_1.*; redimnet_layout)."""
    return synthetic_state_dict(redimnet_layout("", embed_dim), seed)


WAVLM_CONV_LAYERS = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2


def wavlm_layout(cfg, prefix: str = "", old_weight_norm: bool = False) -> list:
    """Key layout of WavLM(cfg) (egs/magicdata-ramc/ts_vad2/wavlm.py:256-305) under `prefix`: (name, shape, kind), the
    kind naming no seeding (wavlm_state_dict seeds these).  old_weight_norm: pos_conv's weight_g / weight_v spelling
    instead of parametrizations.weight.original0 / original1; the loaders accept both."""
    D, F, H, L = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_attention_heads, cfg.encoder_layers
    ln_mode = cfg.extractor_mode == "layer_norm"
    k = [("mask_emb", (D,), "wavlm")]
    cin = 1
    for i, (dim, kw, _) in enumerate(WAVLM_CONV_LAYERS):
        p = f"feature_extractor.conv_layers.{i}."
        k.append((p + "0.weight", (dim, cin, kw), "wavlm"))
        if ln_mode or i == 0:
            n = p + ("2.1" if ln_mode else "2")
            k += [(n + ".weight", (dim,), "wavlm"), (n + ".bias", (dim,), "wavlm")]
        cin = dim
    k += [("post_extract_proj.weight", (D, cin), "wavlm"), ("post_extract_proj.bias", (D,), "wavlm"),
          ("encoder.pos_conv.0.bias", (D,), "wavlm")]
    g, v = ("weight_g", "weight_v") if old_weight_norm else ("parametrizations.weight.original0",
                                                             "parametrizations.weight.original1")
    k += [("encoder.pos_conv.0." + g, (1, 1, 128), "wavlm"), ("encoder.pos_conv.0." + v, (D, D // 16, 128), "wavlm")]
    for i in range(L):
        p = f"encoder.layers.{i}."
        k.append((p + "self_attn.grep_a", (1, H, 1, 1), "wavlm"))
        if i == 0:
            k.append((p + "self_attn.relative_attention_bias.weight", (320, H), "wavlm"))
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            k += [(p + f"self_attn.{n}.weight", (D, D), "wavlm"), (p + f"self_attn.{n}.bias", (D,), "wavlm")]
        k += [(p + "self_attn.grep_linear.weight", (8, D // H), "wavlm"), (p + "self_attn.grep_linear.bias", (8,), "wavlm"),
              (p + "self_attn_layer_norm.weight", (D,), "wavlm"), (p + "self_attn_layer_norm.bias", (D,), "wavlm"),
              (p + "fc1.weight", (F, D), "wavlm"), (p + "fc1.bias", (F,), "wavlm"),
              (p + "fc2.weight", (D, F), "wavlm"), (p + "fc2.bias", (D,), "wavlm"),
              (p + "final_layer_norm.weight", (D,), "wavlm"), (p + "final_layer_norm.bias", (D,), "wavlm")]
    k += [("encoder.layer_norm.weight", (D,), "wavlm"), ("encoder.layer_norm.bias", (D,), "wavlm"),
          ("layer_norm.weight", (cin,), "wavlm"), ("layer_norm.bias", (cin,), "wavlm")]
    return [(prefix + n, s, kind) for n, s, kind in k]


def wavlm_state_dict(cfg, seed: int = 777):
    """Seeded WavLM weights under the reference key names (egs/magicdata-ramc/ts_vad2/wavlm.py:256-305; cfg: a
    WavLMConfig of speaker_diarization_amd.ssl.wavlm or any object with its fields).  The reference's own
    initialisation leaves the gated relative-position bias nearly inert (zeroing the bias table moves a 2-layer output
    of max |x| 4 by 8e-3, zeroing grep_linear by 2e-4), so a golden made from it would pass with either wrong.  Here the
    q / k projections are 6x and the v / out / fc weights 2x the reference's N(0, 0.02), the bias table is N(0, 1.5),
    grep_linear N(0, 0.5), grep_a 1 + 0.5 N, the weight-norm gains g are 0.7 .. 1.3 of |v|, and every bias and norm
    affine is perturbed by 0.1 N: tests/golden/make_golden_wavlm.py asserts that each of these terms moves the stored
    outputs by at least ten times the fp32 bar."""
    rng = np.random.default_rng(seed)
    D, F, H, L = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_attention_heads, cfg.encoder_layers
    ln_mode = cfg.extractor_mode == "layer_norm"
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()

    def put(name, v):
        sd[name] = np.ascontiguousarray(v, dtype=np.float32)

    def normal(shape, std):
        return rng.standard_normal(shape) * std

    def affine(prefix, n):
        put(prefix + ".weight", 1.0 + normal(n, 0.1))
        put(prefix + ".bias", normal(n, 0.1))

    def linear(prefix, n, k, std):
        put(prefix + ".weight", normal((n, k), std))
        put(prefix + ".bias", normal(n, 0.1))

    put("mask_emb", rng.uniform(0.0, 1.0, D))
    cin = 1
    for i, (dim, k, _) in enumerate(WAVLM_CONV_LAYERS):
        p = f"feature_extractor.conv_layers.{i}."
        put(p + "0.weight", normal((dim, cin, k), np.sqrt(2.0 / (cin * k))))
        if ln_mode:
            affine(p + "2.1", dim)
        elif i == 0:
            affine(p + "2", dim)
        cin = dim
    b = 1.0 / np.sqrt(cin)
    put("post_extract_proj.weight", rng.uniform(-b, b, (D, cin)))
    put("post_extract_proj.bias", normal(D, 0.1))
    put("encoder.pos_conv.0.bias", normal(D, 0.1))
    v = normal((D, D // 16, 128), np.sqrt(4.0 / (128 * D)))
    g = np.sqrt((v * v).sum(axis=(0, 1), keepdims=True)) * rng.uniform(0.7, 1.3, (1, 1, 128))
    put("encoder.pos_conv.0.parametrizations.weight.original0", g)
    put("encoder.pos_conv.0.parametrizations.weight.original1", v)
    for i in range(L):
        p = f"encoder.layers.{i}."
        put(p + "self_attn.grep_a", 1.0 + normal((1, H, 1, 1), 0.5))
        if i == 0:
            put(p + "self_attn.relative_attention_bias.weight", normal((320, H), 1.5))
        linear(p + "self_attn.k_proj", D, D, 0.12)
        linear(p + "self_attn.v_proj", D, D, 0.04)
        linear(p + "self_attn.q_proj", D, D, 0.12)
        linear(p + "self_attn.out_proj", D, D, 0.04)
        put(p + "self_attn.grep_linear.weight", normal((8, D // H), 0.5))
        put(p + "self_attn.grep_linear.bias", normal(8, 0.5))
        affine(p + "self_attn_layer_norm", D)
        linear(p + "fc1", F, D, 0.04)
        linear(p + "fc2", D, F, 0.04)
        affine(p + "final_layer_norm", D)
    affine("encoder.layer_norm", D)
    affine("layer_norm", cin)
    return sd


def w2vbert_layout(cfg, prefix: str = "") -> list:
    """Key layout of transformers' Wav2Vec2BertModel(cfg) (modeling_wav2vec2_bert.py:923-945) with relative_key position
    embeddings and no adapter, under `prefix`: (name, shape, kind), in the module's registration order; the kind names no
    seeding (w2vbert_state_dict seeds these).  cfg: a W2vBertConfig of speaker_diarization_amd.ssl.w2vbert or any
    object with its fields."""
    D, F, L = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
    hd = D // cfg.num_attention_heads
    nd = cfg.left_max_position_embeddings + cfg.right_max_position_embeddings + 1
    kk, din = cfg.conv_depthwise_kernel_size, cfg.feature_projection_input_dim

    def ln(p, n):
        return [(p + ".weight", (n,), "w2vbert"), (p + ".bias", (n,), "w2vbert")]

    def lin(p, n, m):
        return [(p + ".weight", (n, m), "w2vbert"), (p + ".bias", (n,), "w2vbert")]

    k = [("masked_spec_embed", (D,), "w2vbert")]
    k += ln("feature_projection.layer_norm", din) + lin("feature_projection.projection", D, din)
    for i in range(L):
        p = f"encoder.layers.{i}."
        k += ln(p + "ffn1_layer_norm", D)
        k += lin(p + "ffn1.intermediate_dense", F, D) + lin(p + "ffn1.output_dense", D, F)
        k += ln(p + "self_attn_layer_norm", D)
        for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
            k += lin(p + "self_attn." + n, D, D)
        k.append((p + "self_attn.distance_embedding.weight", (nd, hd), "w2vbert"))
        k += ln(p + "conv_module.layer_norm", D)
        k.append((p + "conv_module.pointwise_conv1.weight", (2 * D, D, 1), "w2vbert"))
        k.append((p + "conv_module.depthwise_conv.weight", (D, 1, kk), "w2vbert"))
        k += ln(p + "conv_module.depthwise_layer_norm", D)
        k.append((p + "conv_module.pointwise_conv2.weight", (D, D, 1), "w2vbert"))
        k += ln(p + "ffn2_layer_norm", D)
        k += lin(p + "ffn2.intermediate_dense", F, D) + lin(p + "ffn2.output_dense", D, F)
        k += ln(p + "final_layer_norm", D)
    return [(prefix + n, s, kind) for n, s, kind in k]


# Seeded w2v-BERT 2.0 init (w2vbert_layout).  The q / k projections give per-head q . k / 8 a standard deviation of about
# 2.3 on LayerNorm'd rows (q and k entries ~ N(0, 1.5^2): 1.5 * 1.5 * sqrt(64) / 8 = 2.25), and the distance embedding is
# N(0, 1.5^2) too, so q . E / 8 has the same spread: the attention is sharp and the distance term carries half of the
# score variance.  tests/golden/make_golden_w2vbert.py asserts that zeroing it, flipping the distance's sign or swapping
# the clamp bounds each move the stored logits by at least ten fp32 bars.
W2V_QK_STD = 1.5 / 32.0       # on 1024 unit-variance inputs: output std 1.5
W2V_DIST_STD = 1.5


def w2vbert_state_dict(cfg, seed: int = 777):
    """Seeded w2v-BERT 2.0 weights under the HF key names (see W2V_QK_STD above); every bias and norm affine is
    perturbed by 0.1 N, the value / output / FFN / pointwise weights are drawn so that each sub-block's output is O(1)
    on the LayerNorm'd stream, the depthwise taps so that the 31-tap sum has unit gain."""
    rng = np.random.default_rng(seed)
    D, F = cfg.hidden_size, cfg.intermediate_size
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for name, shape, _ in w2vbert_layout(cfg):
        leaf = name.rsplit(".", 2)[-2] if name.count(".") else name
        if name == "masked_spec_embed":
            v = rng.uniform(0.0, 1.0, shape)
        elif name.endswith(".bias"):
            v = rng.standard_normal(shape) * 0.1
        elif "layer_norm" in leaf:
            v = 1.0 + rng.standard_normal(shape) * 0.1
        elif leaf in ("linear_q", "linear_k"):
            v = rng.standard_normal(shape) * W2V_QK_STD
        elif leaf == "distance_embedding":
            v = rng.standard_normal(shape) * W2V_DIST_STD
        elif leaf == "depthwise_conv":
            v = rng.standard_normal(shape) / np.sqrt(shape[-1])
        elif leaf == "pointwise_conv1":
            v = rng.standard_normal(shape) * (1.5 / np.sqrt(shape[1]))   # gates of standard deviation 1.5: a live GLU
        elif leaf == "output_dense":
            v = rng.standard_normal(shape) * (2.0 / np.sqrt(shape[1]))   # swish halves the hidden layer's scale
        else:   # projection, linear_v, linear_out, intermediate_dense, pointwise_conv2
            v = rng.standard_normal(shape) / np.sqrt(shape[1])
        sd[name] = np.ascontiguousarray(v, dtype=np.float32)
    return sd


def whisper_layout(cfg, prefix: str = "") -> list:
    """Key layout of the reference's WhisperEncoder(cfg) (egs/magicdata-ramc/ts_vad2/whisper_encoder.py:150-191) under
    `prefix`: (name, shape, kind) in state_dict order (parameters in registration order, the positional_embedding
    buffer after them, as nn.Module.state_dict lists a module's own parameters before its buffers and both before its
    children); attn.key has no bias (:66).  cfg: a WhisperConfig of speaker_diarization_amd.ssl.whisper or any object
    with ModelDimensions' fields."""
    D, M, L = cfg.n_audio_state, cfg.n_mels, cfg.n_audio_layer
    W = D * (cfg.layer_ed - cfg.layer_st + 1)

    def wb(p, *shape):
        return [(p + ".weight", tuple(shape), "whisper"), (p + ".bias", (shape[0],), "whisper")]

    k = [("positional_embedding", (cfg.n_audio_ctx, D), "whisper")]
    k += wb("conv1", D, M, 3) + wb("conv2", D, D, 3)
    for i in range(L):
        p = f"layers.{i}."
        k += wb(p + "attn.query", D, D)
        k.append((p + "attn.key.weight", (D, D), "whisper"))
        k += wb(p + "attn.value", D, D) + wb(p + "attn.out", D, D)
        k += wb(p + "attn_ln", D)
        k += wb(p + "mlp.0", 4 * D, D) + wb(p + "mlp.2", D, 4 * D)
        k += wb(p + "mlp_ln", D)
    k += wb("ln_post2", W)
    return [(prefix + n, s, kind) for n, s, kind in k]


def whisper_sinusoids(length: int, channels: int) -> np.ndarray:
    """sinusoids() of whisper_encoder.py:50-58, the positional_embedding buffer the reference registers."""
    inc = np.log(10000.0) / (channels // 2 - 1)
    t = np.arange(length)[:, None] * np.exp(-inc * np.arange(channels // 2))[None, :]
    return np.concatenate([np.sin(t), np.cos(t)], axis=1).astype(np.float32)


# Seeded Whisper encoder init (whisper_layout).  query / key rows give per-head q . k / 8 a standard deviation of about 2.3
# on LayerNorm'd rows, as for w2v-BERT above: the attention is sharp.  The positional table is the reference's sinusoids
# PLUS 0.05 N noise: a model that recomputes the table instead of using the loaded buffer misses the goldens.
WHISPER_QK_STD = 1.5


def whisper_state_dict(cfg, seed: int = 888):
    """Seeded Whisper-PMFA encoder weights under the reference class's key names; every bias and norm affine is
    perturbed by 0.1 N, the other weights are drawn so that each sub-block's output is O(1) on the LayerNorm'd
    stream."""
    rng = np.random.default_rng(seed)
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for name, shape, _ in whisper_layout(cfg):
        leaf = name.rsplit(".", 2)[-2] if name.count(".") else name
        if name == "positional_embedding":
            v = whisper_sinusoids(*shape) + rng.standard_normal(shape) * 0.05
        elif name.endswith(".bias"):
            v = rng.standard_normal(shape) * 0.1
        elif leaf in ("attn_ln", "mlp_ln", "ln_post2"):
            v = 1.0 + rng.standard_normal(shape) * 0.1
        elif leaf in ("conv1", "conv2"):
            v = rng.standard_normal(shape) * (1.5 / np.sqrt(shape[1] * shape[2]))
        elif leaf in ("query", "key"):
            v = rng.standard_normal(shape) * (WHISPER_QK_STD / np.sqrt(shape[1]))
        elif leaf == "2":   # mlp.2: GELU halves the hidden layer's scale
            v = rng.standard_normal(shape) * (2.0 / np.sqrt(shape[1]))
        else:   # value, out, mlp.0
            v = rng.standard_normal(shape) / np.sqrt(shape[1])
        sd[name] = np.ascontiguousarray(v, dtype=np.float32)
    return sd


def to_torch(sd):
    import torch
    return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())


def unwrap_checkpoint(obj, kind: str = "tsvad"):
    """Accept the reference's three on-disk layouts and return a flat state_dict."""
    if isinstance(obj, dict) and "model" in obj and isinstance(obj["model"], dict):
        return obj["model"]
    if isinstance(obj, dict) and "state_dict" in obj:
        sd = obj["state_dict"]
        return OrderedDict((k[len("model."):] if k.startswith("model.") else k, v) for k, v in sd.items())
    return obj


# ----------------------------------------------------------------------------- EEND-EDA
@dataclass
class EDAConfig:
    """Constructor arguments of TransformerEdaModel (eend_eda/models.py:161) and
    EendEdaModel (models.py:466-467) as eend_eda/infer_eda.py:50-71 passes them."""
    model_type: str = "TransformerEda"     # "TransformerEda" | "EendEda" | "ConformerEda"
    n_speakers: int = 2
    in_size: int = 345                     # feature.get_input_dim(…, context 7, logmel23*) = 15 * 23
    n_heads: int = 4
    n_units: int = 256
    n_layers: int = 2
    dim_feedforward: int = 2048            # never passed by infer_eda.py
    encoder_type: str = "transformer"      # EendEda: "transformer" | "conformer"

    @property
    def variant(self) -> int:
        """0: TransformerEdaModel, 1: EendEdaModel(transformer), 2: EendEdaModel(conformer)."""
        if self.model_type == "TransformerEda":
            return 0
        if self.model_type == "ConformerEda":
            return 2
        if self.model_type == "EendEda":
            if self.encoder_type == "transformer":
                return 1
            if self.encoder_type == "conformer":
                return 2
            raise NotImplementedError(f"encoder_type not support {self.encoder_type}!!!")
        raise ValueError("Unknown model type.")


def _lstm(k: list, p: str, i: int, h: int):
    k.append((p + "weight_ih_l0", (4 * h, i), "lstm"))
    k.append((p + "weight_hh_l0", (4 * h, h), "lstm"))
    k.append((p + "bias_ih_l0", (4 * h,), "lstm"))
    k.append((p + "bias_hh_l0", (4 * h,), "lstm"))


def eda_layout(cfg: EDAConfig) -> list:
    """Key layout of TransformerEdaModel / EendEdaModel (eend_eda/models.py:161-210,
    466-512; encoder_decoder_attractor.py:8-16)."""
    e, v = cfg.n_units, cfg.variant
    k: list = []
    inp, norm = ("encoder", "encoder_norm") if v == 0 else ("linear", "linear_norm")
    k.append((inp + ".weight", (e, cfg.in_size), "linear"))
    k.append((inp + ".bias", (e,), "small"))
    _ln(k, norm, e)
    if v in (0, 1):
        root = "transformer_encoder" if v == 0 else "encoder"
        for i in range(cfg.n_layers):
            _tfm(k, f"{root}.layers.{i}.", e, cfg.dim_feedforward)
    else:
        for i in range(cfg.n_layers):
            p = f"encoder.conformer_layers.{i}."
            _conformer_layer(k, p, e, cfg.dim_feedforward, 31, group_norm=False)
    _lstm(k, "eda.encoder.", e, e)
    _lstm(k, "eda.decoder.", e, e)
    k.append(("eda.linear.weight", (1, e), "linear"))
    k.append(("eda.linear.bias", (1,), "small"))
    return k


def _conformer_layer(k: list, p: str, e: int, ffn: int, kernel: int, group_norm: bool):
    """torchaudio.models.conformer.ConformerLayer parameter names (2.5.1)."""
    for f in ("ffn1", "ffn2"):
        _ln(k, p + f + ".sequential.0", e)
        k.append((p + f + ".sequential.1.weight", (ffn, e), "linear"))
        k.append((p + f + ".sequential.1.bias", (ffn,), "small"))
        k.append((p + f + ".sequential.4.weight", (e, ffn), "linear"))
        k.append((p + f + ".sequential.4.bias", (e,), "small"))
        if f == "ffn1":
            _ln(k, p + "self_attn_layer_norm", e)
            _mha(k, p + "self_attn.", e)
            _ln(k, p + "conv_module.layer_norm", e)
            k.append((p + "conv_module.sequential.0.weight", (2 * e, e, 1), "conv1d"))
            k.append((p + "conv_module.sequential.0.bias", (2 * e,), "small"))
            k.append((p + "conv_module.sequential.2.weight", (e, 1, kernel), "conv1d"))
            k.append((p + "conv_module.sequential.2.bias", (e,), "small"))
            if group_norm:
                k.append((p + "conv_module.sequential.3.weight", (e,), "ln_w"))
                k.append((p + "conv_module.sequential.3.bias", (e,), "small"))
            else:
                _bn(k, p + "conv_module.sequential.3", e)
            k.append((p + "conv_module.sequential.5.weight", (e, e, 1), "conv1d"))
            k.append((p + "conv_module.sequential.5.bias", (e,), "small"))
    _ln(k, p + "final_layer_norm", e)


def eda_state_dict(cfg: EDAConfig, seed: int = 777):
    return synthetic_state_dict(eda_layout(cfg), seed)


def eend_layout(cfg: EDAConfig) -> list:
    """Key layout of the plain EEND TransformerModel (eend/models.py:17-55)."""
    e = cfg.n_units
    k: list = [("encoder.weight", (e, cfg.in_size), "linear"), ("encoder.bias", (e,), "small")]
    _ln(k, "encoder_norm", e)
    for i in range(cfg.n_layers):
        _tfm(k, f"transformer_encoder.layers.{i}.", e, cfg.dim_feedforward)
    k.append(("decoder.weight", (cfg.n_speakers, e), "linear"))
    k.append(("decoder.bias", (cfg.n_speakers,), "small"))
    return k


# ----------------------------------------------------------------------------- FS-EEND
@dataclass
class FSEENDConfig:
    """OnlineTransformerDADiarization(**configs["model"]["params"]) as fs_eend/train.py:71-75
    builds it from config/spk_onl_tfm_enc_dec_nonautoreg_infer.yaml."""
    n_speakers: int = None
    in_size: int = 345                 # (2 * context_recp + 1) * n_mels
    n_units: int = 256
    n_heads: int = 4
    enc_n_layers: int = 4
    dec_n_layers: int = 2
    dropout: float = 0.1
    has_mask: bool = True
    max_seqlen: int = 10000
    dec_dim_feedforward: int = 2048
    conv_delay: int = 9
    mask_delay: int = 0
    enc_dim_feedforward: int = 2048    # MaskedTransformerEncoderModel default (never passed)
    pe_max_len: int = 5000             # PositionalEncoding default max_len


def fseend_layout(cfg: FSEENDConfig) -> list:
    """Key layout of OnlineTransformerDADiarization (fs_eend/fs_eend.py:20-41, 99-170,
    207-240, 282-333).  The decoder ModuleList holds ONE layer object dec_n_layers
    times, so its keys appear under every index with identical values."""
    e, d = cfg.n_units, cfg.in_size
    k: list = []
    _bn(k, "enc.bn", d)
    k.append(("enc.encoder.weight", (e, d), "linear"))
    k.append(("enc.encoder.bias", (e,), "small"))
    _ln(k, "enc.encoder_norm", e)
    for i in range(cfg.enc_n_layers):
        _tfm(k, f"enc.transformer_encoder.layers.{i}.", e, cfg.enc_dim_feedforward)
    k.append(("dec.encoder.weight", (e, d), "linear"))
    k.append(("dec.encoder.bias", (e,), "small"))
    _ln(k, "dec.encoder_norm", e)
    k.append(("dec.pos_enc.pe", (1, cfg.pe_max_len, e), "pe"))
    k.append(("dec.convert.weight", (e, 2 * e), "linear"))
    k.append(("dec.convert.bias", (e,), "small"))
    for i in range(cfg.dec_n_layers):
        p = f"dec.attractor_decoder.{i}."
        _mha(k, p + "self_attn1.", e)
        _mha(k, p + "self_attn2.", e)
        k.append((p + "linear1.weight", (cfg.dec_dim_feedforward, e), "linear"))
        k.append((p + "linear1.bias", (cfg.dec_dim_feedforward,), "small"))
        k.append((p + "linear2.weight", (e, cfg.dec_dim_feedforward), "linear"))
        k.append((p + "linear2.bias", (e,), "small"))
        for n in ("norm11", "norm12", "norm21", "norm22"):
            _ln(k, p + n, e)
    k.append(("cnn.weight", (e, e, 2 * cfg.conv_delay + 1), "conv1d"))
    k.append(("cnn.bias", (e,), "small"))
    return k


def fseend_state_dict(cfg: FSEENDConfig, seed: int = 777):
    sd = synthetic_state_dict(fseend_layout(cfg), seed)
    sd["dec.pos_enc.pe"] = sinusoid_pe(cfg.pe_max_len, cfg.n_units).reshape(1, cfg.pe_max_len, cfg.n_units)
    # shared decoder layer: every index carries the same tensors (fs_eend.py:118)
    for k in list(sd):
        if k.startswith("dec.attractor_decoder.0."):
            for i in range(1, cfg.dec_n_layers):
                sd[k.replace(".0.", f".{i}.", 1)] = sd[k]
    return sd


# ----------------------------------------------------------------------------- SSND
@dataclass
class SSNDConfig:
    """SSNDModel constructor arguments (egs/alimeeting/ssnd/ssnd_model.py:373-412) the inference
    path reads; extractor 'CAM++_wo_gsp' (ssnd_model.py:107-124)."""
    extractor_model_type: str = "CAM++_wo_gsp"
    feat_dim: int = 80
    emb_dim: int = 256
    q_det_aux_dim: int = 256
    q_rep_aux_dim: int = 256
    d_model: int = 256
    nhead: int = 8
    d_ff: int = 512
    num_layers: int = 4
    max_speakers: int = 4
    vad_out_len: int = 200
    pos_emb_dim: int = 256
    max_seq_len: int = 1000
    n_all_speakers: int = 1000
    conformer_kernel: int = 15      # SSNDConformerEncoder cnn_kernel_size (ssnd_model.py:174)


def _swdecoder(k: list, p: str, d: int, ff: int, d_aux: int, d_pos: int):
    """SWDecoderBlockV2 (ssnd_model.py:225-244) parameter names."""
    k.append((p + "fq.linear.weight", (d, d_aux), "linear"))
    k.append((p + "fq.linear.bias", (d,), "small"))
    k.append((p + "fk.linear.weight", (d, d_pos), "linear"))
    k.append((p + "fk.linear.bias", (d,), "small"))
    _mha(k, p + "cross_attn.", d)
    _mha(k, p + "self_attn.", d)
    k.append((p + "ffn.0.weight", (ff, d), "linear"))
    k.append((p + "ffn.0.bias", (ff,), "small"))
    k.append((p + "ffn.3.weight", (d, ff), "linear"))
    k.append((p + "ffn.3.bias", (d,), "small"))
    for n in (1, 2, 3):
        _ln(k, p + f"norm{n}", d)


def ssnd_layout(cfg: SSNDConfig) -> list:
    """Key layout of SSNDModel(cfg) (ssnd_model.py:373-441), extractor CAM++_wo_gsp."""
    if cfg.extractor_model_type != "CAM++_wo_gsp":
        raise ValueError(f"the MI355X SSND backend builds extractor CAM++_wo_gsp, got {cfg.extractor_model_type}")
    d, e = cfg.d_model, cfg.emb_dim
    k: list = [("pos_emb", (1, cfg.max_seq_len, cfg.pos_emb_dim), "randn"),
               ("E_all", (cfg.n_all_speakers, e), "randn"), ("e_pse", (1, e), "randn"), ("e_non", (1, e), "randn"),
               ("det_query_emb", (cfg.max_speakers, d), "randn"),
               ("rep_query_emb", (cfg.max_speakers, cfg.vad_out_len), "randn")]
    k += campplus_layout("extractor.speech_encoder.", 192)
    k.append(("extractor.speech_encoder.output_proj.weight", (e, 512), "linear"))
    k.append(("extractor.speech_encoder.output_proj.bias", (e,), "small"))
    k.append(("extractor.speech_down_or_up.0.weight", (e, e, 5), "conv1d"))
    k.append(("extractor.speech_down_or_up.0.bias", (e,), "small"))
    _bn(k, "extractor.speech_down_or_up.1.bn", e)
    k.append(("encoder.input_proj.weight", (d, e), "linear"))
    k.append(("encoder.input_proj.bias", (d,), "small"))
    for i in range(cfg.num_layers):
        _conformer_layer(k, f"encoder.encoder.conformer_layers.{i}.", d, cfg.d_ff, cfg.conformer_kernel, False)
    for i in range(cfg.num_layers):
        _swdecoder(k, f"det_decoder.layers.{i}.", d, cfg.d_ff, cfg.q_det_aux_dim, cfg.pos_emb_dim)
    k.append(("det_decoder.out_proj.weight", (cfg.vad_out_len, d), "linear"))
    k.append(("det_decoder.out_proj.bias", (cfg.vad_out_len,), "zero"))
    k.append(("rep_decoder.input_proj.weight", (d, e), "linear"))
    k.append(("rep_decoder.input_proj.bias", (d,), "small"))
    k.append(("rep_decoder.xdec_proj.weight", (d, 1), "randn"))
    k.append(("rep_decoder.xdec_proj.bias", (d,), "small"))
    k.append(("rep_decoder.qaux_proj.weight", (cfg.q_rep_aux_dim, 1), "randn"))
    k.append(("rep_decoder.qaux_proj.bias", (cfg.q_rep_aux_dim,), "small"))
    for i in range(cfg.num_layers):
        _swdecoder(k, f"rep_decoder.layers.{i}.", d, cfg.d_ff, cfg.q_rep_aux_dim, cfg.pos_emb_dim)
    k.append(("rep_decoder.out_proj.weight", (e, d), "linear"))
    k.append(("rep_decoder.out_proj.bias", (e,), "small"))
    return k


def ssnd_state_dict(cfg: SSNDConfig, seed: int = 777):
    return synthetic_state_dict(ssnd_layout(cfg), seed)
