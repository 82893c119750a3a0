"""ctypes binding of libsdiar.so (include/sdiar.h).

The HIP library is the only compute path: if it is missing or fails to load,
every entry point raises immediately — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDIAR_LIB", os.path.join(_HERE, "lib", "libsdiar.so"))

SD_OK = 0
SD_ERR_INVALID = -1
SD_ERR_SHAPE = -2
SD_ERR_PARAM = -3
SD_ERR_HIP = -4
SD_ERR_STATE = -5


class SdiarError(RuntimeError):
    """Device / runtime failure inside libsdiar."""


class TsvadConfig(ctypes.Structure):
    _fields_ = [
        ("variant", c_int),
        ("max_num_speaker", c_int),
        ("rs_len", c_int),
        ("max_batch", c_int),
        ("max_fbank_frames", c_int),
        ("precision", c_int),
        ("num_transformer_layer", c_int),
        ("num_attention_head", c_int),
        ("transformer_embed_dim", c_int),
        ("transformer_ffn_embed_dim", c_int),
        ("speaker_embed_dim", c_int),
        ("backend", c_int),    # 0 the variant's own; 1 mamba2 + transformer; 2 mamba2 + mamba2; 4 conformer + transformer;
                               # 5 conformer + conformer (1, 2, 4, 5: variant 0 only)
        ("d_state", c_int),
        ("expand", c_int),
        # variants 5 / 6 (WavLM / WavLM_weight_sum on the raw waveform); all zero otherwise
        ("wavlm_embed_dim", c_int),
        ("wavlm_layers", c_int),
        ("wavlm_layer_norm_mode", c_int),
        ("wavlm_pre_ln", c_int),
        ("max_samples", c_int),
        # variant 7 (w2v-bert2): encoder layers; zero otherwise
        ("w2vbert_layers", c_int),
    ]


class TsvadConfigEx(TsvadConfig):
    """sd_tsvad_config_ex: sd_tsvad_config followed by the fields added since (ctypes lays a subclass's fields out after
    its base's).  sd_tsvad_create_ex takes it; all new fields zero is sd_tsvad_create."""
    _fields_ = [
        ("frame_level_gsp", c_int),   # 1: speech_encoder_type "CAM++_frame_level_gsp_fc" (variant 0 only)
    ]


class EdaConfig(ctypes.Structure):
    _fields_ = [
        ("variant", c_int),
        ("in_size", c_int),
        ("n_units", c_int),
        ("n_heads", c_int),
        ("n_layers", c_int),
        ("dim_feedforward", c_int),
        ("max_seqs", c_int),
        ("max_frames", c_int),
        ("max_n_speakers", c_int),
        ("precision", c_int),
        ("n_speakers", c_int),
    ]


class FseendConfig(ctypes.Structure):
    _fields_ = [
        ("in_size", c_int),
        ("n_units", c_int),
        ("n_heads", c_int),
        ("enc_n_layers", c_int),
        ("enc_dim_feedforward", c_int),
        ("dec_n_layers", c_int),
        ("dec_dim_feedforward", c_int),
        ("conv_delay", c_int),
        ("mask_delay", c_int),
        ("has_mask", c_int),
        ("max_seqs", c_int),
        ("max_frames", c_int),
        ("max_nspks", c_int),
        ("precision", c_int),
    ]


class CamppConfig(ctypes.Structure):
    _fields_ = [
        ("feat_dim", c_int),
        ("embedding_size", c_int),
        ("max_batch", c_int),
        ("max_frames", c_int),
        ("precision", c_int),
    ]


class Resnet34Config(ctypes.Structure):
    _fields_ = [
        ("feat_dim", c_int),
        ("embed_dim", c_int),
        ("two_emb_layer", c_int),
        ("max_batch", c_int),
        ("max_frames", c_int),
        ("precision", c_int),
    ]


class SimamResnet34Config(ctypes.Structure):
    _fields_ = [
        ("in_planes", c_int),
        ("embed_dim", c_int),
        ("acoustic_dim", c_int),
        ("max_batch", c_int),
        ("max_frames", c_int),
        ("precision", c_int),
    ]


class Eres2netv2Config(ctypes.Structure):
    _fields_ = [
        ("feat_dim", c_int),
        ("embedding_size", c_int),
        ("m_channels", c_int),
        ("base_width", c_int),
        ("scale", c_int),
        ("expansion", c_int),
        ("max_batch", c_int),
        ("max_frames", c_int),
        ("precision", c_int),
    ]


class EcapaConfig(ctypes.Structure):
    _fields_ = [
        ("channels", c_int),
        ("embed_dim", c_int),
        ("max_batch", c_int),
        ("max_frames", c_int),
        ("precision", c_int),
    ]


class RedimnetConfig(ctypes.Structure):
    _fields_ = [
        ("feat_dim", c_int),
        ("embed_dim", c_int),
        ("max_batch", c_int),
        ("max_frames", c_int),
        ("precision", c_int),
    ]


class WavlmConfig(ctypes.Structure):
    _fields_ = [(n, c_int) for n in (
        "embed_dim", "ffn_dim", "heads", "encoder_layers", "extractor_mode", "layer_norm_first", "max_batch",
        "max_samples", "precision")]


class W2vbertConfig(ctypes.Structure):
    _fields_ = [(n, c_int) for n in (
        "hidden", "heads", "ffn", "layers", "conv_kernel", "left", "right", "in_dim", "precision", "max_batch",
        "max_frames", "position_embeddings", "add_adapter")]


class WhisperConfig(ctypes.Structure):
    _fields_ = [(n, c_int) for n in (
        "n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer", "layer_st", "layer_ed", "precision",
        "max_batch", "max_samples")]


class SsndConfig(ctypes.Structure):
    _fields_ = [(n, c_int) for n in (
        "max_batch", "max_fbank_frames", "max_speakers", "feat_dim", "emb_dim", "q_det_aux_dim", "q_rep_aux_dim",
        "d_model", "nhead", "d_ff", "num_layers", "vad_out_len", "pos_emb_dim", "max_seq_len", "n_all_speakers",
        "conformer_kernel", "precision")]


class TsvadStreamConfig(ctypes.Structure):
    _fields_ = [
        ("max_num_speaker", c_int),
        ("max_labels", c_int),
        ("precision", c_int),
        ("num_transformer_layer", c_int),
        ("num_attention_head", c_int),
        ("transformer_embed_dim", c_int),
        ("transformer_ffn_embed_dim", c_int),
        ("speaker_embed_dim", c_int),
        ("max_windows", c_int),
    ]


class RowprogFfn(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("ln_g", "ln_b", "w1", "b1", "w2", "b2", "post_g", "post_b")] + [("hidden", c_int)]


class RowprogOp(ctypes.Structure):
    """sd_rowprog_op (include/sdiar.h): one conformer row program, every pointer a device pointer or None."""
    _fields_ = [
        ("M", c_int), ("flags", c_int),
        ("X", c_void_p), ("Xo", c_void_p),
        ("ts", c_void_p), ("mix", c_void_p),
        ("ldmix", c_int), ("Tmix", c_int), ("NS", c_int), ("T_seq", c_int),
        ("A", c_void_p), ("w0", c_void_p), ("b0", c_void_p),
        ("gn_partial", c_void_p), ("gn_g", c_void_p), ("gn_b", c_void_p),
        ("gn_T", c_int), ("gn_nblk", c_int),
        ("n_ffn", c_int),
        ("ffn", RowprogFfn * 2),
        ("y_g", c_void_p), ("y_b", c_void_p), ("y", c_void_p),
        ("yt", c_void_p), ("yt_NS", c_int),
    ]


class GemmOp(ctypes.Structure):
    """sd_gemm_op (include/sdiar.h): one conv_gemm call, every pointer a device pointer or None."""
    _fields_ = [
        ("precision", c_int),
        ("A", c_void_p), ("a_bf16", c_int), ("a_tiled", c_int),
        ("B", c_int), ("H", c_int), ("W", c_int), ("Cin", c_int), ("lda", c_int), ("a_coff", c_int),
        ("kh", c_int), ("kw", c_int), ("sh", c_int), ("sw", c_int), ("ph", c_int), ("pw", c_int), ("dh", c_int),
        ("dw", c_int),
        ("w", c_void_p), ("N", c_int),
        ("pre_scale", c_void_p), ("pre_shift", c_void_p), ("alpha", c_void_p), ("beta", c_void_p),
        ("res", c_void_p), ("res_bf16", c_int), ("res_ld", c_int),
        ("act", c_int),
        ("post_scale", c_void_p), ("post_shift", c_void_p),
        ("gate", c_void_p), ("gate_seg", c_int), ("gate_nseg", c_int),
        ("out", c_void_p), ("out_bf16", c_int),
        ("o_sb", c_int64), ("o_sh", c_int64), ("o_sw", c_int64), ("o_sn", c_int64),
        ("glu", c_int),
        ("ln_x", c_void_p), ("ln_t", c_void_p), ("ln_t_bf16", c_int), ("ln_g", c_void_p), ("ln_b", c_void_p),
        ("ln_eps", ctypes.c_float), ("ln_out", c_void_p),
        ("pro_mode", c_int), ("pro_p", c_void_p), ("pro_C", c_int), ("pro_pad", c_int),
        ("pro_cursor", c_void_p), ("pro_nvalid", c_void_p),
        ("kv_out", c_void_p), ("kv_cursor", c_void_p), ("kv_mult", c_int), ("kv_col0", c_int), ("kv_ld", c_int64),
        ("ksplit_out", c_void_p), ("slabs", c_void_p), ("slab_cap", c_int),
    ]


_SIGS = {
    "sd_op_conv_gemm": (c_int, [POINTER(GemmOp), c_void_p]),
    "sd_last_error": (c_char_p, []),
    "sd_version": (c_int, []),
    "sd_prof_enable": (None, [c_int]),
    "sd_prof_reset": (None, []),
    "sd_prof_query": (c_int, [c_int, c_char_p, c_int, POINTER(c_int64), POINTER(ctypes.c_double),
                              POINTER(ctypes.c_double), POINTER(ctypes.c_double)]),
    "sd_prof_query_steps": (ctypes.c_double, [c_int]),
    "sd_probe_lstm_granule2": (c_int, [c_int, c_void_p, c_void_p]),
    "sd_probe_lstm_granule": (c_int, [c_int, c_void_p, c_void_p]),
    "sd_probe_lstm_handoff": (c_int, [c_int, c_void_p, c_void_p]),
    "sd_tsvad_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sd_tsvad_status": (c_int, [c_void_p, c_void_p]),
    "sd_tsvad_forward_batched": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                         c_void_p]),
    "sd_tsvad_forward_graph": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_char_p,
                                       c_void_p]),
    "sd_tsvad_debug_buffer": (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_int64)]),
    "sd_tsvad_stream_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                        c_void_p]),
    "sd_ssnd_infer": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sd_ssnd_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sd_campp_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sd_resnet34_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sd_simam_resnet34_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sd_debug_simam_variant": (c_int, [c_int]),
    "sd_eres2netv2_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sd_debug_clamp_route": (c_int, [c_int]),
    "sd_ecapa_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sd_ecapa_debug_stats": (c_int, [c_void_p, POINTER(c_void_p)]),
    "sd_redimnet_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sd_redimnet_debug_generic": (c_int, [c_void_p, c_int]),
    "sd_wavlm_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sd_wavlm_frames": (c_int, [c_int]),
    "sd_probe_wavlm_buckets": (c_int, [c_int, c_void_p]),
    "sd_probe_wavlm_pos_weight": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "sd_op_wavlm_layer0": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                   c_void_p]),
    "sd_op_wavlm_conv": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                 c_void_p]),
    "sd_op_wavlm_pos_conv": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "sd_op_wavlm_bias_table": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "sd_op_wavlm_attention": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int, c_void_p]),
    "sd_op_wavlm_layer_mix": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "sd_op_wavlm_mix_proj_ln": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                        c_int, c_void_p]),
    "sd_w2vbert_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sd_op_w2vbert_attention": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "sd_op_w2vbert_conv_mix": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                       c_void_p]),
    "sd_whisper_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "sd_whisper_frames": (c_int, [c_int]),
    "sd_tsvad_create_whisper": (c_int, [POINTER(TsvadConfig), POINTER(WhisperConfig), POINTER(c_void_p)]),
    "sd_tsvad_create_ex": (c_int, [POINTER(TsvadConfigEx), POINTER(c_void_p)]),
    "sd_op_whisper_logmel": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "sd_op_whisper_stem": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_int, c_void_p]),
    "sd_op_whisper_add": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p]),
    "sd_op_whisper_ln_wide": (c_int, [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                      c_void_p]),
    "sd_op_attention_scaled": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p]),
    "sd_op_redim_block2d": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "sd_op_redim_dwconv1d": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_int, c_void_p]),
    "sd_op_redim_stage_mix": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int, c_void_p]),
    "sd_op_redim_stem": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                 c_void_p]),
    "sd_op_astp_pool_c": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "sd_eda_input_stride": (c_int, [c_void_p]),
    "sd_eda_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "sd_eda_status": (c_int, [c_void_p, c_void_p]),
    "sd_fseend_input_stride": (c_int, [c_void_p]),
    "sd_fseend_test": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "sd_fseend_stream_create": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "sd_fseend_stream_push": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, POINTER(c_int), c_void_p]),
    "sd_fseend_stream_set_audio": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "sd_fseend_stream_push_audio": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, POINTER(c_int), c_void_p]),
    "sd_fseend_stream_flush": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_int), c_void_p]),
    "sd_fseend_stream_reset": (c_int, [c_void_p, c_void_p]),
    "sd_fseend_stream_device_bytes": (c_int64, [c_void_p]),
    "sd_fseend_stream_stats": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int), POINTER(c_int)]),
    "sd_fseend_stream_debug_counters": (c_int, [c_void_p, POINTER(ctypes.c_uint), c_int, POINTER(c_int), c_void_p]),
    "sd_fseend_stream_destroy": (c_int, [c_void_p]),
    "sd_attn_decode_blocks": (c_int, [c_int]),
    "sd_op_attn_decode": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64,
                                  c_int64, c_int, c_int, c_int, c_float, c_void_p, c_int, c_int, c_int, c_void_p,
                                  c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int),
                                  c_void_p]),
    "sd_op_stream_slot_block": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                        c_int, c_int, c_int, c_int, c_float, POINTER(c_int), c_void_p]),
    "sd_op_stream_ffn_pair": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                      c_int, c_int, POINTER(c_int), c_void_p]),
    "sd_op_kv_append": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p, c_int, c_void_p]),
    "sd_op_gather_window": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "sd_op_cursor_advance": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "sd_op_stream_enc_finish": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p]),
    "sd_op_stream_dec_finish": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p]),
    "sd_eend_features": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                 c_void_p, c_void_p, c_int, c_void_p]),
    "sd_fbank_kaldi": (c_int, [c_void_p, c_int64, c_float, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "sd_fbank_kaldi_ex": (c_int, [c_void_p, c_int64, c_float, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "sd_window_cmn": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "sd_window_wave": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "sd_overlap_average": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_void_p, c_void_p]),
    "sd_overlap_mean": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                c_void_p, c_void_p]),
    "sd_postprocess_segments": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "sd_op_add_layernorm": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_int,
                                    c_void_p, c_int, c_void_p]),
    "sd_op_linear": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]),
    "sd_op_gemm_bf16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "sd_debug_cam_dense_probe": (c_int, [c_void_p]),
    "sd_debug_rowprog_probe": (c_int, [c_void_p]),
    "sd_probe_graph_memset": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p]),
    "sd_op_mha_block": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "sd_op_glu_dwconv": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sd_op_rowprog": (c_int, [POINTER(RowprogOp), c_void_p]),
    "sd_debug_conformer_wide_route": (c_int, [c_int]),
    "sd_op_conformer_stack": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int,
                                      c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                      c_void_p]),
    "sd_op_cam_dense": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_int, c_void_p]),
    "sd_op_fcm_block": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "sd_op_fcm_stem_block": (c_int, [c_void_p, c_int, c_int, c_int] + [c_void_p] * 13 + [c_int, c_void_p]),
    "sd_op_conv1d": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_int, c_int, c_void_p, c_int, c_void_p]),
    "sd_op_conv2d": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int,
                             c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "sd_op_res_conv": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "sd_op_tstp_pool": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sd_op_res2_chain": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                 c_int, c_void_p]),
    "sd_op_astp_pool": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "sd_op_asp_pool": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p]),
    "sd_op_simam": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sd_op_res2_conv3x3": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "sd_op_aff_gate": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "sd_op_stem_conv": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                c_void_p]),
    "sd_op_speaker_input_proj": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                         c_int, c_void_p]),
    "sd_op_gsp_down": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                               c_int, c_void_p, c_void_p]),
    "sd_gsp_down_frame_tile": (c_int, []),
    "sd_op_mamba2_stack": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p]),
    "sd_op_attention": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                                c_void_p]),
    "sd_op_attention_grid": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                     c_void_p]),
    "sd_op_attention_chunk": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                      c_void_p]),
    "sd_probe_attention_mask": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                        c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "sd_op_layernorm": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "sd_op_lstm": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p]),
}

# The handle lifecycle, the same five calls for every model kind (include/sdiar.h): create -> set_param* -> finalize
# -> <the kind's forward calls>* -> destroy, device_bytes at any time.
KINDS = {"tsvad": TsvadConfig, "tsvad_stream": TsvadStreamConfig, "eda": EdaConfig, "fseend": FseendConfig,
         "campp": CamppConfig, "resnet34": Resnet34Config, "simam_resnet34": SimamResnet34Config,
         "eres2netv2": Eres2netv2Config, "ecapa": EcapaConfig, "redimnet": RedimnetConfig, "wavlm": WavlmConfig,
         "w2vbert": W2vbertConfig, "whisper": WhisperConfig, "ssnd": SsndConfig}
for _kind, _conf in KINDS.items():
    _SIGS[f"sd_{_kind}_create"] = (c_int, [POINTER(_conf), POINTER(c_void_p)])
    _SIGS[f"sd_{_kind}_set_param"] = (c_int, [c_void_p, c_char_p, c_void_p, POINTER(c_int64), c_int])
    _SIGS[f"sd_{_kind}_finalize"] = (c_int, [c_void_p])
    _SIGS[f"sd_{_kind}_device_bytes"] = (c_int64, [c_void_p])
    _SIGS[f"sd_{_kind}_destroy"] = (c_int, [c_void_p])

EXPORTED = tuple(_SIGS)

_lib = None


def load():
    """Load libsdiar.so (raises if it is missing: the product has no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libsdiar.so not found at {LIB_PATH}; build it with "
            "`python -m speaker_diarization_amd.build` (HIP extension is required)")
    lib = ctypes.CDLL(LIB_PATH)
    # SDIAR_LIB (A/B runs against an older build) may lack entry points added since; the in-tree build
    # must export every one of them
    ab = os.environ.get("SDIAR_LIB") is not None
    for name, (res, args) in _SIGS.items():
        if ab and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str = ""):
    if status == SD_OK:
        return
    msg = load().sd_last_error().decode(errors="replace")
    if what:
        msg = f"{what}: {msg}"
    if status == SD_ERR_INVALID:
        raise ValueError(msg)
    if status == SD_ERR_SHAPE:
        raise AssertionError(msg)
    if status == SD_ERR_PARAM:
        raise RuntimeError(f"Error(s) in loading state_dict: {msg}")
    raise SdiarError(msg)


def has(name: str) -> bool:
    """Whether the loaded library exports `name` (only an older SDIAR_LIB build in an A/B run may not)."""
    return hasattr(load(), name)


def call(name: str, *args):
    check(getattr(load(), name)(*args), name)


PRECISION = {"fp32": 0, "bf16": 1, "bf16x3": 2}


def precision_code(precision: str, allowed=("bf16", "fp32", "bf16x3")) -> int:
    """The C API's precision of a wrapper's `precision` argument; ValueError for one the kind does not build."""
    if precision not in allowed:
        raise ValueError(f"precision must be {', '.join(allowed[:-1])} or {allowed[-1]}, got {precision}")
    return PRECISION[precision]


def hip_device(device, what: str):
    """torch.device of a wrapper's `device` argument (None: the current HIP device); ValueError off the GPU."""
    import torch
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise ValueError(f"{what} (MI355X backend) runs on a HIP device only")
    return dev


def host_state(state_dict) -> dict:
    """state_dict (torch tensors or arrays) -> {key: float32 numpy} on the host."""
    import numpy as np
    return {k: (v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float32))
            for k, v in state_dict.items()}


def load_params(kind: str, h, state):
    """sd_<kind>_set_param for every state_dict entry (reference key names), then sd_<kind>_finalize."""
    import numpy as np
    for k, a in host_state(state).items():
        data = np.ascontiguousarray(a)
        shape = (c_int64 * max(a.ndim, 1))(*a.shape)
        call(f"sd_{kind}_set_param", h, k.encode(), data.ctypes.data_as(c_void_p), shape, a.ndim)
    call(f"sd_{kind}_finalize", h)


def create_handle(kind: str, conf, state) -> ctypes.c_void_p:
    """sd_<kind>_create + load_params; the handle is destroyed again if any step fails."""
    h = ctypes.c_void_p()
    call(f"sd_{kind}_create", ctypes.byref(conf), ctypes.byref(h))
    try:
        load_params(kind, h, state)
    except Exception:
        getattr(load(), f"sd_{kind}_destroy")(h)
        raise
    return h


class Handle:
    """Owner of one sd_<kind> handle, mixed into every model wrapper.  `_h` is the raw c_void_p the kind's forward
    calls take (None while a lazy wrapper has not loaded weights).  Eager wrappers _create() in their constructor and
    _load() in load_state_dict; lazy ones build a loaded handle with create_handle() and _adopt() it."""
    kind = None
    _h = None

    def _create(self, conf):
        h = ctypes.c_void_p()
        call(f"sd_{self.kind}_create", ctypes.byref(conf), ctypes.byref(h))
        self._h = h

    def _load(self, state):
        load_params(self.kind, self._h, state)

    def _adopt(self, h):
        """Replace the handle (the new one exists before the old one goes, so a failed reload keeps the old)."""
        self._release()
        self._h = h

    def _release(self):
        h, self._h = self._h, None
        if h is not None and _lib is not None:      # never loads the library just to destroy nothing
            getattr(_lib, f"sd_{self.kind}_destroy")(h)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _device_bytes(self) -> int:
        return int(getattr(load(), f"sd_{self.kind}_device_bytes")(self._h)) if self._h is not None else 0


def ptr(t) -> int:
    """Raw device/host pointer of a contiguous torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "sdiar expects contiguous tensors"
    return t.data_ptr()


def prof_stats():
    """{family: dict(launches, flops, bytes, ms)} from the library's event timers."""
    lib = load()
    out = {}
    i = 0
    buf = ctypes.create_string_buffer(128)
    while True:
        l, f, b, ms = c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        if not lib.sd_prof_query(i, buf, 128, ctypes.byref(l), ctypes.byref(f), ctypes.byref(b), ctypes.byref(ms)):
            break
        steps = lib.sd_prof_query_steps(i) if hasattr(lib, "sd_prof_query_steps") else 0.0
        out[buf.value.decode()] = dict(launches=l.value, flops=f.value, bytes=b.value, ms=ms.value, steps=steps)
        i += 1
    return out


def stream_ptr(device=None):
    import torch
    return torch.cuda.current_stream(device).cuda_stream
