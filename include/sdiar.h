/*
 * sdiar.h — C ABI of the MI355X (gfx950) diarization inference engine.
 *
 * Plain pointers, sizes and a hipStream_t passed as void*.  Device pointers are
 * caller-owned (torch tensors, hipMalloc); weights are copied from host arrays
 * into a handle-owned device arena.  Every call returns 0 (SD_OK) or a negative
 * status; sd_last_error() returns the message of the last failure on the
 * calling thread.  All compute calls are stream-ordered and do not allocate,
 * so they can be captured into a hipGraph.
 *
 * The reference has no FFI: its boundary is the PyTorch nn.Module surface.
 * Each entry point below names the reference callable it replaces; the Python
 * mirror (speaker_diarization_amd/) binds them with ctypes.
 */
#ifndef SDIAR_H_
#define SDIAR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_OK 0
#define SD_ERR_INVALID (-1)  /* ValueError in the reference                       */
#define SD_ERR_SHAPE (-2)    /* AssertionError (label / feature length mismatch)  */
#define SD_ERR_PARAM (-3)    /* load_state_dict missing/unexpected key            */
#define SD_ERR_HIP (-4)      /* HIP runtime failure                               */
#define SD_ERR_STATE (-5)    /* handle used before finalize                       */

const char* sd_last_error(void);
int sd_version(void);

/* Opt-in kernel-family timing (HIP events on the launch stream) with
 * algorithmic FLOP/byte counts; used by bench.py for the live roofline.
 * sd_prof_query fills family i and returns 1, or returns 0 past the end. */
void sd_prof_enable(int on);
void sd_prof_reset(void);
int sd_prof_query(int i, char* name, int name_len, int64_t* launches, double* flops, double* bytes,
                  double* ms);
/* Sequential steps family i accumulated (latency-bound kernels: the LSTM recurrence counts its time steps). */
double sd_prof_query_steps(int i);
/* The persistent LSTM's exchange floor: one launch of the recurrence's 4-workgroup h hand-off protocol with
 * no gate arithmetic (same publish / poll / payload loads as lstm_group_bf16_kernel, batch 16) over `steps`
 * steps, timed with HIP events on `stream`; *us_per_step = its time / steps. */
int sd_probe_lstm_handoff(int steps, float* us_per_step, void* stream);
/* The same 4-workgroup exchange on data-tagged 8-byte granules (no counter, no barrier; MI355X guide
 * handoff-1to1): the hardware's hand-off price for the recurrence, us per step. */
int sd_probe_lstm_granule(int steps, float* us_per_step, void* stream);
/* Round 6: the granule exchange between TWO workgroups (each lane polls only the other one's half of its operand,
 * 1-to-1): the exchange floor of a recurrence that holds half of W_hh per CU. */
int sd_probe_lstm_granule2(int steps, float* us_per_step, void* stream);

/* ------------------------------------------------------------------ TS-VAD
 * Replaces TSVADModel (egs/alimeeting/ts_vad2/model.py:179-1142):
 *   construction  model.py:180-225 (TSVADConfig model.py:40-110)
 *   load_state_dict  (infer.py:184 loads checkpoint["model"])
 *   forward(ref_speech, target_speech, labels, num_updates)  model.py:899-921
 */
typedef struct sd_tsvad sd_tsvad;

typedef struct {
  int variant;                    /* 0: speech_encoder_type "CAM++", single/multi_backend "transformer"
                                     1: "CAM++_ots_vad", "conformer_ots_vad", "lstm_ots_vad", ots_vad_style "v1"
                                     2: "resnet34_wespeaker" (ResNet34 trunk + SpeechFeatUpsample2 transposed-conv
                                        upsampler, model.py:114-134, 584-606), single/multi_backend "transformer"
                                     3: "ecapa_channel_1024_wespeaker" (ECAPA_TDNN_GLOB_c1024 trunk + Conv1d(1536 ->
                                        speaker_embed_dim, k5, stride 4, pad 2), model.py:631-654), single/multi_backend
                                        "transformer"; any window of 1 .. max_fbank_frames frames runs, T fbank frames
                                        give (T - 1) / 4 + 1 mix frames
                                     4: "ReDimNetB2" (egs/magicdata-ramc/ts_vad2/model.py:694-715: ReDimNetB2 trunk on
                                        72-bin fbank + Conv1d(1152 -> speaker_embed_dim, k5, stride 4, pad 2)),
                                        single/multi_backend "transformer"; ref_speech is (B, T, 72); the MagicData
                                        length rule (:1296-1309): mix frames within 3 of the label length, zero-padded
                                        after the ReLU or cut, SD_ERR_SHAPE beyond
                                     5: "WavLM" (egs/magicdata-ramc/ts_vad2/model.py:867-889, 1171-1179): ref_speech is the
                                        RAW WAVEFORM (B, n_samples); a WavLM of wavlm_layers (= select_encoder_layer_nums)
                                        encoder layers, extract_features(ref_speech)[0] (with the final encoder.layer_norm
                                        in pre-LN mode), then Conv1d(wavlm_embed_dim -> speaker_embed_dim, k5, stride 2,
                                        pad 2); single/multi_backend "transformer".  n samples give T = (n - 400) / 320 + 1
                                        WavLM frames and (T - 1) / 2 + 1 mix frames; variant 4's length rule applies
                                     6: "WavLM_weight_sum" with wavlm_fuse_feat_post_norm (:890-927, 1180-1204): all
                                        wavlm_layers layers run, their outputs (hss[1:], the input to layer 0 dropped)
                                        are summed with `weights` = Linear(L -> 1, no bias), then wavlmproj = Linear(
                                        wavlm_embed_dim -> speaker_embed_dim), wavlmlnorm = LayerNorm, and the same conv
                                        on speaker_embed_dim (192 or 256) channels.  Without wavlm_fuse_feat_post_norm
                                        the reference's forward raises (:1206-1213 unpack (T, B, D, L) in the wrong
                                        order and the view fails): not built.
                                     5 / 6: backend 0 and precision 0 / 1 only (the WavLM trunk has no bf16x3), no
                                        padding mask (the collater's zero padding takes part, as in the reference)
                                     7: "w2v-bert2" (egs/magicdata-ramc/ts_vad2/model.py:805-840, 1225-1237): ref_speech is
                                        80-bin fbank (B, T, 80) with T EVEN (the reference's reshape to (B, T / 2, 160)
                                        raises on an odd T; SD_ERR_INVALID here); the first w2vbert_layers (=
                                        select_encoder_layer_nums) Conformer layers of w2v-BERT 2.0 (sd_w2vbert_* below),
                                        hidden_states[-1], then Conv1d(1024 -> speaker_embed_dim, k5, stride 2, pad 2);
                                        single/multi_backend "transformer".  T frames give T / 2 encoder frames and
                                        (T / 2 - 1) / 2 + 1 mix frames; variant 4's length rule applies.  backend 0 and
                                        precision 0 / 1 only; proj_layer as in variants 5 / 6
                                     8: "whisper" (egs/magicdata-ramc/ts_vad2/model.py:928-955, 1216-1223): ref_speech is
                                        the raw waveform (B, n_samples) as for 5 / 6 (n_samples carried by T_fb, a multiple
                                        of 4 in [400, max_samples]); the Whisper-PMFA encoder (sd_whisper_* below), then
                                        Conv1d(n_audio_state * n_cat -> speaker_embed_dim, k5, stride 2, pad 2);
                                        single/multi_backend "transformer".  n samples give T' = (n / 160 - 1) / 2 + 1
                                        encoder frames (T' > n_audio_ctx is refused) and (T' - 1) / 2 + 1 mix frames;
                                        variant 4's length rule applies.  backend 0 and precision 0 / 1 only.  This struct
                                        has no field for the trunk's geometry: sd_tsvad_create returns SD_ERR_INVALID for
                                        variant 8, sd_tsvad_create_whisper (below) builds it */
  int max_num_speaker;            /* TSVADDataConfig.max_num_speaker (4)                     */
  int rs_len;                     /* seconds; PositionalEncoding max_len = rs_len * 25       */
  int max_batch;                  /* workspace sizing                                        */
  int max_fbank_frames;           /* workspace sizing: 1 + (rs_len*16000 - 400) / 160        */
  int precision;                  /* 0: fp32 (exact-f32 MFMA), 1: bf16 MFMA, fp32 accumulate, 2: bf16x3 (fp32 tensors; the GEMMs as bf16 hi+lo splits: hi·hi + hi·lo + lo·hi) */
  int num_transformer_layer;      /* TSVADConfig defaults: 2, 4, 384, 1536, 192              */
  int num_attention_head;
  int transformer_embed_dim;
  int transformer_ffn_embed_dim;
  int speaker_embed_dim;          /* 192; any other multiple of 8 with 2 * speaker_embed_dim != transformer_embed_dim
                                     (256 for ResNet34 embeddings, run_ts_vad2.sh:3684) adds proj_layer =
                                     nn.Linear(2 * speaker_embed_dim, transformer_embed_dim) (model.py:212-217,
                                     873-874), variants 0, 2 and 3 only: the reference's ots_vad forward never applies
                                     it (model.py:730-731), so variant 1 is refused at create */
  int backend;                    /* 0: the variant's back end above (a zero-initialised config behaves as before)
                                     1: single_backend_type "mamba2", multi_backend_type "transformer"
                                        (egs/magicdata-ramc/run_ts_vad2_based_on_system_sad.sh:58-68, stage 4)
                                     2: "mamba2" for both; adds multi_backend_proj = Linear(2 E, E) before fc
                                     (egs/magicdata-ramc/ts_vad2/model.py:377-403, 488-504, 1337-1399; ts_vad2/mamba.py:
                                     149-213).  variant 0 only, SD_ERR_INVALID otherwise.  Each back end is a
                                     bidirectional Mamba2BlockV2(E, n_layer = num_transformer_layer, d_state, d_conv 4,
                                     expand); backend_down.0 reads 2 * E * max_num_speaker channels.
                                     THE AXIS QUIRK: the reference hands its seq-first (T, B, E) tensor to mamba_ssm's
                                     batch-first modules (model.py:1366-1367, 1393), so the scan, the causal conv and
                                     the backward flip run along the WINDOWS of a reference forward call, one sequence
                                     per (speaker, label frame).  This runner reproduces that: the sequences are the
                                     windows of each forward_batch group of sd_tsvad_forward_batched (the whole call
                                     for sd_tsvad_forward), in order, and never cross groups, so logits depend on
                                     which windows share a group; `force` (a slice of a reference batch) is refused.
                                     mamba_ssm is CUDA-only: the arithmetic restates its published Mamba2 module and
                                     no reference-run golden pins it (parity unpinned, like the Conformer)
                                     4: single_backend_type "conformer", multi_backend_type "transformer"
                                     5: "conformer" for both
                                     (egs/magicdata-ramc/ts_vad2/model.py:290-313, 451-463, 1340-1351, 1382-1390; the
                                     recipes pair them with CAM++, 2 layers, rs_len 4 / 6 / 8, e.g.
                                     egs/magicdata-ramc/run_ts_vad2_hltsz.sh:2571-2700).  variant 0 only, SD_ERR_INVALID
                                     otherwise; d_state / expand are not read.  Each back end is
                                     torchaudio.models.Conformer(E, num_attention_head, transformer_ffn_embed_dim,
                                     num_transformer_layer, depthwise_conv_kernel_size 31): use_group_norm False, so the
                                     conv module carries an eval BatchNorm1d (keys {single,multi}_backend.
                                     conformer_layers.{i}.*, conv_module.sequential.3.{weight, bias, running_mean,
                                     running_var}; num_batches_tracked accepted and ignored).  The sequence axis is TIME
                                     (batch-first calls, lengths all T, no padding mask): windows stay independent and
                                     forward_batch only scopes the BatchNorm1D bypass, as for backend 0; backend_down.0
                                     reads E * max_num_speaker channels.  The Conformer arithmetic restates torchaudio
                                     2.5.1 (parity unpinned); everything around it is pinned by reference runs
                                     (tests/golden/tsvad_conf_*.npz).
                                     3 is not a back end: SD_ERR_INVALID */
  int d_state;                    /* backend 1 / 2: TSVADConfig.d_state (reference default 64, the recipe 128): a
                                     multiple of 16 up to 256 */
  int expand;                     /* backend 1 / 2: TSVADConfig.expand (4): expand * transformer_embed_dim must be a
                                     multiple of 64 (the Mamba2 head dimension) */
  /* variants 5 / 6 (all zero otherwise: a config that ends before these fields, zero-extended, is today's model) */
  int wavlm_embed_dim;            /* 768 (ffn 3072, 12 heads: Base / Base+) or 1024 (4096, 16: Large)             */
  int wavlm_layers;               /* encoder layers that run and that speech_encoder.encoder.layers.* holds, 1..24  */
  int wavlm_layer_norm_mode;      /* extractor_mode "layer_norm" (Large); must equal wavlm_pre_ln                   */
  int wavlm_pre_ln;               /* layer_norm_first                                                                */
  int max_samples;                /* workspace sizing: the longest window in samples (rs_len * 16000), >= 400        */
  /* variant 7 (zero otherwise, and last: a config that ends before it, zero-extended, is today's model) */
  int w2vbert_layers;             /* encoder layers that run and that speech_encoder.encoder.layers.* holds, 1..24   */
} sd_tsvad_config;

int sd_tsvad_create(const sd_tsvad_config* cfg, sd_tsvad** out);

/* sd_tsvad_config followed by the fields added since; sd_tsvad_create(cfg) is sd_tsvad_create_ex of cfg zero-extended,
 * today's model.  Later fields go after frame_level_gsp. */
typedef struct {
  sd_tsvad_config base;
  int frame_level_gsp;            /* 1: speech_encoder_type "CAM++_frame_level_gsp_fc" (egs/magicdata-ramc/ts_vad2/
                                     model.py:543-563 construction, 1275-1287 forward; egs/magicdata-ramc/
                                     run_ts_vad2.sh:8333-8440 and the same stages of run_ts_vad2_aistation.sh, with
                                     single_backend_type "mamba2", d_state 128, rs_len 6).  The CAM++ time output
                                     (B, 512, T') is reduced per frame to its mean and unbiased std over the 512
                                     channels, gsp_fc = Linear(2, 256) maps the pair to 256 features and
                                     speech_down_or_up = Conv1d(256 -> speaker_embed_dim, k5, stride 2, pad 2) +
                                     BatchNorm1D + ReLU follows; everything after is forward_common.  Keys: variant 0's,
                                     plus gsp_fc.weight (256, 2), gsp_fc.bias (256), and speech_down_or_up.0.weight is
                                     (speaker_embed_dim, 256, 5).  base.variant must be 0 (SD_ERR_INVALID otherwise) with
                                     any of its back ends (base.backend 0, 1, 2, 4, 5); speaker_embed_dim a multiple of 32.
                                     gsp_fc and the conv run folded in one kernel (sd_op_gsp_down below); the statistics
                                     and its outputs are fp32 at every precision.  0: base alone */
} sd_tsvad_config_ex;
int sd_tsvad_create_ex(const sd_tsvad_config_ex* cfg, sd_tsvad** out);
/* One state_dict entry by its reference key name (fp32 host data, torch shape). */
int sd_tsvad_set_param(sd_tsvad* h, const char* name, const float* host_data, const int64_t* shape,
                       int ndim);
/* Folds BatchNorms, packs/uploads weights, allocates the workspace.  Fails with
 * SD_ERR_PARAM listing missing or unexpected keys (strict load_state_dict). */
int sd_tsvad_finalize(sd_tsvad* h);
/* ref_speech: device (B, T_fbank, 80) fbank after per-window CMN + batch pad;
 * target_speech: device (B, max_num_speaker, speaker_embed_dim);
 * logits: device (B, max_num_speaker, T_label) — pre-sigmoid, like forward(). */
int sd_tsvad_forward(sd_tsvad* h, const float* ref_speech, const float* target_speech, int B,
                     int T_fbank, int T_label, float* logits, void* stream);
/* Waits for `stream` and returns SD_ERR_HIP if the ots_vad BiLSTM's persistent recurrence of a
 * forward enqueued on it lost workgroup co-residency (its logits are NaN).  The Python mirror
 * calls it after forward(), so the failing forward itself raises (RuntimeError); an
 * uncollected report is raised by the handle's next forward at the latest. */
int sd_tsvad_status(sd_tsvad* h, void* stream);
/* sd_tsvad_forward with the scope of BatchNorm1D's NaN bypass (ts_vad2/model.py:161-171) given per call (no
 * handle state): a window with a non-finite input makes the reference skip speech_down_or_up's (and, variant 0,
 * backend_down's) BatchNorm for every window of ITS batch.  forward_batch: windows per reference forward call
 * (the collater's batch, e.g. infer.py's 64) when this call covers several; 0: the call is one batch.
 * force: this call is a slice of a larger reference batch whose non-finite input lies in another slice —
 * bit 0: a non-finite fbank (both BatchNorms skipped for every window), bit 1: a non-finite variant-0
 * target-speaker embedding (backend_down's skipped).  sd_tsvad_forward = forward_batch 0, force 0.
 * Variants 5 / 6 (here and in sd_tsvad_forward / sd_tsvad_forward_graph): ref_speech is the waveform (B, n_samples) fp32
 * and T_fbank carries n_samples, a multiple of 4 with 400 <= n_samples <= max_samples (SD_ERR_INVALID otherwise); force
 * bit 0 then stands for a non-finite sample. */
int sd_tsvad_forward_batched(sd_tsvad* h, const float* ref_speech, const float* target_speech, int B, int T_fbank,
                             int T_label, int forward_batch, int force, float* logits, void* stream);
int64_t sd_tsvad_device_bytes(const sd_tsvad* h);
/* Diagnostics only (not on the product path, which launches directly): capture sd_tsvad_forward once into a
 * hipGraph, optionally write its DOT dump to `dot_path`, replay it `replays` times on `stream` (each replay
 * rewrites logits) and wait; and the device buffers of the forward's stages (which: 0 mix, 1 mixg, 2 X2,
 * 3 H, 4 Y) for stage-by-stage comparisons.  Variant 2: which 0 is the upsampler output (B, 2 T', speaker_embed_dim)
 * channel-last, the transposed conv + bias before its BatchNorm1D + ReLU, T' the trunk's frame count. */
int sd_tsvad_forward_graph(sd_tsvad* h, const float* ref_speech, const float* target_speech, int B, int T_fbank,
                           int T_label, float* logits, int replays, const char* dot_path, void* stream);
int sd_tsvad_debug_buffer(const sd_tsvad* h, int which, void** ptr, int64_t* bytes);
int sd_tsvad_destroy(sd_tsvad* h);

/* ------------------------------------------------------------------ chunk-streaming TS-VAD
 * Replaces TSVADModel of egs/alimeeting/ts_vad2_streaming/model.py:95-1117 in its streaming
 * decode: forward_chunk_by_chunk(_temp1)(xs, target_speech, labels, decoding_chunk_size,
 * num_decoding_left_chunks) (model.py:368-461, 594-655; called through infer_debug :951-975 with
 * simulate_streaming, B = 1).  The KV caches are expressed as block-causal attention masks, so
 * one call decodes a whole window with the reference's per-chunk results.  State-dict keys are
 * the streaming model's (embed.speech_encoder.*, single_backend.{i}.self_attn.linear_q.*, ...). */
typedef struct sd_tsvad_stream sd_tsvad_stream;

typedef struct {
  int max_num_speaker;            /* 4 */
  int max_labels;                 /* workspace: label frames (25 Hz) per window */
  int precision;                  /* 0: fp32 (exact-f32 MFMA), 1: bf16 MFMA, fp32 accumulate */
  int num_transformer_layer;      /* TSVADConfig defaults (model.py:38-79): 2, 4, 384, 1536, 192 */
  int num_attention_head;
  int transformer_embed_dim;
  int transformer_ffn_embed_dim;
  int speaker_embed_dim;
  int max_windows;                /* workspace: windows per forward call (>= 1) */
} sd_tsvad_stream_config;

int sd_tsvad_stream_create(const sd_tsvad_stream_config* cfg, sd_tsvad_stream** out);
int sd_tsvad_stream_set_param(sd_tsvad_stream* h, const char* name, const float* host_data, const int64_t* shape,
                              int ndim);
int sd_tsvad_stream_finalize(sd_tsvad_stream* h);
/* B independent windows, each decoded as the reference's chunk loop decodes one (infer_debug,
 * batch 1, model.py:951-975).  feats: device (B, 4 * T_label, 80) fbank, already padded / trimmed
 * to 4 x labels (model.py:614-618); ts: device (B, max_num_speaker, speaker_embed_dim); chunk:
 * decoding_chunk_size (>= 1 label frame; a last partial chunk of any length, even 1 label = 4 fbank
 * frames, is decoded as the reference decodes it); left_chunks:
 * num_decoding_left_chunks (< 0: all history); logits: device (B, max_num_speaker, T_label),
 * pre-sigmoid. */
int sd_tsvad_stream_forward(sd_tsvad_stream* h, const float* feats, const float* ts, int B, int T_label, int chunk,
                            int left_chunks, float* logits, void* stream);
int64_t sd_tsvad_stream_device_bytes(const sd_tsvad_stream* h);
int sd_tsvad_stream_destroy(sd_tsvad_stream* h);

/* ------------------------------------------------------------------ CAM++ embeddings
 * Replaces CAMPPlus (egs/alimeeting/ts_vad2/cam_pplus_wespeaker.py:311-399) as the target-speaker
 * embedding extractor of generate_chunk_speaker_embedding_from_modelscope_for_diarization.py:
 *   construction  :256-260 (CAMPPLUS_COMMON: feat_dim 80, embedding_size 192)
 *   forward(x) / forward(x, get_time_out=True)  :264 / cam_pplus_wespeaker.py:388-399
 * State-dict keys are the standalone module's (head.*, xvector.*). */
typedef struct sd_campp sd_campp;

typedef struct {
  int feat_dim;        /* 80 */
  int embedding_size;  /* 192 (CAMPPLUS_COMMON) / 512 (CAMPPLUS_VOX)                     */
  int max_batch;       /* workspace: chunks per forward (extract_embed batch_size 96)      */
  int max_frames;      /* workspace: fbank frames per chunk (598 for 6 s)                  */
  int precision;       /* 0: fp32 (exact-f32 MFMA), 1: bf16 MFMA trunk (the pooled head stays fp32) */
} sd_campp_config;

int sd_campp_create(const sd_campp_config* cfg, sd_campp** out);
int sd_campp_set_param(sd_campp* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_campp_finalize(sd_campp* h);
/* feats: device (B, T, 80) fbank; emb: device (B, embedding_size) or NULL; time_out: device
 * (B, (T-1)/2+1, 512) channel-last = xvector[:-2] output transposed, or NULL (one of the two). */
int sd_campp_forward(sd_campp* h, const float* feats, int B, int T, float* emb, float* time_out, void* stream);
int64_t sd_campp_device_bytes(const sd_campp* h);
int sd_campp_destroy(sd_campp* h);

/* ------------------------------------------------------------------ ResNet34 embeddings
 * Replaces ResNet34(feat_dim=80, embed_dim, pooling_func="TSTP", two_emb_layer, speech_encoder=False)
 * (egs/alimeeting/ts_vad2/resnet_wespeaker.py:108-183, 198-208) as the target-speaker embedding extractor of
 * generate_chunk_speaker_embedding_from_wespeaker_for_diarization.py:
 *   construction  :116-117 (embed_dim 256, two_emb_layer False)
 *   forward(x)    :131-133 (the last element of the returned tuple) / resnet_wespeaker.py:156-183
 * State-dict keys are the standalone module's (conv1.*, bn1.*, layer1..4.*, seg_1.*[, seg_bn_1.*, seg_2.*]); TSTP
 * (pooling_layers_wespeaker.py:66-88) has no parameters, so a pool.* key is unexpected. */
typedef struct sd_resnet34 sd_resnet34;

typedef struct {
  int feat_dim;        /* 80 */
  int embed_dim;       /* 256 (a multiple of 8) */
  int two_emb_layer;   /* 0: embed_a = seg_1(stats); 1: also embed_b = seg_2(seg_bn_1(relu(embed_a))) */
  int max_batch;       /* workspace: chunks per forward (extract_embed batch_size 96)      */
  int max_frames;      /* workspace: fbank frames per chunk (598 for 6 s)                  */
  int precision;       /* 0: fp32 (exact-f32 MFMA), 1: bf16 trunk (TSTP and the seg layers stay fp32) */
} sd_resnet34_config;

/* resnet_wespeaker.py:109-146 */
int sd_resnet34_create(const sd_resnet34_config* cfg, sd_resnet34** out);
/* load_state_dict (generate_chunk_..._wespeaker_...py:125; strict here) */
int sd_resnet34_set_param(sd_resnet34* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_resnet34_finalize(sd_resnet34* h);
/* resnet_wespeaker.py:156-183.  feats: device (B, T, 80) fbank; emb: device (B, embed_dim) or NULL, the last
 * element of the reference's returned tuple (embed_b with two_emb_layer, else embed_a); emb_a: device (B, embed_dim)
 * or NULL, seg_1's output (meaningful with two_emb_layer; without it, written only when emb is NULL); time_out:
 * device (B, T', 2560) channel-last or NULL, T' = three times (n - 1) / 2 + 1 applied to T, channel c * 10 + f
 * (forward(x, get_time_out=True) transposed).  T <= 8 (T' = 1) gives all-NaN embeddings like the reference;
 * time_out needs T >= 8. */
int sd_resnet34_forward(sd_resnet34* h, const float* feats, int B, int T, float* emb, float* emb_a, float* time_out,
                        void* stream);
int64_t sd_resnet34_device_bytes(const sd_resnet34* h);
int sd_resnet34_destroy(sd_resnet34* h);

/* ------------------------------------------------------------------ SimAM-ResNet34 embeddings
 * Replaces SimAM_ResNet34_ASP(in_planes=64, embed_dim=256, acoustic_dim=80, dropout=0, speech_encoder=False)
 * (egs/alimeeting/ts_vad2/samresnet_wespeaker.py:21-160, pooling_layers_wespeaker.py:146-168) as the target-speaker
 * embedding extractor of generate_chunk_speaker_embedding_from_wespeaker_for_diarization.py:
 *   construction  :119-120
 *   forward(x)    :131-133 / samresnet_wespeaker.py:143-160
 * State-dict keys are the standalone module's (front.conv1.*, front.bn1.*, front.layer1..4.*.{conv1, bn1, conv2,
 * bn2, downsample.0, downsample.1}.*, pooling.attention.{0, 2, 3}.*, bottleneck.*).  The encoder-only form
 * (speech_encoder=True with forward(x, get_time_out=True), :146-153) raises NameError in the reference (it reads an
 * undefined `out`), so there is nothing to reproduce and it is not built. */
typedef struct sd_simam_resnet34 sd_simam_resnet34;

typedef struct {
  int in_planes;       /* 64 only (the stem's and stage 1's channels) */
  int embed_dim;       /* 256 (a positive multiple of 8) */
  int acoustic_dim;    /* 80 only */
  int max_batch;       /* workspace: chunks per forward (extract_embed batch_size 96)      */
  int max_frames;      /* workspace: fbank frames per chunk (598 for 6 s)                  */
  int precision;       /* 0: fp32 (exact-f32 MFMA), 1: bf16 trunk (ASP and the bottleneck stay fp32) */
} sd_simam_resnet34_config;

/* samresnet_wespeaker.py:135-141; in_planes != 64 or acoustic_dim != 80 gives SD_ERR_INVALID */
int sd_simam_resnet34_create(const sd_simam_resnet34_config* cfg, sd_simam_resnet34** out);
/* load_state_dict (generate_chunk_..._wespeaker_...py:125; strict here) */
int sd_simam_resnet34_set_param(sd_simam_resnet34* h, const char* name, const float* host_data, const int64_t* shape,
                                int ndim);
int sd_simam_resnet34_finalize(sd_simam_resnet34* h);
/* samresnet_wespeaker.py:143-160.  feats: device (B, T, 80) fbank; emb: device (B, embed_dim) or NULL =
 * bottleneck(pooling(front(x))); front_out: device (B, T', 5120) channel-last fp32 or NULL, T' = three times
 * (n - 1) / 2 + 1 applied to T, channel c * 10 + f: the front's map as ASP.forward flattens it
 * (pooling_layers_wespeaker.py:162), transposed.  T == 8 (T' = 1) is valid: the softmax weight is 1 and sg =
 * sqrt(1e-5).  T < 8 gives SD_ERR_SHAPE: the trunk's kernels are exercised from 8 frames on. */
int sd_simam_resnet34_forward(sd_simam_resnet34* h, const float* feats, int B, int T, float* emb, float* front_out,
                              void* stream);
/* Diagnostics (tools/simam_probe.py): what sd_simam_resnet34 handles finalized from now on build.  0 (the default):
 * the model above; 1: the same trunk with plain BasicBlocks, NOT SimAM-ResNet34 (prices the SimAM kernels, DESIGN.md
 * section 5c).  Never set in production code. */
int sd_debug_simam_variant(int variant);
int64_t sd_simam_resnet34_device_bytes(const sd_simam_resnet34* h);
int sd_simam_resnet34_destroy(sd_simam_resnet34* h);

/* ------------------------------------------------------------------ ERes2NetV2 embeddings
 * Replaces ERes2NetV2(feat_dim=80, embedding_size=192, m_channels=64, baseWidth, scale, expansion, pooling_func="TSTP",
 * two_emb_layer=False) (egs/alimeeting/ts_vad2/ERes2NetV2.py:162-255, fusion.py:10-30,
 * pooling_layers_3d_speaker.py:40-57), the 3D-Speaker extractor
 * generate_chunk_speaker_embedding_from_modelscope_for_diarization.py:110-136 builds for
 * iic/speech_eres2netv2w24s4ep4_sv_zh-cn_16k-common (baseWidth 24, scale 4, expansion 4) and runs on 6 s chunks
 * (:271-300); (26, 2, 2) is the class's default (egs/magicdata-ramc/ots_vad/model.py:496-534).  Parameters under the
 * reference state_dict names (conv1, bn1, layerN.M.{conv1, bn1, convs.i, bns.i, fuse_models.j.local_att.{0,1,3,4},
 * conv3, bn3, shortcut.{0,1}}.*, layer3_ds.weight, fuse34.local_att.{0,1,3,4}.*, seg_1.*).  two_emb_layer=True, the
 * other pooling functions and other size triples are not built. */
typedef struct sd_eres2netv2 sd_eres2netv2;

typedef struct {
  int feat_dim;        /* 80 only */
  int embedding_size;  /* 192 in the recipe; a positive multiple of 8 */
  int m_channels;      /* 64 only */
  int base_width;      /* (base_width, scale, expansion) = (26, 2, 2) or (24, 4, 4) */
  int scale;
  int expansion;
  int max_batch;       /* workspace: chunks per forward (extract_embed batch_size 96)      */
  int max_frames;      /* workspace: fbank frames per chunk (598 for 6 s)                  */
  int precision;       /* 0: fp32 (exact-f32 MFMA), 1: bf16 trunk (fuse34's blend, TSTP and seg_1 stay fp32) */
} sd_eres2netv2_config;

/* ERes2NetV2.__init__ (ERes2NetV2.py:163-226); an unsupported field gives SD_ERR_INVALID */
int sd_eres2netv2_create(const sd_eres2netv2_config* cfg, sd_eres2netv2** out);
/* load_state_dict (generate_chunk_...modelscope...py:133; strict here) */
int sd_eres2netv2_set_param(sd_eres2netv2* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_eres2netv2_finalize(sd_eres2netv2* h);
/* ERes2NetV2.forward (ERes2NetV2.py:236-255).  feats: device (B, T, 80) fbank; emb: device (B, embedding_size) or NULL =
 * seg_1(TSTP(fuse34(out4, layer3_ds(out3)))).  frame_out: device (B, T', 5120 * expansion) channel-last fp32 or NULL:
 * get_frame_level_feat (egs/magicdata-ramc/ots_vad/ERes2NetV2.py:253-258), the fuse34 map, channel f * C + c (the
 * reference transposes to (B, T, F, C) and flattens), transposed; frame25_out: device (B, T3, 5120 * expansion) or
 * NULL: get_frame_level_feat_frame_rate25 (:259-272), out3 in the same order.
 * T3 = twice, T' = three times (n - 1) / 2 + 1 applied to T.  T == 8 (T' = 1) gives the reference's NaN standard
 * deviations and an all-NaN embedding.  T < 8 gives SD_ERR_SHAPE. */
int sd_eres2netv2_forward(sd_eres2netv2* h, const float* feats, int B, int T, float* emb, float* frame_out,
                          float* frame25_out, void* stream);
/* Diagnostics (tools/eres2net_probe.py): which bf16 GEMM kernel serves the Hardtanh(0, 20) epilogue from now on.  0 (the
 * default): the shipped rule; 1: always the register-staged kernel (the first form measured).
 * Never set in production code. */
int sd_debug_clamp_route(int route);
int64_t sd_eres2netv2_device_bytes(const sd_eres2netv2* h);
int sd_eres2netv2_destroy(sd_eres2netv2* h);

/* ------------------------------------------------------------------ ECAPA-TDNN embeddings
 * Replaces ECAPA_TDNN_GLOB_c1024(feat_dim=80, embed_dim=192, pooling_func="ASTP")
 * (egs/alimeeting/ts_vad2/ecapa_tdnn_wespeaker.py:161-271, pooling_layers_wespeaker.py:91-144) as the target-speaker
 * embedding extractor of generate_chunk_speaker_embedding_from_ecapa_tdnn_for_diarization.py:
 *   construction  :111-112
 *   forward(x)    :128-131 / ecapa_tdnn_wespeaker.py:227-254
 * State-dict keys are the standalone module's (layer1.*, layer2..4.se_res2block.*, conv.*, pool.linear1/2.*, bn.*,
 * linear.*); emb_bn is off, so a bn2.* key is unexpected. */
typedef struct sd_ecapa sd_ecapa;

typedef struct {
  int channels;        /* 1024 only (ECAPA_TDNN_GLOB_c1024; the c512 models are not built) */
  int embed_dim;       /* 192 (a multiple of 4) */
  int max_batch;       /* workspace: chunks per forward (extract_embed batch_size 96)      */
  int max_frames;      /* workspace: fbank frames per chunk (598 for 6 s)                  */
  int precision;       /* 0: fp32 (exact-f32 MFMA), 1: bf16 trunk (ASTP, bn and linear stay fp32) */
} sd_ecapa_config;

/* ecapa_tdnn_wespeaker.py:163-225, 264-271; channels != 1024 gives SD_ERR_INVALID */
int sd_ecapa_create(const sd_ecapa_config* cfg, sd_ecapa** out);
/* load_state_dict (generate_chunk_..._ecapa_tdnn_...py:121; strict here) */
int sd_ecapa_set_param(sd_ecapa* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_ecapa_finalize(sd_ecapa* h);
/* ecapa_tdnn_wespeaker.py:227-254.  feats: device (B, T, 80) fbank; emb: device (B, embed_dim) or NULL =
 * linear(bn(pool(out))); time_out: device (B, T, 1536) channel-last fp32 or NULL (forward(x, get_time_out=True)
 * transposed; the time axis is not subsampled).  emb with T == 1 is refused with SD_ERR_SHAPE: the reference's
 * unbiased variance of a single frame (ASTP's global context) is NaN. */
int sd_ecapa_forward(sd_ecapa* h, const float* feats, int B, int T, float* emb, float* time_out, void* stream);
/* Device (B, 3072) pre-bn ASTP statistics [mean | std] of the last forward that wrote embeddings (diagnostics). */
int sd_ecapa_debug_stats(const sd_ecapa* h, void** ptr);
int64_t sd_ecapa_device_bytes(const sd_ecapa* h);
int sd_ecapa_destroy(sd_ecapa* h);

/* ------------------------------------------------------------------ ReDimNetB2 embeddings
 * Replaces ReDimNetB2(feat_dim=72, embed_dim=192, pooling_func="ASTP", two_emb_layer=False)
 * (egs/magicdata-ramc/ts_vad2/redimnet_wespeaker.py:925-948 over ReDimNet :793-872 and ReDimNetBone :623-790,
 * pooling_layers_wespeaker.py:91-144) as the target-speaker embedding extractor of
 * egs/magicdata-ramc/ts_vad2/generate_chunk_speaker_embedding_from_wespeaker_for_diarization.py (72-bin povey fbank).
 * State-dict keys are the module's (backbone.inputs_weights.*, backbone.stem.*, backbone.stage0..5.*,
 * pool.linear1/2.*, seg_1.*). */
typedef struct sd_redimnet sd_redimnet;

typedef struct {
  int feat_dim;        /* 72 only */
  int embed_dim;       /* 192 (a multiple of 4) */
  int max_batch;       /* workspace: chunks per forward (the extractor's batch size 96)    */
  int max_frames;      /* workspace: fbank frames per chunk (598 for 6 s)                  */
  int precision;       /* 0: fp32 (exact-f32 MFMA), 1: bf16 maps (LayerNorms, softmax, ASTP and seg_1 stay fp32),
                          2: bf16x3 (fp32 tensors, split-bf16 GEMMs) */
} sd_redimnet_config;

/* redimnet_wespeaker.py:925-948 (ReDimNet.__init__ :795-845); feat_dim != 72 gives SD_ERR_INVALID */
int sd_redimnet_create(const sd_redimnet_config* cfg, sd_redimnet** out);
/* load_state_dict (strict here) */
int sd_redimnet_set_param(sd_redimnet* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_redimnet_finalize(sd_redimnet* h);
/* ReDimNet.forward (:861-872) and get_frame_level_feat (:855-859).  feats: device (B, T, 72) fbank; emb: device
 * (B, embed_dim) or NULL = seg_1(pool(backbone(x))), the second element of the reference's pair; frames: device
 * (B, T, 1152) channel-last fp32 or NULL, channel f * c + ch as to1d orders it (:758-761; the time axis is not
 * subsampled).  emb with T == 1 is refused with SD_ERR_SHAPE: the reference's unbiased variance of a single
 * frame (ASTP's global context) is NaN; frames work from T == 1. */
int sd_redimnet_forward(sd_redimnet* h, const float* feats, int B, int T, float* emb, float* frames, void* stream);
/* Tests and tools/redimnet_probe.py only: 1 runs the 2-D ConvNeXt-like blocks of a bf16 handle as the generic arm
 * (grouped-conv kernel + conv_gemm) instead of the single-launch kernel; 0 restores the default.  fp32 / bf16x3
 * handles always run the generic arm. */
int sd_redimnet_debug_generic(sd_redimnet* h, int on);
int64_t sd_redimnet_device_bytes(const sd_redimnet* h);
int sd_redimnet_destroy(sd_redimnet* h);

/* Test-only single ops of the ReDimNetB2 trunk (csrc/redimnet.hip); every pointer is a device pointer.
 * precision as above; maps are bf16 at precision 1, else fp32.
 * sd_op_redim_block2d: ConvNeXtLikeBlock dim 2 (:135-165) on x (B, T, 1152 / c, c): dw_w (c, 4, 3, 3) + dw_b, the eval
 *   BatchNorm2d as (bn_s, bn_h), pw_w (c, c) + pw_b; use_generic 0 needs precision 1.
 * sd_op_redim_dwconv1d: depthwise conv (hC, k) + bias, BatchNorm1d as (bn_s, bn_h), erf GELU on x (B, T, hC) fp32.
 * sd_op_redim_stage_mix: y = sum_k w[k] x[k] over n stacked maps x (n, rows, 1152), w (n, 1152) already softmaxed.
 * sd_op_redim_stem: stem conv (16, 3, 3) + bias + channels-first LayerNorm (g, beta) of fbank (B, T, 72).
 * sd_op_astp_pool_c: sd_op_astp_pool at C channels (C % 64 == 0), w1 (128, 3 C), w2 (C, 128). */
int sd_op_redim_block2d(const void* x, int B, int T, int c, const float* dw_w, const float* dw_b, const float* bn_s,
                        const float* bn_h, const float* pw_w, const float* pw_b, void* out, int use_generic,
                        int precision, void* stream);
int sd_op_redim_dwconv1d(const float* x, int B, int T, int hC, int k, const float* w, const float* bias,
                         const float* bn_s, const float* bn_h, void* out, int out_bf16, void* stream);
int sd_op_redim_stage_mix(const void* x, int n, int64_t rows, const float* w, void* out, int bf16, void* stream);
int sd_op_redim_stem(const float* fbank, int B, int T, const float* w, const float* bias, const float* g,
                     const float* beta, void* out, int out_bf16, void* stream);
int sd_op_astp_pool_c(const void* x, int x_bf16, int B, int T, int C, const float* w1, const float* b1, const float* w2,
                      const float* b2, float* stats, void* stream);
/* sd_op_attention with an explicit softmax scale instead of (D / nh)^-0.5: heads zero-padded to a width the kernel has
 * keep the scale of their true width (ReDimNetB2's 24 / 36 / 72 in 32 / 48 / 96).  precision as sd_op_attention's. */
int sd_op_attention_scaled(const float* qkv, int S, int T, int D, int nh, float scale, float* out, int precision,
                           void* stream);

/* ------------------------------------------------------------------ WavLM feature extractor
 * Replaces WavLM.extract_features (egs/magicdata-ramc/ts_vad2/wavlm.py:359-414) of the WavLM class (:256-305) at the
 * two published geometries, Base+ and Large:
 *   feature_extractor     wavlm.py:434-556 (seven unbiased, unpadded Conv1d; "default": GroupNorm(512, 512) on layer 0;
 *                         "layer_norm": LayerNorm(512) on every layer; GELU)
 *   layer_norm + post_extract_proj   :377-384
 *   encoder               :559-675 (x += GELU(pos_conv(x)), weight_norm(dim 2) folded at load; post-LN or pre-LN)
 *   encoder layer         :678-805
 *   attention             modules.py:463-579 (relative_attention_bias of layer 0 through _relative_positions_bucket
 *                         :417-447 and compute_bias :449-461, gated per query by grep_linear / grep_a :533-548)
 * State-dict keys are the module's (mask_emb, feature_extractor.conv_layers.*, layer_norm.*, post_extract_proj.*,
 * encoder.pos_conv.0.{bias, parametrizations.weight.original0 / original1 | weight_g / weight_v}, encoder.layers.*,
 * encoder.layer_norm.*).  Fixed here: conv_feature_layers [(512,10,5)] + [(512,3,2)]*4 + [(512,2,2)]*2, conv_bias
 * False, conv_pos 128, conv_pos_groups 16, relative_position_embedding and gru_rel_pos True, num_buckets 320,
 * max_distance 800, activation_fn "gelu"; no padding_mask, no masking, no waveform normalisation. */
typedef struct sd_wavlm sd_wavlm;

typedef struct {
  int embed_dim;         /* (embed_dim, ffn_dim, heads) = (768, 3072, 12) or (1024, 4096, 16) */
  int ffn_dim;
  int heads;
  int encoder_layers;    /* 1..24 (the TS-VAD recipes cut the stack to 6) */
  int extractor_mode;    /* 0: "default", 1: "layer_norm" */
  int layer_norm_first;  /* 0 with extractor_mode 0 (Base+), 1 with extractor_mode 1 (Large) */
  int max_batch;         /* workspace: windows per forward */
  int max_samples;       /* workspace: samples per window, >= 400 (64000 = 4 s) */
  int precision;         /* 0: fp32 (exact-f32 MFMA), 1: bf16 GEMM / attention operands (layer 0, LayerNorms, softmax,
                            gates and the residual stream stay fp32) */
} sd_wavlm_config;

/* Output frames of the conv front end (wavlm.py:434-556): 400..719 samples -> 1, 16000 -> 49, 64000 -> 199,
 * 96000 -> 299; 0 below 400 samples.  Host only, no handle (exported rather than static so that bindings can call it). */
int sd_wavlm_frames(int n_samples);

/* WavLM.__init__ (wavlm.py:256-305); anything outside the configurations above gives SD_ERR_INVALID with a message
 * naming the field */
int sd_wavlm_create(const sd_wavlm_config* cfg, sd_wavlm** out);
/* load_state_dict (strict here) */
int sd_wavlm_set_param(sd_wavlm* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_wavlm_finalize(sd_wavlm* h);
/* wavlm.py:359-414.  source: device (B, n_samples) fp32 waveforms, n_samples >= 400; T = sd_wavlm_frames(n_samples).
 * output_layer: 0 = None (every layer, and in pre-LN mode the final encoder.layer_norm, wavlm.py:623-624), k >= 1 =
 * stop after layer k (no final norm).  x_out: device (B, T, D) or NULL; features_out: device (B, T, D) or NULL, the
 * projected conv features (ret_conv); layers_out: device (output_layer + 1, B, T, D) or NULL, the input to layer 0
 * then each layer's output (ret_layer_results; needs output_layer >= 1).  At least one output is required. */
int sd_wavlm_forward(sd_wavlm* h, const float* source, int B, int n_samples, int output_layer, float* x_out,
                     float* features_out, float* layers_out, void* stream);
int64_t sd_wavlm_device_bytes(const sd_wavlm* h);
int sd_wavlm_destroy(sd_wavlm* h);

/* Host-only probes (no device): out[r + n - 1] = _relative_positions_bucket(r) (modules.py:417-447) for every
 * relative position r = key - query in [-(n - 1), n - 1]; and the folded positional-conv weight g v / |v| (wavlm.py:
 * 578-580, weight_norm dim 2) of g (128) and v (D, D / 16, 128), D 768 or 1024, into out (D, D / 16, 128). */
int sd_probe_wavlm_buckets(int n, int32_t* out);
int sd_probe_wavlm_pos_weight(const float* g, const float* v, int D, float* out);

/* Test-only single ops of the WavLM trunk (csrc/wavlm.hip); every pointer is a device pointer, precision 0 or 1 as
 * above.
 * sd_op_wavlm_layer0: conv layer 0 + norm + GELU of wav (B, n): w (512, 10), norm affine g / b (512), layer_norm 0 =
 *   GroupNorm per (window, channel), 1 = LayerNorm over channels; out (B, (n - 10) / 5 + 1, 512), bf16 when out_bf16.
 * sd_op_wavlm_conv: one of conv layers 1-6 on x (B, T, 512) fp32: w (512, 512, k), k 2 or 3, stride 2, then GELU, or
 *   LayerNorm(ln_g, ln_b) + GELU when ln_g is given; out (B, (T - k) / 2 + 1, 512) fp32.  Here precision 2 is
 *   precision 1 with a bf16 map out, as the model's bf16 mode runs layers 1-5: with ln_g the raw conv result is
 *   stored in bf16 and the LayerNorm (fp32 statistics) reads that map.
 * sd_op_wavlm_pos_conv: out = x + GELU(conv(x) + bias) on x (B, T, D) with the folded weight w (D, D / 16, 128).
 * sd_op_wavlm_bias_table: table (H, 2 T - 1) from relative_attention_bias.weight emb (320, H).
 * sd_op_wavlm_attention: the gated attention on qkv (B T, 3 H 64) = (q | k | v) and the layer input xin (B T, H 64):
 *   grep_w (8, 64), grep_b (8), grep_a (H), table (H, 2 T - 1); out (B T, H 64) fp32. */
int sd_op_wavlm_layer0(const float* wav, int B, int n, const float* w, const float* g, const float* b, int layer_norm,
                       void* out, int out_bf16, void* stream);
int sd_op_wavlm_conv(const float* x, int B, int T, const float* w, int k, const float* ln_g, const float* ln_b,
                     void* out, int precision, void* stream);
int sd_op_wavlm_pos_conv(const float* x, int B, int T, int D, const float* w, const float* bias, float* out,
                         int precision, void* stream);
int sd_op_wavlm_bias_table(const float* emb, int T, int H, float* table, void* stream);
/* TS-VAD's WavLM_weight_sum head, op by op (test entry points; device pointers).
 * sd_op_wavlm_layer_mix: acc (n) = sum_l w[l] x[l] over L layer outputs x (L, n) fp32, accumulated layer by layer as the
 *   model does (acc = w[0] x[0], then acc += w[l] x[l]); w is a HOST array of L floats; n a multiple of 4.
 * sd_op_wavlm_mix_proj_ln: out (rows, SE) fp32 = LayerNorm(acc (rows, D) W^T + bias) g + beta, W (SE, D) torch layout,
 *   SE 192 or 256, D a multiple of 32; precision 0: exact f32, 1: bf16 operands (acc and W rounded), fp32 accumulation
 *   and LayerNorm, the bf16 output widened to fp32. */
int sd_op_wavlm_layer_mix(const float* x, int L, int64_t n, const float* w_host, float* acc, void* stream);
int sd_op_wavlm_mix_proj_ln(const float* acc, int rows, int D, const float* w, const float* bias, const float* g,
                            const float* beta, int SE, float* out, int precision, void* stream);
int sd_op_wavlm_attention(const float* qkv, const float* xin, int B, int T, int H, const float* grep_w,
                          const float* grep_b, const float* grep_a, const float* table, float* out, int precision,
                          void* stream);

/* ------------------------------------------------------------------ w2v-BERT 2.0 speech encoder
 * Replaces transformers' Wav2Vec2BertModel.forward (models/wav2vec2_bert/modeling_wav2vec2_bert.py:991-1050) in eval
 * mode, as egs/magicdata-ramc/ts_vad2/model.py:805-840 builds it (hidden_act "swish", num_hidden_layers cut to
 * select_encoder_layer_nums), at the published geometry only:
 *   feature_projection    :119-131 (LayerNorm(160) -> Linear(160 -> 1024))
 *   encoder layer         :398-461 (x += 0.5 ffn1(LN x); x += attn(LN x); x += conv(x); x += 0.5 ffn2(LN x); final LN)
 *   self-attention        :229-337, position_embeddings_type "relative_key": scores[l, r] = (q_l . k_r + q_l .
 *                         E[clamp(r - l, -64, 8) + 64]) / 8, E = distance_embedding.weight (73, 64) per layer
 *   conv module           :157-226 (LN, pointwise_conv1 no bias, GLU, LEFT zero pad 30 + depthwise k31 no bias,
 *                         depthwise_layer_norm over channels, swish, pointwise_conv2 no bias)
 * No encoder-level LayerNorm follows the last layer.  State-dict keys are the HF module's (masked_spec_embed, which is
 * loaded and never read; feature_projection.*; encoder.layers.<i>.*).  No attention_mask, no masking, no adapter. */
typedef struct sd_w2vbert sd_w2vbert;

typedef struct {
  int hidden;        /* 1024 */
  int heads;         /* 16 */
  int ffn;           /* 4096 */
  int layers;        /* 1..24 (the TS-VAD recipe cuts the stack to 6) */
  int conv_kernel;   /* 31 */
  int left;          /* 64: left_max_position_embeddings */
  int right;         /* 8: right_max_position_embeddings */
  int in_dim;        /* 160: feature_projection_input_dim */
  int precision;     /* 0: fp32 (exact-f32 MFMA), 1: bf16 GEMM / attention operands (LayerNorms, softmax, the depthwise
                        conv and the residual stream stay fp32) */
  int max_batch;     /* workspace: windows per forward */
  int max_frames;    /* workspace: frames per window after the pairing (200 = 4 s) */
  int position_embeddings;   /* 0: "relative_key" (the only one built) */
  int add_adapter;           /* 0 (the only one built) */
} sd_w2vbert_config;

/* Wav2Vec2BertModel.__init__ (:923-945); anything outside the geometry above gives SD_ERR_INVALID with a message naming
 * the field */
int sd_w2vbert_create(const sd_w2vbert_config* cfg, sd_w2vbert** out);
/* load_state_dict (strict here) */
int sd_w2vbert_set_param(sd_w2vbert* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_w2vbert_finalize(sd_w2vbert* h);
/* Wav2Vec2BertModel.forward (:991-1050).  input_features: device (B, T2, 160) fp32; x_out: device (B, T2, 1024) or NULL,
 * last_hidden_state; layers_out: device (layers + 1, B, T2, 1024) or NULL, hidden_states with output_hidden_states=True
 * (the input to layer 0, then each layer's output).  At least one output is required. */
int sd_w2vbert_forward(sd_w2vbert* h, const float* input_features, int B, int T2, float* x_out, float* layers_out,
                       void* stream);
int64_t sd_w2vbert_device_bytes(const sd_w2vbert* h);
int sd_w2vbert_destroy(sd_w2vbert* h);

/* Test-only single ops of the w2v-BERT trunk (csrc/w2vbert.hip); every pointer is a device pointer, precision 0 or 1.
 * sd_op_w2vbert_attention: Wav2Vec2BertSelfAttention.forward's core (:306-331) on qkv (B T, 3 H 64) = (q | k | v) with
 *   dist = distance_embedding.weight (73, 64); out (B T, H 64) fp32.
 * sd_op_w2vbert_conv_mix: Wav2Vec2BertConvolutionModule.forward's middle (:211-221) on x (B, T, 2048) = pointwise_conv1's
 *   output [value | gate]: GLU, causal depthwise conv w (1024, 31), LayerNorm (g, beta) over channels, swish; out
 *   (B, T, 1024) fp32.  precision 1: x rounded to bf16 on entry and the output rounded to bf16, as in the model. */
int sd_op_w2vbert_attention(const float* qkv, int B, int T, int H, const float* dist, float* out, int precision,
                            void* stream);
int sd_op_w2vbert_conv_mix(const float* x, int B, int T, const float* w, const float* g, const float* beta, float* out,
                           int precision, void* stream);

/* ------------------------------------------------------------------ Whisper-PMFA encoder
 * Replaces WhisperEncoder.forward (egs/magicdata-ramc/ts_vad2/whisper_encoder.py:150-244; ModelDimensions :19-27) in
 * eval mode: per-window whisper.log_mel_spectrogram (no 30-s padding), conv1 k3 + GELU, conv2 k3 stride 2 + GELU, the
 * loaded positional_embedding[:T'], n_audio_layer pre-LN blocks (:116-147; key projection without bias :66), and
 * ln_post2 over the concatenated outputs of blocks layer_st .. layer_ed.  State-dict keys are the reference class's own
 * (conv1.*, conv2.*, positional_embedding, layers.<i>.{attn.{query,key,value,out},attn_ln,mlp.0,mlp.2,mlp_ln}.*,
 * ln_post2.*), plus one key that is not the reference's: mel_filters (n_mels, 201), the slaney mel matrix computed on the
 * host (speaker_diarization_amd.feature.whisper_mel_filters).  The front end is restated from the published formula
 * (torch.stft form), not taken from the whisper package. */
typedef struct sd_whisper sd_whisper;

typedef struct {
  int n_mels;          /* 80 or 128 */
  int n_audio_ctx;     /* rows of positional_embedding (1500); a window of more frames is refused */
  int n_audio_state;   /* 64 * n_audio_head, a multiple of 32 (1280) */
  int n_audio_head;    /* head size 64 only (20) */
  int n_audio_layer;   /* 1..32 (24) */
  int layer_st;        /* 0 <= layer_st <= layer_ed < n_audio_layer (16, 23); n_audio_state * (layer_ed - layer_st + 1) */
  int layer_ed;        /*   at most 16384 */
  int precision;       /* 0: fp32 (exact-f32 MFMA), 1: bf16 GEMM / conv / attention operands (the log-mel front end, the
                          LayerNorms, the softmax, GELU inputs, the residual stream and the output stay fp32) */
  int max_batch;       /* workspace: windows per forward */
  int max_samples;     /* workspace: samples per window (64000 = 4 s) */
} sd_whisper_config;

/* anything outside the ranges above gives SD_ERR_INVALID with a message naming the field */
int sd_whisper_create(const sd_whisper_config* cfg, sd_whisper** out);
/* load_state_dict (strict here) */
int sd_whisper_set_param(sd_whisper* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_whisper_finalize(sd_whisper* h);
/* T' = ((n_samples / 160) - 1) / 2 + 1 frames of a window of n_samples (0 below 400 samples) */
int sd_whisper_frames(int n_samples);
/* wavs: device (B, n_samples) fp32, 400 <= n_samples <= max_samples and T' <= n_audio_ctx (the reference truncates there
 * and TS-VAD's label-length assertion then fails: SD_ERR_INVALID here).  out: device (B, T', n_audio_state * (layer_ed -
 * layer_st + 1)) fp32.  A window holding a non-finite sample comes out all NaN; the other windows are untouched. */
int sd_whisper_forward(sd_whisper* h, const float* wavs, int B, int n_samples, float* out, void* stream);
int64_t sd_whisper_device_bytes(const sd_whisper* h);
int sd_whisper_destroy(sd_whisper* h);

/* TS-VAD variant 8: an sd_tsvad_config with variant 8 and max_samples set, plus the trunk's own geometry; wcfg's precision,
 * max_batch and max_samples are ignored (cfg's hold).  State-dict keys: speech_encoder.<the keys above, mel_filters
 * included>, speech_down_or_up.{0,1.bn}.* and the usual back-end keys.  Any other variant: SD_ERR_INVALID. */
int sd_tsvad_create_whisper(const sd_tsvad_config* cfg, const sd_whisper_config* wcfg, sd_tsvad** out);

/* Test-only single ops of the Whisper trunk (csrc/whisper.hip); every pointer is a device pointer.
 * sd_op_whisper_logmel: the log-mel front end of wav (B, n) with mel (n_mels, 201) -> out (B, n / 160, n_mels) fp32.
 * sd_op_whisper_stem: feat (B, F, n_mels) -> out (B, (F - 1) / 2 + 1, D) = gelu(conv2(gelu(conv1(feat)))) + pe, w1 (D,
 *   n_mels, 3), w2 (D, D, 3), pe (>= T', D); precision 0 or 1.
 * sd_op_whisper_add: out[r, :D] = x[r, :D] + t[r, :D] with x / out rows at strides ldx / ldo, t dense.
 * sd_op_whisper_ln_wide: LayerNorm (eps 1e-5) over rows of W values at stride ldx -> out (rows, W) fp32; precision 1:
 *   the output rounded to bf16, as the model hands it to the next GEMM. */
int sd_op_whisper_logmel(const float* wav, int B, int n, int n_mels, const float* mel, float* out, void* stream);
int sd_op_whisper_stem(const float* feat, int B, int F, int n_mels, int D, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* pe, float* out, int precision, void* stream);
int sd_op_whisper_add(const float* x, int ldx, const float* t, float* out, int ldo, int64_t rows, int D, void* stream);
int sd_op_whisper_ln_wide(const float* x, int ldx, int64_t rows, int W, const float* g, const float* b, float* out,
                          int precision, void* stream);

/* ------------------------------------------------------------------ SSND
 * Replaces SSNDModel.infer (egs/alimeeting/ssnd/ssnd_model.py:752-776) with extractor
 * 'CAM++_wo_gsp' (:107-124), SSNDConformerEncoder (:172-195), DetectionDecoder (:274-296: the
 * speaker-query cross-attention decoder, SWDecoderBlockV2 :224-272) and RepresentationDecoder
 * (:343-370); construction :373-441 (training=False).  State-dict keys are SSNDModel's.  The
 * decoders always run exact fp32; precision selects the extractor / encoder arithmetic. */
typedef struct sd_ssnd sd_ssnd;

typedef struct {
  int max_batch;         /* workspace: blocks per call                                        */
  int max_fbank_frames;  /* workspace: fbank frames per block (800 = 8 s)                    */
  int max_speakers;      /* N: det_query_emb rows                                             */
  int feat_dim;          /* 80 */
  int emb_dim;           /* 256 */
  int q_det_aux_dim;     /* 256 */
  int q_rep_aux_dim;     /* 256 */
  int d_model;           /* 256 */
  int nhead;             /* 8 */
  int d_ff;              /* 512 */
  int num_layers;        /* 4 (encoder and both decoders) */
  int vad_out_len;       /* label frames per block (det_decoder.out_proj rows), 200 for 8 s */
  int pos_emb_dim;       /* 256 */
  int max_seq_len;       /* 1000 (pos_emb rows) */
  int n_all_speakers;    /* 1000 (E_all rows) */
  int conformer_kernel;  /* 15 (SSNDConformerEncoder cnn_kernel_size) */
  int precision;         /* 0: fp32, 1: bf16 MFMA extractor + encoder */
} sd_ssnd_config;

int sd_ssnd_create(const sd_ssnd_config* cfg, sd_ssnd** out);
int sd_ssnd_set_param(sd_ssnd* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_ssnd_finalize(sd_ssnd* h);
/* SSNDModel.infer: feats device (B, T_fbank, 80) with (T_fbank - 1) / 2 + 1 CAM++ frames giving
 * vad_out_len label frames; speaker_embs device (B, max_speakers, emb_dim);
 * vad_pred device (B, max_speakers, vad_out_len) pre-sigmoid; emb_pred device (B, max_speakers, emb_dim). */
int sd_ssnd_infer(sd_ssnd* h, const float* feats, const float* speaker_embs, int B, int T_fbank, float* vad_pred,
                  float* emb_pred, void* stream);
/* The two decoders alone (infer after the encoder, :762-776): enc_out device (B, T, d_model),
 * x_fea device (B, T, emb_dim) (the extractor output), T == vad_out_len. */
int sd_ssnd_decode(sd_ssnd* h, const float* enc_out, const float* x_fea, const float* speaker_embs, int B, int T,
                   float* vad_pred, float* emb_pred, void* stream);
int64_t sd_ssnd_device_bytes(const sd_ssnd* h);
int sd_ssnd_destroy(sd_ssnd* h);

/* ------------------------------------------------------------------ EEND-EDA
 * Replaces TransformerEdaModel (speaker_diarization/eend_eda/models.py:161-347) and
 * EendEdaModel (models.py:466-652) with LstmEncoderDedecoderAttractor
 * (eend_eda/encoder_decoder_attractor.py:8-59):
 *   construction  infer_eda.py:50-71;  load_state_dict  infer_eda.py:88
 *   infer(src, infer_num_speakers, max_n_speakers, attractor_threshold)  models.py:297 / 601
 * The forward computes everything before speaker selection; the selection
 * (sort / first-n / threshold on the max_n_speakers probs) stays on the host.
 */
typedef struct sd_eda sd_eda;

typedef struct {
  int variant;          /* 0: TransformerEdaModel; 1: EendEdaModel(encoder_type "transformer");
                           2: EendEdaModel(encoder_type "conformer") (infer_eda.py model_type ConformerEda) */
  int in_size;          /* 345 = (2*context_size+1) * 23                                     */
  int n_units;          /* hidden_size (256)                                                  */
  int n_heads;          /* transformer_encoder_n_heads (4)                                    */
  int n_layers;         /* transformer_encoder_n_layers (2 / 4)                               */
  int dim_feedforward;  /* 2048 (never passed by infer_eda.py)                                */
  int max_seqs;         /* workspace: sequences (chunks) per forward                          */
  int max_frames;       /* workspace: frames per sequence (chunk_size, 2000)                  */
  int max_n_speakers;   /* attractors decoded (15)                                            */
  int precision;        /* 0: fp32 (exact-f32 MFMA), 1: bf16 MFMA, fp32 accumulate, 2: bf16x3 GEMMs */
  int n_speakers;       /* variant 3 only: decoder outputs                                    */
} sd_eda_config;
/* variant 3 is the plain EEND TransformerModel (speaker_diarization/eend/models.py:17-101,
 * called as model([chunk], activation=torch.sigmoid) from eend/eend_infer.py:69): the same
 * handle API; lengths/perm/probs may be NULL and act receives (S, T, n_speakers) sigmoid outputs. */

int sd_eda_create(const sd_eda_config* cfg, sd_eda** out);
int sd_eda_set_param(sd_eda* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_eda_finalize(sd_eda* h);
/* Row stride (floats) the input features must have: in_size rounded up to 8 (352). */
int sd_eda_input_stride(const sd_eda* h);
/* feats: device (S, T, ld_feats) f32 (pad columns finite, e.g. zero or pad_sequence's -1);
 * lengths: device int32 (S) frames per sequence (ilens); key_len: device int32 (S) attention
 * key mask or NULL (the transformer variants attend to padded frames, models.py:216-226;
 * the conformer variant masks by ilens, :527-528); perm: device int32 (S, T), row s holds
 * torch.randperm(lengths[s]) drawn by the caller on the host CPU generator (models.py:229-233).
 * probs: device (S, max_n_speakers) attractor existence probabilities;
 * act: device (S, T, max_n_speakers - 1) = sigmoid(emb · attractors[:-1]ᵀ). */
int sd_eda_forward(sd_eda* h, const float* feats, int ld_feats, int S, int T, const int* lengths,
                   const int* key_len, const int* perm, float* probs, float* act, void* stream);
/* As sd_tsvad_status for the EDA encoder / decoder LSTMs (encoder_decoder_attractor.py:19-59). */
int sd_eda_status(sd_eda* h, void* stream);
int64_t sd_eda_device_bytes(const sd_eda* h);
int sd_eda_destroy(sd_eda* h);

/* ------------------------------------------------------------------ FS-EEND
 * Replaces OnlineTransformerDADiarization (speaker_diarization/fs_eend/fs_eend.py:20-96):
 *   construction  fs_eend/train.py:71-75 (config/spk_onl_tfm_enc_dec_nonautoreg_infer.yaml)
 *   test(src, ilens, max_nspks) -> (preds, emb, attractors)   fs_eend.py:79-96, called from
 *   fs_eend/model.py:198 with max_nspks = max_speakers + 2.
 * The causal encoder attends to all history: the path does not shard (replicas only). */
typedef struct sd_fseend sd_fseend;

typedef struct {
  int in_size;              /* (2 * context_recp + 1) * n_mels = 345                     */
  int n_units;              /* 256 */
  int n_heads;              /* 4   */
  int enc_n_layers;         /* 4   */
  int enc_dim_feedforward;  /* 2048 (MaskedTransformerEncoderModel default)             */
  int dec_n_layers;         /* 2: applications of the shared fusion layer               */
  int dec_dim_feedforward;  /* 2048 */
  int conv_delay;           /* 9 (Conv1d kernel 19, padding 9)                           */
  int mask_delay;           /* 0 */
  int has_mask;             /* 1: causal encoder                                          */
  int max_seqs;             /* workspace: sequences per call                              */
  int max_frames;           /* workspace: frames per sequence (chunk_size 10000)          */
  int max_nspks;            /* workspace: attractor slots (max_speakers + 2 = 6)         */
  int precision;            /* 0 fp32, 1 bf16 MFMA, 2 bf16x3 GEMMs (fp32 tensors) */
} sd_fseend_config;

int sd_fseend_create(const sd_fseend_config* cfg, sd_fseend** out);
int sd_fseend_set_param(sd_fseend* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int sd_fseend_finalize(sd_fseend* h);
int sd_fseend_input_stride(const sd_fseend* h);
/* feats: device (S, T, ld_feats) f32 = pad_sequence(src, -1) (pad columns finite);
 * ilens_host: host int32 (S); preds: device (S, T, max_nspks); emb: device (S, T, n_units) or NULL;
 * attractors: device (S, T, max_nspks, n_units) or NULL (both L2-normalised, as test() returns). */
int sd_fseend_test(sd_fseend* h, const float* feats, int ld_feats, int S, int T, const int* ilens_host,
                   int max_nspks, float* preds, float* emb, float* attractors, void* stream);
int64_t sd_fseend_device_bytes(const sd_fseend* h);
int sd_fseend_destroy(sd_fseend* h);

/* Streaming test(): the same scores as sd_fseend_test on the concatenated frames, produced
 * chunk by chunk from K/V histories (no reference counterpart: the reference recomputes the
 * causal forward over the whole recording, fs_eend.py:79-96 / fs_eend/model.py:198; the
 * causal masks of every shipped config, mask_delay 0, make the two identical).  A frame's
 * score is final 9 frames later (look-ahead Conv1d, fs_eend.py:41).  chunk: frames per push
 * (1..32; 1 frame = 100 ms at subsampling 10); use_graph: replay each chunk's kernels as a
 * captured hipGraph.  The stream keeps a pointer to its model handle: destroy it first. */
typedef struct sd_fseend_stream sd_fseend_stream;
int sd_fseend_stream_create(sd_fseend* h, int chunk, int max_frames, int max_nspks, int use_graph,
                            sd_fseend_stream** out);
/* feats: device (n, ld_feats) f32, 1 <= n <= chunk (n < chunk ends the input);
 * preds: device (cap, max_nspks) f32; *n_out = frames whose scores were written. */
int sd_fseend_stream_push(sd_fseend_stream* s, const float* feats, int ld_feats, int n, float* preds, int cap,
                          int* n_out, void* stream);
/* Audio input instead of feature rows (latency mode from raw audio): the FS-EEND frontend of
 * fs_eend/dataset.py:217-223 (transform 'logmel23' at the hardcoded 8 kHz: frame_size 200, frame_shift 80,
 * n_fft 256, 23 mels, no CMN) + feature.splice (context_size 7) + [::subsampling 10] (feature.py:130-184)
 * computed incrementally on the device: each chunk's STFT frames, logmel and spliced rows run inside its
 * captured encoder graph, reading the stream's audio history at the device cursor.  mel_fb: device
 * (n_mels, n_fft/2 + 1) f32 (librosa.filters.mel, Slaney), kept by pointer.  Call on a fresh or reset
 * stream; reset() returns the stream to feature rows.  push_audio: n samples (device f32, any n >= 0,
 * e.g. 640 = 80 ms); a model frame (100 ms) is encoded once its last spliced STFT frame has all its
 * samples, and scored 9 frames later (look-ahead); flush() then knows the length (feature.stft's frame
 * count, feature.py:176-184) and finishes.  The rows equal eend_features() of the whole recording bit
 * for bit, so the scores equal sd_fseend_test on them (as for feature pushes). */
int sd_fseend_stream_set_audio(sd_fseend_stream* s, const float* mel_fb, int n_mels, int frame_size, int frame_shift,
                               int context_size, int subsampling);
int sd_fseend_stream_push_audio(sd_fseend_stream* s, const float* samples, int64_t n, float* preds, int cap,
                                int* n_out, void* stream);
int sd_fseend_stream_flush(sd_fseend_stream* s, float* preds, int cap, int* n_out, void* stream);
/* reset: enqueues the cursor reset on `stream` and waits for it (and every chunk enqueued before it), so a
 * following set_audio() on any stream sees no chunk of the previous utterance still in flight. */
int sd_fseend_stream_reset(sd_fseend_stream* s, void* stream);
int64_t sd_fseend_stream_device_bytes(const sd_fseend_stream* s);
/* Counters for the latency model of bench.py's C5 line: encoder / decoder chunks run since creation and the
 * node count of each captured chunk graph (0 before the capture). */
int sd_fseend_stream_stats(const sd_fseend_stream* s, int64_t* enc_runs, int64_t* dec_runs, int* enc_nodes,
                           int* dec_nodes);
/* Diagnostics: the decode attention's per-(slot, head) block-merge counters, then the slot block's arrival
 * counter, copied to host_out (at most cap) after `stream` drains; *n = how many there are.  Each runs
 * 0..blocks-1 by a wrapping increment and is 0 between launches (test_gpu_fseend_stream.py). */
int sd_fseend_stream_debug_counters(const sd_fseend_stream* s, unsigned* host_out, int cap, int* n, void* stream);
int sd_fseend_stream_destroy(sd_fseend_stream* s);

/* Test-only single ops of the FS-EEND streaming kernels (csrc/stream_ops.hip).  Every pointer is a device pointer
 * and the data is already in its io dtype (fp32, or bf16 where a *_bf16 flag says so); nothing is allocated or
 * zeroed for the caller: workspaces, counters and cursors are the caller's.  Counters are unsigned words zeroed
 * ONCE; every launch leaves them at 0 again, so launches that run one after another share them.
 *
 * sd_attn_decode_blocks: partials per (sequence, head) that a history of max_keys rows needs (n_blocks below).
 * sd_op_attn_decode: chunked causal attention, head size 64.  Strides in elements: query i of sequence s at
 *   q + i q_tok + s q_seq (+ 64 head), key / value j at k / v + j kv_tok + s kv_seq (+ 64 head), output at
 *   out + i o_tok + s o_seq (+ 64 head).  Query i sits at *pos + i and sees key j iff j <= *pos + i + delay and
 *   j < *pos + nq.  1 <= nq <= 32; k, v 16-byte aligned with strides of 16-byte multiples.  ws: nseq nh n_blocks nq
 *   66 floats, n_blocks >= sd_attn_decode_blocks(max_keys).  cnt (optional): nseq nh counters; the last block
 *   of each (sequence, head) merges the partials in the same launch (NULL: a separate combine launch).  wo, bo, o2,
 *   ws2, cnt2 (optional, all or none, with cnt): o2 = out-row W_oᵀ + bo in the same launch when nq == 1 and nh <= 4,
 *   wo (nh 64, nh 64) in the io dtype and 16-byte aligned, o2 rows laid out as out's with nh 64 values each, ws2: nseq
 *   nh nq nh 64 floats, cnt2: nseq counters; `out` is not written then.  *ran_out_proj = 1 iff that path ran.
 * sd_op_stream_slot_block: y = LN(ln_x + ln_t) -> ln_out (fp32); out = MHA over the C slots of each of the c frames
 *   of y (w_in (3D, D), w_out (D, D), weights in the w dtype), rows (c C, D).  ln_t may be NULL.  ws: nh c C D
 *   floats, cnt: 1 counter.  *ran = 0 and nothing launched unless D == 256, nh == 4, c C <= 16, C <= 8, ws and cnt
 *   set and ln_x, ln_g, ln_b, ln_out, w_in, w_out 16-byte aligned.
 * sd_op_stream_ffn_pair: y = LN(ln_x + ln_t) -> ln_out; out = relu(y W1ᵀ + b1) W2ᵀ + b2, w1 (F, D), w2 (D, F).
 *   ws: 128 * 8 * D floats, cnt: 1 counter.  *ran = 0 and nothing launched unless D == 256, F == 2048,
 *   1 <= n <= 8, ln_g / ln_b / ln_out / ws / cnt set and w1, w2, ln_x, ln_out, out, ws, b2 16-byte aligned.
 * sd_op_kv_append: dst row (*cursor mult + r) = src row r for r < rows; rows of width_bytes at byte strides
 *   ld_src_bytes / ld_dst_bytes, all 16-byte multiples, 16-byte aligned buffers.
 * sd_op_gather_window: dst (rows, D) = hist rows [*cursor - pad, *cursor - pad + rows), zero outside [0, *n_valid).
 * sd_op_cursor_advance: *cursor += by; *mirror (optional) = the new value.
 * sd_op_stream_enc_finish: hist row (*cursor + r) = LN(x + t)[r] for r < c (t optional; D in 256/512/768/1024), then
 *   *cursor += c and *mirror (optional) = *cursor.
 * sd_op_stream_dec_finish: a = LN(x + t) over the c C rows, scores[r] = emb[r / C] . a[r] / |a[r]| (emb (c, D)), then
 *   *cursor += c. */
int sd_attn_decode_blocks(int max_keys);
int sd_op_attn_decode(const void* q, int64_t q_tok, int64_t q_seq, const void* k, const void* v, int64_t kv_tok,
                      int64_t kv_seq, void* out, int64_t o_tok, int64_t o_seq, int nseq, int nq, int nh, float scale,
                      const int* pos, int delay, int max_keys, int io_bf16, float* ws, int n_blocks, unsigned* cnt,
                      const void* wo, const float* bo, void* o2, float* ws2, unsigned* cnt2, int* ran_out_proj,
                      void* stream);
int sd_op_stream_slot_block(const float* ln_x, const void* ln_t, int t_bf16, const float* ln_g, const float* ln_b,
                            float eps, float* ln_out, const void* w_in, const float* b_in, const void* w_out,
                            const float* b_out, int w_bf16, void* out, int out_bf16, float* ws, unsigned* cnt, int c,
                            int C, int D, int nh, float scale, int* ran, void* stream);
int sd_op_stream_ffn_pair(const float* ln_x, const void* ln_t, int t_bf16, const float* ln_g, const float* ln_b,
                          float eps, float* ln_out, const void* w1, const float* b1, const void* w2, const float* b2,
                          int w_bf16, void* out, int out_bf16, float* ws, unsigned* cnt, int n, int D, int F, int* ran,
                          void* stream);
int sd_op_kv_append(const void* src, int64_t ld_src_bytes, int rows, int width_bytes, void* dst, int64_t ld_dst_bytes,
                    const int* cursor, int mult, void* stream);
int sd_op_gather_window(const float* hist, int D, const int* cursor, const int* n_valid, int pad, int rows, float* dst,
                        void* stream);
int sd_op_cursor_advance(int* cursor, int by, int* mirror, void* stream);
int sd_op_stream_enc_finish(const float* x, const void* t, int t_bf16, const float* g, const float* b, float eps, int c,
                            int D, float* hist, int* cursor, int* mirror, void* stream);
int sd_op_stream_dec_finish(const float* x, const void* t, int t_bf16, const float* g, const float* b, float eps, int c,
                            int C, int D, const float* emb, float* scores, int* cursor, void* stream);

/* feature.stft + feature.transform('logmel23_mn' | 'logmel23') + feature.splice + [::subsampling]
 * (speaker_diarization/feature.py:155-184, 56-73, 130-152; eend_eda/infer_eda.py:94-98).
 * wav: device f32 (n_samples) (soundfile values, computed in float64 like the reference);
 * n_frames: STFT frames = 1 + n_samples/frame_shift, minus one when divisible (feature.py:176-184);
 * mel_fb: device (n_mels, n_fft/2+1) Slaney mel (librosa.filters.mel, host-built);
 * mean_norm: 1 for logmel23_mn; work: device float64 (n_frames*n_mels + n_mels);
 * out: device (ceil(n_frames/subsampling), ld_out) f32, columns >= (2c+1)*n_mels zeroed. */
int sd_eend_features(const float* wav, int64_t n_samples, int frame_size, int frame_shift, int n_frames,
                     const float* mel_fb, int n_mels, int mean_norm, int context_size, int subsampling,
                     double* work, float* out, int ld_out, void* stream);

/* ------------------------------------------------------------------ frontend
 * FBank.__call__ (ts_vad2/ts_vad_dataset.py:29-56) over a whole recording at
 * dither 0: wav (n_samples) device fp32 in [-1,1), in_scale = 32768.
 * mel_fb: device (n_mels, 257) HTK banks (host-built, see frontend.py).
 * out: device (n_frames, n_mels), n_frames = 1 + (n_samples - 400) / 160. */
int sd_fbank_kaldi(const float* wav, int64_t n_samples, float in_scale, int n_frames,
                   const float* mel_fb, int n_mels, float* out, void* stream);
/* Same with the window chosen: window_type 0 hamming (TS-VAD FBank, ts_vad_dataset.py:45-52),
 * 1 povey (kaldi.fbank's default, used by the embedding extractor's FBank,
 * generate_chunk_speaker_embedding_from_modelscope_for_diarization.py:317-331, in_scale 1). */
int sd_fbank_kaldi_ex(const float* wav, int64_t n_samples, float in_scale, int n_frames, const float* mel_fb,
                      int n_mels, int window_type, float* out, void* stream);
/* Window slicing + per-window mean normalisation (mean_nor=True, :55) + the
 * collater's zero pad to the batch max (ts_vad_dataset.py:664-701).
 * win_start / win_n: device int32 (n_win). out: device (n_win, T_out, n_mels). */
/* The same gather on a raw waveform (TS-VAD variants 5 / 6; no mean removal, as ts_vad_dataset.py:185-188 does none):
 * out (n_win, n_out) with out[w, j] = wav[win_start[w] + j] for j < win_n[w] (inside the n_total samples), else 0. */
int sd_window_wave(const float* wav, int64_t n_total, const int* win_start, const int* win_n, int n_win, int n_out,
                   float* out, void* stream);
int sd_window_cmn(const float* feats, int n_mels, const int* win_start, const int* win_n, int n_win,
                  int T_out, float* out, void* stream);

/* ------------------------------------------------------------------ posteriors
 * sigmoid (model.py:945-946) + mean over the overlapping windows covering each
 * label frame, in window order (ts_vad2/infer.py:90-94).  logits: device
 * (n_win, NS, Tw); start/len: device int32 (n_win) in label frames; windows start
 * every `dis` frames and span at most `chunk`.  out: device (NS, n_frames). */
int sd_overlap_average(const float* logits, int n_win, int NS, int Tw, const int* start,
                       const int* len, int dis, int chunk, int n_frames, float* out, void* stream);
/* The same mean over already-sigmoided probabilities (the res_dict lists of
 * TSVADModel.infer, model.py:945-966, averaged by infer.py:90-94): bit-identical to
 * np.mean of each frame's float32 list in window order (float32 sum from 0 in window
 * order, then one correctly rounded division by the count).  NaN where no window
 * covers a frame. */
int sd_overlap_mean(const float* probs, int n_win, int NS, int Tw, const int* start,
                    const int* len, int dis, int chunk, int n_frames, float* out, void* stream);

/* ------------------------------------------------------------------ postprocess
 * Replaces the host loop of ts_vad2/infer.py:72-130 (postprocess): per track
 * (one (meeting, speaker) posterior row of T frames) scipy.signal.medfilt(med_filter)
 * -> for each threshold: >= threshold (float32 compare), change_zeros_to_ones
 * (silence runs <= min_silence_frames become speech, :27-47), change_ones_to_zeros
 * (speech runs <= min_speech_frames become silence, :50-70) -> speech runs as
 * [begin, end) frame pairs.  min_*_frames = int(min_* // frame_len) as the recipe
 * computes it.  post: device (rows, T) f32.  thresholds: HOST array (1..16).
 * seg_begin/seg_end: device int32 (rows * n_thresholds, cap), cap >= (T+1)/2;
 * n_seg: device int32 (rows * n_thresholds), row-major (row, threshold).
 * RTTM formatting stays on the host (speaker_diarization_amd/ts_vad/postprocess.py).
 * flags bit 0: speech iff x > threshold (EEND bin/make_rttm.py:29, medfilt of the 0/1
 * decisions == threshold of the medfilt'd posteriors) instead of >=.
 * T <= 524288 frames. */
int sd_postprocess_segments(const float* post, int rows, int T, int med_filter, const float* thresholds,
                            int n_thresholds, int min_silence_frames, int min_speech_frames, int cap,
                            int* seg_begin, int* seg_end, int* n_seg, int flags, void* stream);

/* ------------------------------------------------------------------ ops (parity tests)
 * precision: 0 fp32, 1 bf16 MFMA (fp32 activations), 2 bf16 MFMA on bf16 activations
 * (the input is converted first; exercises the LDS-DMA GEMM path).
 * Weights are fp32 device arrays in torch layout. */
/* nn.Linear: out (M, N) = act(x (M, K) · w (N, K)ᵀ + b). act: 0 none 1 relu 2 sigmoid 3 silu */
int sd_op_linear(const float* x, int M, int K, const float* w, const float* b, int N, int act,
                 float* out, int precision, void* stream);
/* bf16 GEMM as the encoders run it: x bf16 bits (M rows, stride lda, columns
 * [a_coff, a_coff + K)); optional per-input-channel BN-ReLU prologue
 * x' = relu(x * pre_scale + pre_shift) (CAM++ nonlinear1, model.py dense layers);
 * out bf16 bits (M, ldo) = act(alpha * (x' · wᵀ) + beta). */
int sd_op_gemm_bf16(const void* x, int M, int K, int lda, int a_coff, const float* w, int N,
                    const float* pre_scale, const float* pre_shift, const float* alpha, const float* beta,
                    int act, void* out, int ldo, void* stream);
/* One conv_gemm call with every option of its argument struct (kernels.h ConvGemmArgs), through the production
 * dispatch: which kernel runs follows from the arguments alone, as in the models (tests/test_gpu_gemm_paths.py).
 *   A: channel-last activations, element (b, h, w, c) at A[((b*H + h)*W + w)*lda + a_coff + c], fp32 or bf16 bits
 *      (a_bf16); a_tiled: in the row programs' fragment layout (lda == Cin, rows % 16 == 0).
 *   w: fp32 (N, Cin, kh, kw) in torch order; packed here (rounded to bf16 at precision 1; with glu the rows are
 *      [N/2 values | N/2 gates], as are alpha / beta, and all are interleaved here in groups of 16).
 *   precision: 0 exact fp32, 1 bf16 MFMA, 2 bf16x3 (0 and 2 take fp32 tensors).
 *   x = acc * alpha[n] + beta[n] + res[m * res_ld + n]; x = act(x); x = x * post_scale[n] + post_shift[n];
 *   x *= gate[(b * gate_nseg + wo / gate_seg) * N + n]; out[b*o_sb + ho*o_sh + wo*o_sw + n*o_sn] (fp32 or bf16 bits).
 *   pre_scale / pre_shift [Cin]: a' = relu(a * s + h) on load (padding stays 0).  act: 0 none, 1 relu, 2 sigmoid,
 *   3 silu, 4 clamp to [0, 20], 5 erf GELU, 6 tanh GELU.  glu: out channel c = value_c * sigmoid(gate_c), N / 2 wide.
 *   ln_* / pro_* / kv_*: the prologues and the K-V epilogue of the <= 16-row kernel, as documented in kernels.h.
 *   ksplit_out (device int, nullable): receives gemm_splitk_count; above 1 the product is written as that many fp32
 *   (M, N) slabs to `slabs` (slab_cap of them allocated) instead of `out`, beta in slab 0 only.
 * Every pointer is a device pointer or NULL.  Synchronises `stream` when ksplit_out or glu is set. */
typedef struct sd_gemm_op {
  int precision;
  const void* A;
  int a_bf16, a_tiled;
  int B, H, W, Cin, lda, a_coff;
  int kh, kw, sh, sw, ph, pw, dh, dw;
  const float* w;
  int N;
  const float *pre_scale, *pre_shift, *alpha, *beta;
  const void* res;
  int res_bf16, res_ld;
  int act;
  const float *post_scale, *post_shift;
  const float* gate;
  int gate_seg, gate_nseg;
  void* out;
  int out_bf16;
  int64_t o_sb, o_sh, o_sw, o_sn;
  int glu;
  const float* ln_x;
  const void* ln_t;
  int ln_t_bf16;
  const float *ln_g, *ln_b;
  float ln_eps;
  float* ln_out;
  int pro_mode;
  const float* pro_p;
  int pro_C, pro_pad;
  const int *pro_cursor, *pro_nvalid;
  void* kv_out;
  const int* kv_cursor;
  int kv_mult, kv_col0;
  int64_t kv_ld;
  int* ksplit_out;
  float* slabs;
  int slab_cap;
} sd_gemm_op;
int sd_op_conv_gemm(const sd_gemm_op* op, void* stream);
/* One CAM++ dense layer, bf16 (CAMDenseTDNNLayer + CAMLayer, egs/alimeeting/ts_vad2/cam_pplus_wespeaker.py:
 * 79-168) as the TS-VAD / embedding trunk runs it (cam_dense.hip): x bf16 bits (B, T, ld), input channels
 * [0, cin); out: bf16 bits at x's channels [cin, cin + 32) (out may alias x + cin).  s1/h1: nonlinear1
 * folded [cin]; wb: linear1 weight fp32 (128, cin); a2/b2: nonlinear2 folded [128]; wl: linear_local weight
 * fp32 (32, 128, 3); bl: its bias [32] or NULL; w1/c1: cam_layer.linear1 (64, 128)/(64); w2/c2:
 * cam_layer.linear2 (32, 64)/(32).  T <= 320, dil 1 or 2, cin % 32 == 0, cin <= 992.  repeats: run the
 * launch that many times on the same exchange records / counters (each must give the same bits). */
int sd_op_cam_dense(const void* x, int B, int T, int ld, int cin, int dil, const float* s1, const float* h1,
                    const float* wb, const float* a2, const float* b2, const float* wl, const float* bl,
                    const float* w1, const float* c1, const float* w2, const float* c2, void* out, int repeats,
                    void* stream);
/* One BasicResBlock of the CAM++ FCM head (cam_pplus_wespeaker.py:240-268) on a bf16 NHWC map x (B, H, W, 32):
 * out bf16 NHWC (B, (H - 1) / stride + 1, W, 32) = relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut), 3x3 convs
 * with pad 1, conv1 with freq stride `stride` (1 or 2).  w1 / w2 fp32 (32, 32, 3, 3) (rounded to bf16), a / b the
 * folded BatchNorms [32].  stride 1: identity shortcut, wsc / asc / bsc NULL; stride 2: wsc fp32 (32, 32, 1, 1),
 * shortcut = conv1x1(x, stride (2, 1)) * asc + bsc.  fused 1: one launch (fcm_conv.hip fcm_block_kernel; out
 * must not overlap x); 0: the trunk's two launches on scratch maps.  Both give the same values. */
int sd_op_fcm_block(const void* x, int B, int H, int W, int stride, const float* w1, const float* a1, const float* b1,
                    const float* w2, const float* a2, const float* b2, const float* wsc, const float* asc,
                    const float* bsc, void* out, int fused, void* stream);
/* The CAM++ FCM stem + layer1.0 (cam_pplus_wespeaker.py:240-308) from the fbank (B, W, F) fp32: stem = relu(bn(conv3x3(
 * fbank, 1 -> 32, pad 1))) with stem_w fp32 (32, 1, 3, 3) and stem_alpha / stem_beta the folded BatchNorm [32], then
 * the stride-2 BasicResBlock of sd_op_fcm_block (w1 .. bsc as there; the shortcut is required).  out bf16 NHWC
 * (B, (F - 1) / 2 + 1, W, 32).  fused 1: one launch (fcm_conv.hip fcm_stem_block_kernel; raises where it does not
 * apply, e.g. W < 113; out must not overlap the fbank); 0: the trunk's two launches (stem computed inside conv1) on
 * scratch maps.  Both give the same values wherever fused 1 is accepted. */
int sd_op_fcm_stem_block(const float* fbank, int B, int W, int F, const float* stem_w, const float* stem_alpha,
                         const float* stem_beta, const float* w1, const float* a1, const float* b1, const float* w2,
                         const float* a2, const float* b2, const float* wsc, const float* asc, const float* bsc,
                         void* out, int fused, void* stream);
/* Diagnostics: while `stamps` (device, >= 16 u64 per workgroup of a launch) is non-NULL, every cam_dense
 * launch records its workgroups' phase-boundary s_memrealtime stamps there (tools/cam_dense_probe.py). */
int sd_debug_cam_dense_probe(void* stamps);
/* Diagnostics: while `stamps` (device, >= 64 u64 per workgroup, zeroed) is non-NULL, every conformer pw2 + FFN
 * row-program launch (rowprog.hip, program 5) runs its stamping instantiation: lane 0 of every wave adds the
 * s_memtime cycles of its phases to stamps[(workgroup * 8 + wave) * 8 + k], k = 0 whole launch, 1 piece waits,
 * 2 refill issue, 3 epilogue, 4 tile loads (tools/rowprog_probe.py). */
int sd_debug_rowprog_probe(void* stamps);
/* Diagnostics: a captured graph [memsetAsync(X, 0) -> kernel: Y = X, then X = 7] (fork != 0: the kernel behind
 * an event fork / join of a second captured stream) replayed `replays` times; bad_per_replay (host, replays
 * ints) = Y values that were not 0 after each replay. */
int sd_probe_graph_memset(int n, int replays, int fork, int* bad_per_replay, void* stream);
/* The conformer self-attention block's in-projection + attention (mha_block.hip; torchaudio MHA with
 * batch_first, 8 heads of 48, D 384) on LayerNorm'd bf16 rows y (S, T, 384): w (1152, 384) / bias (1152) the
 * packed in_proj, key_len device int32 (S) or NULL, out bf16 (S, T, 384) = the heads' outputs before out_proj.
 * variant: the kernel layout (-1 or 0: the shipped <2 sequences, 8 waves, 3-slot ring, 48-wide Q / K rows>;
 * 1-7 the round-5 sweep's other layouts, mha_block.hip; tests).  flags (round 6): bit 0 = y given in the row
 * programs' MFMA-fragment layout (RowProgArgs::a_tiled), bit 1 = out written in it (S * T % 16 == 0). */
int sd_op_mha_block(const void* y, const float* w, const float* bias, int S, int T, const int* key_len, void* out,
                    int variant, int flags, void* stream);
/* The conformer conv module's depthwise conv over time (ops.hip glu_dwconv; kernel k odd <= 31, pad (k - 1) / 2, zeros
 * outside each sequence) on S sequences, optionally followed by GroupNorm(1 group) + SiLU (groupnorm_silu).  x (S, T, C)
 * or, with glu_in, the pointwise_conv1 output (S, T, 2 C) whose columns are 32-wide groups [16 values | their 16
 * gates] (the GLU is applied on load); fp32, or bf16 bits with io_bf16 (y too).  w (C, k), bias (C) fp32; C % 16 == 0.
 * mode 0: y = silu(conv) (the BatchNorm-folded form), partial unused; 1: y = conv and partial (S, cdiv(C, 64), 2) fp32 =
 * each 64-channel block's (sum, sum of squares) of y over the sequence; 2: mode 1, then y = silu(GroupNorm(y) * gn_g +
 * gn_b) in place, eps 1e-5.  Which kernel runs follows from the shape alone, as in the product. */
int sd_op_glu_dwconv(const void* x, int S, int T, int C, const float* w, const float* bias, int k, int glu_in,
                     int io_bf16, int mode, const float* gn_g, const float* gn_b, void* y, float* partial,
                     void* stream);
/* One conformer row program (rowprog.hip) over M rows of D = 384, every optional part selectable:
 *   acc = X (fp32 rows), or row (s, t) = [ts[s] | mix[s / NS][t]] (192 + 192; zeros for t >= Tmix) of T_seq rows per
 *         sequence when ts is set (ts (M / T_seq, 192), mix (., Tmix, ldmix) fp32);
 *   acc += A w0^T + b0 when w0 is set (A (M, 384) bf16 bits, w0 (384, 384) fp32 torch layout, rounded to bf16); with
 *         gn_partial, A is first replaced by silu(GroupNorm(A) * gn_g + gn_b), one group per gn_T rows, statistics
 *         from gn_partial (M / gn_T, gn_nblk, 2) = (sum, sum of squares) partial sums;
 *   per FFN i < n_ffn: acc += w2 silu(w1 LN(acc; ln_g, ln_b) + b1) + b2, then acc = LN(acc; post_g, post_b) when post_g
 *         is set; w1 (hidden, 384), w2 (384, hidden) fp32, hidden % 32 == 0, <= 1536.  Nothing is scaled here: a caller
 *         that wants the module's 1/2 passes w2 / b2 halved;
 *   Xo = acc (fp32, nullable, may equal X); y = LN(acc; y_g, y_b) as bf16 bits (nullable); yt (nullable) = bf16(acc) in
 *         the speakers-to-channels layout (M / (yt_NS T_seq), T_seq, yt_NS * 384).
 * All LayerNorms use eps 1e-5.  Every pointer is a device pointer.  flags: bit 0 X, bit 1 Xo, bit 2 A, bit 3 y in the
 * MFMA-tiled layouts (kernels.h RowProgArgs::x_tiled / a_tiled; M % 16 == 0, else SD_ERR_INVALID).  Synchronises
 * `stream` (the weights are packed on the host). */
typedef struct sd_rowprog_ffn {
  const float *ln_g, *ln_b, *w1, *b1, *w2, *b2, *post_g, *post_b;
  int hidden;
} sd_rowprog_ffn;
typedef struct sd_rowprog_op {
  int M, flags;
  const float* X;
  float* Xo;
  const float *ts, *mix;
  int ldmix, Tmix, NS, T_seq;
  const void* A;
  const float *w0, *b0;
  const float *gn_partial, *gn_g, *gn_b;
  int gn_T, gn_nblk;
  int n_ffn;
  sd_rowprog_ffn ffn[2];
  const float *y_g, *y_b;
  void* y;
  void* yt;
  int yt_NS;
} sd_rowprog_op;
int sd_op_rowprog(const sd_rowprog_op* op, void* stream);
/* torchaudio.models.Conformer (input_dim 384, convolution after attention) of n_layers layers on x (S, T, 384) fp32 ->
 * out (S, T, 384) fp32, key_len device int32 (S) or NULL.  weights: one fp32 device array of n_weights floats, for
 * layer 0 .. n_layers - 1 the layer's tensors flattened in its state_dict order: ffn1.sequential.{0.weight, 0.bias,
 * 1.weight (ffn_dim, 384), 1.bias, 4.weight (384, ffn_dim), 4.bias}, self_attn_layer_norm.{weight, bias},
 * self_attn.{in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias}, conv_module.layer_norm.{weight, bias},
 * conv_module.sequential.{0.weight (768, 384, 1), 0.bias, 2.weight (384, 1, kernel), 2.bias, 3.weight, 3.bias,
 * [group_norm 0 only: 3.running_mean, 3.running_var,] 5.weight (384, 384, 1), 5.bias}, ffn2.sequential.* as ffn1,
 * final_layer_norm.{weight, bias}.  They go through the product's loader (the 1/2 fold, the GLU row interleave, the
 * BatchNorm fold, the row-program packing).  precision 0 fp32, 1 bf16, 2 bf16x3.  use_generic 1: one run_conformer per
 * layer; 0: run_conformer_stack's row programs (precision 1 only, SD_ERR_INVALID otherwise).  Speaker-stream mode (ts
 * non-NULL, x NULL, precision 1, use_generic 0): the input rows of sequence s = b * NS + spk are [ts[s] | mix[b][t]]
 * (ts (S, 192), mix (S / NS, Tmix, ldmix) fp32, zeros for t >= Tmix) and out is bf16 (S / NS, T, NS * 384).
 * Synchronises `stream`. */
/* Measurement and tests only (tools/conformer_backend_probe.py): which bf16 path serves a TS-VAD conformer back end
 * (backend 4 / 5) whose FFN hidden size is past 1024.  0: the shipped rule, run_conformer per layer (the fused stack
 * measured no faster there); 1: the row programs, the single stack's last one writing the speakers-to-channels layout.
 * Process-wide; read by each forward. */
int sd_debug_conformer_wide_route(int route);
int sd_op_conformer_stack(const float* x, int S, int T, const float* weights, int64_t n_weights, int n_layers,
                          int ffn_dim, int nh, int kernel, int group_norm, const int* key_len, int precision,
                          int use_generic, const float* ts, const float* mix, int ldmix, int Tmix, int NS, void* out,
                          void* stream);
/* nn.Conv1d on channel-last input x (B, T, Cin) with weight (Cout, Cin, k) -> out (B, To, Cout). */
int sd_op_conv1d(const float* x, int B, int T, int Cin, const float* w, const float* b, int Cout,
                 int k, int stride, int pad, int dil, int act, float* out, int precision, void* stream);
/* nn.Conv2d (Cin % 32 == 0) on NHWC x (B, H, W, Cin), weight (Cout, Cin, kh, kw) -> NHWC out. */
int sd_op_conv2d(const float* x, int B, int H, int W, int Cin, const float* w, int Cout, int kh,
                 int kw, int sh, int sw, int ph, int pw, float* out, int precision, void* stream);
/* The ResNet stems (Cin = 1, 3x3, pad 1 + folded BN + ReLU; resnet_wespeaker.py:127-128, samresnet_wespeaker.py:82-85):
 * fbank (B, T, F) fp32, w (C, 1, 3, 3) fp32, C = 32 or 64 -> out NHWC (B, F, T, C), fp32 or bf16 bits (out_bf16). */
int sd_op_stem_conv(const float* fbank, int B, int T, int F, const float* w, const float* alpha, const float* beta,
                    int C, void* out, int out_bf16, void* stream);
/* One 3x3, pad-1 convolution of the ResNet34 trunk on a bf16 NHWC map x (B, H, W, Cin), weight fp32 (Cout, Cin, 3, 3)
 * (rounded to bf16), Cin and Cout in {32, 64, 128, 256, 512}, stride 1 or 2 (both axes): out bf16 NHWC (B, Ho, Wo, Cout) =
 * relu(conv * alpha + beta [+ res]), res bf16 NHWC like out or NULL.  sc_w (Cout, Cin, 1, 1) or NULL: the block's
 * 1x1 shortcut at the same stride, sc_out bf16 = conv1x1 * sc_alpha + sc_beta (no ReLU).  use_generic 0: res_conv.hip
 * (the shortcut from the centre tap of the same launch); 1: the same arguments through conv_gemm. */
int sd_op_res_conv(const void* x, int B, int H, int W, int Cin, const float* w, int Cout, int stride,
                   const float* alpha, const float* beta, const void* res, const float* sc_w, const float* sc_alpha,
                   const float* sc_beta, void* out, void* sc_out, int use_generic, void* stream);
/* TSTP (pooling_layers_wespeaker.py:66-88) on a channel-last map x (B, T, C), C % 64 == 0, fp32 or bf16 bits
 * (x_bf16): stats (B, 2C) fp32 = [mean over T | sqrt(unbiased variance over T + 1e-7)].  A NaN stays in its
 * channel; T == 1 gives NaN stds. */
int sd_op_tstp_pool(const void* x, int x_bf16, int B, int T, int C, float* stats, void* stream);
/* Res2Conv1dReluBn at scale 8 (ecapa_tdnn_wespeaker.py:30-79) on a channel-last map x (B, T, 1024): stage i = 0..6
 * computes sp_i = relu(conv_i(sp_{i-1} + x[.., 128 i : 128 i + 128]) + bias_i) * s_i + h_i (stage 0 without sp; conv_i
 * 128 -> 128, k3, dilation = padding = `dilation`, zeros outside the window's own [0, T)) into out[.., 128 i : ..],
 * channels 896.. are copied through.  w fp32 (7, 128, 128, 3), bias / s / h fp32 (7, 128) (s, h: the folded BatchNorm
 * that follows the ReLU).  precision 0: x / out fp32, exact; 1: x / out bf16 bits, bf16 MFMA; 2: fp32, bf16x3.
 * use_generic 1: seven conv_gemm launches (the only form of precision 0 and 2); 0: the single-launch kernel of
 * ecapa.hip (precision 1 and dilation <= 4 only, SD_ERR_INVALID otherwise). */
int sd_op_res2_chain(const void* x, int B, int T, int dilation, const float* w, const float* bias, const float* s,
                     const float* h, void* out, int use_generic, int precision, void* stream);
/* ASTP with the global context (pooling_layers_wespeaker.py:91-144) on a channel-last map x (B, T, 1536), fp32 or
 * bf16 bits (x_bf16): stats (B, 3072) fp32 = [sum_t a x | sqrt(clamp(sum_t a x^2 - mean^2, 1e-7))] with a =
 * softmax over T of linear2(tanh(linear1([x | mean | sqrt(unbiased var + 1e-7)]))).  w1 fp32 (128, 4608), b1 (128), w2
 * (1536, 128), b2 (1536).  The statistics are accumulated in fp64 and the two linears run in fp32 whatever x's type.
 * T < 2 gives SD_ERR_SHAPE (the reference's variance of one frame is NaN). */
int sd_op_astp_pool(const void* x, int x_bf16, int B, int T, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* stats, void* stream);
/* ASP (pooling_layers_wespeaker.py:146-168) on a channel-last map x (B, T, C), C % 64 == 0, fp32 or bf16 bits (x_bf16):
 * stats (B, 2 C) fp32 = [mu = sum_t a x | sqrt(clamp(sum_t a x^2 - mu^2, 1e-5))] with a = softmax over T of
 * w2 bn(relu(w1 x + b1)) + b2.  w1 fp32 (128, C), b1 (128), bn_s / bn_h (128) the folded BatchNorm1d that follows the
 * ReLU, w2 (C, 128), b2 (C).  The two linears run in fp32 and the statistics in fp64 whatever x's type.  T == 1 is
 * valid: mu = x and the second half is sqrt(1e-5) exactly.  A NaN poisons the statistics of its own channel only (the
 * attention GEMM's ReLU is a maximum, which drops it; the bottleneck then spreads it over the item's embedding). */
int sd_op_asp_pool(const void* x, int x_bf16, int B, int T, int C, const float* w1, const float* b1, const float* bn_s,
                   const float* bn_h, const float* w2, const float* b2, float* stats, void* stream);
/* The SimAM gate, shortcut and ReLU of a SimAM BasicBlock (samresnet_wespeaker.py:57-70) on an NHWC map y (B, H, W, C),
 * C % 64 == 0, dtype 0 fp32 / 1 bf16 bits: out (NHWC, y's type) = relu(y * sigmoid((y - mean)^2 / (4 (v + 1e-4)) + 0.5)
 * + residual), mean and v = sum (y - mean)^2 / (H W - 1) per (b, c) in fp64 and a fixed order; residual NHWC like y, or
 * NULL.  A NaN stays in its (b, c) channel; an item's result does not depend on the batch. */
int sd_op_simam(const void* y, const void* residual, int dtype, int B, int H, int W, int C, void* out, void* stream);
/* The 3x3 slice conv of an ERes2NetV2 block (ERes2NetV2.py:73-83) on MFMA, bf16: x NHWC (B, H, W, ldx) bf16 bits whose
 * channels [x_coff, x_coff + width) are the input slice; add (NULL, or a map of row length ld_add) channels [add_coff,
 * ..) are summed on load; w (width, width, 3, 3), alpha, beta (width) fp32 device arrays; out NHWC (B, H, W, ldo) bf16:
 * channels [o_coff, o_coff + width) = clamp(alpha conv(x [+ add]) + beta, 0, 20) with NaN kept and +inf -> 20, every
 * other channel untouched.  width even; offsets and row lengths even (4-byte aligned slices). */
int sd_op_res2_conv3x3(const void* x, int B, int H, int W, int ldx, int x_coff, int width, const void* add, int ld_add,
                       int add_coff, const float* w, const float* alpha, const float* beta, void* out, int ldo,
                       int o_coff, void* stream);
/* AFF(channels C, r 4) per pixel (fusion.py:10-30): x, y, out (P, C) rows, dtype 0 fp32 / 1 bf16 bits; w1 (I, 2 C),
 * w2 (C, I) fp32 device arrays; (a1, c1) (I) and (a2, c2) (C) the conv bias + eval BatchNorm folded to scale and
 * shift.  out = x (1 + tanh att) + y (1 - tanh att), att = a2 (w2 SiLU(a1 (w1 [x | y]) + c1)) + c2, in fp32. */
int sd_op_aff_gate(const void* x, const void* y, int dtype, int64_t P, int C, int I, const float* w1, const float* a1,
                   const float* c1, const float* w2, const float* a2, const float* c2, void* out, void* stream);
/* TS-VAD speaker input through proj_layer (model.py:212-217, 870-876), the stage of configurations with
 * 2 * speaker_embed_dim != transformer_embed_dim: out[(b, spk, t), :] = w [ts[b, spk] | relu(bn(mix[b, t]))] + bias
 * + pe[t], with w (E, 2 SE) split on its input axis (one GEMM over the B * NS embeddings, one over the B * Tmix mix
 * frames, a combine pass).  ts (B, NS, SE); mix (B, Tmix, SE) = speech_down_or_up's conv + bias, rows t >= Tmix
 * read as zeros; bn_a / bn_b (SE) the folded BatchNorm1D; grp (nullable) per-group bypass flags of `group`
 * consecutive windows (ReLU only); pe (T, E) or NULL; out (B * NS * T, E) fp32; out_bf16 (nullable) its bf16
 * copy.  SE and E multiples of 8.  precision 0 fp32, 1 bf16 operands, 2 bf16x3. */
int sd_op_speaker_input_proj(const float* ts, const float* mix, int B, int NS, int T, int Tmix, int SE, int E,
                             const float* w, const float* bias, const float* pe, const float* bn_a, const float* bn_b,
                             const int* grp, int group, float* out, void* out_bf16, int precision, void* stream);
/* Bidirectional Mamba2BlockV2 (ts_vad2/mamba.py:149-213 over mamba_ssm's Mamba2: headdim 64, ngroups 1, d_conv 4,
 * gated RMSNorm) on R independent sequences: x (R, L, E) fp32 -> out (R, L, 2 E) fp32 = [forward chain | backward
 * chain on the reversed sequence, reversed back].  weights: one fp32 device array of n_weights floats, for direction
 * (forward_blocks, backward_blocks), for layer 0 .. n_layer - 1, the block's tensors flattened in this order:
 * norm.weight (E), mixer.in_proj.weight (2 d_inner + 2 d_state + H, E), mixer.conv1d.weight (d_inner + 2 d_state, 1, 4),
 * mixer.conv1d.bias, mixer.dt_bias (H), mixer.A_log (H), mixer.D (H), mixer.norm.weight (d_inner),
 * mixer.out_proj.weight (E, d_inner); d_inner = expand * E, H = d_inner / 64.  precision 0 fp32, 1 bf16 (bf16 GEMM
 * operands, zxbcdt / g and the output stored as bf16; the scan itself is fp32), 2 bf16x3.  Synchronises `stream`. */
/* The "CAM++_frame_level_gsp_fc" stage between the CAM++ trunk and the mix embeddings (sd_tsvad_config_ex.
 * frame_level_gsp; egs/magicdata-ramc/ts_vad2/model.py:1275-1287) as the model runs it, all pointers on the device:
 * x (B, T2, 512) the trunk's transit3 map, fp32 or (x_bf16) bf16 bits, before out_nonlinear; s / h (512) that BatchNorm
 * folded to scale / shift (the ReLU follows); gw (256, 2) / gb (256) gsp_fc; w (SE, 256, 5) / cb (SE) speech_down_or_up.0,
 * UNFOLDED: the call folds them on the host as the model does at finalize (float64:
 * A[o,k] = sum_c w[o,c,k] gw[c,0], S with gw[c,1], C with gb[c]).  Per frame mean and unbiased std over the channels of
 * relu(s x + h), then y[b,j,o] = cb[o] + sum over taps k = 0..4 with 0 <= t = 2 j + k - 2 < T2 of
 * (A[o,k] mean[t] + S[o,k] std[t] + C[o,k]): the reference zero-pads gsp_fc's output, so a padded tap contributes nothing.
 * y (B, (T2 - 1) / 2 + 1, SE) fp32 = conv + bias, before speech_down_or_up.1.  SE a multiple of 32 and T2 >= 1
 * (SD_ERR_INVALID otherwise).  Synchronises `stream`.  sd_gsp_down_frame_tile: the input frames one workgroup's tile
 * covers (a 2-frame halo on each side comes on top), for tests that cross a tile boundary. */
int sd_op_gsp_down(const void* x, int x_bf16, const float* s, const float* h, const float* gw, const float* gb,
                   const float* w, const float* cb, int B, int T2, int SE, float* y, void* stream);
int sd_gsp_down_frame_tile(void);
int sd_op_mamba2_stack(const float* x, int R, int L, int E, const float* weights, int64_t n_weights, int n_layer,
                       int d_state, int expand, int precision, float* out, void* stream);
/* Attention core on packed qkv (S*T, 3D) -> out (S*T, D). */
int sd_op_attention(const float* qkv, int S, int T, int D, int nh, int causal, int causal_delay,
                    const int* key_len, float* out, int precision, void* stream);
/* Chunk-streaming attention (ts_vad2_streaming forward_chunk_by_chunk's KV caches as one
 * block-causal mask): query i sees key j iff j / chunk <= i / chunk and, when left >= 0,
 * j / chunk >= i / chunk - left.  precision as sd_op_attention. */
/* Test op: time attention over a (S, T, C) token grid — qkv (S, T, C, 3D) rows, out (S, T, C, D) —
 * one sequence per (s, c) whose tokens are C rows apart, as the FS-EEND fusion decoder runs it
 * (fs_eend.py:459-478: MHA over time per speaker slot, causal mask).  precision as sd_op_attention. */
int sd_op_attention_grid(const float* qkv, int S, int T, int C, int D, int nh, int causal, int causal_delay,
                         float* out, int precision, void* stream);
int sd_op_attention_chunk(const float* qkv, int S, int T, int D, int nh, int chunk, int left, float* out,
                          int precision, void* stream);
/* Test probe: the attention above (causal / key_len / chunk terms as given) with every visited
 * (query, key) decision of sequence 0, head 0 written to mask_dump (T*T int32, caller-zeroed:
 * 0 = tile not visited, 1 = visible, 2 = masked).  Used by the mask tests only. */
int sd_probe_attention_mask(const float* qkv, int S, int T, int D, int nh, int causal, int causal_delay,
                            const int* key_len, int chunk, int left, int* mask_dump, float* out,
                            int precision, void* stream);
int sd_op_layernorm(const float* x, int rows, int D, const float* g, const float* b, float eps,
                    float* y, void* stream);
/* Residual add + LayerNorm of the encoder blocks: s = x + t (t fp32, or bf16 bits when
 * t_bf16); x <- s when write_x; y = LN(s) (bf16 bits when y_bf16). */
int sd_op_add_layernorm(float* x, const void* t, int t_bf16, int rows, int D, const float* g, const float* b,
                        float eps, int write_x, void* y, int y_bf16, void* stream);
/* LSTM recurrence on precomputed gx (B, T, ndir*4H) (biases included); whh (ndir, 4H, H). */
int sd_op_lstm(const float* gx, int B, int T, int H, int ndir, const float* whh, const int* lengths,
               float* out, float* hT, float* cT, float* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDIAR_H_ */
