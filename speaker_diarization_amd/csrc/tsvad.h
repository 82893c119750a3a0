// Native TS-VAD inference runner (owns folded weights + workspace).
#pragma once
#include <functional>
#include <memory>
#include <vector>
#include "campp.h"
#include "ecapa.h"
#include "mamba2.h"
#include "redimnet.h"
#include "resnet.h"
#include "wavlm.h"
#include "w2vbert.h"
#include "whisper.h"

namespace sd {

struct TsvadConfig {
  int variant = 0;            // 0: CAM++ + transformer (model.py:758-897); 1: CAM++_ots_vad (669-756);
                              // 2: resnet34_wespeaker + SpeechFeatUpsample2 + transformer (584-606, 114-134)
                              // 3: ecapa_channel_1024_wespeaker + conv k5 stride 4 + transformer (631-654)
                              // 4: ReDimNetB2 on 72-bin fbank + conv k5 stride 4 + transformer
                              //    (egs/magicdata-ramc/ts_vad2/model.py:694-715, 1246-1262, 1296-1309)
                              // 5: WavLM on the raw waveform (wavlm_layers = select_encoder_layer_nums encoder layers,
                              //    extract_features(ref_speech)[0]) + conv k5 stride 2 + transformer (:867-889, 1171-1179)
                              // 6: WavLM_weight_sum with wavlm_fuse_feat_post_norm: every layer's output weighted by
                              //    `weights`, wavlmproj, wavlmlnorm, the same conv (:890-927, 1180-1204)
                              // 7: w2v-bert2 on 80-bin fbank paired to (B, T / 2, 160): the first w2vbert_layers Conformer
                              //    layers of w2v-BERT 2.0, hidden_states[-1] + conv k5 stride 2 + transformer (:805-840,
                              //    1225-1237)
                              // 8: whisper on the raw waveform: the Whisper-PMFA encoder (whisper.h; `whisper` below),
                              //    ln_post2 over the concatenated blocks + conv k5 stride 2 + transformer (:928-955,
                              //    1216-1223)
  int max_num_speaker = 4;
  int rs_len = 4;
  int max_batch = 64;
  int max_fbank_frames = 398;
  bool bf16 = false;
  int num_transformer_layer = 2;
  int num_attention_head = 4;
  int embed_dim = 384;
  int ffn_dim = 1536;
  int speaker_embed_dim = 192;
  int conformer_layers = 6;
  int conformer_heads = 8;
  int conformer_ffn = 512;
  int conformer_kernel = 31;
  int lstm_hidden = 256;
  // 4: single_backend "conformer" + multi_backend "transformer"; 5: "conformer" for both (torchaudio Conformer(E,
  // num_attention_head, ffn_dim, num_transformer_layer, kernel 31), BatchNorm conv module, along TIME; magicdata
  // model.py:290-313, 451-463, 1340-1351, 1382-1390; variant 0 only; d_state / expand unread).  3 is not a back end.
  // 0: the variant's own back end; 1: single_backend "mamba2" + multi_backend "transformer"; 2: "mamba2" for both
  // (egs/magicdata-ramc/ts_vad2/model.py:377-403, 488-504, 1337-1399; variant 0 only).  The Mamba2BlockV2 stacks scan
  // ALONG THE WINDOWS of a reference forward call (forward's forward_batch groups), as the reference's seq-first call
  // of a batch-first module does (model.py:1366-1367, 1393; mamba2.h)
  int backend = 0;
  // speech_encoder_type "CAM++_frame_level_gsp_fc" (egs/magicdata-ramc/ts_vad2/model.py:543-563, 1275-1287): variant 0's
  // trunk and back ends (any of 0, 1, 2, 4, 5) with the stage in between replaced: per-frame mean / unbiased std over the
  // 512 channels of the CAM++ time output, gsp_fc = Linear(2, 256), then Conv1d(256 -> speaker_embed_dim, k5, stride 2,
  // pad 2), run folded as one gsp_down launch (kernels.h).  variant 0 only.
  bool frame_level_gsp = false;
  int d_state = 64;
  int expand = 4;
  // variants 5 / 6: the WavLM geometry (the checkpoint's cfg) and the longest window; ref_speech is (B, n_samples)
  int wavlm_embed_dim = 0;            // 768 (ffn 3072, 12 heads) or 1024 (4096, 16)
  int wavlm_layers = 0;               // encoder layers that run (and that the state_dict holds)
  bool wavlm_layer_norm_mode = false; // extractor_mode "layer_norm"
  bool wavlm_pre_ln = false;          // layer_norm_first
  int max_samples = 0;
  int w2vbert_layers = 0;             // variant 7: encoder layers that run (and that the state_dict holds)
  // variant 8: the trunk's own geometry (sd_tsvad_create_whisper); its max_batch / max_samples / bf16 follow the above
  WhisperConfig whisper;
};

class TsvadModel : public ModelCore {
 public:
  explicit TsvadModel(const TsvadConfig& c) : cfg_(c) {}
  // Raises kErrInvalid for a configuration the runner does not build (sd_tsvad_create calls it): with
  // speaker_embed_dim * 2 != embed_dim the reference inserts proj_layer (model.py:212-217), built for variants 0, 2 and 3.
  static void validate(const TsvadConfig& c);
  // ref_speech (B, T_fb, 80) fbank ((B, T_fb, 72) for variant 4; variants 5 / 6: (B, n_samples) waveform, T_fb carries
  // n_samples, a multiple of 4 in [400, max_samples]), target_speech (B, NS, speaker_embed_dim), logits out (B, NS, T_lab).
  // forward_batch: windows per reference forward call, the scope of BatchNorm1D's NaN bypass (model.py:161-171),
  // i.e. the batch a NaN window disables speech_down_or_up's / backend_down's BatchNorm for; 0: the whole call.
  // force: the call is part of a larger reference batch that holds a non-finite input elsewhere: bit 0 skips
  // both BatchNorms for every window (a non-finite fbank), bit 1 backend_down's (a non-finite v0 embedding).
  void forward(const float* ref_speech, const float* target_speech, int B, int T_fb, int T_lab,
               float* logits, hipStream_t st, int forward_batch = 0, int force = 0);
  // Diagnostics (graph-replay investigation): captures forward() once into a hipGraph on a capture stream
  // (the fork / join side stream included), then replays it `replays` times on st; `dot` (nullable) receives
  // hipGraphDebugDotPrint of the captured graph.
  void forward_graph(const float* ref_speech, const float* target_speech, int B, int T_fb, int T_lab, float* logits,
                     int replays, const char* dot, hipStream_t st);
  // Device buffers of the forward's stages for stage-by-stage comparisons: 0 mix (speech_down_or_up conv),
  // 1 mixg (gsp_fc), 2 X2 (conformer stack output), 3 H (BiLSTM gates), 4 Y (BiLSTM output).
  void debug_buffer(int which, void** ptr, int64_t* bytes) const;
  // waits for `st` and raises kErrHip if a persistent LSTM of the forwards enqueued on it timed out
  void status(hipStream_t st) {
    SD_HIP(hipStreamSynchronize(st));
    raise_if_set();
  }
  ~TsvadModel();

 private:
  void build() override;
  ConvL conv_bn(const std::string& wname, const std::string& bn, const std::string& bias = "");
  LayerLoader loader() { return LayerLoader{ps_, arena_, cfg_.bf16}; }
  ConformerL conformer_layer(const std::string& prefix);
  EncoderWork enc_work() const { return EncoderWork{Y_, QKV_, AO_, H_, partial_, cfg_.bf16}; }
  // Workspace sizes at max_batch windows of max_fbank_frames: frames of a mix row block, label frames of a token
  // row block, token rows, and the elements of the mix (B, T3, SE) and token (rows, E) buffers.
  struct Geometry { int64_t T3, Tl, rows, mix_elems, token_elems; };
  Geometry geometry() const;
  void alloc_workspace();
  // an earlier forward's report nobody collected with sd_tsvad_status: a persistent LSTM's, cam_dense's
  void raise_if_set() {
    lstm_err_.raise_if_set();
    if (cam_) cam_->raise_if_set();
  }
  // The reference's label-length rules (model.py:703-710 / 849-854) and the positional encoding's length.
  void check_label_frames(int T3, int Tl) const;
  // body(b0, Bh, stream) over the batch's windows: once over all of them on st, or (two) over two window slices, the
  // second on side_ between a fork from and a join to st.
  void run_sliced(int B, bool two, hipStream_t st, const std::function<void(int b0, int Bh, hipStream_t s)>& body);
  // speech_encoder.* over windows [b0, b0 + Bh) of the batch, and the speech_down_or_up GEMM over Bh windows of it
  Tens trunk_forward(const float* ref, int Bh, int Tf, hipStream_t s, int b0) const;
  ConvGemmArgs down_gemm(Tens x, int Bh, int Tf, float* out) const;
  void conformer_slice(const float* ts, int T3, int b0, int Bh, int Tl, hipStream_t s, const BnRelu& sd_bn);
  void ots_vad_backend(const float* ts, int T3, int B, int Tl, float* logits, hipStream_t st, const BnRelu& sd_bn,
                       bool conformer_done);
  void transformer_backend(const float* ts, int T3, int B, int Tl, float* logits, hipStream_t st, const BnRelu& sd_bn,
                           const BnRelu& bd_bn);

  TsvadConfig cfg_;
  PinnedFlags lstm_err_;   // poll-timeout reports of the persistent LSTMs (lstm.hip), one slot each

  // speech_encoder.* (get_time_out=True): the one trunk the variant uses, the other stays empty
  std::unique_ptr<CamTrunk> cam_;   // CAM++, variants 0 and 1
  std::unique_ptr<ResTrunk> res_;   // ResNet34, variant 2
  std::unique_ptr<EcapaTrunk> ecapa_;   // ECAPA-TDNN c1024, variant 3
  std::unique_ptr<RedimTrunk> redim_;   // ReDimNetB2, variant 4
  std::unique_ptr<WavlmTrunk> wavlm_;   // WavLM on the waveform, variants 5 and 6
  std::unique_ptr<W2vBertTrunk> w2v_;   // w2v-BERT 2.0 on paired fbank frames, variant 7
  std::unique_ptr<WhisperTrunk> whisper_;   // Whisper-PMFA on the waveform, variant 8
  // values per frame of ref_speech: mel bins, or 1 for the waveform variants
  int feat_dim() const { return waveform() ? 1 : cfg_.variant == 4 ? RedimTrunk::kF : 80; }
  bool waveform() const { return cfg_.variant == 5 || cfg_.variant == 6 || cfg_.variant == 8; }
  // the longest ref_speech time axis: fbank frames, or samples
  int max_input() const { return waveform() ? cfg_.max_samples : cfg_.max_fbank_frames; }
  // frames of the speech_down_or_up output for T_fb fbank frames (the conv's stride 2, the upsampler's 2 T', or
  // ECAPA's and ReDimNetB2's stride 4 on the unsubsampled time axis)
  int mix_frames(int Tf) const {
    if (cfg_.variant == 8) return (WhisperTrunk::frames(Tf) - 1) / 2 + 1;   // Whisper's 50 frames / s likewise
    if (waveform()) return (WavlmTrunk::frames(Tf) - 1) / 2 + 1;   // WavLM's 50 frames / s through the stride-2 conv
    if (cfg_.variant == 3 || cfg_.variant == 4) return (Tf - 1) / 4 + 1;
    if (cfg_.variant == 7) return (Tf / 2 - 1) / 2 + 1;   // w2v-BERT's 50 frames / s through the stride-2 conv
    return cfg_.variant == 2 ? 2 * ResTrunk::out_frames(Tf) : (CamTrunk::out_frames(Tf) - 1) / 2 + 1;
  }
  // the back end of forward_common (variant 0's; also behind the ResNet34 and ECAPA encoders)
  bool transformer_variant() const { return cfg_.variant != 1; }
  bool mamba2_backend() const { return cfg_.backend == 1 || cfg_.backend == 2; }
  bool conformer_backend() const { return cfg_.backend == 4 || cfg_.backend == 5; }
  static constexpr int kConformerKernel = 31;   // depthwise_conv_kernel_size of backend 4 / 5 (magicdata model.py:290-313)
  // speech_down_or_up conv: epilogue = + bias only (its BatchNorm1D is down_bn_).  Variant 2: the transposed conv
  // ConvTranspose1d(2560 -> D, k5, stride 2, pad 2, output_padding 1) as ONE k-3 pad-1 conv with 2 D outputs per
  // input frame j, [even phase y[2j] | odd phase y[2j+1]] = two consecutive rows of the (B, 2 T', D) output.
  ConvL down_;
  // frame_level_gsp: no down_ GEMM; gsp_fc and the conv folded to (5, 3, SE) coefficients + the conv bias (gsp_down)
  const float *gsp_coef_ = nullptr, *gsp_cb_ = nullptr;
  // variant 6: `weights` (L), wavlmproj (SE, D) + wavlmlnorm; acc_ (B T, D) fp32 takes the layer-weighted sum as the
  // layers run, z_ (B T, SE) the projected and normalised map (bf16 in bf16 mode), the conv's A operand
  std::vector<float> mix_w_;
  ConvL wproj_;
  const float *wln_g_ = nullptr, *wln_b_ = nullptr;
  float* acc_ = nullptr;
  void* z_ = nullptr;
  BnRelu down_bn_, backend_bn_;   // folded BatchNorms, applied (or bypassed) by the consumers
  int* nonfinite_ = nullptr;      // [win_fbank B | win_ts B | grp_speech B | grp_backend B]
  const float *gsp_w_ = nullptr, *gsp_b_ = nullptr;
  const float* pe_ = nullptr;
  int pe_len_ = 0;
  // proj_layer (2 SE != E only): weight columns [0, SE) / [SE, 2 SE), bias; P_ts (B NS, E) / P_mix (B T3, E) scratch
  PackedW proj_ts_, proj_mix_;
  const float* proj_b_ = nullptr;
  float *pts_ = nullptr, *pmix_ = nullptr;
  std::vector<TransformerL> single_, multi_;
  // backend 1 / 2: single_backend (and, 2, multi_backend + multi_backend_proj) as Mamba2BlockV2 stacks
  std::unique_ptr<Mamba2Stack> single_m_, multi_m_;
  // backend 4 / 5: single_backend (and, 5, multi_backend) as torchaudio Conformers with a BatchNorm conv module
  std::vector<ConformerL> single_c_, multi_c_;
  ConvL multi_proj_;
  ConvL backend_down_;
  std::vector<ConformerL> conf_;
  PackedW lstm_ih_;
  const float *lstm_b_ = nullptr, *lstm_hh_ = nullptr;
  const void* lstm_hh_bf_ = nullptr;   // bf16 copy of W_hh (bf16 mode; the hi part in fp32 mode)
  const void* lstm_hh_lo_ = nullptr;   // bf16(W_hh - hi) (fp32 handles: the bf16x3 split recurrence)
  ConvL fc_;

  // run_sliced: the speech encoder of a large batch as two window slices, the second on side_ (fork / join
  // events on the caller's stream; all three created by the first such forward): the per-layer launches of one
  // slice fill the CUs the other slice's last round of workgroups leaves idle (cam_dense: 600 items on 256 CUs =
  // 2.34 rounds of 3).
  hipStream_t side_ = nullptr;
  hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;

  // Workspace.
  float *mix_ = nullptr, *mixg_ = nullptr;
  float *X_ = nullptr, *Y_ = nullptr, *QKV_ = nullptr, *AO_ = nullptr, *H_ = nullptr;
  float *X2_ = nullptr, *partial_ = nullptr, *lstm_work_ = nullptr;
};

}  // namespace sd
