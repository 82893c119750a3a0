// WeSpeaker ECAPA-TDNN (egs/alimeeting/ts_vad2/ecapa_tdnn_wespeaker.py:161-254, channels 1024, global-context ASTP)
// on gfx950: the TS-VAD speech encoder of speech_encoder_type "ecapa_channel_1024_wespeaker" (model.py:631-654),
// i.e. ECAPA_TDNN_GLOB_c1024(feat_dim 80, speech_encoder=True).forward(x, get_time_out=True), and the stand-alone
// 192-d target-speaker embedding extractor (generate_chunk_speaker_embedding_from_ecapa_tdnn_for_diarization.py:95-172).
//
// EcapaTrunk mirrors ResTrunk's interface.  layer1 conv(80 -> 1024, k5) -> ReLU -> BN, then three SE-Res2 blocks
// (dilation 2, 3, 4): x + SE(conv1x1(Res2(conv1x1(x)))), each block's output written straight into its channel slice
// of one (B, T, 3072) buffer (no concat copy), then conv 1x1 3072 -> 1536 + ReLU.  Every BatchNorm of the trunk
// FOLLOWS a ReLU, so it is conv_gemm's post-activation affine (ConvGemmArgs::post_scale), never folded into a conv.
// Maps are channel-last (B, T, C), bf16 in bf16 mode; the time axis is never subsampled.
#pragma once
#include <string>
#include "campp.h"

namespace sd {

// Conv1dReluBn (:85-108): relu(conv + bias) * s + h
struct EcapaConv {
  PackedW w;
  const float *bias = nullptr, *s = nullptr, *h = nullptr;
};

// Res2Conv1dReluBn (:30-79, Res2ChainW in kernels.h): x (B, T, 1024) -> out (B, T, 1024).  Stage i reads sp_{i-1} +
// split_i (stage 0: split_0) and writes sp_i = relu(conv + bias) * s + h to channels [128 i, 128 i + 128); group 7 is
// copied through.  Every stage's input is zero outside [0, T) of its own window.  x, out and tmp (B T, 128) are bf16
// when bf16, else fp32 (exact fp32, or bf16x3 under a GemmX3Scope).  generic: seven conv_gemm launches (the only
// form of fp32 / bf16x3); else, in bf16, the single-launch kernel (res2_chain_fused).
void res2_chain(const void* x, int B, int T, int dilation, const Res2ChainW& W, void* tmp, void* out, bool bf16,
                bool generic, hipStream_t st);

class EcapaTrunk {
 public:
  static constexpr int kC = 1024, kCat = 3072, kChannels = 1536;
  // Reads `prefix`{layer1, layer2..4.se_res2block.{0,1,2,3}, conv}.*; kErrParam naming the key on a wrong shape.
  void load(ParamStore& ps, DeviceArena& arena, const std::string& prefix, bool bf16);
  void alloc(DeviceArena& arena, int max_batch, int max_frames);
  // fbank (B, T, 80) fp32 -> (B, T, 1536) channel-last.  b0: the call covers windows [b0, b0 + B) of a batch (fbank =
  // the batch's base; the result is the batch's output map with this slice filled in), so disjoint slices may run on
  // different streams.  The SE means run over all T frames of the call (zero-padded frames included, as in the
  // reference).  No allocation or synchronisation inside.
  Tens forward(const float* fbank, int B, int T, hipStream_t st, int b0 = 0) const;
  bool bf16() const { return bf16_; }

 private:
  struct Block {
    EcapaConv in, out;
    Res2ChainW chain;
    const float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;   // SE_Connect, fp32, both weights transposed
  };
  bool bf16_ = false;
  EcapaConv layer1_;   // packed as a 1x1 conv over ecapa_im2col's 400-wide rows
  Block blocks_[3];
  ConvL conv_;         // 3072 -> 1536 + bias (ReLU)
  void *col_ = nullptr, *h1_ = nullptr, *ya_ = nullptr, *yb_ = nullptr, *tmp_ = nullptr, *cat_ = nullptr, *out_ = nullptr;
  float *mean_ = nullptr, *gate_ = nullptr;
};

struct EcapaConfig {
  int embed_dim = 192;
  int max_batch = 96;        // extract_embed batch_size default (generate_chunk_..._ecapa_tdnn_...py:59-61)
  int max_frames = 598;      // 6 s chunks: 1 + (96000 - 400) / 160
  bool bf16 = false;         // bf16 trunk (maps and conv operands); ASTP, bn and linear stay fp32
};

class EcapaModel : public ModelCore {
 public:
  explicit EcapaModel(const EcapaConfig& c) : cfg_(c) {}
  // fbank (B, T, 80) -> emb (B, E) (nullable): linear(bn(ASTP(trunk))) (:250-254, emb_bn off); time_out (B, T, 1536)
  // channel-last fp32 (nullable): forward(x, get_time_out=True) (:247-249).  emb with T < 2 raises kErrShape.
  void forward(const float* fbank, int B, int T, float* emb, float* time_out, hipStream_t st);
  // the pre-bn ASTP statistics (B, 3072) of the last forward that produced embeddings
  const float* stats() const { return stats_; }

 private:
  void build() override;
  EcapaConfig cfg_;
  EcapaTrunk trunk_;
  PackedW w1x_, w2_;                                   // pool.linear1.weight[:, :1536], pool.linear2.weight (fp32)
  const float *w1c_ = nullptr, *b1_ = nullptr, *b2_ = nullptr;
  ConvL linear_;                                       // linear with bn folded into its input side (fp32)
  float *stats_ = nullptr, *ctx_ = nullptr, *cv_ = nullptr, *x32_ = nullptr, *h_ = nullptr, *e_ = nullptr;
};

}  // namespace sd
