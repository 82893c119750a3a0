// w2v-BERT 2.0 speech encoder: transformers' Wav2Vec2BertModel.forward (modeling_wav2vec2_bert.py:991-1050) in eval
// mode with position_embeddings_type "relative_key" and no adapter, as egs/magicdata-ramc/ts_vad2/model.py:805-840 builds
// it (Wav2Vec2BertFeatureProjection :119-131, Wav2Vec2BertEncoderLayer :398-461, Wav2Vec2BertSelfAttention :229-337,
// Wav2Vec2BertConvolutionModule :157-226, Wav2Vec2BertFeedForward :134-154) on gfx950.
//
// Input (B, T2, 160): pairs of 80-bin fbank frames.  LayerNorm(160) -> Linear(160 -> 1024) -> the fp32 residual stream
// (B T2, 1024).  Each layer: x += 0.5 FFN1(LN(x)) (swish; the 0.5 folded into the down projection at load);
// x += Attn(LN(x)) (packed q | k | v projection, relative-key attention of w2vbert.hip, linear_out); x += Conv(x) (LN,
// pointwise_conv1 without bias as plain [value | gate] halves, the conv mix of w2vbert.hip, pointwise_conv2);
// x += 0.5 FFN2(LN(x)); x = final_layer_norm(x).  No encoder-level LayerNorm follows the last layer.  Every residual add
// rides in the LayerNorm that follows it (add_layernorm).  bf16 mode: bf16 GEMM operands (every projection, Q K^T,
// Q E^T and P V; pointwise_conv1's output, which the conv mix reads) with fp32 accumulation; the sub-block outputs, every
// LayerNorm, the softmax, the depthwise conv and the residual stream stay fp32.
#pragma once
#include <string>
#include <vector>
#include "encoder.h"

namespace sd {

struct W2vBertConfig {
  int layers = 6;
  int max_batch = 64;
  int max_frames = 200;   // T2, frames after the pairing
  bool bf16 = false;
};

// The model without its handle, in the manner of WavlmTrunk: owned by W2vBertModel (sd_w2vbert_*) and by TsvadModel
// under the prefix "speech_encoder." (variant 7, tsvad.h).
class W2vBertTrunk {
 public:
  static constexpr int kHidden = 1024, kHeads = 16, kFfn = 4096, kInDim = 160, kConvK = 31, kLeft = 64, kRight = 8;
  explicit W2vBertTrunk(const W2vBertConfig& c) : cfg_(c) {}
  // Reads `prefix`{masked_spec_embed, feature_projection.*, encoder.layers.<i>.*} for cfg.layers layers; kErrParam
  // naming the key on a wrong shape.  masked_spec_embed is training-time masking only: loaded, never read.
  void load(ParamStore& ps, DeviceArena& arena, const std::string& prefix);
  void alloc(DeviceArena& arena);   // workspace for cfg.max_batch windows of cfg.max_frames
  // input_features (B, T2, 160) fp32 -> x_out (B, T2, 1024) = last_hidden_state; layers_out (layers + 1, B, T2, 1024) =
  // hidden_states (the input to layer 0 and every layer's output).  Each nullable.  No allocation or synchronisation.
  void forward(const float* in, int B, int T2, float* x_out, float* layers_out, hipStream_t st);
  // hidden_states[-1] for a consumer inside the library, left in the trunk's workspace (B T2, 1024): bf16 bits in bf16
  // mode (the A operand of the GEMM that follows), else fp32.  Valid until the next call.
  Tens encode(const float* in, int B, int T2, hipStream_t st);
  const W2vBertConfig& config() const { return cfg_; }

 private:
  struct Layer {
    PackedW f1_up, f1_down, in_proj, out_proj, pw1, pw2, f2_up, f2_down;
    const float *f1_g, *f1_b, *f1_b1, *f1_b2, *at_g, *at_b, *in_b, *out_b, *cv_g, *cv_b, *dw_w, *dn_g, *dn_b, *f2_g,
        *f2_b, *f2_b1, *f2_b2, *fin_g, *fin_b;
    const void* dist;   // distance_embedding.weight padded to (kW2vDistRows, 64), bf16 bits in bf16 mode
  };
  void check_input(int B, int T2) const;
  void stem(const float* in, int rows, hipStream_t st);   // feature_projection -> X_
  void run_layer(const Layer& L, int B, int T2, hipStream_t st);
  W2vBertConfig cfg_;
  const float *fp_g_ = nullptr, *fp_b_ = nullptr;
  ConvL proj_;
  std::vector<Layer> layers_;
  // workspace: Fn_ (rows, 160) normalised features; X_ residual stream; T_ a sub-block's output (fp32); Y_ LayerNorm
  // output / AO_ attention and conv-mix output (GEMM A operands, bf16 in bf16 mode); QKV_ (rows, 3072); H_ (rows, 4096)
  // FFN hidden and pointwise_conv1's (rows, 2048); Xb_ bf16 copy of the last layer's output
  void *Fn_ = nullptr, *Y_ = nullptr, *AO_ = nullptr, *QKV_ = nullptr, *H_ = nullptr;
  float *X_ = nullptr, *T_ = nullptr;
  uint16_t* Xb_ = nullptr;
};

// The extractor handle (sd_w2vbert_*): the trunk under no prefix.
class W2vBertModel : public ModelCore {
 public:
  explicit W2vBertModel(const W2vBertConfig& c) : trunk_(c) {}
  void forward(const float* in, int B, int T2, float* x_out, float* layers_out, hipStream_t st) {
    require_finalized();
    trunk_.forward(in, B, T2, x_out, layers_out, st);
  }

 private:
  void build() override {
    trunk_.load(ps_, arena_, "");
    ps_.require_all_used();
    trunk_.alloc(arena_);
  }
  W2vBertTrunk trunk_;
};

}  // namespace sd
