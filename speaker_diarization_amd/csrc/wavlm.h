// WavLM (Base+ / Large) waveform feature extractor, WavLM.extract_features of egs/magicdata-ramc/ts_vad2/wavlm.py:359-414
// (ConvFeatureExtractionModel :434-556, TransformerEncoder :559-675, TransformerSentenceEncoderLayer :678-805,
// MultiheadAttention modules.py:463-579) on gfx950.
//
// Conv front end: layer 0 (1 -> 512, k 10, stride 5) with its norm and GELU straight from the waveform (wavlm.hip),
// layers 1-6 (k 3 / 2, stride 2, unpadded) as conv_gemm's multi-tap strided form on channel-last maps with the erf-GELU
// epilogue ("default") or followed by LayerNorm + GELU ("layer_norm").  The front end runs in slices of kSlice windows,
// so its two ping-pong maps do not grow with max_batch.  Then LayerNorm(512), post_extract_proj, x += GELU(pos_conv(x))
// (wavlm.hip), and the encoder layers on an fp32 residual stream (B T, D): packed q | k | v projection, attention with
// the gated relative-position bias (wavlm.hip), out_proj, fc1 + erf GELU, fc2, post-LN or pre-LN.  bf16 mode: bf16 GEMM
// operands (conv layers 1-6, post_extract_proj, pos_conv, q k v / out / fc, Q K^T and P V) with fp32 accumulation;
// layer 0, every LayerNorm, the softmax, the gates and the residual stream stay fp32.
#pragma once
#include <functional>
#include <string>
#include <vector>
#include "encoder.h"

namespace sd {

struct WavlmConfig {
  int embed_dim = 768, ffn_dim = 3072, heads = 12;   // or (1024, 4096, 16)
  int layers = 12;
  bool layer_norm_mode = false;   // extractor_mode "layer_norm" (else "default")
  bool pre_ln = false;            // layer_norm_first
  int max_batch = 64;
  int max_samples = 64000;
  bool bf16 = false;
  // Split-K FFN down-projections where they pay (post-LN layers).  Their split count depends on the row count, so
  // TS-VAD, whose windows are sharded over ranks with bit-identical results for any world size, turns them off.
  bool split_k = true;
};

// _relative_positions_bucket (modules.py:417-447) of the relative position rel = key - query: bidirectional, 160
// buckets per sign, exact below 80, logarithmic up to max_distance 800.
int wavlm_bucket(int rel);
// weight_norm(dim = 2) of the positional conv folded on the host: out[n, c, tap] = g[tap] v[n, c, tap] / |v[:, :, tap]|
// over v (D, D / 16, 128), the norm taken over the output and input channels of each tap in fp64.
void wavlm_fold_pos_weight(const float* g, const float* v, int D, float* out);

// The model without its handle, in the manner of RedimTrunk: owned by WavlmModel (the extractor) and by TsvadModel under
// the prefix "speech_encoder." (variants 5 and 6, tsvad.h).
class WavlmTrunk {
 public:
  static constexpr int kMinSamples = 400;
  static constexpr int kSlice = 8;   // windows per pass of the conv front end
  // Called on the caller's stream after encoder layer `layer` (0-based) with the residual stream x (B T, D) fp32: the
  // layer's output (ret_layer_results' entry layer + 1), valid until the next layer runs.
  using LayerSink = std::function<void(int layer, const float* x, hipStream_t st)>;
  explicit WavlmTrunk(const WavlmConfig& c) : cfg_(c) {}
  static int frames(int n_samples);          // output frames of the conv front end (0 below 400 samples)
  static int conv_frames(int n, int layer);  // frames after conv layer `layer` (0..6)
  // Reads `prefix`{mask_emb, feature_extractor.*, layer_norm.*, post_extract_proj.*, encoder.*} for cfg.layers encoder
  // layers (both weight-norm spellings of pos_conv); kErrParam naming the key on a wrong shape.
  void load(ParamStore& ps, DeviceArena& arena, const std::string& prefix);
  void alloc(DeviceArena& arena);   // workspace for cfg.max_batch windows of cfg.max_samples
  // source (B, n_samples) fp32 -> x_out (B, T, D) after `output_layer` layers (0: all of them, and in pre-LN mode the
  // final encoder.layer_norm, which extract_features applies only then); features_out (B, T, D) = post_extract_proj's
  // output (ret_conv); layers_out (output_layer + 1, B, T, D) = the input to layer 0 and every layer's output
  // (ret_layer_results; needs output_layer >= 1).  Each nullable.  No allocation or synchronisation.
  void forward(const float* source, int B, int n_samples, int output_layer, float* x_out, float* features_out,
               float* layers_out, hipStream_t st);
  // extract_features(source)[0] for a consumer inside the library: every layer, and in pre-LN mode the final
  // encoder.layer_norm, left in the trunk's own workspace (B T, D): bf16 bits in bf16 mode (the A operand of the GEMM
  // that follows), else fp32.  Valid until the next call.
  Tens encode(const float* source, int B, int n_samples, hipStream_t st);
  // Every layer with `sink` called after each (no final layer_norm: ret_layer_results with output_layer = layers).
  void encode_layers(const float* source, int B, int n_samples, const LayerSink& sink, hipStream_t st);
  const WavlmConfig& config() const { return cfg_; }

 private:
  struct Layer {
    PackedW in_proj, out_proj, fc1, fc2;
    const float *in_b, *out_b, *b1, *b2, *n1g, *n1b, *n2g, *n2b, *grep_w, *grep_b, *grep_a;
  };
  void check_input(int B, int n_samples) const;
  void front_end(const float* source, int B, int n, hipStream_t st);
  // front end, projection, positional conv, bias table: leaves the input to layer 0 in X_ and the features in F_
  void stem(const float* source, int B, int n_samples, hipStream_t st);
  void run_layer(const Layer& L, int B, int T, hipStream_t st);
  WavlmConfig cfg_;
  const float* c0_w_ = nullptr;
  const float *cn_g_[7] = {}, *cn_b_[7] = {};   // layer norms of the conv layers (default mode: layer 0's group norm)
  PackedW conv_[7];                             // layers 1..6
  const float *ln_g_ = nullptr, *ln_b_ = nullptr;
  ConvL proj_;
  PackedW pos_w_;
  const float* pos_b_ = nullptr;
  std::vector<Layer> layers_;
  const float *enc_g_ = nullptr, *enc_b_ = nullptr, *rel_emb_ = nullptr;
  const int* bmap_ = nullptr;
  int max_T_ = 0;
  // workspace
  float *mapA_ = nullptr, *mapB_ = nullptr, *partial_ = nullptr, *ss_ = nullptr;
  float *feat_ = nullptr, *featn_ = nullptr, *F_ = nullptr, *X_ = nullptr, *Y_ = nullptr, *QKV_ = nullptr, *AO_ = nullptr,
        *H_ = nullptr, *table_ = nullptr;
  uint16_t* Yb_ = nullptr;
};

// The extractor handle (sd_wavlm_*): the trunk under no prefix.
class WavlmModel : public ModelCore {
 public:
  static constexpr int kMinSamples = WavlmTrunk::kMinSamples;
  static constexpr int kSlice = WavlmTrunk::kSlice;
  explicit WavlmModel(const WavlmConfig& c) : trunk_(c) {}
  static int frames(int n_samples) { return WavlmTrunk::frames(n_samples); }
  // WavlmTrunk::forward
  void forward(const float* source, int B, int n_samples, int output_layer, float* x_out, float* features_out,
               float* layers_out, hipStream_t st) {
    require_finalized();
    trunk_.forward(source, B, n_samples, output_layer, x_out, features_out, layers_out, st);
  }

 private:
  void build() override {
    trunk_.load(ps_, arena_, "");
    ps_.require_all_used();
    trunk_.alloc(arena_);
  }
  WavlmTrunk trunk_;
};

}  // namespace sd
