// Whisper-PMFA speech encoder: WhisperEncoder.forward of egs/magicdata-ramc/ts_vad2/whisper_encoder.py:150-244
// (ModelDimensions :19-27, MultiHeadAttention :61-113, ResidualAttentionBlock :116-147) in eval mode on gfx950.
//
// wavs (B, n) -> log-mel (B, F, n_mels), F = n / 160 (whisper.hip; fp32 in both precisions) -> conv1 (k3, pad 1) + erf
// GELU -> conv2 (k3, stride 2, pad 1) + erf GELU -> + positional_embedding[:T'], T' = (F - 1) / 2 + 1 -> pre-LN blocks
// x += out(attn(attn_ln(x))); x += mlp.2(GELU(mlp.0(mlp_ln(x)))) -> ln_post2 over the concatenation of the outputs of
// blocks layer_st .. layer_ed.  Both convs and every projection are conv_gemm calls; q | k | v come from one packed GEMM
// with a zero bias on the key third; the reference's 64^-0.25 on q and on k is scale 0.125 on their product in
// sd::attention (head size 64).  No concat copy exists: from block layer_st on, the fp32 residual stream lives in column
// slice (i - layer_st) * D of one (B T', W) buffer, block i + 1 reading slice i and writing slice i + 1 (whisper_add),
// and ln_post2 (whisper_ln_wide) reads that buffer.  Blocks after layer_ed cannot reach the output: their weights are
// loaded (strict) and never run.  bf16 mode: bf16 GEMM, conv and attention operands with fp32 accumulation; the log-mel
// front end, every LayerNorm, the softmax, the GELU inputs, the residual stream and the output stay fp32.
#pragma once
#include <string>
#include <vector>
#include "encoder.h"

namespace sd {

struct WhisperConfig {
  int n_mels = 80, n_ctx = 1500, state = 1280, heads = 20, layers = 24, layer_st = 16, layer_ed = 23;
  int max_batch = 64;
  int max_samples = 64000;
  bool bf16 = false;
};

// The conv stem on log-mel rows feat (B, F, mel_ld) (fp32, or bf16 bits in bf16 mode; columns past n_mels zero):
// X (B, T', D) fp32 = gelu(conv2(gelu(conv1(feat)))) + pe[:T'], T' = (F - 1) / 2 + 1 (:216-231).  conv1: packed
// Wt[D][3 mel_ld], conv2: Wt[D][3 D]; c1: scratch (B F, D) in feat's type.
struct WhisperStemW {
  const void *conv1 = nullptr, *conv2 = nullptr;
  const float *b1 = nullptr, *b2 = nullptr, *pe = nullptr;
  int mel_ld = 0, D = 0;
};
void whisper_stem(const WhisperStemW& w, const void* feat, int B, int F, bool bf16, void* c1, float* X, hipStream_t st);

// The model without its handle, in the manner of WavlmTrunk.
class WhisperTrunk {
 public:
  static constexpr int kMinSamples = 400;
  explicit WhisperTrunk(const WhisperConfig& c) : cfg_(c) {}
  static int mel_frames(int n_samples) { return n_samples / kWhisperHop; }
  static int frames(int n_samples) { return (mel_frames(n_samples) - 1) / 2 + 1; }
  int n_cat() const { return cfg_.layer_ed - cfg_.layer_st + 1; }
  int wide() const { return cfg_.state * n_cat(); }
  // Reads `prefix`{conv1, conv2, positional_embedding, layers.<i>.*, ln_post2} under the reference class's own keys,
  // plus `prefix`mel_filters (n_mels, 201), the host-computed mel matrix; kErrParam naming the key on a wrong shape.
  void load(ParamStore& ps, DeviceArena& arena, const std::string& prefix);
  // workspace for cfg.max_batch windows of cfg.max_samples; with_encode_out: the (B T', W) map encode() returns
  void alloc(DeviceArena& arena, bool with_encode_out = false);
  // wavs (B, n_samples) fp32 -> out (B, T', wide()) fp32.  No allocation or synchronisation.
  void forward(const float* wavs, int B, int n_samples, float* out, hipStream_t st);
  // The same output for a consumer inside the library, left in the trunk's workspace (B T', wide()): bf16 bits in bf16
  // mode (the A operand of the conv that follows), else fp32.  Valid until the next call.
  Tens encode(const float* wavs, int B, int n_samples, hipStream_t st);
  const WhisperConfig& config() const { return cfg_; }

 private:
  struct Layer {
    PackedW in_proj, out_proj, fc1, fc2;
    const float *in_b, *out_b, *b1, *b2, *ag, *ab, *mg, *mb;
  };
  void check_input(int B, int n_samples) const;
  void run(const float* wavs, int B, int n_samples, hipStream_t st);   // the stem and the blocks -> Wide_
  void stem(const float* wavs, int B, int n_samples, hipStream_t st);   // log-mel, conv1, conv2, positions -> X_
  void ln(const float* x, int ldx, int rows, const float* g, const float* b, hipStream_t st);   // a block's LN -> Y_
  // one block reading rows of stride ldx at x and writing rows of stride ldo at out (out may be x)
  void run_layer(const Layer& L, const float* x, int ldx, float* out, int ldo, int B, int T, hipStream_t st);
  WhisperConfig cfg_;
  int mel_ld_ = 0;   // n_mels rounded up to a multiple of 32: the log-mel rows' length, conv1's Cin
  PackedW conv1_, conv2_;
  const float *c1_b_ = nullptr, *c2_b_ = nullptr, *pe_ = nullptr, *post_g_ = nullptr, *post_b_ = nullptr;
  const float *hann_ = nullptr, *basis_ = nullptr, *melT_ = nullptr;
  std::vector<Layer> layers_;
  // workspace: frames_ / spec_ / raw_ / wmax_ the front end's scratch; feat_ (B F, mel_ld_) log-mel and c1_ (B F, D)
  // conv1's output (bf16 in bf16 mode); X_ (B T', D) the residual stream before layer_st; Wide_ (B T', W) after it;
  // T_ a sub-block's output (fp32); Y_ LayerNorm output, QKV_, AO_, H_ GEMM operands (bf16 in bf16 mode)
  float *frames_ = nullptr, *spec_ = nullptr, *raw_ = nullptr, *X_ = nullptr, *Wide_ = nullptr, *T_ = nullptr;
  uint32_t* wmax_ = nullptr;
  void *feat_ = nullptr, *c1_ = nullptr, *Y_ = nullptr, *QKV_ = nullptr, *AO_ = nullptr, *H_ = nullptr;
  void* Out_ = nullptr;   // encode()'s ln_post2 output
};

// The encoder handle (sd_whisper_*): the trunk under no prefix.
class WhisperModel : public ModelCore {
 public:
  explicit WhisperModel(const WhisperConfig& c) : trunk_(c) {}
  void forward(const float* wavs, int B, int n_samples, float* out, hipStream_t st) {
    require_finalized();
    trunk_.forward(wavs, B, n_samples, out, st);
  }

 private:
  void build() override {
    trunk_.load(ps_, arena_, "");
    ps_.require_all_used();
    trunk_.alloc(arena_);
  }
  WhisperTrunk trunk_;
};

}  // namespace sd
