// WeSpeaker ReDimNetB2 (egs/magicdata-ramc/ts_vad2/redimnet_wespeaker.py:925-948: ReDimNet :793-872 over ReDimNetBone
// :623-790 at C 16, F 72, group_divisor 4, "convnext_like" 2-D blocks and "conv+att" 1-D blocks, ASTP with the global
// context) on gfx950: the stand-alone 192-d target-speaker embedding extractor of
// generate_chunk_speaker_embedding_from_wespeaker_for_diarization.py (72-bin povey fbank, 6 s chunks).
//
// RedimTrunk mirrors EcapaTrunk's interface.  Every map is channel-last (B, T, 1152) with 1-D channel f * c + ch, so
// to1d / to2d are views, a stage's (stride, 1) entry conv is a per-pixel linear on stride * c contiguous values, and
// the time axis is never subsampled.  Maps are bf16 in bf16 mode; the 1-D blocks keep their (B T, hC) residual stream
// in fp32 (LayerNorms and softmax in fp32), the transformer heads (24 / 36 / 72 wide) are zero-padded to 32 / 48 / 96
// at upload, which is exact.
#pragma once
#include <string>
#include <vector>
#include "campp.h"

namespace sd {

class RedimTrunk {
 public:
  static constexpr int kF = 72, kC = 16, kChannels = kRedimCF, kStages = 6, kHeads = 4;
  // Reads `prefix`backbone.{inputs_weights.*, stem.*, stage0..5.*}; kErrParam naming the key on a wrong shape.
  void load(ParamStore& ps, DeviceArena& arena, const std::string& prefix, bool bf16);
  void alloc(DeviceArena& arena, int max_batch, int max_frames);
  // fbank (B, T, 72) fp32 -> the frame-level map (B, T, 1152) channel-last (ReDimNet.get_frame_level_feat, :855-859).
  // No allocation or synchronisation inside.
  Tens forward(const float* fbank, int B, int T, hipStream_t st) const;
  bool bf16() const { return bf16_; }
  // Test / measurement only (sd_redimnet_debug_generic): the 2-D blocks' generic arm in bf16 mode too.
  void set_generic(bool on) { generic_ = on; }

 private:
  struct Block1d {   // ConvNeXtLikeBlock, dim 1
    int k = 0;
    const float *dw = nullptr, *dw_b = nullptr;   // (k, hC) with the BatchNorm folded, hC
    ConvL pw;
  };
  struct Stage {
    int stride = 1, c = 0, f = 0, hC = 0, hdp = 0;   // c / f after the entry conv; hdp: padded head width
    float scale = 1.f;                                // head_dim^-0.5 of the TRUE head width
    const float* mix = nullptr;                       // softmax(inputs_weights[i]) (i + 1, 1152); stage 0: none
    ConvL entry;                                      // Wt[stride c_prev][stride c_prev] + bias
    std::vector<RedimBlock2dW> blocks;
    ConvL red;                                        // 1152 -> hC (+ bias), then the channels-first LayerNorm
    const float *red_g = nullptr, *red_b = nullptr;
    Block1d conv[4];
    ConvL qkv, proj, ff1, ff2, exp;                   // padded in / out projections, FFN, hC -> 1152
    const float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  };
  void run_block1d(const Stage& s, const void* map2d, int B, int T, void* out, hipStream_t st) const;

  bool bf16_ = false, generic_ = false;
  const float *stem_w_ = nullptr, *stem_b_ = nullptr, *stem_g_ = nullptr, *stem_beta_ = nullptr;
  Stage stages_[kStages];
  const float* mix_out_ = nullptr;   // softmax(inputs_weights[6]) (7, 1152)
  // workspace: the seven 1-D outputs, the mixed input / final map, two rotating 2-D maps and the generic arm's h
  void* outs_[kStages + 1] = {};
  void *mix_ = nullptr, *a_ = nullptr, *b_ = nullptr, *tmp_ = nullptr;
  float *x0_ = nullptr, *x1_ = nullptr;                  // (B T, 288) fp32 residual stream, two copies
  void *z_ = nullptr, *qkv_ = nullptr, *ao_ = nullptr;   // (B T, 288), (B T, 3 * 384), (B T, 384) in the map type
};

struct RedimNetConfig {
  int feat_dim = 72;
  int embed_dim = 192;
  int max_batch = 96;        // the extractor's batch size
  int max_frames = 598;      // 6 s chunks: 1 + (96000 - 400) / 160
  bool bf16 = false;         // bf16 maps and conv operands; LayerNorms, softmax, ASTP and seg_1 stay fp32
};

class RedimNetModel : public ModelCore {
 public:
  explicit RedimNetModel(const RedimNetConfig& c) : cfg_(c) {}
  // fbank (B, T, 72) -> emb (B, E) (nullable) = seg_1(ASTP(trunk)) (ReDimNet.forward, :861-872) and / or frames
  // (B, T, 1152) channel-last fp32 (nullable) = get_frame_level_feat (:855-859).  emb with T < 2 raises kErrShape.
  void forward(const float* fbank, int B, int T, float* emb, float* frames, hipStream_t st);
  void set_generic(bool on) { trunk_.set_generic(on); }

 private:
  void build() override;
  RedimNetConfig cfg_;
  RedimTrunk trunk_;
  PackedW w1x_, w2_;                                   // pool.linear1.weight[:, :1152], pool.linear2.weight (fp32)
  const float *w1c_ = nullptr, *b1_ = nullptr, *b2_ = nullptr;
  ConvL seg1_;
  float *stats_ = nullptr, *ctx_ = nullptr, *cv_ = nullptr, *x32_ = nullptr, *h_ = nullptr, *e_ = nullptr;
};

}  // namespace sd
