// WeSpeaker SimAM-ResNet34 target-speaker embedding extractor (egs/alimeeting/ts_vad2/samresnet_wespeaker.py:134-160
// with speech_encoder=False) on gfx950: SimAM_ResNet34_ASP(in_planes 64, embed_dim, acoustic_dim 80), the model
// generate_chunk_speaker_embedding_from_wespeaker_for_diarization.py:119-120 runs on 6 s chunks.
//
// ResTrunk (resnet.h; prefix "front.", base 64, `downsample` keys, SimAM blocks) -> ASP over time
// (pooling_layers_wespeaker.py:146-168; asp_pool, kernels.h) -> bottleneck Linear(10240 -> E).  The pooled head is fp32
// in both precisions, like ResNet34's and ECAPA's.  The encoder-only form (forward(x, get_time_out=True), :146-153)
// reads an undefined name in the reference and raises NameError there: it is not built.
#pragma once
#include "resnet.h"

namespace sd {

struct SimamEmbConfig {
  int in_planes = 64;
  int embed_dim = 256;
  int acoustic_dim = 80;
  int max_batch = 96;        // extract_embed batch_size default (generate_chunk_...wespeaker...py:61)
  int max_frames = 598;      // 6 s chunks: 1 + (96000 - 400) / 160
  bool bf16 = false;         // bf16 trunk (maps and conv operands); ASP and the bottleneck stay fp32
};

// Measurement only (tools/simam_probe.py, sd_debug_simam_variant): what models finalized from now on build.  0: the
// shipped model; 1: the same trunk with plain BasicBlocks (not SimAM-ResNet34: prices the SimAM kernels).
void simam_debug_variant(int v);

class SimamEmbModel : public ModelCore {
 public:
  static constexpr int kMinFrames = 8;
  explicit SimamEmbModel(const SimamEmbConfig& c) : cfg_(c) {}
  // fbank (B, Tf, 80) -> emb (B, E) (:156-160; nullable) and / or front_out (B, T', 5120) channel-last fp32 (nullable):
  // the stage-4 map as ASP.forward's x.reshape(B, -1, T) orders it, channel c * 10 + f.  T' == 1 (Tf == 8) is valid
  // here: softmax weight 1 and sg = sqrt(1e-5).  Tf < 8 raises kErrShape: the trunk's kernels are exercised from 8
  // frames on.
  void forward(const float* fbank, int B, int Tf, float* emb, float* front_out, hipStream_t st);

 private:
  void build() override;
  SimamEmbConfig cfg_;
  ResTrunk trunk_;
  PackedW w1_, w2_;                                     // attention.0 (128, 5120), attention.3 (5120, 128)
  const float *b1_ = nullptr, *b2_ = nullptr;
  const float *bn_s_ = nullptr, *bn_h_ = nullptr;       // attention.2 folded
  ConvL bottleneck_;
  float *stats_ = nullptr, *x32_ = nullptr, *h_ = nullptr, *e_ = nullptr;
};

}  // namespace sd
