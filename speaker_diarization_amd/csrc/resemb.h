// WeSpeaker ResNet34 target-speaker embedding extractor (egs/alimeeting/ts_vad2/resnet_wespeaker.py:108-183 with
// speech_encoder=False) on gfx950: ResNet34(feat_dim 80, embed_dim, pooling_func "TSTP", two_emb_layer), the model
// generate_chunk_speaker_embedding_from_wespeaker_for_diarization.py:116-133 runs on 6 s chunks to write the
// (n_chunks, 256) embeddings ts_vad_dataset.py:494-537 reads back.
//
// ResTrunk (resnet.h, prefix "") -> TSTP over time (tstp_pool.hip) -> seg_1 Linear(5120 -> E) = embed_a
// [-> ReLU -> seg_bn_1 (BatchNorm1d affine=False, folded into seg_2's input side) -> seg_2 = embed_b].
// The pooled head is fp32 in both precisions, like CAM++'s (campp.h).
#pragma once
#include "resnet.h"

namespace sd {

struct ResEmbConfig {
  int feat_dim = 80;
  int embed_dim = 256;
  bool two_emb_layer = false;
  int max_batch = 96;        // extract_embed batch_size default (generate_chunk_...wespeaker...py:61)
  int max_frames = 598;      // 6 s chunks: 1 + (96000 - 400) / 160
  bool bf16 = false;         // bf16 trunk (maps and conv operands); TSTP and the seg layers stay fp32
};

class ResEmbModel : public ModelCore {
 public:
  explicit ResEmbModel(const ResEmbConfig& c) : cfg_(c) {}
  // fbank (B, Tf, 80) -> emb (B, E): the last element of the reference's returned tuple (embed_b with
  // two_emb_layer, else embed_a; :176-183); emb_a (B, E, nullable): seg_1's output; time_out (B, T', 2560)
  // channel-last (nullable): forward(x, get_time_out=True) (:165-171).  T' == 1 (Tf <= 8) gives all-NaN embeddings
  // like the reference (the unbiased variance of one frame); for Tf < 8 they are written without running the
  // trunk, whose stage-1 kernels are exercised from 8 frames on, and time_out is refused.
  void forward(const float* fbank, int B, int Tf, float* emb, float* emb_a, float* time_out, hipStream_t st);

 private:
  void build() override;
  ResEmbConfig cfg_;
  ResTrunk trunk_;
  ConvL seg1_, seg2_;        // seg_2: W2 diag(s) and W2 h + b2 with seg_bn_1 = (s, h)
  float* stats_ = nullptr;   // (max_batch, 5120) [mean | std]
  float* ea_ = nullptr;      // (max_batch, E) embed_a when the caller does not take it
  float* relu_ = nullptr;    // (max_batch, E) relu(embed_a)
};

}  // namespace sd
