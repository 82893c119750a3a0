// ResNet34 embedding extractor on gfx950 (see resemb.h).
#include "resemb.h"

namespace sd {

void ResEmbModel::build() {
  SD_CHECK(cfg_.feat_dim == 80, kErrInvalid, "ResNet34 (MI355X backend) supports feat_dim 80 only");
  const int E = cfg_.embed_dim, C2 = 2 * ResTrunk::kChannels;
  trunk_.load(ps_, arena_, "", cfg_.bf16);   // resnet_wespeaker.py:127-134
  // seg_1 (:140): the pooled head is tiny (B x 5120 x E) and stays fp32 in both modes (seg_linear, tstp_pool.hip)
  LayerLoader fp32{ps_, arena_, false};
  seg1_ = fp32.linear("seg_1");
  SD_CHECK(seg1_.w.N == E && seg1_.w.K == C2, kErrParam, "seg_1.weight must be (embed_dim, 5120)");
  SD_CHECK(ps_.get("seg_1.bias").numel() == E, kErrParam, "seg_1.bias size");
  if (cfg_.two_emb_layer) {
    // seg_bn_1 is BatchNorm1d(affine=False) (:142): a weight / bias key is unexpected, not a gamma / beta
    for (const char* k : {"seg_bn_1.weight", "seg_bn_1.bias"})
      ps_.require_absent(k);
    // embed_b = W2 (s relu(a) + h) + b2 = (W2 diag(s)) relu(a) + (W2 h + b2)   (:178-180)
    std::vector<float> s, h;
    ps_.bn_fold("seg_bn_1", s, h);
    const HostTensor& w2 = ps_.get("seg_2.weight");
    const HostTensor& b2 = ps_.get("seg_2.bias");
    SD_CHECK(w2.shape.size() == 2 && w2.shape[0] == E && w2.shape[1] == E && (int)s.size() == E, kErrParam,
             "seg_2.weight must be (embed_dim, embed_dim)");
    SD_CHECK(b2.numel() == E, kErrParam, "seg_2.bias size");
    std::vector<float> w(w2.data.size()), b(E);
    for (int n = 0; n < E; ++n) {
      double acc = b2.data[n];
      for (int k = 0; k < E; ++k) {
        w[(size_t)n * E + k] = w2.data[(size_t)n * E + k] * s[k];
        acc += (double)w2.data[(size_t)n * E + k] * h[k];
      }
      b[n] = (float)acc;
    }
    seg2_.w = upload_packed(arena_, w, E, E, 1, 1, false);
    seg2_.beta = arena_.upload(b);
  }
  ps_.require_all_used();   // pool.* (TSTP has no parameters), seg_2.* without two_emb_layer, ...
  trunk_.alloc(arena_, cfg_.max_batch, cfg_.max_frames);
  stats_ = static_cast<float*>(arena_.alloc((size_t)cfg_.max_batch * C2 * sizeof(float)));
  ea_ = static_cast<float*>(arena_.alloc((size_t)cfg_.max_batch * E * sizeof(float)));
  relu_ = static_cast<float*>(arena_.alloc((size_t)cfg_.max_batch * E * sizeof(float)));
}

void ResEmbModel::forward(const float* fbank, int B, int Tf, float* emb, float* emb_a, float* time_out,
                          hipStream_t st) {
  require_finalized();
  SD_CHECK(B >= 1 && B <= cfg_.max_batch, kErrInvalid, "batch exceeds max_batch");
  SD_CHECK(Tf >= 1 && Tf <= cfg_.max_frames, kErrInvalid, "fbank frames exceed max_frames");
  const int E = cfg_.embed_dim, C = ResTrunk::kChannels;
  if (Tf < 8) {
    // T' == 1: every std is NaN (0 / 0), and seg_1 sums all 5120 statistics into every output
    SD_CHECK(!time_out, kErrInvalid, "get_time_out needs at least 8 fbank frames");
    if (emb) fill_u32(emb, (size_t)B * E * sizeof(float), 0x7fc00000u, st);
    if (emb_a) fill_u32(emb_a, (size_t)B * E * sizeof(float), 0x7fc00000u, st);
    return;
  }
  const Tens x4 = trunk_.forward(fbank, B, Tf, st);
  const int T4 = ResTrunk::out_frames(Tf);
  const bool want = emb || emb_a;
  tstp_pool(x4.p, x4.bf, B, T4, C, want ? stats_ : nullptr, time_out, st);   // pool (:174)
  if (!want) return;
  float* const a = !cfg_.two_emb_layer ? (emb ? emb : emb_a) : (emb_a ? emb_a : ea_);
  seg_linear(stats_, B, 2 * C, static_cast<const float*>(seg1_.w.w), seg1_.beta, E, a, st);   // seg_1 (:176)
  if (!cfg_.two_emb_layer || !emb) return;   // one layer: emb IS embed_a (emb_a is written only when emb is null)
  relu_keep_nan(a, (int64_t)B * E, relu_, st);   // F.relu (:178)
  seg_linear(relu_, B, E, static_cast<const float*>(seg2_.w.w), seg2_.beta, E, emb, st);   // :179-180
}

}  // namespace sd
