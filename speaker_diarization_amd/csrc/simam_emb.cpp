// SimAM-ResNet34 embedding extractor on gfx950 (see simam_emb.h).
#include "simam_emb.h"

#include <algorithm>

namespace sd {

namespace {
int g_variant = 0;
}
void simam_debug_variant(int v) { g_variant = v; }

void SimamEmbModel::build() {
  SD_CHECK(cfg_.in_planes == 64 && cfg_.acoustic_dim == 80, kErrInvalid,
           "SimAM_ResNet34_ASP (MI355X backend) supports in_planes 64 and acoustic_dim 80 only");
  constexpr int H = 128;
  const int E = cfg_.embed_dim;
  ResTrunkSpec spec;
  spec.base = cfg_.in_planes;
  spec.sc_key = "downsample";
  spec.simam = g_variant != 1;
  trunk_.load(ps_, arena_, "front.", cfg_.bf16, spec);   // samresnet_wespeaker.py:137
  const int C = trunk_.channels();
  auto vec = [&](const std::string& key, int n) {
    const HostTensor& t = ps_.get(key);
    SD_CHECK(t.numel() == n, kErrParam, key + " size");
    return arena_.upload(t.data);
  };
  // pooling.attention (pooling_layers_wespeaker.py:153-159): Conv1d(C, 128, 1), ReLU, BatchNorm1d(128), Conv1d(128, C, 1)
  {
    int N, Cin, kh, kw;
    auto w1 = ps_.pack("pooling.attention.0.weight", N, Cin, kh, kw);
    SD_CHECK(N == H && Cin == C && kh == 1 && kw == 1, kErrParam, "pooling.attention.0.weight must be (128, 5120, 1)");
    w1_ = upload_packed(arena_, w1, N, Cin, 1, 1, false);
    b1_ = vec("pooling.attention.0.bias", H);
    std::vector<float> s, h;
    ps_.bn_fold("pooling.attention.2", s, h);
    SD_CHECK((int)s.size() == H, kErrParam, "pooling.attention.2 size");
    bn_s_ = arena_.upload(s);
    bn_h_ = arena_.upload(h);
    auto w2 = ps_.pack("pooling.attention.3.weight", N, Cin, kh, kw);
    SD_CHECK(N == C && Cin == H && kh == 1 && kw == 1, kErrParam, "pooling.attention.3.weight must be (5120, 128, 1)");
    w2_ = upload_packed(arena_, w2, N, Cin, 1, 1, false);
    b2_ = vec("pooling.attention.3.bias", C);
  }
  LayerLoader fp32{ps_, arena_, false};
  bottleneck_ = fp32.linear("bottleneck");   // samresnet_wespeaker.py:140
  SD_CHECK(bottleneck_.w.N == E && bottleneck_.w.K == 2 * C, kErrParam, "bottleneck.weight must be (embed_dim, 10240)");
  SD_CHECK(ps_.get("bottleneck.bias").numel() == E, kErrParam, "bottleneck.bias size");
  ps_.require_all_used();
  trunk_.alloc(arena_, cfg_.max_batch, cfg_.max_frames);
  const size_t Bm = cfg_.max_batch, rows = Bm * ResTrunk::out_frames(cfg_.max_frames);
  const size_t gemm_rows = std::max<size_t>(rows, kAspMinRows);
  stats_ = ws(Bm * 2 * C);
  h_ = ws(gemm_rows * H);
  e_ = ws(gemm_rows * C);
  if (cfg_.bf16) x32_ = ws(rows * C);
}

void SimamEmbModel::forward(const float* fbank, int B, int Tf, float* emb, float* front_out, hipStream_t st) {
  require_finalized();
  SD_CHECK(B >= 1 && B <= cfg_.max_batch, kErrInvalid, "batch exceeds max_batch");
  SD_CHECK(Tf >= 1 && Tf <= cfg_.max_frames, kErrInvalid, "fbank frames exceed max_frames");
  SD_CHECK(Tf >= kMinFrames, kErrShape, "SimAM_ResNet34_ASP needs at least 8 fbank frames");
  const int C = trunk_.channels(), T4 = ResTrunk::out_frames(Tf);
  const Tens x = trunk_.forward(fbank, B, Tf, st);   // front (:144-145)
  const int64_t n = (int64_t)B * T4 * C;
  if (front_out) {
    if (x.bf) bf16_to_f32(x.p, n, front_out, st);
    else SD_HIP(hipMemcpyAsync(front_out, x.p, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (!emb) return;
  AspArgs a;
  a.x = x.p; a.x_bf16 = x.bf; a.B = B; a.T = T4; a.C = C;
  a.w1 = w1_.w; a.b1 = b1_; a.bn_s = bn_s_; a.bn_h = bn_h_; a.w2 = w2_.w; a.b2 = b2_;
  a.stats = stats_; a.x32 = x32_; a.h = h_; a.e = e_;
  asp_pool(a, st);   // pooling (:156)
  // bottleneck (:159); dropout 0 builds no Dropout (:141)
  seg_linear(stats_, B, 2 * C, static_cast<const float*>(bottleneck_.w.w), bottleneck_.beta, cfg_.embed_dim, emb, st);
}

}  // namespace sd
