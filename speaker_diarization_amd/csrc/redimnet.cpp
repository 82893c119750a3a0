// ReDimNetB2 trunk and embedding extractor on gfx950 (see redimnet.h).
#include "redimnet.h"

#include <algorithm>
#include <cmath>

namespace sd {

namespace {

// stages_setup of ReDimNetB2 (redimnet_wespeaker.py:934-941): (stride, blocks, 1-D reduction)
const int kSetup[RedimTrunk::kStages][3] = {{1, 2, 12}, {2, 2, 12}, {1, 3, 12}, {2, 4, 8}, {1, 4, 8}, {2, 4, 4}};
const int kKernels[4] = {7, 19, 31, 59};   // TimeContextBlock1d "conv+att" (:586-607)
constexpr float kLnEps = 1e-6f;

const HostTensor& shaped(ParamStore& ps, const std::string& key, std::initializer_list<int64_t> shape) {
  const HostTensor& t = ps.get(key);
  bool ok = t.shape.size() == shape.size();
  size_t i = 0;
  for (int64_t d : shape) ok = ok && t.shape[i++] == d;
  SD_CHECK(ok, kErrParam, key + " shape");
  return t;
}

// softmax over the first axis of inputs_weights[i] (1, n, 1152, 1), in fp32 as the reference computes it
const float* load_mix(ParamStore& ps, DeviceArena& arena, const std::string& key, int n) {
  const HostTensor& t = shaped(ps, key, {1, n, kRedimCF, 1});
  std::vector<float> w((size_t)n * kRedimCF);
  for (int ch = 0; ch < kRedimCF; ++ch) {
    float mx = t.data[ch];
    for (int k = 1; k < n; ++k) mx = std::max(mx, t.data[(size_t)k * kRedimCF + ch]);
    float sum = 0.f;
    for (int k = 0; k < n; ++k) sum += (w[(size_t)k * kRedimCF + ch] = std::exp(t.data[(size_t)k * kRedimCF + ch] - mx));
    for (int k = 0; k < n; ++k) w[(size_t)k * kRedimCF + ch] /= sum;
  }
  return arena.upload(w);
}

ConvL linear_checked(LayerLoader& ld, const std::string& prefix, int N, int K) {
  ConvL L = ld.linear(prefix);
  SD_CHECK(L.w.N == N && L.w.K == K && L.w.kh * L.w.kw == 1, kErrParam, prefix + ".weight shape");
  SD_CHECK(ld.ps.get(prefix + ".bias").numel() == N, kErrParam, prefix + ".bias size");
  return L;
}

}  // namespace

void RedimTrunk::load(ParamStore& ps, DeviceArena& arena, const std::string& pre, bool bf16) {
  bf16_ = bf16;
  const std::string bb = pre + "backbone.";
  LayerLoader ld{ps, arena, bf16};
  shaped(ps, bb + "inputs_weights.0", {1, 1, 1, 1});   // one input: its softmax is 1
  stem_w_ = arena.upload(shaped(ps, bb + "stem.0.weight", {kC, 1, 3, 3}).data);
  stem_b_ = arena.upload(shaped(ps, bb + "stem.0.bias", {kC}).data);
  stem_g_ = arena.upload(shaped(ps, bb + "stem.1.weight", {kC}).data);
  stem_beta_ = arena.upload(shaped(ps, bb + "stem.1.bias", {kC}).data);
  int c = kC, f = kF;
  for (int i = 0; i < kStages; ++i) {
    Stage& s = stages_[i];
    const std::string sp = bb + "stage" + std::to_string(i) + ".";
    const int stride = kSetup[i][0], nb = kSetup[i][1], cin = c;
    s.stride = stride;
    c *= stride;
    f /= stride;
    s.c = c;
    s.f = f;
    s.hC = kRedimCF / kSetup[i][2];
    const int hd = s.hC / kHeads;
    s.hdp = hd <= 32 ? 32 : hd <= 48 ? 48 : hd <= 64 ? 64 : 96;   // head widths attention() has: 24 / 36 / 72 -> 32 / 48 / 96
    SD_CHECK(hd <= 96, kErrParam, "ReDimNetB2 head width");
    s.scale = 1.f / std::sqrt((float)hd);
    if (i > 0) s.mix = load_mix(ps, arena, bb + "inputs_weights." + std::to_string(i), i + 1);
    // Conv2d(cin -> c, (stride, 1), stride (stride, 1)) (:690-697): tap-major packing = a linear on stride * cin values
    shaped(ps, sp + "0.weight", {c, cin, stride, 1});
    s.entry = ld.linear(sp + "0");
    SD_CHECK(s.entry.w.N == c && s.entry.w.K == stride * cin, kErrParam, sp + "0.weight shape");
    SD_CHECK(ps.get(sp + "0.bias").numel() == c, kErrParam, sp + "0.bias size");
    s.entry.w.Cin = s.entry.w.K;
    s.entry.w.kh = s.entry.w.kw = 1;
    for (int b = 0; b < nb; ++b) {
      const std::string q = sp + std::to_string(b + 1) + ".conv_block.";
      const HostTensor& w = shaped(ps, q + "dwconvs.0.weight", {c, 4, 3, 3});
      const HostTensor& wb = shaped(ps, q + "dwconvs.0.bias", {c});
      std::vector<float> sc, sh, dw, dwb;
      ps.bn_fold(q + "norm", sc, sh);
      SD_CHECK((int)sc.size() == c, kErrParam, q + "norm size");
      redim_pack_dw(w.data.data(), wb.data.data(), sc.data(), sh.data(), c, dw, dwb);
      RedimBlock2dW W;
      W.dw = arena.upload(dw);
      W.dw_b = arena.upload(dwb);
      shaped(ps, q + "pwconv1.weight", {c, c, 1, 1});
      const ConvL pwl = linear_checked(ld, q + "pwconv1", c, c);
      W.pw = pwl.w.w;
      W.pw_b = pwl.beta;
      s.blocks.push_back(W);
    }
    // TimeContextBlock1d (:541-620) sits after to1d, which has no parameters
    const std::string t = sp + std::to_string(nb + 2) + ".";
    const int hC = s.hC;
    shaped(ps, t + "red_dim_conv.0.weight", {hC, kRedimCF, 1});
    s.red = linear_checked(ld, t + "red_dim_conv.0", hC, kRedimCF);
    s.red_g = arena.upload(shaped(ps, t + "red_dim_conv.1.weight", {hC}).data);
    s.red_b = arena.upload(shaped(ps, t + "red_dim_conv.1.bias", {hC}).data);
    for (int j = 0; j < 4; ++j) {
      const std::string q = t + "tcm." + std::to_string(j) + ".";
      const int k = kKernels[j];
      const HostTensor& w = shaped(ps, q + "dwconvs.0.weight", {hC, 1, k});
      const HostTensor& wb = shaped(ps, q + "dwconvs.0.bias", {hC});
      std::vector<float> sc, sh;
      ps.bn_fold(q + "norm", sc, sh);
      SD_CHECK((int)sc.size() == hC, kErrParam, q + "norm size");
      std::vector<float> wt((size_t)k * hC), b(hC);
      for (int ch = 0; ch < hC; ++ch) {
        for (int jj = 0; jj < k; ++jj) wt[(size_t)jj * hC + ch] = (float)((double)w.data[(size_t)ch * k + jj] * sc[ch]);
        b[ch] = (float)((double)wb.data[ch] * sc[ch] + sh[ch]);
      }
      s.conv[j].k = k;
      s.conv[j].dw = arena.upload(wt);
      s.conv[j].dw_b = arena.upload(b);
      shaped(ps, q + "pwconv1.weight", {hC, hC, 1});
      s.conv[j].pw = linear_checked(ld, q + "pwconv1", hC, hC);
    }
    // TransformerEncoderLayer (:277-329): heads of hd padded to hdp with zero rows (q / k / v) and zero columns (out)
    const std::string a = t + "tcm.4.";
    const int Dp = kHeads * s.hdp;
    {
      std::vector<float> w((size_t)3 * Dp * hC, 0.f), b((size_t)3 * Dp, 0.f);
      const char* names[3] = {"q_proj", "k_proj", "v_proj"};
      for (int which = 0; which < 3; ++which) {
        const HostTensor& pw = shaped(ps, a + "attention." + names[which] + ".weight", {hC, hC});
        const HostTensor& pb = shaped(ps, a + "attention." + names[which] + ".bias", {hC});
        for (int h = 0; h < kHeads; ++h)
          for (int j = 0; j < hd; ++j) {
            const size_t dst = (size_t)which * Dp + h * s.hdp + j, src = (size_t)h * hd + j;
            std::copy(pw.data.begin() + src * hC, pw.data.begin() + (src + 1) * hC, w.begin() + dst * hC);
            b[dst] = pb.data[src];
          }
      }
      s.qkv.w = upload_packed(arena, w, 3 * Dp, hC, 1, 1, bf16);
      s.qkv.beta = arena.upload(b);
      const HostTensor& ow = shaped(ps, a + "attention.out_proj.weight", {hC, hC});
      std::vector<float> o((size_t)hC * Dp, 0.f);
      for (int n = 0; n < hC; ++n)
        for (int h = 0; h < kHeads; ++h)
          for (int j = 0; j < hd; ++j) o[(size_t)n * Dp + h * s.hdp + j] = ow.data[(size_t)n * hC + h * hd + j];
      s.proj.w = upload_packed(arena, o, hC, Dp, 1, 1, bf16);
      s.proj.beta = arena.upload(shaped(ps, a + "attention.out_proj.bias", {hC}).data);
    }
    s.ln1_g = arena.upload(shaped(ps, a + "layer_norm.weight", {hC}).data);
    s.ln1_b = arena.upload(shaped(ps, a + "layer_norm.bias", {hC}).data);
    s.ff1 = linear_checked(ld, a + "feed_forward.intermediate_dense", hC, hC);
    s.ff2 = linear_checked(ld, a + "feed_forward.output_dense", hC, hC);
    s.ln2_g = arena.upload(shaped(ps, a + "final_layer_norm.weight", {hC}).data);
    s.ln2_b = arena.upload(shaped(ps, a + "final_layer_norm.bias", {hC}).data);
    shaped(ps, t + "exp_dim_conv.weight", {kRedimCF, hC, 1});
    s.exp = linear_checked(ld, t + "exp_dim_conv", kRedimCF, hC);
  }
  SD_CHECK(c == 128 && f == 9, kErrParam, "ReDimNetB2 stage table");
  mix_out_ = load_mix(ps, arena, bb + "inputs_weights." + std::to_string(kStages), kStages + 1);
}

void RedimTrunk::alloc(DeviceArena& a, int max_batch, int max_frames) {
  const size_t rows = (size_t)max_batch * max_frames, esz = bf16_ ? 2 : 4;
  auto map = [&](size_t ch) { return a.alloc(rows * ch * esz); };
  for (void*& o : outs_) o = map(kRedimCF);
  mix_ = map(kRedimCF);
  a_ = map(kRedimCF);
  b_ = map(kRedimCF);
  tmp_ = map(kRedimCF);
  x0_ = static_cast<float*>(a.alloc(rows * 288 * sizeof(float)));
  x1_ = static_cast<float*>(a.alloc(rows * 288 * sizeof(float)));
  z_ = map(288);
  qkv_ = map(3 * 384);
  ao_ = map(384);
}

void RedimTrunk::run_block1d(const Stage& s, const void* map2d, int B, int T, void* out, hipStream_t st) const {
  const bool bf = bf16_;
  const int rows = B * T, hC = s.hC, Dp = kHeads * s.hdp;
  const Tens m{const_cast<void*>(map2d), bf}, z{z_, bf}, qkv{qkv_, bf}, ao{ao_, bf};
  float *X = x0_, *Y = x1_;
  // red_dim_conv: 1x1 conv 1152 -> hC, then LayerNorm over the hC channels of each frame (:554-556)
  conv_gemm(lin(m, rows, kRedimCF, s.red.w, s.red.beta, Tens{Y, false}, hC), bf, st);
  layernorm(Y, rows, hC, hC, s.red_g, s.red_b, kLnEps, X, hC, false, st);
  for (int j = 0; j < 4; ++j) {   // x + pwconv1(gelu(bn(dwconv(x))))
    redim_dwconv1d(X, B, T, hC, s.conv[j].k, s.conv[j].dw, s.conv[j].dw_b, z.p, bf, st);
    ConvGemmArgs p = lin(z, rows, hC, s.conv[j].pw.w, s.conv[j].pw.beta, Tens{Y, false}, hC);
    p.res = X; p.res_bf16 = false; p.res_ld = hC;
    conv_gemm(p, bf, st);
    std::swap(X, Y);
  }
  // post-LN transformer layer: X = LN(X + MHA(X)); X = LN(X + FFN(X))
  const Tens x{X, false};
  conv_gemm(lin(x, rows, hC, s.qkv.w, s.qkv.beta, qkv, 3 * Dp), bf, st);
  AttnArgs a;
  a.qkv = qkv.p; a.io_bf16 = bf; a.S = B; a.T = T; a.D = Dp; a.nh = kHeads; a.ld_qkv = 3 * Dp;
  a.out = ao.p; a.ldo = Dp; a.scale = s.scale;
  attention(a, bf, st);
  conv_gemm(lin(ao, rows, Dp, s.proj.w, s.proj.beta, z, hC), bf, st);
  add_layernorm(X, z.p, bf, rows, hC, s.ln1_g, s.ln1_b, kLnEps, false, X, false, st);
  // the FFN's hidden rows (B T, hC) go to the q | k | v buffer, which is dead after the attention
  ConvGemmArgs f1 = lin(x, rows, hC, s.ff1.w, s.ff1.beta, qkv, hC);
  f1.act = kActGeluTanh;
  conv_gemm(f1, bf, st);
  conv_gemm(lin(qkv, rows, hC, s.ff2.w, s.ff2.beta, z, hC), bf, st);
  add_layernorm(X, z.p, bf, rows, hC, s.ln2_g, s.ln2_b, kLnEps, false, X, false, st);
  // exp_dim_conv + the block's skip (:619-620)
  ConvGemmArgs e = lin(x, rows, hC, s.exp.w, s.exp.beta, Tens{out, bf}, kRedimCF);
  e.res = map2d; e.res_bf16 = bf; e.res_ld = kRedimCF;
  conv_gemm(e, bf, st);
}

Tens RedimTrunk::forward(const float* fbank, int B, int T, hipStream_t st) const {
  const bool bf = bf16_;
  const int64_t rows = (int64_t)B * T;
  redim_stem(fbank, B, T, stem_w_, stem_b_, stem_g_, stem_beta_, outs_[0], bf, st);
  auto mix = [&](const float* w, int n) {
    RedimMixArgs a;
    for (int k = 0; k < n; ++k) a.x[k] = outs_[k];
    a.n = n;
    a.w = w;
    redim_stage_mix(a, rows, mix_, bf, st);
  };
  for (int i = 0; i < kStages; ++i) {
    const Stage& s = stages_[i];
    void* in = outs_[0];
    if (i > 0) {
      mix(s.mix, i + 1);
      in = mix_;
    }
    void *cur = a_, *nxt = b_;
    conv_gemm(lin(Tens{in, bf}, (int)(rows * s.f), s.c, s.entry.w, s.entry.beta, Tens{cur, bf}, s.c), bf, st);
    for (const RedimBlock2dW& W : s.blocks) {
      redim_block2d(cur, B, T, s.c, W, tmp_, nxt, bf, !bf || generic_, st);
      std::swap(cur, nxt);
    }
    run_block1d(s, cur, B, T, outs_[i + 1], st);
  }
  mix(mix_out_, kStages + 1);
  return Tens{mix_, bf};
}

void RedimNetModel::build() {
  SD_CHECK(cfg_.feat_dim == RedimTrunk::kF, kErrInvalid, "ReDimNetB2 (MI355X backend) supports feat_dim 72 only");
  const int E = cfg_.embed_dim, C = RedimTrunk::kChannels, H = 128;
  trunk_.load(ps_, arena_, "", cfg_.bf16);
  // pool (pooling_layers_wespeaker.py:100-114): linear1 (128, 3 C, 1) split into its per-frame and context halves
  {
    const HostTensor& w = ps_.get("pool.linear1.weight");
    SD_CHECK(w.numel() == (int64_t)H * 3 * C && w.shape.size() >= 2 && w.shape[0] == H && w.shape[1] == 3 * C, kErrParam,
             "pool.linear1.weight must be (128, 3456, 1)");
    std::vector<float> wx((size_t)H * C), wc((size_t)H * 2 * C);
    for (int n = 0; n < H; ++n) {
      const float* r = w.data.data() + (size_t)n * 3 * C;
      std::copy(r, r + C, wx.begin() + (size_t)n * C);
      std::copy(r + C, r + 3 * C, wc.begin() + (size_t)n * 2 * C);
    }
    w1x_ = upload_packed(arena_, wx, H, C, 1, 1, false);
    w1c_ = arena_.upload(wc);
    const HostTensor& b1 = ps_.get("pool.linear1.bias");
    SD_CHECK(b1.numel() == H, kErrParam, "pool.linear1.bias size");
    b1_ = arena_.upload(b1.data);
    int N, Cin, kh, kw;
    auto w2 = ps_.pack("pool.linear2.weight", N, Cin, kh, kw);
    SD_CHECK(N == C && Cin == H && kh == 1 && kw == 1, kErrParam, "pool.linear2.weight must be (1152, 128, 1)");
    w2_ = upload_packed(arena_, w2, N, Cin, 1, 1, false);
    const HostTensor& b2 = ps_.get("pool.linear2.bias");
    SD_CHECK(b2.numel() == C, kErrParam, "pool.linear2.bias size");
    b2_ = arena_.upload(b2.data);
  }
  LayerLoader fp32{ps_, arena_, false};
  seg1_ = fp32.linear("seg_1");   // :839
  SD_CHECK(seg1_.w.N == E && seg1_.w.K == 2 * C, kErrParam, "seg_1.weight must be (embed_dim, 2304)");
  SD_CHECK(ps_.get("seg_1.bias").numel() == E, kErrParam, "seg_1.bias size");
  ps_.require_all_used();
  trunk_.alloc(arena_, cfg_.max_batch, cfg_.max_frames);
  const size_t Bm = cfg_.max_batch, rows = Bm * cfg_.max_frames;
  stats_ = ws(Bm * 2 * C);
  ctx_ = ws(Bm * 2 * C);
  cv_ = ws(Bm * H);
  h_ = ws(rows * H);
  e_ = ws(rows * C);
  if (cfg_.bf16) x32_ = ws(rows * C);
}

void RedimNetModel::forward(const float* fbank, int B, int T, float* emb, float* frames, hipStream_t st) {
  require_finalized();
  SD_CHECK(B >= 1 && B <= cfg_.max_batch, kErrInvalid, "batch exceeds max_batch");
  SD_CHECK(T >= 1 && T <= cfg_.max_frames, kErrInvalid, "fbank frames exceed max_frames");
  SD_CHECK(!emb || T >= 2, kErrShape,
           "ReDimNetB2 embeddings need at least 2 fbank frames (ASTP's unbiased variance of one frame is NaN)");
  const int C = RedimTrunk::kChannels;
  const Tens x = trunk_.forward(fbank, B, T, st);
  const int64_t n = (int64_t)B * T * C;
  if (frames) {
    if (x.bf) bf16_to_f32(x.p, n, frames, st);
    else SD_HIP(hipMemcpyAsync(frames, x.p, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (!emb) return;
  AstpArgs a;
  a.C = C;
  a.x = x.p; a.x_bf16 = x.bf; a.B = B; a.T = T;
  a.w1x = w1x_.w; a.w1c = w1c_; a.b1 = b1_; a.w2 = w2_.w; a.b2 = b2_;
  a.stats = stats_; a.ctx = ctx_; a.cv = cv_; a.x32 = x32_; a.h = h_; a.e = e_;
  astp_pool(a, st);   // pool (:864)
  seg_linear(stats_, B, 2 * C, static_cast<const float*>(seg1_.w.w), seg1_.beta, cfg_.embed_dim, emb, st);   // :865
}

}  // namespace sd
