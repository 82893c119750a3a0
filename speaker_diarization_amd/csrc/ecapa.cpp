// ECAPA-TDNN trunk and embedding extractor on gfx950 (see ecapa.h).
#include "ecapa.h"

namespace sd {

namespace {

constexpr int kF = 80, kTaps1 = 5;

// `p`{conv.weight (cout, cin, taps), conv.bias, bn.*}
EcapaConv load_conv_relu_bn(ParamStore& ps, DeviceArena& arena, bool bf16, const std::string& p, int cout, int cin,
                            int taps) {
  EcapaConv L;
  int N, Cin, kh, kw;
  auto w = ps.pack(p + "conv.weight", N, Cin, kh, kw);
  SD_CHECK(N == cout && Cin == cin && kh == 1 && kw == taps, kErrParam, p + "conv.weight shape");
  SD_CHECK(ps.get(p + "conv.bias").numel() == cout, kErrParam, p + "conv.bias size");
  L.w = upload_packed(arena, w, N, Cin, kh, kw, bf16);
  L.bias = arena.upload(ps.get(p + "conv.bias").data);
  std::vector<float> s, h;
  ps.bn_fold(p + "bn", s, h);
  SD_CHECK((int)s.size() == cout, kErrParam, p + "bn size");
  L.s = arena.upload(s);
  L.h = arena.upload(h);
  return L;
}

const float* load_fp32(ParamStore& ps, DeviceArena& arena, const std::string& key, int64_t d0, int64_t d1) {
  const HostTensor& t = ps.get(key);
  const bool ok = d1 ? (t.shape.size() == 2 && t.shape[0] == d0 && t.shape[1] == d1) : t.numel() == d0;
  SD_CHECK(ok, kErrParam, key + " shape");
  return arena.upload(t.data);
}

ConvGemmArgs pointwise(const void* A, int lda, int a_coff, int64_t M, const EcapaConv& L, void* out, int ldo, bool bf) {
  ConvGemmArgs p = linear_args(A, (int)M, L.w.K, lda, L.w.w, L.w.N, out, ldo);
  p.a_coff = a_coff;
  p.a_bf16 = bf;
  p.out_bf16 = bf;
  p.beta = L.bias;
  p.act = kActRelu;
  p.post_scale = L.s;
  p.post_shift = L.h;
  return p;
}

}  // namespace

void res2_chain(const void* x, int B, int T, int dil, const Res2ChainW& W, void* tmp, void* out, bool bf,
                bool generic, hipStream_t st) {
  constexpr int C = 1024, G = Res2ChainW::kWidth, NS = Res2ChainW::kStages;
  SD_CHECK(x && tmp && out && B >= 1 && T >= 1 && dil >= 1, kErrInvalid, "res2_chain: bad argument");
  if (!generic) {
    SD_CHECK(bf && res2_chain_fused_supported(dil), kErrInvalid,
             "res2_chain: the fused kernel is bf16 with dilation 1..4 (fp32 and bf16x3 take the generic arm)");
    res2_chain_fused(x, B, T, dil, W, out, st);
    return;
  }
  const int64_t esz = bf ? 2 : 4, rows = (int64_t)B * T;
  auto at = [&](const void* p, int64_t elems) { return static_cast<const char*>(p) + elems * esz; };
  auto at_w = [&](void* p, int64_t elems) { return static_cast<char*>(p) + elems * esz; };
  for (int i = 0; i < NS; ++i) {
    if (i > 0) ecapa_add_slice(at(out, (int64_t)(i - 1) * G), C, at(x, (int64_t)i * G), C, rows, tmp, G, bf, st);
    ConvGemmArgs p;
    p.A = i == 0 ? x : tmp; p.a_bf16 = bf; p.lda = i == 0 ? C : G;
    p.B = B; p.H = 1; p.W = T; p.Cin = G; p.Ho = 1; p.Wo = T;
    p.kh = 1; p.kw = 3; p.pw = dil; p.dw = dil;
    p.Wt = W.w[i]; p.N = G; p.K = 3 * G;
    p.beta = W.bias[i]; p.act = kActRelu; p.post_scale = W.s[i]; p.post_shift = W.h[i];
    p.out = at_w(out, (int64_t)i * G); p.out_bf16 = bf;
    p.o_sb = (int64_t)T * C; p.o_sh = 0; p.o_sw = C; p.o_sn = 1;
    conv_gemm(p, bf, st);
  }
  ecapa_add_slice(at(x, (int64_t)NS * G), C, nullptr, 0, rows, at_w(out, (int64_t)NS * G), C, bf, st);
}

void EcapaTrunk::load(ParamStore& ps, DeviceArena& arena, const std::string& pre, bool bf16) {
  bf16_ = bf16;
  layer1_ = load_conv_relu_bn(ps, arena, bf16, pre + "layer1.", kC, kF, kTaps1);
  // as a 1x1 conv over the im2col rows: the same tap-major K = 5 * 80 packing
  layer1_.w.Cin = layer1_.w.K;
  layer1_.w.kw = 1;
  for (int l = 0; l < 3; ++l) {
    Block& b = blocks_[l];
    const std::string q = pre + "layer" + std::to_string(l + 2) + ".se_res2block.";
    b.in = load_conv_relu_bn(ps, arena, bf16, q + "0.", kC, kC, 1);
    for (int i = 0; i < Res2ChainW::kStages; ++i) {
      const std::string c = q + "1.convs." + std::to_string(i) + ".", n = q + "1.bns." + std::to_string(i);
      int N, Cin, kh, kw;
      auto w = ps.pack(c + "weight", N, Cin, kh, kw);
      SD_CHECK(N == 128 && Cin == 128 && kh == 1 && kw == 3, kErrParam, c + "weight must be (128, 128, 3)");
      b.chain.w[i] = upload_packed(arena, w, N, Cin, kh, kw, bf16).w;
      b.chain.bias[i] = load_fp32(ps, arena, c + "bias", 128, 0);
      std::vector<float> s, h;
      ps.bn_fold(n, s, h);
      SD_CHECK(s.size() == 128, kErrParam, n + " size");
      b.chain.s[i] = arena.upload(s);
      b.chain.h[i] = arena.upload(h);
    }
    b.out = load_conv_relu_bn(ps, arena, bf16, q + "2.", kC, kC, 1);
    // SE_Connect's linears (128, 1024) / (1024, 128) uploaded transposed: ecapa_se_fc reads consecutive outputs of one k
    auto transposed = [&](const std::string& key, int rows, int cols) {
      const HostTensor& t = ps.get(key);
      SD_CHECK(t.shape.size() == 2 && t.shape[0] == rows && t.shape[1] == cols, kErrParam, key + " shape");
      std::vector<float> wt(t.data.size());
      for (int r = 0; r < rows; ++r)
        for (int k = 0; k < cols; ++k) wt[(size_t)k * rows + r] = t.data[(size_t)r * cols + k];
      return arena.upload(wt);
    };
    b.w1 = transposed(q + "3.linear1.weight", 128, kC);
    b.b1 = load_fp32(ps, arena, q + "3.linear1.bias", 128, 0);
    b.w2 = transposed(q + "3.linear2.weight", kC, 128);
    b.b2 = load_fp32(ps, arena, q + "3.linear2.bias", kC, 0);
  }
  conv_ = load_conv_bn(ps, arena, bf16, pre + "conv.weight", "", pre + "conv.bias");
  SD_CHECK(conv_.w.N == kChannels && conv_.w.Cin == kCat && conv_.w.kw == 1, kErrParam,
           pre + "conv.weight must be (1536, 3072, 1)");
  SD_CHECK(ps.get(pre + "conv.bias").numel() == kChannels, kErrParam, pre + "conv.bias size");
}

void EcapaTrunk::alloc(DeviceArena& a, int max_batch, int max_frames) {
  // fp32 elements cover both modes
  const size_t rows = (size_t)max_batch * max_frames;
  auto map = [&](int ch) { return a.alloc(rows * ch * sizeof(float)); };
  col_ = map(kTaps1 * kF);
  h1_ = map(kC);
  ya_ = map(kC);
  yb_ = map(kC);
  tmp_ = map(Res2ChainW::kWidth);
  cat_ = map(kCat);
  out_ = map(kChannels);
  mean_ = static_cast<float*>(a.alloc((size_t)max_batch * kC * sizeof(float)));
  gate_ = static_cast<float*>(a.alloc((size_t)max_batch * kC * sizeof(float)));
}

Tens EcapaTrunk::forward(const float* fbank, int B, int T, hipStream_t st, int b0) const {
  const bool bf = bf16_;
  // SDIAR_RES2_GENERIC (A/B runs, tools/ecapa_probe.py): the seven-launch chain in bf16 mode too
  static const bool chain_generic = getenv("SDIAR_RES2_GENERIC") != nullptr;
  const int64_t esz = bf ? 2 : 4, rows = (int64_t)B * T;
  // window slice b0: every buffer addressed from its window-b0 part
  auto sl = [&](void* p, int ch) { return static_cast<char*>(p) + (int64_t)b0 * T * ch * esz; };
  char *col = sl(col_, kTaps1 * kF), *h1 = sl(h1_, kC), *ya = sl(ya_, kC), *yb = sl(yb_, kC);
  char *tmp = sl(tmp_, Res2ChainW::kWidth), *cat = sl(cat_, kCat), *out = sl(out_, kChannels);
  float *mean = mean_ + (int64_t)b0 * kC, *gate = gate_ + (int64_t)b0 * kC;
  // layer1 (:193-196): k5 pad-2 conv + bias -> ReLU -> BN
  ecapa_im2col(fbank + (int64_t)b0 * T * kF, B, T, col, bf, st);
  conv_gemm(pointwise(col, kTaps1 * kF, 0, rows, layer1_, h1, kC, bf), bf, st);
  const char* xin = h1;   // the block's input: layer1's map, then the previous block's slice of the concat buffer
  int ldx = kC;
  for (int l = 0; l < 3; ++l) {
    const Block& b = blocks_[l];
    conv_gemm(pointwise(xin, ldx, 0, rows, b.in, ya, kC, bf), bf, st);
    res2_chain(ya, B, T, l + 2, b.chain, tmp, yb, bf, !bf || chain_generic, st);
    conv_gemm(pointwise(yb, kC, 0, rows, b.out, ya, kC, bf), bf, st);
    ecapa_se_gate(ya, bf, B, T, b.w1, b.b1, b.w2, b.b2, mean, gate, st);
    char* slice = cat + (int64_t)l * kC * esz;
    ecapa_se_apply(xin, ldx, ya, gate, B, T, slice, kCat, bf, st);
    xin = slice;
    ldx = kCat;
  }
  // cat(out2, out3, out4) -> conv 1x1 -> ReLU (:241-242)
  ConvGemmArgs p = linear_args(cat, (int)rows, kCat, kCat, conv_.w.w, kChannels, out, kChannels);
  p.a_bf16 = bf;
  p.out_bf16 = bf;
  p.beta = conv_.beta;
  p.act = kActRelu;
  conv_gemm(p, bf, st);
  return Tens{out, bf};
}

void EcapaModel::build() {
  const int E = cfg_.embed_dim, C = EcapaTrunk::kChannels, H = 128;
  trunk_.load(ps_, arena_, "", cfg_.bf16);
  // pool (pooling_layers_wespeaker.py:100-114): linear1 (128, 3 C, 1) split into its per-frame and context halves
  {
    const HostTensor& w = ps_.get("pool.linear1.weight");
    SD_CHECK(w.numel() == (int64_t)H * 3 * C && w.shape.size() >= 2 && w.shape[0] == H && w.shape[1] == 3 * C, kErrParam,
             "pool.linear1.weight must be (128, 4608, 1)");
    std::vector<float> wx((size_t)H * C), wc((size_t)H * 2 * C);
    for (int n = 0; n < H; ++n) {
      const float* r = w.data.data() + (size_t)n * 3 * C;
      std::copy(r, r + C, wx.begin() + (size_t)n * C);
      std::copy(r + C, r + 3 * C, wc.begin() + (size_t)n * 2 * C);
    }
    w1x_ = upload_packed(arena_, wx, H, C, 1, 1, false);
    w1c_ = arena_.upload(wc);
    b1_ = load_fp32(ps_, arena_, "pool.linear1.bias", H, 0);
    int N, Cin, kh, kw;
    auto w2 = ps_.pack("pool.linear2.weight", N, Cin, kh, kw);
    SD_CHECK(N == C && Cin == H && kh == 1 && kw == 1, kErrParam, "pool.linear2.weight must be (1536, 128, 1)");
    w2_ = upload_packed(arena_, w2, N, Cin, 1, 1, false);
    b2_ = load_fp32(ps_, arena_, "pool.linear2.bias", C, 0);
  }
  // emb = W (s z + h) + b = (W diag(s)) z + (W h + b)   (:250-251; bn(3072) then linear)
  {
    std::vector<float> s, h;
    ps_.bn_fold("bn", s, h);
    const HostTensor& w = ps_.get("linear.weight");
    const HostTensor& b = ps_.get("linear.bias");
    SD_CHECK(w.shape.size() == 2 && w.shape[0] == E && w.shape[1] == 2 * C && (int)s.size() == 2 * C, kErrParam,
             "linear.weight must be (embed_dim, 3072)");
    SD_CHECK(b.numel() == E, kErrParam, "linear.bias size");
    std::vector<float> wf(w.data.size()), bf(E);
    for (int n = 0; n < E; ++n) {
      double acc = b.data[n];
      for (int k = 0; k < 2 * C; ++k) {
        wf[(size_t)n * 2 * C + k] = w.data[(size_t)n * 2 * C + k] * s[k];
        acc += (double)w.data[(size_t)n * 2 * C + k] * h[k];
      }
      bf[n] = (float)acc;
    }
    linear_.w = upload_packed(arena_, wf, E, 2 * C, 1, 1, false);
    linear_.beta = arena_.upload(bf);
  }
  ps_.require_all_used();   // bn2.* (emb_bn is off), ...
  trunk_.alloc(arena_, cfg_.max_batch, cfg_.max_frames);
  const size_t Bm = cfg_.max_batch, rows = Bm * cfg_.max_frames;
  stats_ = ws(Bm * 2 * C);
  ctx_ = ws(Bm * 2 * C);
  cv_ = ws(Bm * H);
  h_ = ws(rows * H);
  e_ = ws(rows * C);
  if (cfg_.bf16) x32_ = ws(rows * C);
}

void EcapaModel::forward(const float* fbank, int B, int T, float* emb, float* time_out, hipStream_t st) {
  require_finalized();
  SD_CHECK(B >= 1 && B <= cfg_.max_batch, kErrInvalid, "batch exceeds max_batch");
  SD_CHECK(T >= 1 && T <= cfg_.max_frames, kErrInvalid, "fbank frames exceed max_frames");
  SD_CHECK(!emb || T >= 2, kErrShape,
           "ECAPA embeddings need at least 2 fbank frames (ASTP's unbiased variance of one frame is NaN)");
  const int C = EcapaTrunk::kChannels;
  const Tens x = trunk_.forward(fbank, B, T, st);
  const int64_t n = (int64_t)B * T * C;
  if (time_out) {
    if (x.bf) bf16_to_f32(x.p, n, time_out, st);
    else SD_HIP(hipMemcpyAsync(time_out, x.p, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (!emb) return;
  AstpArgs a;
  a.x = x.p; a.x_bf16 = x.bf; a.B = B; a.T = T;
  a.w1x = w1x_.w; a.w1c = w1c_; a.b1 = b1_; a.w2 = w2_.w; a.b2 = b2_;
  a.stats = stats_; a.ctx = ctx_; a.cv = cv_; a.x32 = x32_; a.h = h_; a.e = e_;
  astp_pool(a, st);   // pool (:250)
  seg_linear(stats_, B, 2 * C, static_cast<const float*>(linear_.w.w), linear_.beta, cfg_.embed_dim, emb, st);
}

}  // namespace sd
