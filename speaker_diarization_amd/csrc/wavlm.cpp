// WavLM feature extractor on gfx950 (see wavlm.h).
#include "wavlm.h"

#include <algorithm>
#include <cmath>

namespace sd {

namespace {

constexpr int kConvC = 512;
const int kConvK[7] = {10, 3, 3, 3, 3, 2, 2};
const int kConvS[7] = {5, 2, 2, 2, 2, 2, 2};
constexpr int kPosTaps = 128, kPosGroups = 16;

void copy_async(float* dst, const float* src, size_t n, hipStream_t st) {
  SD_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
}

}  // namespace

int wavlm_bucket(int rel) {
  // evaluated in double in the reference's order, log(n / 80) / log(800 / 80) * 80: distance 713 lies 3.7e-5 below a
  // bucket edge, and this order gives the reference's row for every distance the tests pin (up to 3000)
  const int nb = 160, exact = 80;
  const int sign = rel > 0 ? nb : 0, a = std::abs(rel);
  if (a < exact) return sign + a;
  const int large = exact + (int)(std::log((double)a / exact) / std::log(800.0 / exact) * (nb - exact));
  return sign + std::min(large, nb - 1);
}

void wavlm_fold_pos_weight(const float* g, const float* v, int D, float* out) {
  const int Dg = D / kPosGroups;
  const size_t n = (size_t)D * Dg * kPosTaps;
  std::vector<double> nrm(kPosTaps, 0.0);
  for (size_t i = 0; i < n; ++i) nrm[i % kPosTaps] += (double)v[i] * v[i];
  for (size_t i = 0; i < n; ++i) out[i] = (float)((double)g[i % kPosTaps] * v[i] / std::sqrt(nrm[i % kPosTaps]));
}

int WavlmTrunk::conv_frames(int n, int layer) {
  for (int i = 0; i <= layer; ++i) n = n < kConvK[i] ? 0 : (n - kConvK[i]) / kConvS[i] + 1;
  return n;
}

int WavlmTrunk::frames(int n_samples) { return conv_frames(n_samples, 6); }

void WavlmTrunk::load(ParamStore& ps_, DeviceArena& arena_, const std::string& pre) {
  const int D = cfg_.embed_dim, F = cfg_.ffn_dim, H = cfg_.heads, Dg = D / kPosGroups;
  const bool bf = cfg_.bf16, lnm = cfg_.layer_norm_mode;
  SD_CHECK((D == 768 && F == 3072 && H == 12) || (D == 1024 && F == 4096 && H == 16), kErrInvalid,
           "WavLM (MI355X backend) builds (embed_dim, ffn_dim, heads) = (768, 3072, 12) or (1024, 4096, 16) only");
  LayerLoader ld{ps_, arena_, bf}, f32{ps_, arena_, false};
  SD_CHECK(ps_.get(pre + "mask_emb").numel() == D, kErrParam, pre + "mask_emb size");   // training-time masking only
  {
    const std::string p = pre + "feature_extractor.conv_layers.";
    const HostTensor& w0 = ps_.get(p + "0.0.weight");
    SD_CHECK(w0.shape.size() == 3 && w0.shape[0] == kConvC && w0.shape[1] == 1 && w0.shape[2] == kConvK[0], kErrParam,
             p + "0.0.weight must be (512,1,10)");
    c0_w_ = arena_.upload(w0.data);
    for (int i = 0; i < 7; ++i) {
      const std::string q = p + std::to_string(i);
      if (lnm || i == 0) {
        const std::string nrm = q + (lnm ? ".2.1" : ".2");
        SD_CHECK(ps_.get(nrm + ".weight").numel() == kConvC && ps_.get(nrm + ".bias").numel() == kConvC, kErrParam,
                 nrm + " size");
        cn_g_[i] = f32.up(nrm + ".weight");
        cn_b_[i] = f32.up(nrm + ".bias");
      }
      if (i == 0) continue;
      conv_[i] = ld.packed(q + ".0.weight");
      SD_CHECK(conv_[i].N == kConvC && conv_[i].Cin == kConvC && conv_[i].kw == kConvK[i] && conv_[i].kh == 1, kErrParam,
               q + ".0.weight must be (512,512," + std::to_string(kConvK[i]) + ")");
    }
  }
  SD_CHECK(ps_.get(pre + "layer_norm.weight").numel() == kConvC && ps_.get(pre + "layer_norm.bias").numel() == kConvC, kErrParam,
           pre + "layer_norm size");
  ln_g_ = f32.up(pre + "layer_norm.weight");
  ln_b_ = f32.up(pre + "layer_norm.bias");
  proj_ = ld.linear(pre + "post_extract_proj");
  SD_CHECK(proj_.w.N == D && proj_.w.K == kConvC, kErrParam, pre + "post_extract_proj.weight must be (embed_dim,512)");
  {
    // weight_norm(dim = 2) of pos_conv (wavlm.py:578-580): w[n, c, tap] = g[tap] v[n, c, tap] / |v[:, :, tap]|, the
    // norm over the output and input channels of each tap; both spellings of the pair
    const std::string p = pre + "encoder.pos_conv.0.";
    const bool old_keys = ps_.has(p + "weight_g");
    const HostTensor& g = ps_.get(p + (old_keys ? "weight_g" : "parametrizations.weight.original0"));
    const HostTensor& v = ps_.get(p + (old_keys ? "weight_v" : "parametrizations.weight.original1"));
    SD_CHECK(g.numel() == kPosTaps, kErrParam, p + "weight g must be (1,1,128)");
    SD_CHECK(v.shape.size() == 3 && v.shape[0] == D && v.shape[1] == Dg && v.shape[2] == kPosTaps, kErrParam,
             p + "weight v must be (embed_dim,embed_dim/16,128)");
    std::vector<float> folded(v.data.size()), w(v.data.size());
    wavlm_fold_pos_weight(g.data.data(), v.data.data(), D, folded.data());
    for (int n = 0; n < D; ++n)   // (n, c, tap) -> [n][tap * Dg + c], the kernel's tap-major K
      for (int c = 0; c < Dg; ++c)
        for (int t = 0; t < kPosTaps; ++t)
          w[((size_t)n * kPosTaps + t) * Dg + c] = folded[((size_t)n * Dg + c) * kPosTaps + t];
    pos_w_ = upload_packed(arena_, w, D, Dg, 1, kPosTaps, bf);
    SD_CHECK(ps_.get(p + "bias").numel() == D, kErrParam, p + "bias size");
    pos_b_ = f32.up(p + "bias");
  }
  for (int i = 0; i < cfg_.layers; ++i) {
    const std::string p = pre + "encoder.layers." + std::to_string(i) + ".", a = p + "self_attn.";
    Layer L;
    std::vector<float> w, b;
    for (const char* nm : {"q_proj", "k_proj", "v_proj"}) {   // k_proj has a bias, as in F.multi_head_attention_forward
      const HostTensor& wi = ps_.get(a + nm + ".weight");
      const HostTensor& bi = ps_.get(a + nm + ".bias");
      SD_CHECK(wi.shape.size() == 2 && wi.shape[0] == D && wi.shape[1] == D && bi.numel() == D, kErrParam,
               a + nm + " must be (embed_dim,embed_dim) with a bias");
      w.insert(w.end(), wi.data.begin(), wi.data.end());
      b.insert(b.end(), bi.data.begin(), bi.data.end());
    }
    L.in_proj = upload_packed(arena_, w, 3 * D, D, 1, 1, bf);
    L.in_b = arena_.upload(b);
    const ConvL o = ld.linear(a + "out_proj"), l1 = ld.linear(p + "fc1"), l2 = ld.linear(p + "fc2");
    SD_CHECK(o.w.N == D && o.w.K == D, kErrParam, a + "out_proj.weight shape");
    SD_CHECK(l1.w.N == F && l1.w.K == D && l2.w.N == D && l2.w.K == F, kErrParam, p + "fc1 / fc2 weight shape");
    L.out_proj = o.w; L.out_b = o.beta;
    L.fc1 = l1.w; L.b1 = l1.beta;
    L.fc2 = l2.w; L.b2 = l2.beta;
    for (const char* nm : {"self_attn_layer_norm", "final_layer_norm"})
      SD_CHECK(ps_.get(p + nm + ".weight").numel() == D && ps_.get(p + nm + ".bias").numel() == D, kErrParam,
               p + nm + " size");
    L.n1g = f32.up(p + "self_attn_layer_norm.weight"); L.n1b = f32.up(p + "self_attn_layer_norm.bias");
    L.n2g = f32.up(p + "final_layer_norm.weight"); L.n2b = f32.up(p + "final_layer_norm.bias");
    SD_CHECK(ps_.get(a + "grep_linear.weight").numel() == 8 * 64 && ps_.get(a + "grep_linear.bias").numel() == 8 &&
                 ps_.get(a + "grep_a").numel() == H, kErrParam, a + "grep_linear (8,64) / grep_a (1,heads,1,1) shape");
    L.grep_w = f32.up(a + "grep_linear.weight");
    L.grep_b = f32.up(a + "grep_linear.bias");
    L.grep_a = f32.up(a + "grep_a");
    if (i == 0) {   // only layer 0 owns the table; every layer reuses its bias (wavlm.py:603-605, 656-662)
      const HostTensor& e = ps_.get(a + "relative_attention_bias.weight");
      SD_CHECK(e.shape.size() == 2 && e.shape[0] == 320 && e.shape[1] == H, kErrParam,
               a + "relative_attention_bias.weight must be (320,heads)");
      rel_emb_ = arena_.upload(e.data);
    }
    layers_.push_back(L);
  }
  SD_CHECK(ps_.get(pre + "encoder.layer_norm.weight").numel() == D && ps_.get(pre + "encoder.layer_norm.bias").numel() == D,
           kErrParam, pre + "encoder.layer_norm size");
  enc_g_ = f32.up(pre + "encoder.layer_norm.weight");
  enc_b_ = f32.up(pre + "encoder.layer_norm.bias");
}

void WavlmTrunk::alloc(DeviceArena& arena_) {
  const int D = cfg_.embed_dim, F = cfg_.ffn_dim, H = cfg_.heads;
  const bool bf = cfg_.bf16, lnm = cfg_.layer_norm_mode;
  auto ws = [&](size_t n) { return static_cast<float*>(arena_.alloc(n * sizeof(float))); };
  max_T_ = frames(cfg_.max_samples);
  SD_CHECK(max_T_ >= 1, kErrInvalid, "max_samples must be at least 400");
  {
    std::vector<int> bm(2 * max_T_ - 1);
    for (int r = -(max_T_ - 1); r <= max_T_ - 1; ++r) bm[r + max_T_ - 1] = wavlm_bucket(r);
    int* d = static_cast<int*>(arena_.alloc(bm.size() * sizeof(int)));
    SD_HIP(hipMemcpy(d, bm.data(), bm.size() * sizeof(int), hipMemcpyHostToDevice));
    bmap_ = d;
  }
  const size_t esz = bf ? 2 : 4, S = std::min(cfg_.max_batch, kSlice);
  const size_t T0 = conv_frames(cfg_.max_samples, 0), T1 = conv_frames(cfg_.max_samples, 1);
  mapA_ = static_cast<float*>(arena_.alloc(S * T0 * kConvC * esz));
  mapB_ = static_cast<float*>(arena_.alloc(S * T1 * kConvC * esz));
  if (!lnm) {
    partial_ = ws(S * wavlm_l0_parts((int)T0) * 3 * kConvC);
    ss_ = ws(S * 2 * kConvC);
  }
  const size_t rows = (size_t)cfg_.max_batch * max_T_;
  feat_ = ws(rows * kConvC);
  featn_ = static_cast<float*>(arena_.alloc(rows * kConvC * esz));
  F_ = ws(rows * D);
  X_ = ws(rows * D);
  Y_ = ws(rows * D);
  QKV_ = static_cast<float*>(arena_.alloc(rows * 3 * D * esz));   // bf16 in bf16 mode
  AO_ = static_cast<float*>(arena_.alloc(rows * D * esz));
  H_ = ws(rows * F);   // fp32 size in both modes: the bf16 hidden layer leaves the upper half to the split-K slabs
  if (bf) Yb_ = static_cast<uint16_t*>(arena_.alloc(rows * D * 2));
  table_ = ws((size_t)H * (2 * max_T_ - 1));
}

void WavlmTrunk::front_end(const float* source, int B, int n, hipStream_t st) {
  const bool bf = cfg_.bf16, lnm = cfg_.layer_norm_mode;
  const int T = frames(n);
  for (int b0 = 0; b0 < B; b0 += kSlice) {
    const int Bs = std::min(kSlice, B - b0);
    wavlm_layer0(source + (size_t)b0 * n, Bs, n, c0_w_, cn_g_[0], cn_b_[0], lnm, partial_, ss_, mapA_, bf, st);
    float* cur = mapA_;
    int Ti = conv_frames(n, 0);
    for (int i = 1; i < 7; ++i) {
      const bool last = i == 6;
      const int To = (Ti - kConvK[i]) / kConvS[i] + 1;
      // channel-last, a k-tap stride-2 unpadded conv is a GEMM whose A rows overlap: row t starts at frame 2 t and
      // is k * 512 long -- conv_gemm's multi-tap strided form
      ConvGemmArgs p;
      p.A = cur; p.a_bf16 = bf; p.B = Bs; p.H = 1; p.W = Ti; p.Cin = kConvC; p.lda = kConvC;
      p.kh = 1; p.kw = kConvK[i]; p.sh = 1; p.sw = kConvS[i]; p.Ho = 1; p.Wo = To;
      p.Wt = conv_[i].w; p.N = kConvC; p.K = conv_[i].K;
      p.act = lnm ? kActNone : kActGelu;
      float* out = last ? feat_ + (size_t)b0 * T * kConvC : (cur == mapA_ ? mapB_ : mapA_);
      p.out = out; p.out_bf16 = bf && !last;   // the last map feeds an fp32 LayerNorm
      p.o_sb = (int64_t)To * kConvC; p.o_sw = kConvC; p.o_sn = 1;
      conv_gemm(p, bf, st);
      if (lnm) wavlm_ln_gelu(out, p.out_bf16, (int64_t)Bs * To, cn_g_[i], cn_b_[i], st);
      cur = out;
      Ti = To;
    }
    SD_CHECK(Ti == T, kErrShape, "WavLM conv front end frame count mismatch");
  }
}

void WavlmTrunk::run_layer(const Layer& L, int B, int T, hipStream_t st) {
  const bool bf = cfg_.bf16;
  const int D = cfg_.embed_dim, rows = B * T;
  const Tens qkv{QKV_, bf}, ao{AO_, bf}, t{Y_, bf}, h{H_, bf};
  WavlmAttnArgs a;
  a.qkv = QKV_; a.bf16 = bf; a.B = B; a.T = T; a.D = D; a.H = cfg_.heads;
  a.grep_w = L.grep_w; a.grep_b = L.grep_b; a.grep_a = L.grep_a; a.table = table_;
  a.scale = 0.125f;   // head_dim^-0.5 at head size 64
  a.out = AO_; a.out_bf16 = bf;
  if (!cfg_.pre_ln) {
    // post-LN (wavlm.py:778-803): X = LN1(X + SA(X)); X = LN2(X + FFN(X)); Yb_ holds bf16(X) in bf16 mode
    const Tens xa = bf ? Tens{Yb_, true} : Tens{X_, false};
    conv_gemm(lin(xa, rows, D, L.in_proj, L.in_b, qkv, 3 * D), bf, st);
    a.xin = X_;   // the gate reads the layer's input, not q
    wavlm_attention(a, st);
    conv_gemm(lin(ao, rows, D, L.out_proj, L.out_b, t, D), bf, st);
    add_layernorm(X_, Y_, bf, rows, D, L.n1g, L.n1b, 1e-5f, false, X_, false, st, Yb_);
    ConvGemmArgs p = lin(xa, rows, D, L.fc1, L.b1, h, L.fc1.N);
    p.act = kActGelu;
    conv_gemm(p, bf, st);
    ffn_down_add_ln(lin(h, rows, L.fc1.N, L.fc2, L.b2, t, D), H_, X_, L.n2g, L.n2b, bf, Yb_, st, cfg_.split_k);
    return;
  }
  // pre-LN (:754-777): X += SA(LN1(X)); X += FFN(LN2(X)); the gate reads the normalised input in fp32
  layernorm(X_, rows, D, D, L.n1g, L.n1b, 1e-5f, Y_, D, false, st, Yb_);
  const Tens ya = bf ? Tens{Yb_, true} : Tens{Y_, false};
  conv_gemm(lin(ya, rows, D, L.in_proj, L.in_b, qkv, 3 * D), bf, st);
  a.xin = Y_;
  wavlm_attention(a, st);
  conv_gemm(lin(ao, rows, D, L.out_proj, L.out_b, t, D), bf, st);
  wavlm_add(X_, Y_, bf, (int64_t)rows * D, st);
  layernorm(X_, rows, D, D, L.n2g, L.n2b, 1e-5f, ya.p, D, bf, st);
  ConvGemmArgs p = lin(ya, rows, D, L.fc1, L.b1, h, L.fc1.N);
  p.act = kActGelu;
  conv_gemm(p, bf, st);
  conv_gemm(lin(h, rows, L.fc1.N, L.fc2, L.b2, t, D), bf, st);
  wavlm_add(X_, Y_, bf, (int64_t)rows * D, st);
}

void WavlmTrunk::check_input(int B, int n_samples) const {
  SD_CHECK(B >= 1 && B <= cfg_.max_batch, kErrInvalid, "batch exceeds max_batch");
  SD_CHECK(n_samples >= kMinSamples, kErrInvalid, "n_samples must be at least 400");
  SD_CHECK(n_samples <= cfg_.max_samples, kErrInvalid, "n_samples exceeds max_samples");
}

void WavlmTrunk::stem(const float* source, int B, int n_samples, hipStream_t st) {
  const bool bf = cfg_.bf16;
  const int D = cfg_.embed_dim, T = frames(n_samples), rows = B * T;
  front_end(source, B, n_samples, st);
  // features = post_extract_proj(LayerNorm(conv features)) (wavlm.py:377-384)
  layernorm(feat_, rows, kConvC, kConvC, ln_g_, ln_b_, 1e-5f, featn_, kConvC, bf, st);
  conv_gemm(lin(Tens{featn_, bf}, rows, kConvC, proj_.w, proj_.beta, Tens{F_, false}, D), bf, st);
}

void WavlmTrunk::forward(const float* source, int B, int n_samples, int output_layer, float* x_out,
                         float* features_out, float* layers_out, hipStream_t st) {
  check_input(B, n_samples);
  SD_CHECK(output_layer >= 0 && output_layer <= cfg_.layers, kErrInvalid,
           "output_layer must be 0 (all layers) or 1..encoder_layers");
  SD_CHECK(!layers_out || output_layer >= 1, kErrInvalid, "layers_out needs output_layer >= 1");
  const int D = cfg_.embed_dim, T = frames(n_samples), rows = B * T;
  const size_t nx = (size_t)rows * D;
  stem(source, B, n_samples, st);
  if (features_out) copy_async(features_out, F_, nx, st);
  if (!x_out && !layers_out) return;
  // x = x + GELU(pos_conv(x)); post-LN mode normalises right after (wavlm.py:635-640)
  if (cfg_.pre_ln) {
    wavlm_pos_conv(F_, B, T, D, pos_w_.w, cfg_.bf16, pos_b_, X_, st);
  } else {
    wavlm_pos_conv(F_, B, T, D, pos_w_.w, cfg_.bf16, pos_b_, Y_, st);
    layernorm(Y_, rows, D, D, enc_g_, enc_b_, 1e-5f, X_, D, false, st, Yb_);
  }
  wavlm_bias_table(rel_emb_, bmap_, max_T_ - 1, T, cfg_.heads, table_, st);
  if (layers_out) copy_async(layers_out, X_, nx, st);
  const int n_layers = output_layer ? output_layer : cfg_.layers;
  for (int i = 0; i < n_layers; ++i) {
    run_layer(layers_[i], B, T, st);
    if (layers_out) copy_async(layers_out + (size_t)(i + 1) * nx, X_, nx, st);
  }
  if (!x_out) return;
  // the final encoder.layer_norm of pre-LN mode only without output_layer (wavlm.py:623-624)
  if (cfg_.pre_ln && output_layer == 0)
    layernorm(X_, rows, D, D, enc_g_, enc_b_, 1e-5f, x_out, D, false, st);
  else
    copy_async(x_out, X_, nx, st);
}

void WavlmTrunk::encode_layers(const float* source, int B, int n_samples, const LayerSink& sink, hipStream_t st) {
  check_input(B, n_samples);
  const int D = cfg_.embed_dim, T = frames(n_samples), rows = B * T;
  stem(source, B, n_samples, st);
  if (cfg_.pre_ln) {
    wavlm_pos_conv(F_, B, T, D, pos_w_.w, cfg_.bf16, pos_b_, X_, st);
  } else {
    wavlm_pos_conv(F_, B, T, D, pos_w_.w, cfg_.bf16, pos_b_, Y_, st);
    layernorm(Y_, rows, D, D, enc_g_, enc_b_, 1e-5f, X_, D, false, st, Yb_);
  }
  wavlm_bias_table(rel_emb_, bmap_, max_T_ - 1, T, cfg_.heads, table_, st);
  for (int i = 0; i < cfg_.layers; ++i) {
    run_layer(layers_[i], B, T, st);
    if (sink) sink(i, X_, st);
  }
}

Tens WavlmTrunk::encode(const float* source, int B, int n_samples, hipStream_t st) {
  encode_layers(source, B, n_samples, nullptr, st);
  const bool bf = cfg_.bf16;
  const int D = cfg_.embed_dim, rows = B * frames(n_samples);
  if (cfg_.pre_ln) {   // the final encoder.layer_norm (wavlm.py:623-624) into the layers' scratch
    layernorm(X_, rows, D, D, enc_g_, enc_b_, 1e-5f, Y_, D, bf, st);
    return Tens{Y_, bf};
  }
  // post-LN: the last layer's LayerNorm left bf16(X) beside X in bf16 mode
  return bf ? Tens{Yb_, true} : Tens{X_, false};
}

}  // namespace sd
