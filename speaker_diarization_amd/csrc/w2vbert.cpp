// w2v-BERT 2.0 speech encoder on gfx950 (see w2vbert.h).
#include "w2vbert.h"

#include <algorithm>

namespace sd {

namespace {

void copy_async(float* dst, const float* src, size_t n, hipStream_t st) {
  SD_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
}

}  // namespace

void W2vBertTrunk::load(ParamStore& ps_, DeviceArena& arena_, const std::string& pre) {
  const int D = kHidden, F = kFfn;
  const bool bf = cfg_.bf16;
  LayerLoader ld{ps_, arena_, bf};
  auto vec = [&](const std::string& key, int n) {
    SD_CHECK(ps_.get(key).numel() == n, kErrParam, key + " must hold " + std::to_string(n) + " values");
    return ld.up(key);
  };
  auto norm = [&](const std::string& p, int n, const float*& g, const float*& b) {
    g = vec(p + ".weight", n);
    b = vec(p + ".bias", n);
  };
  auto linear = [&](const std::string& p, int n, int k, float mult, PackedW& w, const float*& b) {
    const HostTensor& wt = ps_.get(p + ".weight");
    SD_CHECK(wt.shape.size() == 2 && wt.shape[0] == n && wt.shape[1] == k && ps_.get(p + ".bias").numel() == n, kErrParam,
             p + ".weight must be (" + std::to_string(n) + "," + std::to_string(k) + ") with a bias");
    const ConvL l = ld.linear(p, mult);
    w = l.w;
    b = l.beta;
  };
  SD_CHECK(ps_.get(pre + "masked_spec_embed").numel() == D, kErrParam, pre + "masked_spec_embed size");
  norm(pre + "feature_projection.layer_norm", kInDim, fp_g_, fp_b_);
  linear(pre + "feature_projection.projection", D, kInDim, 1.f, proj_.w, proj_.beta);
  for (int i = 0; i < cfg_.layers; ++i) {
    const std::string p = pre + "encoder.layers." + std::to_string(i) + ".", a = p + "self_attn.", c = p + "conv_module.";
    Layer L;
    // x = x + 0.5 ffn(LN(x)) (:432-435, 455-458): the 0.5 folded into output_dense (exact)
    norm(p + "ffn1_layer_norm", D, L.f1_g, L.f1_b);
    linear(p + "ffn1.intermediate_dense", F, D, 1.f, L.f1_up, L.f1_b1);
    linear(p + "ffn1.output_dense", D, F, 0.5f, L.f1_down, L.f1_b2);
    norm(p + "self_attn_layer_norm", D, L.at_g, L.at_b);
    std::vector<float> w, b;
    for (const char* nm : {"linear_q", "linear_k", "linear_v"}) {
      const HostTensor& wi = ps_.get(a + nm + ".weight");
      const HostTensor& bi = ps_.get(a + nm + ".bias");
      SD_CHECK(wi.shape.size() == 2 && wi.shape[0] == D && wi.shape[1] == D && bi.numel() == D, kErrParam,
               a + nm + " must be (1024,1024) with a bias");
      w.insert(w.end(), wi.data.begin(), wi.data.end());
      b.insert(b.end(), bi.data.begin(), bi.data.end());
    }
    L.in_proj = upload_packed(arena_, w, 3 * D, D, 1, 1, bf);
    L.in_b = arena_.upload(b);
    linear(a + "linear_out", D, D, 1.f, L.out_proj, L.out_b);
    {
      // nn.Embedding(left + right + 1, head_size) shared by the heads (:257-261), zero-padded to 80 rows
      const HostTensor& e = ps_.get(a + "distance_embedding.weight");
      SD_CHECK(e.shape.size() == 2 && e.shape[0] == kLeft + kRight + 1 && e.shape[1] == 64, kErrParam,
               a + "distance_embedding.weight must be (73,64)");
      std::vector<float> ep((size_t)kW2vDistRows * 64, 0.f);
      std::copy(e.data.begin(), e.data.end(), ep.begin());
      L.dist = upload_packed(arena_, ep, kW2vDistRows, 64, 1, 1, bf).w;
    }
    norm(c + "layer_norm", D, L.cv_g, L.cv_b);
    L.pw1 = ld.packed(c + "pointwise_conv1.weight");   // plain [value | gate] halves: the conv mix reads both
    SD_CHECK(L.pw1.N == 2 * D && L.pw1.K == D, kErrParam, c + "pointwise_conv1.weight must be (2048,1024,1)");
    const HostTensor& dw = ps_.get(c + "depthwise_conv.weight");
    SD_CHECK(dw.shape.size() == 3 && dw.shape[0] == D && dw.shape[1] == 1 && dw.shape[2] == kConvK, kErrParam,
             c + "depthwise_conv.weight must be (1024,1,31)");
    L.dw_w = arena_.upload(dw.data);
    norm(c + "depthwise_layer_norm", D, L.dn_g, L.dn_b);
    L.pw2 = ld.packed(c + "pointwise_conv2.weight");
    SD_CHECK(L.pw2.N == D && L.pw2.K == D, kErrParam, c + "pointwise_conv2.weight must be (1024,1024,1)");
    norm(p + "ffn2_layer_norm", D, L.f2_g, L.f2_b);
    linear(p + "ffn2.intermediate_dense", F, D, 1.f, L.f2_up, L.f2_b1);
    linear(p + "ffn2.output_dense", D, F, 0.5f, L.f2_down, L.f2_b2);
    norm(p + "final_layer_norm", D, L.fin_g, L.fin_b);
    layers_.push_back(L);
  }
}

void W2vBertTrunk::alloc(DeviceArena& arena_) {
  const bool bf = cfg_.bf16;
  const size_t esz = bf ? 2 : 4, rows = (size_t)cfg_.max_batch * cfg_.max_frames;
  auto ws = [&](size_t n) { return static_cast<float*>(arena_.alloc(n * sizeof(float))); };
  Fn_ = arena_.alloc(rows * kInDim * esz);
  X_ = ws(rows * kHidden);
  T_ = ws(rows * kHidden);
  Y_ = arena_.alloc(rows * kHidden * esz);
  AO_ = arena_.alloc(rows * kHidden * esz);
  QKV_ = arena_.alloc(rows * 3 * kHidden * esz);
  H_ = arena_.alloc(rows * kFfn * esz);
  if (bf) Xb_ = static_cast<uint16_t*>(arena_.alloc(rows * kHidden * 2));
}

void W2vBertTrunk::check_input(int B, int T2) const {
  SD_CHECK(B >= 1 && B <= cfg_.max_batch, kErrInvalid, "batch exceeds max_batch");
  SD_CHECK(T2 >= 1, kErrInvalid, "at least one frame pair");
  SD_CHECK(T2 <= cfg_.max_frames, kErrInvalid, "frames exceed max_frames");
  SD_CHECK(!gemm_x3(), kErrInvalid, "the w2v-BERT 2.0 trunk does not build bf16x3: it runs in fp32 or bf16");
}

void W2vBertTrunk::stem(const float* in, int rows, hipStream_t st) {
  const bool bf = cfg_.bf16;
  // hidden_states = projection(layer_norm(input_features)) (:126-131); no masking in eval
  layernorm(in, rows, kInDim, kInDim, fp_g_, fp_b_, 1e-5f, Fn_, kInDim, bf, st);
  conv_gemm(lin(Tens{Fn_, bf}, rows, kInDim, proj_.w, proj_.beta, Tens{X_, false}, kHidden), bf, st);
}

void W2vBertTrunk::run_layer(const Layer& L, int B, int T2, hipStream_t st) {
  const bool bf = cfg_.bf16;
  const int D = kHidden, rows = B * T2;
  const Tens y{Y_, bf}, qkv{QKV_, bf}, ao{AO_, bf}, h{H_, bf}, t{T_, false};
  auto ffn = [&](const PackedW& up, const float* b1, const PackedW& down, const float* b2) {
    ConvGemmArgs p = lin(y, rows, D, up, b1, h, kFfn);
    p.act = kActSilu;
    conv_gemm(p, bf, st);
    conv_gemm(lin(h, rows, kFfn, down, b2, t, D), bf, st);   // weights and bias pre-scaled by 0.5
  };
  // ffn1 (:431-435)
  layernorm(X_, rows, D, D, L.f1_g, L.f1_b, 1e-5f, Y_, D, bf, st);
  ffn(L.f1_up, L.f1_b1, L.f1_down, L.f1_b2);
  // self-attention (:437-447): X += ffn1's half step, Y = self_attn_layer_norm(X)
  add_layernorm(X_, T_, false, rows, D, L.at_g, L.at_b, 1e-5f, true, Y_, bf, st);
  conv_gemm(lin(y, rows, D, L.in_proj, L.in_b, qkv, 3 * D), bf, st);
  W2vAttnArgs a;
  a.qkv = QKV_; a.bf16 = bf; a.dist = L.dist; a.B = B; a.T = T2; a.D = D; a.H = kHeads;
  a.scale = 0.125f;   // 1 / sqrt(head_size), applied to q . k and q . E alike (:306, 320)
  a.out = AO_; a.out_bf16 = bf;
  w2vbert_attention(a, st);
  conv_gemm(lin(ao, rows, D, L.out_proj, L.out_b, t, D), bf, st);
  // conv module (:449-452, 196-226)
  add_layernorm(X_, T_, false, rows, D, L.cv_g, L.cv_b, 1e-5f, true, Y_, bf, st);
  conv_gemm(lin(y, rows, D, L.pw1, nullptr, h, 2 * D), bf, st);
  w2vbert_conv_mix(H_, B, T2, L.dw_w, L.dn_g, L.dn_b, AO_, bf, st);
  conv_gemm(lin(ao, rows, D, L.pw2, nullptr, t, D), bf, st);
  // ffn2 (:454-458) and final_layer_norm (:459)
  add_layernorm(X_, T_, false, rows, D, L.f2_g, L.f2_b, 1e-5f, true, Y_, bf, st);
  ffn(L.f2_up, L.f2_b1, L.f2_down, L.f2_b2);
  add_layernorm(X_, T_, false, rows, D, L.fin_g, L.fin_b, 1e-5f, false, X_, false, st, Xb_);
}

void W2vBertTrunk::forward(const float* in, int B, int T2, float* x_out, float* layers_out, hipStream_t st) {
  check_input(B, T2);
  const int rows = B * T2;
  const size_t nx = (size_t)rows * kHidden;
  stem(in, rows, st);
  if (layers_out) copy_async(layers_out, X_, nx, st);
  for (int i = 0; i < cfg_.layers; ++i) {
    run_layer(layers_[i], B, T2, st);
    if (layers_out) copy_async(layers_out + (size_t)(i + 1) * nx, X_, nx, st);
  }
  if (x_out) copy_async(x_out, X_, nx, st);
}

Tens W2vBertTrunk::encode(const float* in, int B, int T2, hipStream_t st) {
  check_input(B, T2);
  stem(in, B * T2, st);
  for (int i = 0; i < cfg_.layers; ++i) run_layer(layers_[i], B, T2, st);
  // the last layer's final_layer_norm left bf16(X) beside X in bf16 mode
  return cfg_.bf16 ? Tens{Xb_, true} : Tens{X_, false};
}

}  // namespace sd
