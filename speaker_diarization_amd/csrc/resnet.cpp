// ResNet34 speech-encoder trunk on gfx950 (see resnet.h).
#include "resnet.h"
#include "campp.h"

namespace sd {

namespace {

constexpr int kF = 80;
const int kPlanes[4] = {32, 64, 128, 256};
const int kBlocks[4] = {3, 4, 6, 3};

// Square-stride conv on an NHWC map (C = L.w.Cin) -> NHWC out.
ConvGemmArgs conv2d(Tens in, int B, int H, int W, const ConvL& L, int s, int pad, Tens out) {
  ConvGemmArgs p;
  p.A = in.p; p.a_bf16 = in.bf; p.B = B; p.H = H; p.W = W; p.Cin = L.w.Cin; p.lda = L.w.Cin; p.a_coff = 0;
  p.kh = L.w.kh; p.kw = L.w.kw; p.sh = s; p.sw = s; p.ph = pad; p.pw = pad; p.dh = 1; p.dw = 1;
  p.Ho = (H + 2 * pad - L.w.kh) / s + 1;
  p.Wo = (W + 2 * pad - L.w.kw) / s + 1;
  p.Wt = L.w.w; p.N = L.w.N; p.K = L.w.K;
  p.alpha = L.alpha; p.beta = L.beta;
  p.out = out.p; p.out_bf16 = out.bf;
  p.o_sb = (int64_t)p.Ho * p.Wo * p.N; p.o_sh = (int64_t)p.Wo * p.N; p.o_sw = p.N; p.o_sn = 1;
  return p;
}

}  // namespace

void ResTrunk::load(ParamStore& ps, DeviceArena& arena, const std::string& pre, bool bf16) {
  bf16_ = bf16;
  auto conv_bn = [&](const std::string& w, const std::string& bn) { return load_conv_bn(ps, arena, bf16, w, bn); };
  {
    const HostTensor& w = ps.get(pre + "conv1.weight");
    SD_CHECK(w.numel() == 32 * 9, kErrParam, "speech_encoder.conv1.weight must be (32,1,3,3)");
    stem_.pre_s = arena.upload(w.data);
    std::vector<float> s, h;
    ps.bn_fold(pre + "bn1", s, h);
    stem_.alpha = arena.upload(s);
    stem_.beta = arena.upload(h);
  }
  int cin = 32;
  for (int layer = 0; layer < 4; ++layer)
    for (int blk = 0; blk < kBlocks[layer]; ++blk) {
      const std::string p = pre + "layer" + std::to_string(layer + 1) + "." + std::to_string(blk) + ".";
      Block rb;
      rb.stride = (blk == 0 && layer > 0) ? 2 : 1;
      rb.c1 = conv_bn(p + "conv1.weight", p + "bn1");
      rb.c2 = conv_bn(p + "conv2.weight", p + "bn2");
      rb.has_sc = rb.stride != 1 || cin != kPlanes[layer];
      if (rb.has_sc) {
        rb.sc = conv_bn(p + "shortcut.0.weight", p + "shortcut.1");
        SD_CHECK(rb.sc.w.N == kPlanes[layer] && rb.sc.w.Cin == cin && rb.sc.w.kh == 1 && rb.sc.w.kw == 1, kErrParam,
                 p + "shortcut.0.weight shape");
      }
      SD_CHECK(rb.c1.w.N == kPlanes[layer] && rb.c1.w.Cin == cin && rb.c1.w.kh == 3 && rb.c1.w.kw == 3, kErrParam,
               p + "conv1.weight shape");
      SD_CHECK(rb.c2.w.N == kPlanes[layer] && rb.c2.w.Cin == kPlanes[layer] && rb.c2.w.kh == 3 && rb.c2.w.kw == 3,
               kErrParam, p + "conv2.weight shape");
      cin = kPlanes[layer];
      blocks_.push_back(rb);
    }
}

void ResTrunk::alloc(DeviceArena& a, int max_batch, int max_frames) {
  // the stage-1 map is the largest (every stride-2 stage halves the bytes); fp32 elements cover both modes
  const size_t map = (size_t)max_batch * kF * max_frames * 32;
  for (float*& b : buf_) b = static_cast<float*>(a.alloc(map * sizeof(float)));
  out_ = static_cast<float*>(a.alloc((size_t)max_batch * out_frames(max_frames) * kChannels * sizeof(float)));
}

Tens ResTrunk::forward(const float* fbank, int B, int Tf, hipStream_t st, int b0) const {
  const bool bf = bf16_;
  const int64_t esz = bf ? 2 : 4;
  // window slice b0: every buffer addressed from its window-b0 part, the stage-1 map as the per-window stride
  auto sl = [&](float* p, int64_t per) { return reinterpret_cast<float*>(reinterpret_cast<char*>(p) + b0 * per * esz); };
  const float* ref = fbank + (int64_t)b0 * Tf * kF;
  float* bufs[3] = {sl(buf_[0], (int64_t)kF * Tf * 32), sl(buf_[1], (int64_t)kF * Tf * 32), sl(buf_[2], (int64_t)kF * Tf * 32)};
  const int T4 = out_frames(Tf);
  float* const out = sl(out_, (int64_t)T4 * kChannels);
  // stem: conv1 (1 -> 32, 3x3, pad 1) + bn1 + relu, fbank (B, T, 80) -> NHWC (B, 80, T, 32)
  fcm_conv1(ref, B, Tf, kF, stem_.pre_s, stem_.alpha, stem_.beta, bufs[0], bf, st);
  float* cur = bufs[0];
  int H = kF, W = Tf;
  for (size_t i = 0; i < blocks_.size(); ++i) {
    const Block& rb = blocks_[i];
    float* others[2];
    int k = 0;
    for (float* b : bufs) if (b != cur) others[k++] = b;
    float* const t1 = others[0];
    float* const t2 = others[1];
    // conv1 + bn1 + relu (+ the opener's shortcut conv + BN from the same staged pixels)
    ConvGemmArgs p = conv2d(Tens{cur, bf}, B, H, W, rb.c1, rb.stride, 1, Tens{t1, bf});
    p.act = kActRelu;
    const bool k1 = bf && res_conv_supported(p);
    ResFuse fu;
    if (rb.has_sc && k1) {
      fu.sc_w = rb.sc.w.w; fu.sc_alpha = rb.sc.alpha; fu.sc_beta = rb.sc.beta; fu.sc_out = t2;
    }
    if (k1) res_conv3x3(p, fu, st);
    else conv_gemm(p, bf, st);
    const int Ho = p.Ho, Wo = p.Wo;
    const float* res = cur;
    float* outb = t2;
    if (rb.has_sc) {
      if (!k1) conv_gemm(conv2d(Tens{cur, bf}, B, H, W, rb.sc, rb.stride, 0, Tens{t2, bf}), bf, st);
      res = t2;
      outb = cur;   // the block's input is no longer needed
    }
    // conv2 + bn2 + residual + relu
    ConvGemmArgs r = conv2d(Tens{t1, bf}, B, Ho, Wo, rb.c2, 1, 1, Tens{outb, bf});
    r.res = res; r.res_bf16 = bf; r.res_ld = rb.c2.w.N;
    r.act = kActRelu;
    if (i + 1 == blocks_.size()) {
      // the stage-4 map leaves as (B, T', C * F') with channel c * F' + f
      SD_CHECK(Ho * r.N == kChannels && Wo == T4, kErrShape, "ResNet34 output map mismatch");
      r.out = out;
      r.o_sb = (int64_t)Wo * kChannels; r.o_sh = 1; r.o_sw = kChannels; r.o_sn = Ho;
    }
    if (bf && res_conv_supported(r)) res_conv3x3(r, ResFuse{}, st);
    else conv_gemm(r, bf, st);
    cur = outb;
    H = Ho;
    W = Wo;
  }
  return Tens{out, bf};
}

}  // namespace sd
