// ResNet34 / SimAM-ResNet34 trunk on gfx950 (see resnet.h).
#include "resnet.h"

#include <algorithm>

namespace sd {

namespace {

constexpr int kF = 80;
const int kBlocks[4] = {3, 4, 6, 3};

}  // namespace

void ResTrunk::load(ParamStore& ps, DeviceArena& arena, const std::string& pre, bool bf16, const ResTrunkSpec& spec) {
  SD_CHECK(spec.base == 32 || spec.base == 64, kErrInvalid, "ResTrunk: base width 32 or 64");
  bf16_ = bf16;
  spec_ = spec;
  const int base = spec.base;
  {
    const HostTensor& w = ps.get(pre + "conv1.weight");
    SD_CHECK(w.numel() == base * 9, kErrParam,
             pre + "conv1.weight must be (" + std::to_string(base) + ",1,3,3)");
    stem_.pre_s = arena.upload(w.data);
    std::vector<float> s, h;
    ps.bn_fold(pre + "bn1", s, h);
    stem_.alpha = arena.upload(s);
    stem_.beta = arena.upload(h);
  }
  int cin = base;
  for (int layer = 0; layer < 4; ++layer) {
    const int planes = base << layer;
    for (int blk = 0; blk < kBlocks[layer]; ++blk) {
      const std::string p = pre + "layer" + std::to_string(layer + 1) + "." + std::to_string(blk) + ".";
      const int stride = (blk == 0 && layer > 0) ? 2 : 1;
      ResBlockL rb = load_res_block(ps, arena, bf16, p, stride, stride != 1 || cin != planes, spec.sc_key);
      rb.simam = spec.simam;
      if (rb.has_sc)
        SD_CHECK(rb.sc.w.N == planes && rb.sc.w.Cin == cin && rb.sc.w.kh == 1 && rb.sc.w.kw == 1, kErrParam,
                 p + spec.sc_key + ".0.weight shape");
      SD_CHECK(rb.c1.w.N == planes && rb.c1.w.Cin == cin && rb.c1.w.kh == 3 && rb.c1.w.kw == 3, kErrParam,
               p + "conv1.weight shape");
      SD_CHECK(rb.c2.w.N == planes && rb.c2.w.Cin == planes && rb.c2.w.kh == 3 && rb.c2.w.kw == 3, kErrParam,
               p + "conv2.weight shape");
      cin = planes;
      blocks_.push_back(rb);
    }
  }
}

void ResTrunk::alloc(DeviceArena& a, int max_batch, int max_frames) {
  // the stage-1 map is the largest (every stride-2 stage halves the bytes); fp32 elements cover both modes
  const size_t map = (size_t)max_batch * kF * max_frames * spec_.base;
  for (float*& b : buf_) b = static_cast<float*>(a.alloc(map * sizeof(float)));
  out_ = static_cast<float*>(a.alloc((size_t)max_batch * out_frames(max_frames) * channels() * sizeof(float)));
  if (!spec_.simam) return;
  int H = kF, W = max_frames;
  for (int layer = 0; layer < 4; ++layer) {
    if (layer) { H = down(H); W = down(W); }
    partial_per_win_ = std::max(partial_per_win_, (size_t)simam_tiles(H * W) * (spec_.base << layer) * 24);
  }
  stat_per_win_ = (size_t)(spec_.base << 3) * 16;
  simam_partial_ = static_cast<char*>(a.alloc(max_batch * partial_per_win_));
  simam_stat_ = static_cast<char*>(a.alloc(max_batch * stat_per_win_));
}

Tens ResTrunk::forward(const float* fbank, int B, int Tf, hipStream_t st, int b0) const {
  const bool bf = bf16_;
  const int64_t esz = bf ? 2 : 4;
  const int base = spec_.base, C4 = channels();
  // window slice b0: every buffer addressed from its window-b0 part, the stage-1 map as the per-window stride
  auto sl = [&](float* p, int64_t per) { return reinterpret_cast<float*>(reinterpret_cast<char*>(p) + b0 * per * esz); };
  const float* ref = fbank + (int64_t)b0 * Tf * kF;
  const int64_t map = (int64_t)kF * Tf * base;
  float* const bufs[3] = {sl(buf_[0], map), sl(buf_[1], map), sl(buf_[2], map)};
  const int T4 = out_frames(Tf);
  float* const out = sl(out_, (int64_t)T4 * C4);
  ResBlockIO io;
  if (spec_.simam) {
    io.simam_partial = simam_partial_ + b0 * partial_per_win_;
    io.simam_stat = simam_stat_ + b0 * stat_per_win_;
  }
  // stem: conv1 (1 -> base, 3x3, pad 1) + bn1 + relu, fbank (B, T, 80) -> NHWC (B, 80, T, base)
  fcm_conv1(ref, B, Tf, kF, stem_.pre_s, stem_.alpha, stem_.beta, bufs[0], bf, st, base);
  float* cur = bufs[0];
  int H = kF, W = Tf;
  for (size_t i = 0; i < blocks_.size(); ++i) {
    const ResBlockL& rb = blocks_[i];
    // conv1 + bn1 + relu (+ the opener's shortcut conv + BN from the same staged pixels)
    auto conv1 = [&](const ConvGemmArgs& p, float* t2) {
      const bool k1 = bf && res_conv_supported(p);
      ResFuse fu;
      if (rb.has_sc && k1) {
        fu.sc_w = rb.sc.w.w; fu.sc_alpha = rb.sc.alpha; fu.sc_beta = rb.sc.beta; fu.sc_out = t2;
      }
      if (k1) res_conv3x3(p, fu, st);
      else conv_gemm(p, bf, st);
      return k1;
    };
    // conv2 + bn2 (+ residual + relu on a plain block)
    auto conv2 = [&](ConvGemmArgs& r) {
      if (bf && res_conv_supported(r)) res_conv3x3(r, ResFuse{}, st);
      else conv_gemm(r, bf, st);
    };
    if (i + 1 == blocks_.size()) {
      // the stage-4 map leaves as (B, T', C * F') with channel c * F' + f
      SD_CHECK(rb.stride == 1 && H * rb.c2.w.N == C4 && W == T4, kErrShape, "ResNet34 output map mismatch");
      io.out = out;
      io.o_sb = (int64_t)T4 * C4; io.o_sh = 1; io.o_sw = C4; io.o_sn = H;
    }
    cur = run_res_block(rb, bufs, cur, bf, B, H, W, rb.stride, conv1, conv2, st, io);
  }
  return Tens{out, bf};
}

}  // namespace sd
