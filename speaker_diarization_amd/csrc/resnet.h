// WeSpeaker ResNet34 speech encoder (egs/alimeeting/ts_vad2/resnet_wespeaker.py:35-67, 108-171, 198-208) on
// gfx950: the TS-VAD speech encoder of speech_encoder_type "resnet34_wespeaker" (model.py:584-606), i.e.
// ResNet34(feat_dim 80, speech_encoder=True).forward(x, get_time_out=True); and, by ResTrunkSpec, the front of
// SimAM_ResNet34_ASP (samresnet_wespeaker.py:21-127).
//
// ResTrunk mirrors CamTrunk's interface.  Stem conv 1 -> base + BN + ReLU on the (80, T) map, then BasicBlocks
// [3, 4, 6, 3] at base x {1, 2, 4, 8} channels, stages 2-4 opening with stride 2 in both axes and a 1x1 stride-2
// shortcut; every BatchNorm2d is folded into its conv's alpha / beta.  Maps are NHWC (B, F, T, C), bf16 in bf16
// mode.  bf16: res_conv.hip (the shortcut fused into the opener's conv1), fcm_conv.hip's kernels for the 32 -> 32
// stride-1 convs; fp32 / bf16x3: conv_gemm.  SimAM blocks run conv2 with bn2 alone and close with simam.hip.
#pragma once
#include <string>
#include <vector>
#include "campp.h"

namespace sd {

// What distinguishes the trunks built on these blocks.  ResNet34 (the default): base 32, `shortcut.{0,1}` keys, plain
// BasicBlocks.  SimAM-ResNet34: base 64, `downsample.{0,1}` keys, the SimAM gate between bn2 and the residual sum.
struct ResTrunkSpec {
  int base = 32;                       // 32 | 64: channels of the stem and of stage 1
  const char* sc_key = "shortcut";     // key of the opener's 1x1 conv + BN pair
  bool simam = false;                  // block epilogue: plain | SimAM
};

class ResTrunk {
 public:
  static constexpr int kChannels = 2560;   // ResNet34 (base 32): 256 channels x 10 frequency rows, channel c * 10 + f
  // Reads `prefix`{conv1, bn1, layer1..4.*}.
  void load(ParamStore& ps, DeviceArena& arena, const std::string& prefix, bool bf16,
            const ResTrunkSpec& spec = ResTrunkSpec());
  void alloc(DeviceArena& arena, int max_batch, int max_frames);
  static int down(int n) { return (n - 1) / 2 + 1; }
  static int out_frames(int Tf) { return down(down(down(Tf))); }
  int channels() const { return spec_.base * 80; }   // 8 base channels x 10 frequency rows
  // fbank (B, Tf, 80) fp32 -> stage-4 map channel-last (B, out_frames(Tf), channels()), the channel axis ordered
  // c * 10 + f as out.reshape(B, C * F, T) (resnet_wespeaker.py:168; pooling_layers_wespeaker.py:162).  b0: the call
  // covers windows [b0, b0 + B) of a batch (fbank = the batch's base; the result is the batch's output map with this
  // slice filled in), so disjoint slices may run on different streams.  No allocation or synchronisation inside.
  Tens forward(const float* fbank, int B, int Tf, hipStream_t st, int b0 = 0) const;
  bool bf16() const { return bf16_; }

 private:
  bool bf16_ = false;
  ResTrunkSpec spec_;
  ConvL stem_;   // raw base x 9 fp32 weights (pre_s) + folded bn1 for the direct stem kernel
  std::vector<ResBlockL> blocks_;
  float *buf_[3] = {nullptr, nullptr, nullptr}, *out_ = nullptr;
  // SimAM scratch (simam.hip), per window: tile partials of the largest map, and (mean, scale) per channel
  char *simam_partial_ = nullptr, *simam_stat_ = nullptr;
  size_t partial_per_win_ = 0, stat_per_win_ = 0;
};

}  // namespace sd
