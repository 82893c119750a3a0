// 3D-Speaker ERes2NetV2 target-speaker embedding extractor (egs/alimeeting/ts_vad2/ERes2NetV2.py:162-255, fusion.py,
// pooling_layers_3d_speaker.py:40-57) on gfx950: ERes2NetV2(feat_dim 80, embedding_size, m_channels 64, baseWidth, scale,
// expansion, pooling_func "TSTP", two_emb_layer False), the model generate_chunk_speaker_embedding_from_modelscope_for_
// diarization.py:110-136 builds for iic/speech_eres2netv2w24s4ep4_sv_zh-cn_16k-common (24, 4, 4) and the class
// egs/magicdata-ramc/ots_vad/model.py:496-534 builds at its defaults (26, 2, 2).
//
// ERes2Trunk: stem conv 1 -> 64 + BN + ReLU on the (80, T) map, then Res2Net blocks [3, 4, 6, 3] at planes 64 .. 512,
// stages 2-4 opening with a stride-2 1x1 conv1 and shortcut.  Maps are NHWC (B, F, T, C), bf16 in bf16 mode.  Inside a
// block the `scale` slices of width floor(planes baseWidth / 64) are each padded to a multiple of 32 channels (zero rows
// in conv1 / the slice convs / AFF, zero columns in conv3; the pad channels are exactly zero through the clamp), so
// every slice is 16-byte aligned and conv_gemm's multi-tap form applies in fp32.  bf16: 1x1 convs on conv_gemm with the
// clamp epilogue, slice convs on res2_conv3x3, AFF on aff_gate.  fp32 / bf16x3: conv_gemm throughout plus the fp32
// element-wise kernels.  The pooled head (fuse34's blend, TSTP, seg_1) is fp32 in both precisions.
#pragma once
#include <string>
#include <vector>
#include "campp.h"

namespace sd {

struct ERes2NetV2Config {
  int feat_dim = 80;
  int embedding_size = 192;
  int m_channels = 64;
  int base_width = 26, scale = 2, expansion = 2;   // (26, 2, 2) or (24, 4, 4)
  int max_batch = 96;        // extract_embed batch_size default (generate_chunk_...modelscope...py:45)
  int max_frames = 598;      // 6 s chunks: 1 + (96000 - 400) / 160
  bool bf16 = false;         // bf16 trunk (maps and conv operands); the blend, TSTP and seg_1 stay fp32
};

struct AffL {      // device images of aff_pack
  const float *w1 = nullptr, *a1 = nullptr, *c1 = nullptr, *w2 = nullptr, *a2 = nullptr, *c2 = nullptr;
  int I = 0;
};

struct Res2BlockL {
  ConvL c1, c3, sc;
  std::vector<ConvL> convs;   // padded (wp, wp, 3, 3) + folded bns.i
  std::vector<AffL> aff;      // stages 3-4: fuse_models.j
  bool has_sc = false;
  int stride = 1, width = 0, wp = 0, planes_out = 0;
};

class ERes2Trunk {
 public:
  void load(ParamStore& ps, DeviceArena& arena, bool bf16, int base_width, int scale, int expansion);
  void alloc(DeviceArena& arena, int max_batch, int max_frames);
  static int down(int n) { return (n - 1) / 2 + 1; }
  static int frames25(int Tf) { return down(down(Tf)); }
  static int out_frames(int Tf) { return down(down(down(Tf))); }
  int c3() const { return 256 * expansion_; }   // out3 channels (20 frequency rows)
  int c4() const { return 512 * expansion_; }   // out4 / fuse34 channels (10 frequency rows)
  static constexpr int kMinRows = 17;   // fuse34's GEMMs run on at least this many rows (never conv_gemm's skinny form)
  // fbank (B, Tf, 80) fp32 -> out3 NHWC (B, 20, T3, c3()) and the `cat` map NHWC (B, 10, T4, 2 c4()): channels
  // [0, c4()) = out4, [c4(), 2 c4()) = layer3_ds(out3) (ERes2NetV2.py:239-244).  No allocation or synchronisation.
  void forward(const float* fbank, int B, int Tf, hipStream_t st) const;
  Tens out3() const { return Tens{out3_, bf16_}; }
  Tens cat() const { return Tens{cat_, bf16_}; }
  bool bf16() const { return bf16_; }

 private:
  void run_block(const Res2BlockL& rb, const float* cur, int B, int& H, int& W, float* out, int64_t o_ld,
                 hipStream_t st) const;
  bool bf16_ = false;
  int scale_ = 2, expansion_ = 2;
  ConvL stem_;
  std::vector<Res2BlockL> blocks_;
  ConvL ds_;   // layer3_ds
  float *io_[2] = {nullptr, nullptr}, *r_ = nullptr, *u_ = nullptr, *v_ = nullptr, *out3_ = nullptr, *cat_ = nullptr;
};

class ERes2NetV2Model : public ModelCore {
 public:
  static constexpr int kMinFrames = 8;
  explicit ERes2NetV2Model(const ERes2NetV2Config& c) : cfg_(c) {}
  // fbank (B, Tf, 80) -> emb (B, E) (forward, :236-255); frame_out (B, T', 10 c4) channel-last fp32 = the fuse34 map
  // as get_frame_level_feat orders it (ots_vad ERes2NetV2.py:253-258: transpose(1, 3) then flatten), channel f * c4 + c;
  // frame25_out (B, T3, 20 c3) = out3 (get_frame_level_feat_frame_rate25, :259-272), channel f * c3 + c.  Each
  // nullable.  T' == 1 (Tf == 8) gives NaN stds and an all-NaN embedding like the reference.  Tf < 8 raises kErrShape.
  void forward(const float* fbank, int B, int Tf, float* emb, float* frame_out, float* frame25_out, hipStream_t st);

 private:
  void build() override;
  ERes2NetV2Config cfg_;
  ERes2Trunk trunk_;
  ConvL f1_, f2_;   // fuse34.local_att.{0 + 1, 3 + 4}
  ConvL seg1_;
  float *h_ = nullptr, *att_ = nullptr, *fuse_ = nullptr, *stats_ = nullptr;
};

}  // namespace sd
