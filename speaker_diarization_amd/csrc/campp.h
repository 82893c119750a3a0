// CAM++ (egs/alimeeting/ts_vad2/cam_pplus_wespeaker.py) on gfx950.
//
// CamTrunk is the FCM head + xvector up to transit3 (cam_pplus_wespeaker.py:271-372),
// shared by the TS-VAD speech encoder (get_time_out=True, model.py:385-395) and the
// target-speaker embedding extractor CamppModel (get_time_out=False: out_nonlinear ->
// StatsPool -> DenseLayer(batchnorm_), :374-399), which produces the (n_chunks, 192)
// embeddings generate_chunk_speaker_embedding_from_modelscope_for_diarization.py:271-304
// writes and ts_vad_dataset.py:494-537 reads back.
#pragma once
#include <functional>
#include <string>
#include <vector>
#include "encoder.h"

namespace sd {

struct DenseL {
  ConvL bottleneck;       // nonlinear1 (prologue) -> linear1 (1x1) -> nonlinear2 (epilogue, relu)
  ConvL local;            // cam_layer.linear_local (k3, dilation)
  int dil = 1;
  const float *c1w = nullptr, *c1b = nullptr, *c2w = nullptr, *c2b = nullptr;
  int c1 = 0, c2 = 0;
};

// 1-D conv (channel-last rows of stride lda) as an implicit GEMM; out row stride ldo.
ConvGemmArgs cam_conv1d(Tens in, int B, int T, int lda, const ConvL& L, int stride, int pad, int dil, Tens out,
                        int ldo);
// TS-VAD's output layer: fc over the rows (b, t) of x (B, T, lda) fp32, written as logits (B, NS, T).
ConvGemmArgs logits_fc(float* x, int B, int T, int lda, const ConvL& fc, int NS, float* logits);
// 2-D conv on an NHWC map (C = L.w.Cin) as an implicit GEMM -> NHWC out.
ConvGemmArgs conv2d(Tens in, int B, int H, int W, const ConvL& L, int sh, int sw, int ph, int pw, Tens out);
// Conv weight + optional folded BatchNorm (alpha/beta epilogue) + optional conv bias.
ConvL load_conv_bn(ParamStore& ps, DeviceArena& arena, bool bf16, const std::string& wname,
                   const std::string& bn, const std::string& bias = "");

// BasicResBlock of the CAM++ FCM head (cam_pplus_wespeaker.py:236-268), of the ResNet34 trunk
// (resnet_wespeaker.py:35-67) and, with `simam`, of SimAM-ResNet34 (samresnet_wespeaker.py:21-70): conv3x3 + BN +
// ReLU, conv3x3 + BN [SimAM gate], + (1x1 conv + BN shortcut | input), ReLU.
struct ResBlockL {
  ConvL c1, c2, sc;
  bool has_sc = false;
  int stride = 1;
  bool simam = false;
};
// Reads `p`{conv1.weight, bn1, conv2.weight, bn2} and, with has_sc, `p`{<sc_key>.0.weight, <sc_key>.1}.
ResBlockL load_res_block(ParamStore& ps, DeviceArena& arena, bool bf16, const std::string& p, int stride, bool has_sc,
                         const std::string& sc_key = "shortcut");
// Where a block's output goes instead of a rotating buffer: element strides of (b, h, w, c); the map's type follows
// the trunk's precision.  simam_partial / simam_stat: the SimAM blocks' scratch (SimamArgs), unused by plain blocks.
struct ResBlockIO {
  float* out = nullptr;
  int64_t o_sb = 0, o_sh = 0, o_sw = 0, o_sn = 1;
  void *simam_partial = nullptr, *simam_stat = nullptr;
};
// One block over the (B, H, W, C) map in `cur`, one of the three rotating buffers; H / W become the output map's
// and the buffer that holds it is returned (io.out when that is set).  sw: conv1's and the shortcut's stride along W
// (rb.stride along H).  The trunk chooses the kernels: conv1(p, t2) launches conv1 + BN + ReLU and returns whether it
// also wrote the shortcut branch to t2 (else conv_gemm computes it); conv2(r) launches conv2 + BN and r's epilogue:
// + residual + ReLU, or for a SimAM block nothing (the gate, the residual and the ReLU follow in simam_gate).
float* run_res_block(const ResBlockL& rb, float* const bufs[3], float* cur, bool bf, int B, int& H, int& W, int sw,
                     const std::function<bool(const ConvGemmArgs& p, float* t2)>& conv1,
                     const std::function<void(ConvGemmArgs& r)>& conv2, hipStream_t st,
                     const ResBlockIO& io = ResBlockIO());

// One BasicResBlock of the CAM++ FCM head as its two launches (the path beside conv_fcm_block, and what
// sd_op_fcm_block's fused = 0 runs).  stem.fbank set (layer1.0): the block's input is the FCM stem of that fbank.
float* fcm_block_pair(const ResBlockL& rb, float* const bufs[3], float* cur, bool bf, int B, int& H, int& W,
                      const FcmFuse& stem, hipStream_t st);

class CamTrunk {
 public:
  static constexpr int kChannels = 512;   // transit3 output width
  // Reads `prefix`head.* and `prefix`xvector.{tdnn,block*,transit*,out_nonlinear}.*.
  void load(ParamStore& ps, DeviceArena& arena, const std::string& prefix, bool bf16);
  void alloc(DeviceArena& arena, int max_batch, int max_frames);
  static int out_frames(int Tf) { return (Tf - 1) / 2 + 1; }
  // fbank (B, Tf, 80) fp32 -> transit3 output (B, out_frames(Tf), 512), before out_nonlinear.
  // b0: the call covers windows [b0, b0 + B) of a batch (fbank = the batch's base; the result points at
  // window b0 of the batch's output map, the slice this call filled in), so disjoint slices may run on different streams.
  Tens forward(const float* fbank, int B, int Tf, hipStream_t st, int b0 = 0) const;
  // Folded out_nonlinear BatchNorm (the ReLU follows it).
  const float* out_s() const { return out_s_; }
  const float* out_h() const { return out_h_; }
  bool bf16() const { return bf16_; }
  // kErrHip if a cam_dense launch of an earlier forward lost a split item's exchange (its outputs are NaN;
  // cannot happen by construction, reported instead of hanging the GPU)
  void raise_if_set() const {
    err_.raise_if_set("cam_dense: the two parts of a split item lost their exchange (outputs poisoned with NaN)");
  }

 private:
  float* ws(DeviceArena& a, size_t n) { return static_cast<float*>(a.alloc(n * sizeof(float))); }
  bool bf16_ = false;
  ConvL fcm_conv1_;  // fp32 3x3 Cin=1 weights (32x9) + folded bn
  std::vector<ResBlockL> fcm_blocks_;
  ConvL fcm_conv2_;
  ConvL tdnn_;
  std::vector<std::vector<DenseL>> dense_;
  std::vector<ConvL> transit_;
  const float *out_s_ = nullptr, *out_h_ = nullptr;
  // Workspace.
  float *fcmA_ = nullptr, *fcmB_ = nullptr, *fcmC_ = nullptr, *x0_ = nullptr;
  float *d_[3] = {nullptr, nullptr, nullptr}, *x4_ = nullptr, *tmp_ = nullptr, *gate_ = nullptr;
  void* dense_rec_ = nullptr;          // cam_dense exchange records, one per window
  unsigned* dense_cnt_ = nullptr;      // cam_dense counters, one set per window (zeroed once)
  mutable PinnedFlags err_;            // cam_dense's sticky lost-exchange report (slot 0)
};

struct CamppConfig {
  int feat_dim = 80;
  int embedding_size = 192;
  int max_batch = 96;        // extract_embed batch_size default (generate_chunk_...py:45)
  int max_frames = 598;      // 6 s chunks: 1 + (96000 - 400) / 160
  bool bf16 = false;
};

class CamppModel : public ModelCore {
 public:
  explicit CamppModel(const CamppConfig& c) : cfg_(c) {}
  // fbank (B, Tf, 80) -> emb (B, embedding_size) (forward(x), :388-399) and/or
  // time_out (B, T', 512) channel-last = relu(out_nonlinear(x)) (forward(x, get_time_out=True)).
  void forward(const float* fbank, int B, int Tf, float* emb, float* time_out, hipStream_t st);

 private:
  void build() override;
  CamppConfig cfg_;
  CamTrunk trunk_;
  ConvL dense_;            // xvector.dense: Conv1d(1024 -> E, 1, bias=False) + BatchNorm1d(affine=False)
  float* stats_ = nullptr; // (max_batch, 1024) [mean | std]
};

}  // namespace sd
