// Launchers for the gfx950 kernels (internal C++ API; the C-ABI is in capi.cpp).
#pragma once
#include <type_traits>
#include <vector>
#include "common.h"

namespace sd {

// ---------------------------------------------------------------- conv_gemm
struct ConvGemmArgs {
  // Input activation, channel-last: element (b, h, w, c) at
  // A[((b*H + h)*W + w)*lda + a_coff + c]; fp32, or bf16 when a_bf16.
  const void* A = nullptr;
  bool a_bf16 = false;
  int B = 1, H = 1, W = 1, Cin = 0, lda = 0, a_coff = 0;
  // A (bf16, lda == K, M % 16 == 0) in the row programs' tiled fragment layout (RowProgArgs::a_tiled): only the
  // register-A GEMM takes it (conv_gemm refuses it otherwise)
  int a_tiled = 0;
  int Ho = 1, Wo = 1;
  int kh = 1, kw = 1, sh = 1, sw = 1, ph = 0, pw = 0, dh = 1, dw = 1;
  // Packed weights Wt[N][K] (bf16 bits or fp32), K = kh*kw*Cin, tap-major.
  const void* Wt = nullptr;
  int N = 0, K = 0;
  const float* pre_scale = nullptr;  // per input channel; a' = relu(a*s + h)
  const float* pre_shift = nullptr;
  const float* alpha = nullptr;      // per output channel scale
  const float* beta = nullptr;       // per output channel shift
  const void* res = nullptr;         // residual at the output's (m, n) address map, stride res_ld
  bool res_bf16 = false;
  int res_ld = 0;
  int act = kActNone;
  // Post-activation affine per output channel, v = act(v) * post_scale[n] + post_shift[n]: a BatchNorm that FOLLOWS
  // the ReLU (ECAPA's Conv1dReluBn).  Null (the default): off.  On the exact / bf16x3 kernels, the ring GEMM (N > 128)
  // and the register-staged bf16 kernel; conv_gemm selects one of these (the other bf16 paths do not read it).
  const float* post_scale = nullptr;
  const float* post_shift = nullptr;
  const float* gate = nullptr;       // gate[(b*gate_nseg + wo/gate_seg)*N + n]
  int gate_seg = 1, gate_nseg = 1;
  void* out = nullptr;               // out[b*o_sb + ho*o_sh + wo*o_sw + n*o_sn]
  bool out_bf16 = false;
  int64_t o_sb = 0, o_sh = 0, o_sw = 0, o_sn = 1;
  // GLU epilogue (streaming path only): the N GEMM columns are 32-wide groups [a 16 | gate 16]
  // (weights permuted by glu_interleave_rows); output channel g*16 + j = a * sigmoid(gate), N/2 wide.
  int glu = 0;
  // Skinny path only (gemm_skinny_supported; streaming FS-EEND).  LayerNorm prologue: the staged
  // A rows are LN(ln_x + ln_t)*ln_g + ln_b over K (ln_x fp32 rows of K, ln_t fp32/bf16 or null);
  // workgroup 0 also stores them to ln_out (the next residual stream; must not alias ln_x).
  const float* ln_x = nullptr;
  const void* ln_t = nullptr;
  bool ln_t_bf16 = false;
  const float* ln_g = nullptr;
  const float* ln_b = nullptr;
  float ln_eps = 1e-5f;
  float* ln_out = nullptr;
  // Other skinny-only A prologues (pro_mode; ln_g unset):
  //   1  rows of ln_x (fp32, K wide, K <= 512) scaled to unit L2 norm with row_l2norm's arithmetic;
  //      workgroup 0 stores them to ln_out
  //   2  row r of A = ln_x[r / pro_C] + pro_p[r % pro_C] (slot_init's sum); workgroup 0 stores them to ln_out
  //   3  the staged span (the rows a stride-1 1-D conv reads) = rows [*pro_cursor - pro_pad, ...) of ln_x
  //      (row stride lda), zero outside [0, *pro_nvalid) (gather_window's window; p.A unused)
  int pro_mode = 0;
  const float* pro_p = nullptr;
  int pro_C = 1, pro_pad = 0;
  const int* pro_cursor = nullptr;
  const int* pro_nvalid = nullptr;
  // K/V history epilogue: columns n >= kv_col0 are also stored (out dtype) at
  // kv_out[(*kv_cursor * kv_mult + m) * kv_ld + n - kv_col0].
  void* kv_out = nullptr;
  const int* kv_cursor = nullptr;
  int kv_mult = 1, kv_col0 = 0;
  int64_t kv_ld = 0;
  // Split-K (gemm_dma path only, via conv_gemm_splitk): blockIdx.y = split z sums k-tiles of its share of
  // K into fp32 slab z at out + z * split_stride (bias in slab 0 only; no act / alpha / residual).
  int ksplit = 1;
  int64_t split_stride = 0;
};
// Row order of a GLU projection (2C, K) -> groups of [16 value rows | their 16 gate rows].
inline int glu_interleave_row(int r, int C) {   // new row index of original row r
  const bool gate = r >= C;
  const int c = gate ? r - C : r;
  return (c / 16) * 32 + (gate ? 16 : 0) + c % 16;
}
void conv_gemm(const ConvGemmArgs& p, bool bf16, hipStream_t st);
// Arithmetic of conv_gemm's exact (non-bf16) path on this host thread: false = the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32); true = "bf16x3": each fp32 operand split into bf16 hi + lo, acc += hi·hi + hi·lo +
// lo·hi on v_mfma_f32_16x16x32_bf16 (fp32 accumulate; ~2^-16 relative per product, 5.3x the f32 MFMA rate).
// Handles created with precision 2 set it around their compute calls (capi.cpp, GemmX3Scope).
bool gemm_x3();
struct GemmX3Scope {
  explicit GemmX3Scope(bool on);
  ~GemmX3Scope();
  bool prev;
};
void conv_gemm_bf16(const ConvGemmArgs& p, hipStream_t st);   // bf16-MFMA production kernel
// Measurement only (tools/eres2net_probe.py, sd_debug_clamp_route): which bf16 kernel serves act == kActClamp20.  0: the
// shipped rule (the LDS-DMA kernel where gemm_dma_supported, else the register-staged one); 1: always the latter.
void clamp_route_debug(int route);
bool gemm_dma_supported(const ConvGemmArgs& p);               // bf16 A, no prologue, taps==1 or Cin%64==0
// Split-K: the split count worth using for p on the gemm_dma path (1 = none), and the launch writing
// ksplit fp32 row-major (M x N) slabs to `slabs` (the consumer sums them, e.g. add_layernorm's t_slabs).
int gemm_splitk_count(const ConvGemmArgs& p);
void conv_gemm_splitk(const ConvGemmArgs& p, int ksplit, float* slabs, hipStream_t st);
bool gemm_ring_supported(const ConvGemmArgs& p);             // bf16 A/out, taps==1, K<=1024, N>=96, tall M
void conv_gemm_ring(const ConvGemmArgs& p, hipStream_t st);
bool gemm_stream_supported(const ConvGemmArgs& p);            // bf16 A linear, K%64==0, K<=768, no res
void conv_gemm_stream(const ConvGemmArgs& p, hipStream_t st);
bool fcm_conv_supported(const ConvGemmArgs& p);               // bf16 3x3 32->32, pad 1, freq stride 1|2
void conv_fcm3x3(const ConvGemmArgs& p, hipStream_t st);
// CAM++ BasicResBlock entry conv (3x3, freq stride 2, bf16 NHWC out) with the block's 1x1 shortcut as a
// second output and/or the FCM stem (head.conv1 + BN + ReLU of the fbank) computed in LDS instead of
// read from HBM (p.A unused then; p.H = fb_F = 80, p.W = frames).
struct FcmFuse {
  const void* sc_w = nullptr;                 // packed bf16 Wt[32][32]
  const float *sc_alpha = nullptr, *sc_beta = nullptr;
  void* sc_out = nullptr;                     // bf16 NHWC (B, Ho, Wo, 32)
  const float* fbank = nullptr;               // (B, W, fb_F) fp32
  int fb_F = 0;
  const float *stem_w = nullptr, *stem_alpha = nullptr, *stem_beta = nullptr;   // 32x9 raw, folded BN
};
bool fcm_fused_supported(const ConvGemmArgs& p, const FcmFuse& f);
void conv_fcm3x3_fused(const ConvGemmArgs& p, const FcmFuse& f, hipStream_t st);
// One whole CAM++ FCM BasicResBlock (cam_pplus_wespeaker.py:240-268) in one launch (fcm_conv.hip, fcm_block_kernel):
// out = relu(bn2(conv2(relu(bn1(conv1(x))))) + (x | bn_sc(conv1x1_sc(x)))) on bf16 NHWC maps of C = 32 channels,
// 3x3 pad 1, freq stride 1 (identity residual) or 2 (1x1 stride-2 shortcut; wsc set).  The intermediate map and the
// shortcut stay in LDS; the arithmetic is that of the two launches (conv_fcm3x3[_fused]), value for value.  w1 / w2:
// packed bf16 Wt[32][288], wsc: packed bf16 Wt[32][32]; a* / b*: folded BN per channel.  out must not overlap x.
struct FcmBlockArgs {
  const void* x = nullptr;
  int B = 0, H = 0, W = 0, C = 32, stride = 1;
  bool bf16 = true;
  const void *w1 = nullptr, *w2 = nullptr, *wsc = nullptr;
  const float *a1 = nullptr, *b1 = nullptr, *a2 = nullptr, *b2 = nullptr, *asc = nullptr, *bsc = nullptr;
  void* out = nullptr;   // (B, (H - 1) / stride + 1, W, 32)
};
bool fcm_block_supported(const FcmBlockArgs& a);   // false: fp32 maps, C != 32, a map of 2 GiB or more
bool fcm_block_enabled();                          // false with SDIAR_NO_FCM_BLOCK set (read once): the two launches
void conv_fcm_block(const FcmBlockArgs& a, hipStream_t st);
// CAM++ FCM layer1.0 in one launch (fcm_conv.hip, fcm_stem_block_kernel): the stem (head.conv1 1 -> 32, 3x3, pad 1,
// + BN + ReLU) of the fbank (B, W, F) fp32, computed in LDS, then the strided BasicResBlock with its 1x1 shortcut as
// in FcmBlockArgs (stride 2); out is bf16 NHWC (B, (F - 1) / 2 + 1, W, 32).  The arithmetic is that of the block's two
// launches with the stem-fused conv1 (conv_fcm3x3_fused + conv_fcm3x3), value for value, and it is supported exactly
// where that conv1 is (fcm_fused_supported with the fbank and the shortcut: W >= 113, a stem map under 2 GiB).
struct FcmStemBlockArgs {
  const float* fbank = nullptr;
  int B = 0, W = 0, F = 0;
  const float *stem_w = nullptr, *stem_alpha = nullptr, *stem_beta = nullptr;   // 32x9 raw, folded BN
  const void *w1 = nullptr, *w2 = nullptr, *wsc = nullptr;
  const float *a1 = nullptr, *b1 = nullptr, *a2 = nullptr, *b2 = nullptr, *asc = nullptr, *bsc = nullptr;
  void* out = nullptr;
};
bool fcm_stem_block_supported(const FcmStemBlockArgs& a);
void conv_fcm_stem_block(const FcmStemBlockArgs& a, hipStream_t st);   // CamTrunk::forward: under fcm_block_enabled()
// ResNet34 trunk 3x3 convs (res_conv.hip): bf16 NHWC in, pad 1, stride 1 or 2 in BOTH axes, Cin / Cout in
// {32, 64, 128, 256, 512}, folded BN + optional bf16 residual + ReLU (NaN kept), bf16 out (NHWC as 16-B stores, or any
// o_s* strides per element).  ResFuse: the block's 1x1 shortcut at the same stride (+ its BN, no ReLU) from the
// centre tap's staged pixels, stored NHWC to sc_out.
struct ResFuse {
  const void* sc_w = nullptr;                 // packed bf16 Wt[Cout][Cin]
  const float *sc_alpha = nullptr, *sc_beta = nullptr;
  void* sc_out = nullptr;                     // bf16 NHWC (B, Ho, Wo, Cout)
};
bool res_conv_runs(const ConvGemmArgs& p);        // the kernel can compute p
bool res_conv_supported(const ConvGemmArgs& p);   // ... and measured faster than conv_gemm on p's shape class
void res_conv3x3(const ConvGemmArgs& p, const ResFuse& f, hipStream_t st);
void conv_gemm_dma(const ConvGemmArgs& p, hipStream_t st);     // LDS-DMA fed variant
bool gemm_areg_supported(const ConvGemmArgs& p);             // bf16 A linear, K in {192,256,384}, N % 64 == 0, N >= 768
void conv_gemm_areg(const ConvGemmArgs& p, hipStream_t st);
bool gemm_skinny_supported(const ConvGemmArgs& p);            // <= 16 rows, linear or stride-1 1-D conv
void conv_gemm_skinny(const ConvGemmArgs& p, bool w_bf16, hipStream_t st);

// Output row (b, ho, wo) sits at linear row m = (b*Ho + ho)*Wo + wo, stride o_sw
// (strides of size-1 dimensions do not matter).
__host__ __device__ inline bool out_rows_linear(const ConvGemmArgs& p) {
  return (p.Ho == 1 || p.o_sh == (int64_t)p.Wo * p.o_sw) && (p.B == 1 || p.o_sb == (int64_t)p.Ho * p.Wo * p.o_sw);
}
// A 1x1 conv whose input row m is output row m (stride 1, no padding): a plain GEMM on A.
inline bool a_rows_linear(const ConvGemmArgs& p) {
  return p.kh * p.kw == 1 && p.sh == 1 && p.sw == 1 && p.ph == 0 && p.pw == 0 && p.H == p.Ho && p.W == p.Wo;
}

// Plain row-major linear layer helper: out[m*ldo + o_coff + n] = act(A[m*lda+k]·W[n][k] * alpha + beta (+res)).
ConvGemmArgs linear_args(const void* A, int M, int K, int lda, const void* Wt, int N,
                         void* out, int ldo);

// ---------------------------------------------------------------- fcm / cam++
// First FCM conv (Cin = 1, 3x3, pad 1) + folded BN + ReLU.  fbank (B, T, F) ->
// NHWC (B, F, T, C), C = 32 (cam_pplus_wespeaker.py:277-301, the ResNet34 stem) or 64 (the SimAM-ResNet34 stem,
// samresnet_wespeaker.py:82-85, 118).
void fcm_conv1(const float* fbank, int B, int T, int F, const float* w /*Cx9*/,
               const float* alpha, const float* beta, void* out, bool out_bf16, hipStream_t st, int C = 32);

// CAMLayer context gate (cam_pplus_wespeaker.py:106-123):
// ctx[b,s,c] = mean_t x[b,t,c] + mean_{t in seg s} x[b,t,c];
// gate[b,s,:] = sigmoid(W2·relu(W1·ctx + b1) + b2).
void cam_context(const void* x, bool x_bf16, int B, int T, int C, int ldx, int seg_len,
                 const float* w1, const float* b1, int C1, const float* w2, const float* b2,
                 int C2, float* gate, hipStream_t st);
// CAM++ dense-layer tail fused (cam_fused.hip): context gate + linear_local k3 conv + gating
// for one bf16 bottleneck map x (B, T, 128) -> out (B, T, 32) at row stride ldo (bf16).
// One CAM++ dense layer (bottleneck BN-ReLU-1x1-BN-ReLU, CAMLayer context gate, k-3 local conv x gate) in
// one launch, h kept in LDS (cam_dense.hip); x: (B, T, ld) bf16 map whose channels [0, cin) are the
// input, out: its channel slice at cin.  bf16, T <= 320.  Items of more than 160 frames run as two
// workgroups that meet through `records` (cam_dense_record_bytes(B), 16-B aligned) and `counters`
// (cam_dense_counter_bytes(B), zeroed ONCE when allocated, then owned by the launches: never shared by
// launches that may run concurrently).
bool cam_dense_supported(int T, int cin, int ld, int bn, int C1, int C2, int N, int taps, int dil, int seg_len,
                         bool bf16);
size_t cam_dense_record_bytes(int B);
void cam_dense_set_probe(void* stamps);
void rowprog_set_probe(void* stamps);
// Graph-replay diagnostic (diag.hip): [memset(X, 0) -> kernel Y = X; X = 7] replayed `replays` times;
// bad_per_replay[r] = non-zero Y values after replay r (host array).
void graph_memset_probe(int n, int replays, bool fork, int* bad_per_replay, hipStream_t st);   // test-only phase stamps ([grid][16] u64), null = off
size_t cam_dense_counter_bytes(int B);
void cam_dense(const void* x, int B, int T, int ld, int cin, int dil, const float* s1, const float* h1,
               const void* wb, const float* a2, const float* b2, const void* wl, const float* bl, const float* w1,
               const float* c1, const float* w2, const float* c2, void* out, void* records, unsigned* counters,
               hipStream_t st, int* err = nullptr);   // err: device address of a PinnedFlags slot (lost exchange)
bool cam_local_fused_supported(int C, int C1, int C2, int N, int taps, int dil, int seg_len, int ldo, bool bf16);
void cam_local_fused(const void* x, int B, int T, int dil, const void* wt, const float* bias, const float* w1,
                     const float* b1, const float* w2, const float* b2, void* out, int ldo, hipStream_t st);
// The conv + gating half alone, gate (B, nseg, 32) from cam_context().
void cam_local_conv(const void* x, int B, int T, int dil, const void* wt, const float* bias, const float* gate,
                    void* out, int ldo, hipStream_t st);
// CAM++ out_nonlinear + StatsPool (cam_pplus_wespeaker.py:28-39, 372-379):
// v = relu(x * s + h) over x (B, T, C) channel-last (C % 64 == 0);
// stats (B, 2C) = [mean_t v | unbiased std_t v] (nullable); tout (B, T, C) = v (nullable).
void stats_pool(const void* x, bool x_bf16, int B, int T, int C, const float* s, const float* h,
                float* stats, float* tout, hipStream_t st);
// ResNet34 TSTP (pooling_layers_wespeaker.py:66-88) over x (B, T, C) channel-last (C % 64 == 0), no BN / ReLU:
// stats (B, 2C) = [mean_t x | sqrt(unbiased var_t x + 1e-7)] (nullable); tout (B, T, C) = x in fp32 (nullable).
// NaN stays in its channel; T == 1 gives NaN stds (tstp_pool.hip).  eps: 1e-7 is WeSpeaker's; 3D-Speaker's TSTP
// (pooling_layers_3d_speaker.py:52) adds 1e-8.
void tstp_pool(const void* x, bool x_bf16, int B, int T, int C, float* stats, float* tout, hipStream_t st,
               double eps = 1e-7);
// y (B, N) = x (B, K) w^T + bias, fp32 FMA with a summation order fixed by K alone (a row's result does not depend
// on B): the ResNet34 head's seg_1 / seg_2 (resnet_wespeaker.py:176-180).  w (N, K) row-major, K % 4 == 0.
void seg_linear(const float* x, int B, int K, const float* w, const float* bias, int N, float* y, hipStream_t st);
// y = x < 0 ? 0 : x over n floats: F.relu that keeps NaN (resnet_wespeaker.py:178).
void relu_keep_nan(const float* x, int64_t n, float* y, hipStream_t st);

// ---------------------------------------------------------------- ecapa-tdnn (ecapa.hip)
// layer1's input rows: out (B, T, 400) = the k5 pad-2 window [t - 2, t + 2] of fbank (B, T, 80), tap-major, zeros
// outside the window's own [0, T) (ecapa_tdnn_wespeaker.py:193-196).
void ecapa_im2col(const float* fbank, int B, int T, void* out, bool out_bf16, hipStream_t st);
// out[r, 0..128) = a[r, 0..128) (+ b[r, 0..128), nullable) over `rows` rows of strides lda / ldb / ldo (elements;
// the pointers already at their channel slice): a Res2 stage's input sp + split_i, or the pass-through group (:66-76).
void ecapa_add_slice(const void* a, int lda, const void* b, int ldb, int64_t rows, void* out, int ldo, bool bf16,
                     hipStream_t st);
// Res2Conv1dReluBn at scale 8 (:30-79): seven 128 -> 128 k3 dilated stages, weights packed Wt[128][tap * 128 + c]
// (bf16 bits or fp32), bias and the folded BatchNorm (s, h) that follows each stage's ReLU.
struct Res2ChainW {
  static constexpr int kStages = 7, kWidth = 128;
  const void* w[kStages] = {};
  const float *bias[kStages] = {}, *s[kStages] = {}, *h[kStages] = {};
};
// The whole chain of a bf16 map x (B, T, 1024) -> out (B, T, 1024) in ONE launch (ecapa.hip): a workgroup owns 64
// output frames of one window, recomputes a halo of 7 * dilation frames per side, keeps every intermediate in LDS and
// holds each stage's weights in registers as MFMA operands.  bf16 weights; dilation 1..4.
bool res2_chain_fused_supported(int dilation);
void res2_chain_fused(const void* x, int B, int T, int dilation, const Res2ChainW& W, void* out, hipStream_t st);
// SE_Connect's gate (:119-123) of y (B, T, 1024): mean (B, 1024) scratch = mean over all T frames (fixed-order fp64
// sums, no atomics), gate (B, 1024) = sigmoid(W2 relu(W1 mean + b1) + b2); both weights transposed, w1t
// (1024, 128) and w2t (128, 1024), fp32.
void ecapa_se_gate(const void* y, bool y_bf16, int B, int T, const float* w1t, const float* b1, const float* w2t,
                   const float* b2, float* mean, float* gate, hipStream_t st);
// out[b, t, c] = x[b, t, c] + y[b, t, c] * gate[b, c], c < 1024 (:124, :158); x / out at row strides ldx / ldo.
void ecapa_se_apply(const void* x, int ldx, const void* y, const float* gate, int B, int T, void* out, int ldo,
                    bool bf16, hipStream_t st);
// ASTP with global_context_att (pooling_layers_wespeaker.py:91-144) over x (B, T, 1536) channel-last:
// stats (B, 3072) = [sum_t a x | sqrt(clamp(sum_t a x^2 - mean^2, 1e-7))], a = softmax_t(W2 tanh(W1 [x | mean |
// std] + b1) + b2).  The context statistics and the weighted sums are fp64, the two GEMMs exact fp32 (bf16x3 under a
// GemmX3Scope) whatever x's type.  T < 2 raises kErrShape (the reference's unbiased variance of one frame is NaN).
struct AstpArgs {
  const void* x = nullptr;
  bool x_bf16 = false;
  int B = 0, T = 0;
  const void* w1x = nullptr;   // packed fp32 [128][1536]: linear1.weight[:, :1536]
  const float* w1c = nullptr;  // (128, 3072) row-major: linear1.weight[:, 1536:]
  const float* b1 = nullptr;
  const void* w2 = nullptr;    // packed fp32 [1536][128]
  const float* b2 = nullptr;
  float* stats = nullptr;      // (B, 3072)
  float *ctx = nullptr, *cv = nullptr;   // scratch (B, 3072), (B, 128)
  float *x32 = nullptr, *h = nullptr, *e = nullptr;   // scratch (B T, 1536) (bf16 x only), (B T, 128), (B T, 1536)
  // channels of x, C % 64 == 0: 1536 (ECAPA) or 1152 (ReDimNetB2); every 1536 / 3072 above scales with it
  int C = 1536;
};
void astp_pool(const AstpArgs& a, hipStream_t st);
// The pooling both attentive heads end with: a = softmax over T of the scores e (B, T, C) fp32, then in fp64 and a
// fixed order stats (B, 2 C) = [m = sum_t a x | sqrt(max(var, clamp))] over x (B, T, C) channel-last, C % 64 == 0.
// ASTP (asp false): var = sum_t a x^2 - m^2, clamp 1e-7.  ASP: var = sum_t a (x - m)^2, clamp the fp32 1e-5; T == 1
// gives weight 1, m = x and the second half sqrt(1e-5) exactly, and a NaN variance stays NaN (torch.clamp keeps it).
void softmax_stats(const void* x, bool x_bf16, const float* e, int B, int T, int C, bool asp, float* stats,
                   hipStream_t st);
// ASP (pooling_layers_wespeaker.py:146-168) over x (B, T, C) channel-last: e = W2 bn(relu(W1 x + b1)) + b2 on the
// exact fp32 GEMM (bf16x3 under a GemmX3Scope) whatever x's type, the BatchNorm1d as the post-activation affine
// (bn_s, bn_h), then softmax_stats with the clamp 1e-5.  Unlike ASTP there is no global context and T == 1 is valid.
struct AspArgs {
  const void* x = nullptr;
  bool x_bf16 = false;
  int B = 0, T = 0, C = 0;
  const void* w1 = nullptr;    // packed fp32 [128][C]: attention.0.weight
  const float* b1 = nullptr;
  const float *bn_s = nullptr, *bn_h = nullptr;   // attention.2 folded
  const void* w2 = nullptr;    // packed fp32 [C][128]: attention.3.weight
  const float* b2 = nullptr;
  float* stats = nullptr;      // (B, 2 C)
  // scratch (B T, C) (bf16 x only), (R, 128), (R, C) with R = max(B T, kAspMinRows)
  float *x32 = nullptr, *h = nullptr, *e = nullptr;
};
constexpr int kAspMinRows = 17;
void asp_pool(const AspArgs& a, hipStream_t st);

// ---------------------------------------------------------------- simam (simam.hip)
// SimAM gate + shortcut + ReLU of a SimAM BasicBlock (samresnet_wespeaker.py:57-70) on an NHWC map y (B, H, W, C),
// bf16 or fp32, C % 64 == 0: out = relu(y * sigmoid((y - mean)^2 / (4 (v + 1e-4)) + 0.5) + res), mean and v = sum (y -
// mean)^2 / (H W - 1) per (b, c) in fp64 and a fixed order (no atomics; an item's result does not depend on the
// batch), NaN kept in its channel.  res: NHWC like y, or null.  out: y's type at element strides o_s* of (b, h, w, c);
// NHWC strides may alias y.  partial: scratch of B * simam_tiles(H W) * C records of (n, mean, M2) doubles (24 bytes),
// item b's records at b times the per-item size; stat: scratch of B * C * 16 bytes.
struct SimamArgs {
  const void* y = nullptr;
  const void* res = nullptr;
  bool bf16 = false;
  int B = 0, H = 0, W = 0, C = 0;
  void* out = nullptr;
  int64_t o_sb = 0, o_sh = 0, o_sw = 0, o_sn = 1;
  void *partial = nullptr, *stat = nullptr;
};
int simam_tiles(int HW);
void simam_gate(const SimamArgs& a, hipStream_t st);

// ---------------------------------------------------------------- eres2net (eres2net.hip)
// The 3x3 slice conv of a Res2Net block (ERes2NetV2.py:73-83, 140-151), bf16 on MFMA: pad 1, stride 1, `width` -> `width`
// channels (even, <= 512) on NHWC maps of B x H x W pixels.  Reads channels [x_coff, x_coff + width) of rows of ldx
// elements, plus (add != null) channels [add_coff, ..) of `add` summed on load in fp32; writes clamp(alpha conv + beta, 0,
// 20) with NaN kept and +inf -> 20 to channels [o_coff, o_coff + width) of rows of ldo elements and touches no other
// channel.  Offsets and row lengths need 4-byte alignment only (16-byte aligned slices load 16 B per lane).  w: bf16
// Wt[Cp][9 * Cp], Cp = res2_padded(width), tap-major like conv_gemm's packing of the zero-padded (Cp, Cp, 3, 3) weight;
// alpha / beta: Cp floats.
struct Res2ConvArgs {
  const void* x = nullptr;
  int ldx = 0, x_coff = 0;
  const void* add = nullptr;
  int ld_add = 0, add_coff = 0;
  int B = 0, H = 0, W = 0, width = 0;
  const void* w = nullptr;
  const float *alpha = nullptr, *beta = nullptr;
  void* out = nullptr;
  int ldo = 0, o_coff = 0;
};
__host__ __device__ inline int res2_padded(int width) { return (width + 31) / 32 * 32; }
bool res2_conv_supported(const Res2ConvArgs& a);
void res2_conv3x3(const Res2ConvArgs& a, hipStream_t st);
// The in-block attentional fusion AFF(channels C, r 4) (fusion.py:10-30) per pixel, one pass: h = SiLU(a1 (W1 [x | y]) +
// c1), att = a2 (W2 h) + c2, out = x (1 + tanh att) + y (1 - tanh att); the two conv biases and eval BatchNorms are
// folded into (a1, c1) and (a2, c2).  x / y / out: C-channel slices (4-byte aligned) of rows of P pixels, bf16 or fp32;
// out may alias x or y.  SiLU, tanh and every sum are fp32.  The weights are aff_pack's images, with Cp == C.
struct AffGateArgs {
  const void* x = nullptr;
  int ldx = 0, x_coff = 0;
  const void* y = nullptr;
  int ldy = 0, y_coff = 0;
  void* out = nullptr;
  int ldo = 0, o_coff = 0;
  bool bf16 = false;
  int64_t P = 0;
  int C = 0, I = 0;
  const float *w1 = nullptr, *a1 = nullptr, *c1 = nullptr, *w2 = nullptr, *a2 = nullptr, *c2 = nullptr;
};
int aff_ipt(int I);   // hidden units per thread: I <= 52 padded to 4 * aff_ipt(I)
struct AffPacked {
  std::vector<float> w1, a1, c1, w2, a2, c2;
};
// Host images of W1 (I, 2 C), W2 (C, I) and the folded affines for slices padded from C to Cp channels (pad channels:
// zero weights and a2 = c2 = 0, so att = 0 and out = x + y = 0 there).
AffPacked aff_pack(const float* w1, const float* a1, const float* c1, const float* w2, const float* a2,
                   const float* c2, int C, int I, int Cp);
void aff_gate(const AffGateArgs& a, hipStream_t st);
// fuse34's blend: out = x (1 + tanh att) + y (1 - tanh att) over NHWC pixel rows x / y (row lengths ldx / ldy, bf16 or
// fp32), att (B H W, C) fp32, out fp32 at element strides o_s* of (b, h, w, c).
void aff_blend(const void* x, int ldx, const void* y, int ldy, bool bf16, const float* att, int B, int H, int W, int C,
               float* out, int64_t o_sb, int64_t o_sh, int64_t o_sw, int64_t o_sn, hipStream_t st);
// x[p, 0..C) += y[p, 0..C) over P pixel rows of lengths ldx / ldy (the pointers at their channel slice).
void slice_add(void* x, int ldx, const void* y, int ldy, bool bf16, int64_t P, int C, hipStream_t st);
// NHWC (B, H, W, C) -> fp32 (B, W, H * C) with channel h * C + c (get_frame_level_feat's transpose(1, 3) + flatten,
// channel-last).
void nhwc_to_frames(const void* x, bool bf16, int B, int H, int W, int C, float* out, hipStream_t st);

// ---------------------------------------------------------------- redimnet (redimnet.hip)
// ReDimNetB2 (redimnet_wespeaker.py:623-790) keeps every map channel-last as (B, T, 1152) with 1-D channel f * c + ch
// (to1d's order, :758-761): the 2-D view (B, T, f, c) of a stage is the same memory, so to1d / to2d cost nothing.
constexpr int kRedimCF = 1152;   // C * F = 16 * 72 at every stage
// ConvNeXtLikeBlock, dim 2 (:135-165) on a (B, T, f, c) map, c in {16, 32, 64, 128}, f = 1152 / c: grouped 3x3 conv (4
// channels per group, zero "same" padding at the time and the frequency edges of each window) + BatchNorm2d + erf GELU
// + 1x1 conv + bias + skip.  dw: the grouped conv with the BatchNorm folded in, fp32, laid out
// [tap = df * 3 + dt][group][out 4][in 4] (redim_pack_dw); dw_b: c folded biases.  pw: conv_gemm's packed Wt[c][c]
// (bf16 bits or fp32), pw_b: c.
struct RedimBlock2dW {
  const float *dw = nullptr, *dw_b = nullptr;
  const void* pw = nullptr;
  const float* pw_b = nullptr;
};
// torch's (c, 4, 3, 3) grouped weight (kernel axes: frequency, time), its bias and the folded BatchNorm (s, h) ->
// the dw / dw_b images above
void redim_pack_dw(const float* w, const float* bias, const float* s, const float* h, int c, std::vector<float>& dw,
                   std::vector<float>& dw_b);
// The whole block in ONE launch (bf16 maps): a workgroup stages 8 time rows + a one-row halo of one window in LDS,
// runs the grouped conv + GELU on the VALU into a second LDS map and the pointwise conv on MFMA, adds bias and skip
// from the staged tile: one read and one write of the map.  out must not alias x.
void redim_block2d_fused(const void* x, int B, int T, int c, const RedimBlock2dW& W, void* out, hipStream_t st);
// The generic arm's first half: h = gelu(conv3x3_grouped(x) + b) to a map of x's type (fp32 or bf16); the pointwise
// conv, bias and skip follow on conv_gemm with its residual.
void redim_gconv3x3(const void* x, bool bf16, int B, int T, int c, const float* dw, const float* dw_b, void* h,
                    hipStream_t st);
// Both arms behind one call: generic (the only form of fp32 / bf16x3) or fused (bf16).  tmp: a map for the generic arm.
void redim_block2d(const void* x, int B, int T, int c, const RedimBlock2dW& W, void* tmp, void* out, bool bf16,
                   bool generic, hipStream_t st);
// The front half of ConvNeXtLikeBlock, dim 1 (:586-607): depthwise conv over time (odd k <= 59, zero "same" padding
// inside each window) + BatchNorm1d + erf GELU on x (B, T, hC) fp32, hC % 48 == 0 -> y (fp32 or bf16).  wt: (k, hC)
// fp32 with the BatchNorm folded in, bias: hC folded.
void redim_dwconv1d(const float* x, int B, int T, int hC, int k, const float* wt, const float* bias, void* y,
                    bool y_bf16, hipStream_t st);
// weigth1d (:768-772): y[r, ch] = sum_k w[k, ch] x_k[r, ch] over n = 2..7 maps of `rows` x 1152, w = softmax over k of
// inputs_weights[i] (n, 1152) fp32, computed at upload.
struct RedimMixArgs {
  static constexpr int kMax = 7;
  const void* x[kMax] = {};
  int n = 0;
  const float* w = nullptr;
};
void redim_stage_mix(const RedimMixArgs& a, int64_t rows, void* y, bool bf16, hipStream_t st);
// stem (:670-673): Conv2d(1 -> 16, 3x3, same) on the (72, T) fbank map + channels-first LayerNorm over the 16
// channels (eps 1e-6), written as (B, T, 72, 16).  w: (16, 3, 3) torch order (frequency, time), fp32.
void redim_stem(const float* fbank, int B, int T, const float* w, const float* bias, const float* g, const float* beta,
                void* out, bool out_bf16, hipStream_t st);

// ---------------------------------------------------------------- norms
// y = LN(x) * g + b over the last dim D; rows of x at stride ldx, y at ldy.
// y may be bf16 (y_bf16); x is fp32 (the residual stream).
// y2 (optional, fp32 y only): a bf16 copy of y, the A operand of the GEMMs that read it.
void layernorm(const float* x, int rows, int D, int ldx, const float* g, const float* b,
               float eps, void* y, int ldy, bool y_bf16, hipStream_t st, uint16_t* y2 = nullptr);
// Residual add fused into LayerNorm: v = x + t (t fp32 or bf16, rows of D); write_x: x = v;
// y = LN(v) (y may alias x or t: each row is read completely before it is written).
// t_slabs > 1 (fp32 t only): t is the sum of t_slabs slabs t + i * rows * D (a split-K GEMM's partials).
void add_layernorm(float* x, const void* t, bool t_bf16, int rows, int D, const float* g, const float* b,
                   float eps, bool write_x, void* y, bool y_bf16, hipStream_t st, uint16_t* y2 = nullptr,
                   int t_slabs = 1);

// ---------------------------------------------------------------- attention
// Multi-head self-attention core on a packed in-projection output.
// qkv: (S*T, 3*D) row-major (q | k | v), heads of size hd = D/nh.
// out: (S*T, ldo) at column h*hd.  Optional causal mask (key > query + delay is
// masked) and per-sequence key lengths (keys >= len[s] masked).
struct AttnArgs {
  const void* qkv = nullptr;       // fp32, or bf16 when io_bf16 (also the output dtype)
  bool io_bf16 = false;
  int S = 0, T = 0, D = 0, nh = 0;
  int ld_qkv = 0;
  void* out = nullptr;
  int ldo = 0;
  float scale = 1.f;
  int causal = 0, causal_delay = 0;
  const int* key_len = nullptr;
  // Token t of sequence s lives at row (s / seq_inner) * seq_outer + (s % seq_inner) * seq_inner_stride
  // + t * tok_stride of qkv / out.  Defaults (seq_outer 0 -> T) give contiguous sequences; the FS-EEND
  // decoder runs its time attention over the slots of a (T, C) token grid with tok_stride C.
  // Chunk-streaming mask (ts_vad2_streaming forward_chunk_by_chunk with KV caches, expressed as
  // one forward): query i sees key j iff chunk(j) <= chunk(i) and, when left >= 0,
  // chunk(j) >= chunk(i) - left, with chunk(x) = x / chunk.  chunk 0: off.
  int chunk = 0, left = -1;
  int seq_inner = 1;
  int64_t seq_outer = 0;
  int seq_inner_stride = 0;
  int tok_stride = 1;
  // Test probe (sd_probe_attention_mask): mask_dump (T*T int32, zeroed) receives 1/2 = visible/masked
  // for each visited pair of seq 0, head 0.
  int* mask_dump = nullptr;
  int xcd_small = 0;   // set by the launcher: the small-grid XCD grouping of attn_long (attention.hip)
};
void attention(const AttnArgs& a, bool bf16, hipStream_t st);

// ---------------------------------------------------------------- mha_block.hip
// Conformer self-attention block in one launch (bf16, D 384, 8 heads, T <= 160): q|k|v = y · W_inᵀ + bias
// (y the LayerNorm'd bf16 rows, W_in packed bf16 (3D, D)), per head softmax(q kᵀ * scale) v -> out (S*T
// rows of stride ldo, bf16).  key_len (device int32 per sequence) optional.
struct MhaBlockArgs {
  const void* y = nullptr;   // bf16 rows, already LayerNorm'd (self_attn_layer_norm)
  const float* ln_g = nullptr;   // (informational: the norm the rows went through)
  const float* ln_b = nullptr;
  float eps = 1e-5f;
  const void* W = nullptr;
  const float* bias = nullptr;
  void* out = nullptr;
  int ldo = 0;
  int S = 0, T = 0, D = 0, nh = 0;
  float scale = 1.f;
  const int* key_len = nullptr;
  // out in the row programs' tiled A layout (RowProgArgs::a_tiled; needs S * T % 16 == 0, ldo == D) instead of
  // row-major rows of stride ldo
  int out_tiled = 0;
  int y_tiled = 0;   // y in that layout too (RowProgArgs::y_tiled)
};
bool mha_block_supported(int D, int nh, int T, bool bf16);


// ---------------------------------------------------------------- rowprog.hip
// Conformer per-token row program (bf16 weights, D 384): acc = X; [acc += A·W0ᵀ + b0];
// per FFN i: acc += W2·silu(W1·LN_i(acc) + b1) + b2 (the ½ folded into W2 / b2), [acc = LN_post_i(acc)];
// Xo = acc (may alias X); [y = LN_y(acc) bf16].  Weights packed by rowprog_pack_pre / rowprog_pack_ffn.
struct RowFfnArgs {
  const void* w = nullptr;     // rowprog_pack_ffn pieces (the FFN's LayerNorm affine folded in)
  int hidden = 0;
  const float *b1 = nullptr, *b2 = nullptr;   // b1 folded by rowprog_pack_ffn
  const float *post_g = nullptr, *post_b = nullptr;
};
struct RowProgArgs {
  const float* X = nullptr;
  float* Xo = nullptr;
  int M = 0;
  const void* A = nullptr;     // (M, 384) bf16 rows of the pre-GEMM
  const void* w0 = nullptr;    // rowprog_pack_pre pieces (384 x 384)
  const float* b0 = nullptr;
  int n_ffn = 0;
  RowFfnArgs ffn[2];
  const float *y_g = nullptr, *y_b = nullptr;
  void* y = nullptr;
  float eps = 1e-5f;
  // optional A transform of the pre-GEMM: A = silu(GroupNorm(A)) (one group per sequence of gn_T rows),
  // statistics from glu_dwconv's partial sums (gn_nblk pairs per sequence)
  const float* gn_partial = nullptr;
  int gn_nblk = 0, gn_T = 0;
  const float *gn_g = nullptr, *gn_b = nullptr;
  // optional X source instead of X: the TS-VAD per-speaker input rows [ts_embed | mix] built on load
  // (build_speaker_input_kernel's layout, no positional encoding): row (s = b*NS + spk, t) of T_seq
  // rows per sequence = ts[s][0..SE) | mix[b][t][0..SE) (zeros for t >= Tmix), SE = 192
  const float* x_ts = nullptr;
  const float* x_mix = nullptr;
  int x_ldmix = 0, x_Tmix = 0, x_NS = 0, T_seq = 0;
  // optional output: bf16(acc) in the speakers-to-channels layout (B, T_seq, NS * 384), row (b*NS + spk, t)
  // -> (b, t) columns spk*384 .. (speakers_to_channels); with Xo == nullptr the fp32 rows are not written
  void* yt = nullptr;
  int yt_NS = 0;
  // start offset of the odd workgroups, in s_sleep(64) units (set by rowprog()):
  // half the CUs run their epilogue store burst while the other half streams MFMAs
  int stagger = 0;
  // diagnostics (sd_debug_rowprog_probe): per wave, lane 0 accumulates s_memtime cycles of the tile's phases
  // into probe[(block * 8 + wave) * 8 + k] (k: 0 whole, 1 piece waits, 2 refill issue, 3 epilogue, 4 loads)
  unsigned long long* probe = nullptr;
  // X / Xo in the MFMA-tiled layout (M % 16 == 0): 16-row group g, feature f = 16 ft + 4 q + r of row 16 g + l at
  // float ((g * 24 + ft) * 64 + l + 16 q) * 4 + r -- each wave's 16 x 384 fp32 residual block is 24 contiguous
  // 1-KiB runs, one per load / store instruction (row-major it is 16 scattered 64-B pieces per instruction).  The
  // residual stream between row programs is private to them (run_conformer_stack), so it stays tiled in between.
  int x_tiled = 0, xo_tiled = 0;
  // A in the tiled layout of the pre-GEMM's B-operand fragments (M % 16 == 0): row 16 g + l, feature
  // f = 32 kk + 8 q + j at bf16 ((g * 12 + kk) * 64 + l + 16 q) * 8 + j, so fragment kk of a 16-row group is one
  // contiguous 1-KiB run (mha_block writes it with out_tiled)
  int a_tiled = 0;
  int y_tiled = 0;   // y written in the a_tiled layout (for mha_block, MhaBlockArgs::y_tiled)
};
bool rowprog_supported(int D, int hidden, bool bf16);
void rowprog(const RowProgArgs& a, const char* name, hipStream_t st);
// Host packers (bf16 MFMA fragment pieces): W0 (384, 384) row-major; W1 (hidden, 384), W2 (384, hidden).
std::vector<uint16_t> rowprog_pack_pre(const std::vector<float>& W, int N, int K);
// The FFN's LayerNorm (ln_g, ln_b) is folded: W1' = W1 diag(ln_g), b1_folded = W1 ln_b + b1.
std::vector<uint16_t> rowprog_pack_ffn(const std::vector<float>& W1, const std::vector<float>& W2, int hidden,
                                       const std::vector<float>& ln_g, const std::vector<float>& ln_b,
                                       const std::vector<float>& b1, std::vector<float>& b1_folded);
void mha_block(const MhaBlockArgs& a, hipStream_t st, int variant = -1);   // variant: tests (-1: the env's)

// ---------------------------------------------------------------- ssnd_ops.hip
// Multi-head attention core on separate fp32 q / k / v row sets (SSND decoder cross and self
// attention, ssnd_model.py:261-266): row i of batch b at ptr + b * bs + i * ld, head h at
// columns h*hd..; out (B, Nq) rows likewise.  key_len (device int32 per b) optional.
struct MhaSmallArgs {
  const float* q = nullptr; int ldq = 0; int64_t q_bs = 0;
  const float* k = nullptr; int ldk = 0; int64_t k_bs = 0;
  const float* v = nullptr; int ldv = 0; int64_t v_bs = 0;
  float* o = nullptr; int ldo = 0; int64_t o_bs = 0;
  int B = 0, Nq = 0, Tk = 0, nh = 0, hd = 0;
  float scale = 1.f;
  const int* key_len = nullptr;
};
void mha_small(const MhaSmallArgs& a, hipStream_t st);
// dst row r = src row r % src_rows (D floats per row).
void tile_rows(const float* src, int src_rows, int D, float* dst, int dst_rows, hipStream_t st);
// out[r, j] = mean_t sigmoid(x[r, t]) * w[j] + b[j], t < T, j < N.
void mean_sigmoid_affine(const float* x, int rows, int T, int ldx, const float* w, const float* b, int N, float* out,
                         int ldo, hipStream_t st);

// Stream-ordered zeroing of `bytes` (4-byte words) as a kernel: every forward uses it instead of
// hipMemsetAsync so that a captured forward holds no memset node (ops.hip).
void zero_fill(void* p, size_t bytes, hipStream_t st);
void fill_u32(void* p, size_t bytes, uint32_t value, hipStream_t st);   // the same with any 32-bit word

// ---------------------------------------------------------------- ts-vad glue
// BatchNorm1D + ReLU applied by the consumer of a conv output x = conv + bias (model.py:161-171, used at :255
// and :393): v = relu(a[c] x + b[c]), or v = relu(x) for every window of a reference forward (a group of
// `group` consecutive windows) whose BN input held a non-finite value: BatchNorm1D skips its BatchNorm for the
// WHOLE batch then.  a == null: v = x (no BN here).  grp: per-group flags (nonfinite_windows) or null.
struct BnRelu {
  const float* a = nullptr;
  const float* b = nullptr;
  const int* grp = nullptr;
  int group = 1;
  int win0 = 0;   // the kernel's window 0 is window win0 of the batch (a window slice): group (w + win0) / group
};
// Non-finite scan of per-window inputs x (B windows of per_win floats, 16-B aligned rows): win[w] |= 1 and
// grp_a[w / group] |= 1, grp_b[w / group] |= 1 (each nullable) for every window holding a NaN / Inf.  The
// flags must be zeroed before (stream-ordered).  The reference's NaN reaches every BN input value of its
// window (torch's conv / BN / ReLU / mean propagate it; CAM++'s context mean spreads it over all frames),
// while these kernels' ReLUs (v_max_f32) drop NaN, so the flag is taken at the source.
void nonfinite_windows(const float* x, int B, int64_t per_win, int group, int* win, int* grp_a, int* grp_b,
                       hipStream_t st);
// rows of `per_win` floats of every window w with win_a[w] | win_b[w] set -> NaN (the reference's logits of a
// window with a non-finite input are NaN; win_b nullable).
void poison_windows(float* x, int B, int64_t per_win, const int* win_a, const int* win_b, hipStream_t st);
// rows (b, spk, t) of a (B*NS*T, 2E) buffer: [ts[b,spk,:] | mix[b,t,:]] (+ pe[t]).
// mix rows t >= Tmix read as zeros (the pad of model.py:703-710 / :852-854).
// model.py:862-877 (ts_embeds repeat + cat) and :876 PositionalEncoding.
void build_speaker_input(const float* ts, const float* mix, int ldmix, int Tmix, int B, int NS,
                         int T, int E, const float* pe, float* out, hipStream_t st, const BnRelu& mix_bn = BnRelu());

// The same rows through proj_layer = nn.Linear(2 SE, E) (model.py:212-217, 873-876; configurations with
// 2 SE != E): out[(b, spk, t), :] = W [ts[b, spk] | relu(bn(mix[b, t]))] + bias + pe[t], computed as
// P_ts[b, spk] + P_mix[b, t] + pe[t] with W = [W_ts | W_mix] split on its input axis (ops.hip).  mix rows t >= Tmix
// read as zeros.  The GEMMs follow conv_gemm's arithmetic for `bf16` (bf16 operands, or exact fp32 / bf16x3).
struct SpeakerProjArgs {
  const float* ts = nullptr;     // (B * NS, SE)
  const float* mix = nullptr;    // (B, Tmix, ldmix): speech_down_or_up's conv + bias, columns 0 .. SE - 1
  int ldmix = 0, Tmix = 0, B = 0, NS = 0, T = 0, SE = 0, E = 0;
  const void* w_ts = nullptr;    // packed [E][SE]: proj_layer.weight[:, :SE] (bf16 bits in bf16 mode, else fp32)
  const void* w_mix = nullptr;   // packed [E][SE]: proj_layer.weight[:, SE:]
  const float* bias = nullptr;   // (E)
  const float* pe = nullptr;     // (>= T, E), nullable
  BnRelu bn;                     // speech_down_or_up's BatchNorm1D + ReLU, window = row / Tmix
  void* mix_a = nullptr;         // scratch (B * Tmix, SE): the mix GEMM's A operand, bf16 in bf16 mode else fp32
  float* p_ts = nullptr;         // scratch (B * NS, E)
  float* p_mix = nullptr;        // scratch (B * Tmix, E)
  float* out = nullptr;          // (B * NS * T, E)
  uint16_t* xb = nullptr;        // nullable: bf16 copy of out
};
bool speaker_input_proj_supported(int SE, int E);   // both multiples of 8 (16-byte accesses)
void speaker_input_proj(const SpeakerProjArgs& a, bool bf16, hipStream_t st);

// Chunk-streaming speaker input (ts_vad2_streaming/model.py:767-777): row (b, spk, t) =
// [ts[b, spk] | mix[b, t]] * scale + pe[pos(t)], pos(t) = start(t / C) + t % C with start(c) = 0
// (left < 0: the whole history is cached) or max(0, c - left) * C.  out (B * NS * T, 2E).
void build_stream_input(const float* ts, const float* mix, int B, int T, int NS, int E, float scale,
                        const float* pe, int C, int left, float* out, hipStream_t st);
// x[r, :] += pe[r % T, :]  (rows of length D at stride ld)
// (bn: the rows' BatchNorm1D + ReLU first, window = row / T)
void add_pe(float* x, int rows, int T, int D, int ld, const float* pe, hipStream_t st, const BnRelu& bn = BnRelu());

// Per-frame mean/std over channels then Linear(2 -> E): model.py:689-696.
// bn: speech_down_or_up's BatchNorm1D + ReLU applied to x first (window = row / rows_per_window).
void gsp_fc(const float* x, int rows, int C, int ldx, const float* w /*E x 2*/,
            const float* bias, int E, float* out, int ldo, hipStream_t st, const BnRelu& bn = BnRelu(),
            int rows_per_window = 1);

// Frame-level GSP + gsp_fc + the speech_down_or_up conv of speech_encoder_type "CAM++_frame_level_gsp_fc"
// (egs/magicdata-ramc/ts_vad2/model.py:543-563, 1275-1287) in one launch: x (B, T2, 512) the CAM++ transit3 map (fp32 or
// bf16) before out_nonlinear, s / h (512) that BatchNorm folded (the ReLU follows); per frame mean and unbiased std over
// the channels, then the folded Linear(2, 256) + Conv1d(256 -> SE, k5, stride 2, pad 2):
//   y[b, j, o] = cb[o] + sum over k = 0..4 with 0 <= t = 2 j + k - 2 < T2 of (A[o,k] mean[t] + S[o,k] std[t] + C[o,k])
// (the reference zero-pads gsp_fc's output, so a padded tap drops its C term too).  y (B, (T2 - 1) / 2 + 1, SE) fp32 =
// conv + bias, before speech_down_or_up.1's BatchNorm1D + ReLU.  SE a multiple of 32.  coef (5, 3, SE) = [k][A | S | C][o]
// from gsp_down_fold (float64 sums over the 256 gsp_fc features): gw (256, 2), gb (256), w (SE, 256, 5), all host.
constexpr int kGspChannels = 512;   // CamTrunk::kChannels
constexpr int kGspFcDim = 256;      // gsp_fc = nn.Linear(2, 256)
void gsp_down_fold(const float* gw, const float* gb, const float* w, int SE, std::vector<float>& coef);
void gsp_down(const void* x, bool x_bf16, int B, int T2, const float* s, const float* h, const float* coef,
              const float* cb, int SE, float* y, hipStream_t st);
int gsp_down_frame_tile();   // input frames per workgroup tile (without the 2-frame halos), for tests

// (B*NS, T, E) speaker-major rows -> (B, T, NS*E) channel-concatenated rows.
void speakers_to_channels(const float* x, int B, int NS, int T, int E, void* out, bool out_bf16,
                          hipStream_t st);

// ---------------------------------------------------------------- conformer conv module
// Depthwise conv over time (kernel k, pad (k-1)/2, with bias), y: (S, T, C).
// glu_in: x is the pw1 output (S, T, 2C) with rows interleaved [16 values | 16 gates]
// (glu_interleave_row) and the GLU is applied on load; else x is already gated (S, T, C).
// Writes per (sequence, channel-block) partial sums for GroupNorm(1, C), or with
// fused_silu (BatchNorm already folded into w/bias) stores SiLU(y) and no partials.
void glu_dwconv(const void* x, int S, int T, int C, const float* w /*C x k*/,
                const float* bias, int k, void* y, float* partial /*S x nblk x 2*/, bool fused_silu,
                bool glu_in, bool io_bf16, hipStream_t st);
// GroupNorm(num_groups=1) over (T, C) of each sequence, affine, then SiLU (in place).
void groupnorm_silu(void* y, int S, int T, int C, const float* partial, const float* g,
                    const float* b, float eps, bool io_bf16, hipStream_t st);

// ---------------------------------------------------------------- lstm
// One bidirectional (or unidirectional) LSTM layer recurrence given the
// precomputed input projections gx (B, T, ndir*4H) (bias_ih + bias_hh folded in).
// whh: (ndir, 4H, H) fp32.  out: (B, T, ldo) at column dir*H.
// h0/c0 optional (ndir, B, H); hT/cT optional outputs (ndir, B, H).
// whh_bf16 (optional, same layout in bf16 bits): bf16-MFMA recurrence (bf16 mode); the
// cell state, gates and h stay fp32, h is rounded to bf16 only as the MFMA operand.
// whh_lo (optional, with whh_bf16 = bf16(W) as the hi part): bf16(W - hi), the bf16x3 mode's split
// recurrence (W_lo h_hi + W_hi h_lo + W_hi h_hi, h exchanged as hi + lo); where the persistent kernel cannot
// run, the exact-f32 step kernel (never the bf16 one).
// work: per-handle device scratch of lstm_work_floats(B, H, ndir) floats (the persistent bf16
// kernel keeps its h exchange and counters there).  host_err (optional, the DEVICE address of a pinned
// slot of the handle's PinnedFlags): a persistent launch whose poll timed out sets it to 1 from the
// kernel itself and nothing ever writes 0 there but the host's take(), so the report is sticky across
// any number of forwards enqueued before the handle raises kErrHip (sd_tsvad_status / sd_eda_status after
// the forward, or at the latest its next call).
int64_t lstm_work_floats(int B, int H, int ndir);
// Exchange floor of the persistent recurrence (sd_probe_lstm_handoff): us per step of its hand-off alone.
float lstm_handoff_probe(int steps, hipStream_t st);
// The same exchange on 8-byte {data, tag} granules (sd_probe_lstm_granule; lstm.hip): us per step.
// nwg 2: the two-workgroup 1-to-1 form (each lane polls only the other workgroup's half of its operand).
float lstm_granule_probe(int steps, hipStream_t st, int nwg = 4);
void lstm_recurrence(const float* gx, int B, int T, int H, int ndir, const float* whh,
                     const int* lengths, const float* h0, const float* c0, float* out, int ldo,
                     float* hT, float* cT, float* work, hipStream_t st, const void* whh_bf16 = nullptr,
                     int* host_err = nullptr, const void* whh_lo = nullptr);

// ---------------------------------------------------------------- frontend
// Kaldi fbank (torchaudio.compliance.kaldi.fbank semantics used by
// ts_vad_dataset.py:39-52): 25 ms / 10 ms frames, snip_edges, DC removal,
// pre-emphasis 0.97, hamming, 512-point power spectrum, HTK mel, log(max(.,eps)).
void fbank_kaldi(const float* wav, int64_t n_samples, float in_scale, int n_frames,
                 const float* mel_fb /*n_mels x 257*/, int n_mels, float* out,
                 hipStream_t st, int window = 0 /*0 hamming, 1 povey*/);

// Per-window CMN + zero pad: out[w, j, :] = feats[start_w + j, :] - mean_w for j < n_w,
// 0 for n_w <= j < T_out (ts_vad_dataset.py:55 + collater padding :676).
void window_cmn(const float* feats, int n_mels, const int* win_start, const int* win_n,
                int n_win, int T_out, float* out, hipStream_t st);

}  // namespace sd

namespace sd {
// Device-side weight packing (test ops): torch (N, Cin, taps) -> conv_gemm layout.
void pack_weight(const float* w, int N, int Cin, int taps, void* out, bool bf16, hipStream_t st);
}  // namespace sd

namespace sd {
// sigmoid=false: inputs are probabilities already (sd_overlap_mean).  numpy's pairwise
// summation is reproduced for up to kOverlapMaxWindows covering windows per frame.
constexpr int kOverlapMaxDepth = 6;
constexpr int kOverlapMaxWindows = (128 << kOverlapMaxDepth) / 2;
void overlap_average(const float* logits, int n_win, int NS, int Tw, const int* start, const int* len,
                     int dis, int chunk, int n_frames, float* out, hipStream_t st, bool sigmoid = true);

// ---------------------------------------------------------------- postprocess.hip
struct ThresholdSet {
  static constexpr int kMax = 16;
  int n = 0;
  int strict = 0;   // 1: speech iff x > thr (EEND make_rttm.py), 0: x >= thr (TS-VAD infer.py)
  float v[kMax] = {};
};
int segments_max_frames();
// scipy.signal.medfilt (zero padded, odd k <= 63) over each of `rows` tracks of T frames.
void medfilt(const float* x, int rows, int T, int k, float* y, hipStream_t st);
// Per (row, threshold): binarise, fill short silences, drop short speech, emit
// [begin, end) runs.  seg_*: (rows * thr.n, cap); n_seg: (rows * thr.n).
void run_segments(const float* med, int rows, int T, const ThresholdSet& thr, int lim_sil, int lim_sp, int cap,
                  int* seg_begin, int* seg_end, int* n_seg, hipStream_t st);
}  // namespace sd

namespace sd {
void f32_to_bf16(const float* x, int64_t n, void* y, hipStream_t st);
void bf16_to_f32(const void* x, int64_t n, float* y, hipStream_t st);

// ---------------------------------------------------------------- eend frontend + EDA glue (eend.hip)
// librosa-style centred STFT (float64) -> log10 mel power: out (n_frames, n_mels) float64.
void stft_logmel(const float* wav, int64_t n_samples, int n_frames, int n_fft, int hop, int win_len,
                 const float* mel_fb /*(n_mels, n_fft/2+1)*/, int n_mels, double* out, hipStream_t st);
// Streaming frontend of one FS-EEND chunk (sd_fseend_stream_push_audio): the logmel frames the splice of
// model frames [cursor[0], cursor[0] + rows) reads (frame0 = cursor[0] * sub - context, (rows - 1) * sub +
// 2 context + 1 frames into lm), then the spliced rows into out (rows, ld_out).  bound (device int[2]):
// [0] samples of the input (INT_MAX while open), [1] STFT frames of the input (INT_MAX while open).
// Per frame the arithmetic of stft_logmel + splice_subsample, bit for bit.
void stream_frontend(const float* wav, int64_t cap_samples, int rows, int n_fft, int hop, int win_len,
                     const float* mel_fb, int n_mels, int context, int sub, const int* cursor, const int* bound,
                     double* lm, float* out, int ld_out, hipStream_t st);
void col_mean(const double* x, int rows, int cols, double* mean, hipStream_t st);
// out (n_out, ld_out) f32: row r = splice of frame r*sub (±context, zero pad), minus mean (nullable).
void splice_subsample(const double* lm, int n_frames, int n_mels, const double* mean, int context, int sub,
                      int n_out, float* out, int ld_out, hipStream_t st);
// y[s, t] = x[s, perm[s, t]] for t < lengths[s], else x[s, t].  Rows of D floats.
void gather_rows(const float* x, int S, int T, int D, const int* perm, const int* lengths, float* y,
                 hipStream_t st);
void fill_rows(const float* row, int D, int rows, float* y, hipStream_t st);
// probs (S, n_att) = sigmoid(att · lw + lb); act (S, T, n_att-1) = sigmoid(emb · att[:-1]ᵀ).
void attractor_scores(const float* emb, int S, int T, int E, const float* att, int n_att, const float* lw,
                      const float* lb, float* probs, float* act, hipStream_t st);

// ---------------------------------------------------------------- fs-eend glue (fseend_ops.hip)
// y = x / |x| per row (D <= 512); slabs > 1: x is the sum of split-K slabs x + k * rows * D
void row_l2norm(const float* x, int rows, int D, float* y, hipStream_t st, int slabs = 1);
// out (T*C, D): out[t*C + c] = g[t] + p[c]
void slot_init(const float* g, int T, int C, int D, const float* p, float* out, hipStream_t st);
// scores (T, C) = emb[t]·att[t,c]/|att[t,c]|; write_norm: att normalised in place.
void slot_scores(const float* emb, float* att, int T, int C, int D, float* scores, bool write_norm,
                 hipStream_t st);
}  // namespace sd

namespace sd {
// ---------------------------------------------------------------- streaming (stream_ops.hip)
// Chunked causal attention against a K/V history (see stream_ops.hip).  Element offsets:
// query i of sequence s at q + i*q_tok + s*q_seq (+ head*64); key j at k/v + j*kv_tok + s*kv_seq;
// output like the query.  Query i sits at absolute position *pos + i and sees keys
// j <= *pos + i + delay; keys [0, *pos + nq) must be in the history.
struct DecodeAttnArgs {
  const void* q = nullptr;
  int64_t q_tok = 0, q_seq = 0;
  const void* k = nullptr;
  const void* v = nullptr;
  int64_t kv_tok = 0, kv_seq = 0;
  void* out = nullptr;
  int64_t o_tok = 0, o_seq = 0;
  int nseq = 1, nq = 1, nh = 1, hd = 64;
  float scale = 1.f;
  const int* pos = nullptr;   // device cursor
  int delay = 0;
  int max_keys = 0;           // history capacity: grid coverage
  int n_blocks = 0;           // workspace partials per (sequence, head) >= attn_decode_blocks(max_keys)
  float* ws = nullptr;        // nseq*nh*n_blocks*nq*(2+hd) floats
  bool io_bf16 = false;
  // optional: nseq*nh counters, zeroed once when allocated and shared only by launches that run one after
  // another -- the last block of each (sequence, head) then merges the partials (no combine launch)
  unsigned* cnt = nullptr;
  // optional, with cnt: the out-projection in the same launch (o2 = o W_outᵀ + b_out, rows laid out as out's, D =
  // nh * 64 <= 256): each (sequence, head)'s merging block publishes its head's partial write-through to ws2
  // (nseq*nh*nq*D floats) and the last head of a sequence (cnt2: nseq counters, zeroed once) sums them in head order
  const void* wo = nullptr;   // packed [D][D], io dtype
  const float* bo = nullptr;
  void* o2 = nullptr;
  float* ws2 = nullptr;
  unsigned* cnt2 = nullptr;
};
int attn_decode_blocks(int max_keys);
// FS-EEND streaming decoder, slot-attention sub-block of the fusion layer (fs_eend.py:468-471) for one chunk:
//   y = LN(x + t) (-> ln_out, the next residual);  qkv = y W_inᵀ + b_in;  o = softmax(q kᵀ scale) v across the
//   C slots of each frame, per head;  out = o W_outᵀ + b_out.
// ONE launch of nh workgroups (one per head): a head's q/k/v and attention stay in LDS, its out-projection
// partial (the head's 64 input features) is published write-through and the last workgroup to count itself
// sums the nh partials in head order (MI355X guide hand-off row 1; cnt monotonic, zeroed once).
// Supported: D == 256, D / nh == 64, c * C <= 16, C <= 8, 16-B aligned ln_x / ln_g / ln_b / ln_out / w_in / w_out
// (ln_t: 8 B when bf16); returns false otherwise (caller runs the three-launch path).
struct SlotBlockArgs {
  const float* ln_x = nullptr;
  const void* ln_t = nullptr;
  bool t_bf16 = false;
  const float *ln_g = nullptr, *ln_b = nullptr;
  float eps = 1e-5f;
  float* ln_out = nullptr;
  const void* w_in = nullptr;   // packed [3D][D]
  const float* b_in = nullptr;
  const void* w_out = nullptr;  // packed [D][D]
  const float* b_out = nullptr;
  bool w_bf16 = false;
  void* out = nullptr;          // (c*C, D), bf16 when out_bf16
  bool out_bf16 = false;
  float* ws = nullptr;          // nh * c*C * D floats
  unsigned* cnt = nullptr;
  int c = 1, C = 1, D = 256, nh = 4;
  float scale = 0.125f;
};
bool stream_slot_block(const SlotBlockArgs& a, hipStream_t st);
// FS-EEND streaming feed-forward sub-block (nn.TransformerEncoderLayer linear1 -> relu -> linear2, fs_eend.py:
// 196-204 / 474-477) for one chunk of n rows, its input post-LN folded in:  y = LN(x + t) (-> ln_out);
// out = relu(y W1ᵀ + b1) W2ᵀ + b2.  ONE launch: each workgroup owns a slice of the hidden units, its down-projection
// partial is published write-through and the last workgroup to count itself sums the partials in workgroup order
// (cnt wraps to 0 per launch, zeroed once).  Supported: D == 256, F == 2048, 1 <= n <= 8, 16-B aligned operands;
// returns false otherwise (caller runs the two skinny GEMMs).  ws: 128 * 8 * D floats.
struct FfnPairArgs {
  const float* ln_x = nullptr;
  const void* ln_t = nullptr;
  bool t_bf16 = false;
  const float *ln_g = nullptr, *ln_b = nullptr;
  float eps = 1e-5f;
  float* ln_out = nullptr;
  const void* w1 = nullptr;   // packed [F][D]
  const float* b1 = nullptr;
  const void* w2 = nullptr;   // packed [D][F]
  const float* b2 = nullptr;
  bool w_bf16 = false;
  void* out = nullptr;        // (n, D), bf16 when out_bf16
  bool out_bf16 = false;
  float* ws = nullptr;
  unsigned* cnt = nullptr;
  int n = 1, D = 256, F = 2048;
};
bool stream_ffn_pair(const FfnPairArgs& a, hipStream_t st);
// returns true when it also ran the out-projection (wo set, the fused merge taken)
bool attn_decode(const DecodeAttnArgs& a, hipStream_t st);
// dst row (cursor*mult + r) = src row r, r < rows (16-B aligned rows of width_bytes).
void kv_append(const void* src, int64_t ld_src_bytes, int rows, int width_bytes, void* dst, int64_t ld_dst_bytes,
               const int* cursor, int mult, hipStream_t st);
// dst (rows, D) = hist rows [*cursor - pad, ...), zero outside [0, *n_valid).
void gather_window(const float* hist, int D, const int* cursor, const int* n_valid, int pad, int rows, float* dst,
                   hipStream_t st);
// *cursor += by; mirror (optional) = new value.
void cursor_advance(int* cursor, int by, int* mirror, hipStream_t st);
// Encoder chunk tail: v = LN(x + t)*g + b for rows < c (D % 256 == 0, D <= 1024); v -> hist row
// (*cursor + r); then *cursor += c and *mirror = *cursor.
void stream_enc_finish(const float* x, const void* t, bool t_bf16, const float* g, const float* b, float eps, int c,
                       int D, float* hist, int* cursor, int* mirror, hipStream_t st);
// Decoder chunk tail: a = LN(x + t)*g + b for the c*C (frame, slot) rows, scores[f, s] =
// emb[f]·a/|a| (fs_eend.py:88-90); then *cursor += c.
void stream_dec_finish(const float* x, const void* t, bool t_bf16, const float* g, const float* b, float eps, int c,
                       int C, int D, const float* emb, float* scores, int* cursor, hipStream_t st);
}  // namespace sd

namespace sd {
// ---------------------------------------------------------------- mamba2 (mamba2.hip)
// Kernels of the bidirectional Mamba2BlockV2 back end (mamba2.h).  Token rows are (window b, inner i) at row b * I + i,
// `rows` = B * I of them; every per-direction buffer is [forward | backward], `rows` rows each.  A sequence is the rows
// of one inner index over the windows of one group of G consecutive windows (the last group may be shorter), walked in
// window order by the forward chain and in reversed order by the backward chain: reversed indexing, no flipped copies.
constexpr int kMamba2HeadDim = 64;    // mamba_ssm's headdim default
constexpr int kMamba2MaxState = 256;
constexpr float kMamba2Eps = 1e-5f;   // RMSNorm(eps=1e-5) and the mixer's gated RMSNorm
// The residual sum of a block and the RMSNorm of the next one, per row and direction:
//   r = r_in (+ t * rsqrt(sum_h ssq / d_inner + eps): the previous mixer's out_proj output, its gated RMSNorm's per-row
//   scale applied here because norm.weight is folded into out_proj's columns);  r_out = r (t given);
//   y = r * rsqrt(mean(r^2) + eps) * w   (the in_proj A operand, bf16 bits when y_bf16);
//   dt_raw = y (unrounded) . w_dt^T: in_proj's nh dt rows in fp32, whatever the GEMMs' precision (Mamba2ScanArgs).
struct Mamba2NormArgs {
  int64_t rows = 0;
  int E = 0;
  const float* r_in = nullptr;
  int64_t r_in_dir = 0;        // elements between the directions' r_in (0: both read the stack's input)
  const float* t = nullptr;    // (2, rows, E) or null
  const float* ssq = nullptr;  // (2, rows, nh) per-head sums of g^2 (with t)
  int nh = 0, d_inner = 0;     // heads; d_inner with t
  float* r_out = nullptr;      // (2, rows, E), required with t; may alias r_in
  const float* w = nullptr;    // (2, E)
  void* y = nullptr;           // (2, rows, E)
  bool y_bf16 = false;
  const float* w_dt = nullptr; // (2, nh, E): the last nh rows of in_proj.weight
  float* dt_raw = nullptr;     // (2, rows, nh)
};
void mamba2_norm(const Mamba2NormArgs& a, hipStream_t st);
// The stack's output h_n + r_n (r_in, t, ssq as above) of token row (b, spk, tt) = (b * NS + spk) * T + tt, written to
// out row b * T + tt at columns spk * 2 E + dir * E + e: the slot speakers_to_channels would give it (NS = 1, T = rows:
// plain (rows, 2 E) rows).
struct Mamba2FinishArgs {
  int64_t rows = 0;
  int E = 0;
  const float* r_in = nullptr;
  int64_t r_in_dir = 0;
  const float* t = nullptr;
  const float* ssq = nullptr;
  int nh = 0, d_inner = 0;
  int NS = 1, T = 1;
  void* out = nullptr;
  bool out_bf16 = false;
};
void mamba2_finish(const Mamba2FinishArgs& a, hipStream_t st);
// The mixer between in_proj and out_proj, one workgroup per (sequence, head, direction): causal depthwise conv (k 4,
// left zero pad) + bias + SiLU on x | Bm | Cm, dt = softplus(dt_raw + dt_bias), the recurrence
//   S_l = exp(dt_l A) S_{l-1} + dt_l x_l (x) Bm_l,   y_l = S_l Cm_l + D x_l
// with the 64 x d_state state in registers (fp32 whatever the i/o type, any sequence length), g = y * silu(z) and the
// head's sum of g^2 per row for the gated RMSNorm.
struct Mamba2ScanArgs {
  const void* zx = nullptr;    // (2, rows, ldz): in_proj's [z | x | Bm | Cm | dt_raw], bf16 bits when bf16
  int ldz = 0;
  bool bf16 = false;
  // (2, rows, heads) fp32 from mamba2_norm, read instead of zx's dt columns: exp(dt A) with A down to -16 turns the
  // 2^-9 relative rounding of bf16 operands or of a bf16 dt_raw into percents of the decay
  const float* dt_raw = nullptr;
  int64_t rows = 0;
  int B = 0, G = 0, I = 0;
  int d_inner = 0, d_state = 0;
  const float *conv_w = nullptr, *conv_b = nullptr;   // (2, conv_dim, 4), (2, conv_dim)
  const float *dt_bias = nullptr, *A = nullptr, *D = nullptr;   // (2, heads); A = -exp(A_log)
  void* g = nullptr;           // (2, rows, d_inner), zx's type
  float* ssq = nullptr;        // (2, rows, heads)
};
void mamba2_scan(const Mamba2ScanArgs& a, hipStream_t st);
// rows of `per_win` floats of every window of a group g with grp[g] set -> NaN: with a scan over the windows of a
// reference forward, a non-finite input reaches every window of its group (both directions meet in backend_down).
void poison_groups(float* x, int B, int64_t per_win, const int* grp, int group, hipStream_t st);

// ---------------------------------------------------------------- wavlm (wavlm.hip)
// Conv front end, layer 0 (wavlm.py:447-505): Conv1d(1 -> 512, k 10, stride 5, no bias, no padding) straight from the
// waveforms wav (B, n) fp32, its norm and the erf GELU, written channel-last as out (B, T0, 512), T0 = (n - 10) / 5 + 1.
// K = 10, so the conv is VALU work and is recomputed by every pass rather than stored.
//   layer_norm false ("default"): Fp32GroupNorm(512, 512), one group per channel over the T0 frames of a window.  A
//     statistics pass leaves (count, mean, M2) per 64 frames (two passes over each run, fp32), a second kernel merges
//     them pairwise in fp64 (Chan) into scale / shift per (window, channel), the third normalises.  partial: scratch
//     of B * wavlm_l0_parts(T0) * 3 * 512 floats, ss: B * 2 * 512 floats.
//   layer_norm true: Fp32LayerNorm(512) over the channels of each frame, one pass (partial / ss unused).
// w: (512, 10) fp32; g, b: the norm's affine (512 each).
int wavlm_l0_parts(int T0);
void wavlm_layer0(const float* wav, int B, int n, const float* w, const float* g, const float* b, bool layer_norm,
                  float* partial, float* ss, void* out, bool out_bf16, hipStream_t st);
// x = GELU(LayerNorm(x) g + b) in place over `rows` rows of 512 values (fp32, or bf16 bits): what follows the conv
// of layers 1..6 in layer_norm mode; fp32 statistics, eps 1e-5.
void wavlm_ln_gelu(void* x, bool bf16, int64_t rows, const float* g, const float* b, hipStream_t st);
// x[i] += t[i] over n values, t fp32 or bf16 bits (the pre-LN layers' residual adds).
void wavlm_add(float* x, const void* t, bool t_bf16, int64_t n, hipStream_t st);
// The positional conv of the encoder (wavlm.py:566-581, 635-637): out = x + GELU(conv(x) + bias) with Conv1d(D, D, 128,
// padding 64, groups 16) and SamePad dropping the last frame, on x (B, T, D) fp32 channel-last, D / 16 = 48 or 64.  Per
// (window, group, 64 frames) one workgroup stages the 191 zero-padded frames of the group's channels in LDS, where
// row t of the implicit GEMM's A (K = 128 D / 16, tap-major) is the contiguous run starting at frame t, and reads
// the weights as MFMA B fragments: bf16 operands (v_mfma_f32_16x16x32_bf16) or exact f32 (v_mfma_f32_16x16x4_f32).
// wt: [D][128 * D / 16] with k = tap * (D / 16) + c, bf16 bits or fp32 (weight norm folded); out must not alias x.
void wavlm_pos_conv(const float* x, int B, int T, int D, const void* wt, bool bf16, const float* bias, float* out,
                    hipStream_t st);
// table (H, 2 T - 1): table[h][r + T - 1] = emb[bmap[r + off]][h] for the relative positions r = key - query in
// [-(T - 1), T - 1] (compute_bias, modules.py:449-461); emb (320, H), bmap: the bucket of position r at r + off.
void wavlm_bias_table(const float* emb, const int* bmap, int off, int T, int H, float* table, hipStream_t st);
// Self-attention with the gated relative-position bias (modules.py:530-578), head size 64, any T >= 1:
//   gate[b, h, q] = ga (gb grep_a[h] - 1) + 2, (ga, gb) = sigmoid(sums of 4 of grep_w xin[b, q, h] + grep_b)
//   out[b, q, h] = softmax_k(q k^T scale + gate * table[h][k - q + T - 1]) v
// on a packed projection qkv (B T, 3 D) = (q | k | v), fp32 or bf16 bits.  xin (B T, D) fp32 is the layer's INPUT
// (the normalised one in pre-LN mode), not q.  One workgroup per (16 queries, head, window) walks the keys 64 at a
// time with a running max / sum (fp32 softmax); Q K^T and P V run on MFMA, bf16 operands when qkv is bf16, else exact
// f32.  out (B T, D) at column h * 64, bf16 bits when out_bf16.
struct WavlmAttnArgs {
  const void* qkv = nullptr;
  bool bf16 = false;
  const float* xin = nullptr;
  int B = 0, T = 0, D = 0, H = 0;
  const float *grep_w = nullptr, *grep_b = nullptr, *grep_a = nullptr;   // (8, 64), (8), (H)
  const float* table = nullptr;                                          // (H, 2 T - 1)
  float scale = 0.125f;
  void* out = nullptr;
  bool out_bf16 = false;
};
void wavlm_attention(const WavlmAttnArgs& a, hipStream_t st);

// TS-VAD's WavLM_weight_sum head (egs/magicdata-ramc/ts_vad2/model.py:1193-1203).
// The layer-weighted sum, accumulated as the encoder layers run: acc[i] = w x[i] (first) or acc[i] += w x[i] over n
// fp32 values, n a multiple of 4, 16-byte aligned pointers.  `weights` = Linear(L -> 1, no bias) over the stacked layer
// outputs is acc = sum_l w_l x_{l+1}; no (layers, rows, D) buffer exists.
void wavlm_layer_mix(float* acc, const float* x, float w, bool first, int64_t n, hipStream_t st);
// out (rows, SE) = LayerNorm_SE(acc (rows, D) Wt^T + bias) g + beta, eps 1e-5 (wavlmproj + wavlmlnorm): one MFMA GEMM
// over K = D whose N tile spans the whole SE row (SE 192 or 256, four waves of SE / 4 columns over 16 rows), so the
// LayerNorm runs in the epilogue on the fp32 accumulators (two passes, the row sums exchanged through LDS).  bf16:
// Wt [SE][D] bf16 bits, acc rounded to bf16 on load (v_mfma_f32_16x16x32_bf16), out bf16 bits; else Wt fp32, exact f32
// (v_mfma_f32_16x16x4_f32), out fp32.  D a multiple of 32.  out is what speech_down_or_up's conv_gemm reads as A.
void wavlm_mix_proj_ln(const float* acc, int rows, int D, const void* wt, bool bf16, const float* bias, const float* g,
                       const float* beta, int SE, void* out, hipStream_t st);
// The pipeline's window gather on raw waveform, window_cmn's counterpart (no mean removal: ts_vad_dataset.py:185-188,
// 759-761 hand the samples over as they are, the collater zero-pads :693-707): out[w, j] = wav[start_w + j] for
// j < n_w (and start_w + j < n_total), else 0, for j < n_out.
void window_wave(const float* wav, int64_t n_total, const int* win_start, const int* win_n, int n_win, int n_out,
                 float* out, hipStream_t st);

// ---------------------------------------------------------------- w2v-BERT 2.0 (w2vbert.hip)
// Self-attention with the relative_key distance embedding (transformers' Wav2Vec2BertSelfAttention.forward,
// modeling_wav2vec2_bert.py:263-337), head size 64, left 64 / right 8, no mask, any T >= 1:
//   out[b, l, h] = softmax_r((q_l . k_r + q_l . E[clamp(r - l, -64, 8) + 64]) scale) v
// on a packed projection qkv (B T, 3 D) = (q | k | v), fp32 or bf16 bits.  dist: the layer's distance_embedding.weight
// (73, 64), shared by the heads, zero-padded to kW2vDistRows rows, in qkv's type.  One workgroup per (16 queries, head,
// window) computes R = Q E^T (16 x 80) on MFMA once into LDS, then walks the keys 64 at a time with a running max / sum
// (fp32 softmax), adding R[l][clamp(r - l)] to Q K^T before the scale; Q K^T and P V on MFMA, bf16 operands when qkv is
// bf16, else exact f32.  Keys >= T score -inf, queries >= T are not stored.  out (B T, D) at column h * 64, bf16 bits
// when out_bf16.  Nothing of size (T, T) exists in global memory.
constexpr int kW2vDistRows = 80;
struct W2vAttnArgs {
  const void* qkv = nullptr;
  bool bf16 = false;
  const void* dist = nullptr;   // (kW2vDistRows, 64)
  int B = 0, T = 0, D = 0, H = 0;
  float scale = 0.125f;
  void* out = nullptr;
  bool out_bf16 = false;
};
void w2vbert_attention(const W2vAttnArgs& a, hipStream_t st);
// The middle of Wav2Vec2BertConvolutionModule.forward (:211-221) in one launch: GLU over channels, left zero pad of 30
// + depthwise Conv1d(k 31, no bias) (causal), depthwise_layer_norm over the 1024 channels (fp32 statistics, eps 1e-5),
// swish.  x (B, T, 2048): pointwise_conv1's output as plain halves [value 1024 | gate 1024], fp32 or bf16 bits; w
// (1024, 31) fp32; g / beta: the LayerNorm affine; out (B, T, 1024) in x's type.  A workgroup owns kW2vConvTile frames of
// one window with all channels; its 30-frame left halo reads zeros before the window's first frame, never another
// window's frames.  out must not alias x.
constexpr int kW2vConvC = 1024, kW2vConvK = 31, kW2vConvTile = 16;
void w2vbert_conv_mix(const void* x, int B, int T, const float* w, const float* g, const float* beta, void* out,
                      bool bf16, hipStream_t st);

// ---------------------------------------------------------------- whisper (whisper.hip)
// whisper.log_mel_spectrogram(wav, n_mels) per window, no 30-s padding (the published formula: torch.stft(wav, 400, 160,
// hann_window(400)) with center=True / reflect, the last frame dropped, |.|^2, the (n_mels, 201) slaney mel matrix,
// log10(clamp(., 1e-10)), maximum(., max over the WHOLE window - 8), (. + 4) / 4), all fp32.  wav (B, n), n >= 400,
// F = n / 160 frames.  The 400-point DFT runs as conv_gemm's exact-f32 MFMA GEMM of the windowed frames (B F, 400)
// against `basis` (402, 400) = [cos | -sin] rows (whisper_dft_basis), whatever the caller's precision.  The window
// maximum is an unsigned atomic max over an order-preserving key (bit-identical for any order) in which NaN ranks top:
// a non-finite sample makes every feature of its window NaN, as torch's max / maximum do, and leaves the other windows
// untouched.  wmax is re-initialised in the stream by every call.  out (B F, ldo): columns [0, n_mels) the features,
// columns [n_mels, ldo) zeros (conv_gemm's multi-tap form needs Cin % 32 == 0: 80 mels ride in rows of 96); fp32, or
// bf16 bits when out_bf16.
constexpr int kWhisperNfft = 400, kWhisperHop = 160, kWhisperBins = 201, kWhisperMaxWide = 16384;
struct WhisperLogmelArgs {
  const float* wav = nullptr;
  int B = 0, n = 0, n_mels = 0;
  const float* hann = nullptr;    // (400)
  const float* basis = nullptr;   // (402, 400) fp32, conv_gemm's Wt[N][K]
  const float* melT = nullptr;    // (201, n_mels): the mel matrix transposed
  float* frames = nullptr;        // scratch (B F, 400)
  float* spec = nullptr;          // scratch (B F, 402)
  float* raw = nullptr;           // scratch (B F, n_mels)
  uint32_t* wmax = nullptr;       // scratch (B)
  void* out = nullptr;
  int ldo = 0;
  bool out_bf16 = false;
};
void whisper_dft_basis(std::vector<float>& basis, std::vector<float>& hann);   // host images, angles reduced exactly
void whisper_logmel(const WhisperLogmelArgs& a, hipStream_t st);
// out[r, 0..D) = x[r, 0..D) + t[r, 0..D) over `rows` rows: x at stride ldx, t (rows, D) dense, out at stride ldo (the
// pointers already at their column slice; out may alias x).  The PMFA residual stream: block i + 1 reads slice i of the
// wide buffer and writes slice i + 1.  D, ldx, ldo multiples of 4, 16-byte aligned pointers.
void whisper_add(const float* x, int ldx, const float* t, float* out, int ldo, int64_t rows, int D, hipStream_t st);
// y = LN(x) g + b over rows of W <= 16384 floats (W % 4 == 0) at strides ldx / ldy: one workgroup per row, the row in
// registers, two-pass fp32 statistics; y fp32 or bf16 bits (the A operand of the GEMM that follows).  ln_post2 over the
// concatenated block outputs, and the blocks' own LayerNorms where the state is wider than layernorm()'s 1024.
void whisper_ln_wide(const float* x, int64_t ldx, int64_t rows, int W, const float* g, const float* b, float eps,
                     void* y, int64_t ldy, bool y_bf16, hipStream_t st);
}  // namespace sd
