// Bidirectional Mamba2BlockV2 (egs/*/ts_vad2/mamba.py:149-213) as a TS-VAD back end stage:
//   Block(mlp_cls=nn.Identity, fused_add_norm=False, norm_cls=RMSNorm(eps=1e-5)) x n_layer per direction,
//   r_1 = u, h_i = mixer_i(rmsnorm_i(r_i)), r_{i+1} = h_i + r_i, output cat(h_n + r_n of the forward chain, of the
//   backward chain on the flipped sequence, flipped back).
// The mixer is mamba_ssm's Mamba2 at its defaults (headdim 64, ngroups 1, d_conv 4, rmsnorm, no projection biases);
// mamba_ssm is not available where this was written, so the arithmetic restates the published module (parity unpinned).
#pragma once
#include <string>
#include <vector>
#include "encoder.h"

namespace sd {

class Mamba2Stack {
 public:
  // `prefix`forward_blocks.{i}. / backward_blocks.{i}. keys of the state dict (strict: every key read is marked)
  void load(ParamStore& ps, DeviceArena& arena, const std::string& prefix, int E, int n_layer, int d_state, int expand,
            bool bf16);
  static void validate(int E, int d_state, int expand);   // kErrInvalid naming d_state / expand
  void alloc(DeviceArena& arena, int64_t max_rows);
  // x (B * I, E) fp32 token rows (window b, inner i) at row b * I + i, left unchanged; sequences over the windows of
  // each group of G consecutive windows (kernels.h).  out: row (b, spk, tt) = (b * NS + spk) * T + tt -> out row
  // b * T + tt, columns spk * 2 E + [forward E | backward E], bf16 bits when out_bf16; I % (NS * T) == 0.
  void forward(const float* x, int B, int G, int I, void* out, bool out_bf16, int NS, int T, hipStream_t st) const;
  int d_inner() const { return d_inner_; }
  int d_in_proj() const { return 2 * d_inner_ + 2 * N_ + heads_; }

 private:
  struct Layer {
    PackedW in_proj[2], out_proj[2];   // per direction; in_proj zero-padded to ldz_ rows, out_proj x mixer.norm.weight
    // both directions, [forward | backward]; w_dt: in_proj's dt rows in fp32 (mamba2_norm computes dt_raw from them)
    const float *norm_w, *w_dt, *conv_w, *conv_b, *dt_bias, *A, *D;
  };
  std::vector<Layer> layers_;
  int E_ = 0, N_ = 0, d_inner_ = 0, heads_ = 0, ldz_ = 0;
  bool bf16_ = false;
  int64_t max_rows_ = 0;
  void *xn_ = nullptr, *zx_ = nullptr, *g_ = nullptr;   // (2, rows, E | ldz | d_inner), bf16 bits in bf16 mode
  float *t_ = nullptr, *res_ = nullptr, *ssq_ = nullptr;   // (2, rows, E), (2, rows, E), (2, rows, heads)
  float* dt_ = nullptr;                                    // (2, rows, heads): dt_raw in fp32
};

}  // namespace sd
