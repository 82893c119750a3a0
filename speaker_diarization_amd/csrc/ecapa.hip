// ECAPA-TDNN glue kernels on gfx950 (egs/alimeeting/ts_vad2/ecapa_tdnn_wespeaker.py, pooling_layers_wespeaker.py):
// what the trunk (ecapa.cpp) needs around its conv_gemm launches, and attentive statistics pooling.
//
//   ecapa_im2col      layer1's k5 pad-2 window of the 80-bin fbank as one 400-wide row per frame (80 is no multiple
//                     of the GEMM kernels' 32-channel tap step), zeros outside [0, T) of the frame's own window
//   ecapa_add_slice   Res2 stage input sp_prev + split_i (:68-71), or the group-7 pass-through copy (:75-76)
//   res2_chain_kernel the whole Res2 chain of a bf16 map in one launch (:30-79; described at the kernel)
//   ecapa_col_mean    SE_Connect's mean over time (:121), one fixed-order fp64 sum per (window, channel): no atomics,
//                     so a graph replay repeats it bit for bit
//   ecapa_se_fc       the two SE linears: gate = sigmoid(W2 relu(W1 mean + b1) + b2) (:122-123), fp32 in every mode,
//                     every sum in a fixed order
//   ecapa_se_apply    out = x + y * gate into the block's channel slice of the (B, T, 3072) concat buffer (:124, :158)
//   astp_context / astp_tanh / astp_softmax_stats   ASTP with the global context (pooling_layers_wespeaker.py:91-144)
//
// All maps are channel-last (B, T, C) rows, fp32 or bf16 bits; every kernel addresses a window's frames through its
// own (b, t), so a tile never reads another window's frames.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "launch.h"
#include "prof.h"

namespace sd {
namespace {

template <bool BF>
__global__ __launch_bounds__(256) void ecapa_im2col_kernel(const float* __restrict__ fb, int B, int T,
                                                           act_t<BF>* __restrict__ out) {
  constexpr int F = 80, K = 5 * F;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T * K) return;
  const int k = (int)(i % K);
  const int64_t row = i / K;
  const int t = (int)(row % T), tap = k / F, c = k - tap * F, ts = t + tap - 2;
  const float v = (ts >= 0 && ts < T) ? fb[(row - t + ts) * F + c] : 0.f;
  st_act(out, i, v);
}

// out[r, c] = a[r * lda + c] (+ b[r * ldb + c]), c < 128
template <bool BF>
__global__ __launch_bounds__(256) void ecapa_add_slice_kernel(const act_t<BF>* __restrict__ a, int lda,
                                                              const act_t<BF>* __restrict__ b, int ldb, int64_t rows,
                                                              act_t<BF>* __restrict__ out, int ldo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * 128) return;
  const int64_t r = i >> 7;
  const int c = (int)(i & 127);
  float v = ld_act(a, r * lda + c);
  if (b) v += ld_act(b, r * ldb + c);
  st_act(out, r * ldo + c, v);
}

// mean[b, c] = (1 / T) sum_t x[b, t, c]: a workgroup owns 64 channels of one window, its 4 waves split the frames
template <bool BF>
__global__ __launch_bounds__(256) void ecapa_col_mean_kernel(const act_t<BF>* __restrict__ x, int T, int C,
                                                             float* __restrict__ mean) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, b = blockIdx.y;
  const int c = blockIdx.x * 64 + lane;
  const act_t<BF>* xb = x + (int64_t)b * T * C + c;
  double s = 0.0;
  for (int t = g; t < T; t += 4) s += (double)ld_act(xb, (int64_t)t * C);
  red[g][lane] = s;
  __syncthreads();
  if (g == 0) mean[(int64_t)b * C + c] = (float)((red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (double)T);
}

// One 1024-thread workgroup per window.  h = relu(W1 m + b1) (128): thread (part, o) sums 128 of the 1024 inputs of
// output o, the eight parts are added in part order; gate = sigmoid(W2 h + b2) (1024): one output per thread.  Both
// weights are transposed (w1t (1024, 128), w2t (128, 1024)), so a wave reads consecutive outputs of one k, and the
// k loops are unrolled 16-fold to keep that many loads in flight (per-output sequential dot products measured 190 us
// per launch at B = 64, latency-bound).
__global__ __launch_bounds__(1024) void ecapa_se_fc_kernel(const float* __restrict__ mean, const float* __restrict__ w1t,
                                                           const float* __restrict__ b1, const float* __restrict__ w2t,
                                                           const float* __restrict__ b2, float* __restrict__ gate) {
  constexpr int C = 1024, H = 128, PARTS = 8, KP = C / PARTS;
  __shared__ float m[C];
  __shared__ float part[PARTS][H];
  __shared__ float h[H];
  const int tid = threadIdx.x, b = blockIdx.x;
  m[tid] = mean[(int64_t)b * C + tid];
  __syncthreads();
  {
    const int o = tid & (H - 1), pt = tid >> 7;
    const float* w = w1t + (int64_t)pt * KP * H + o;
    float acc = 0.f;
#pragma unroll 16
    for (int k = 0; k < KP; ++k) acc = fmaf(w[(int64_t)k * H], m[pt * KP + k], acc);
    part[pt][o] = acc;
  }
  __syncthreads();
  if (tid < H) {
    float acc = part[0][tid];
#pragma unroll
    for (int pt = 1; pt < PARTS; ++pt) acc += part[pt][tid];
    h[tid] = fmaxf(acc + b1[tid], 0.f);
  }
  __syncthreads();
  float acc = 0.f;
#pragma unroll 16
  for (int k = 0; k < H; ++k) acc = fmaf(w2t[(int64_t)k * C + tid], h[k], acc);
  gate[(int64_t)b * C + tid] = 1.f / (1.f + expf(-(acc + b2[tid])));
}

// out[b, t, c] = x[b, t, c] + y[b, t, c] * gate[b, c], c < 1024 (x / out: channel slices of rows ldx / ldo)
template <bool BF>
__global__ __launch_bounds__(256) void ecapa_se_apply_kernel(const act_t<BF>* __restrict__ x, int ldx,
                                                             const act_t<BF>* __restrict__ y,
                                                             const float* __restrict__ gate, int T, int64_t rows,
                                                             act_t<BF>* __restrict__ out, int ldo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * 1024) return;
  const int64_t r = i >> 10;
  const int c = (int)(i & 1023);
  const float g = gate[(r / T) * 1024 + c];
  st_act(out, r * ldo + c, ld_act(x, r * ldx + c) + ld_act(y, i) * g);
}

// ---------------------------------------------------------------- fused Res2 chain (bf16)
// One workgroup = 64 output frames of one window, all seven stages.  It works on E = 64 + 14 d frames (rounded up to
// a multiple of 16): the 7 d-frame halo per side is recomputed, and a stage's rows lose d valid frames per side to the
// tile edge, so after seven stages exactly the 64 owned frames are valid.  Two LDS maps (E rows x 128 channels bf16,
// 272-B rows: the 16 rows of a fragment read fall on 16 different 16-B bank slots) hold the stage input
// sp_{i-1} + split_i and the next one; d zero rows on either side stand for the taps beyond the tile.  Frames outside
// the window's own [0, T) are written as zeros, the reference's zero padding of every stage input; nothing of another
// window is read.  Each wave owns 32 output channels and keeps the stage's 32 x 384 weights in registers as 24 MFMA
// B fragments (96 VGPRs) read straight from global memory (98 KB per stage, L2-resident across workgroups); the A
// fragments are ds_read_b128 from the LDS map, k ascending tap by tap as in conv_gemm.  The rounding points are the
// generic arm's: sp_i to bf16, then bf16(sp_i + split_{i+1}).
constexpr int kChainTT = 64, kChainLd = 136, kChainPad = 4;

__host__ __device__ inline int chain_rows(int d) { return (kChainTT + 14 * d + 15) / 16 * 16; }

__global__ __launch_bounds__(256) void res2_chain_kernel(const uint16_t* __restrict__ x, int T, int d, Res2ChainW W,
                                                         uint16_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint16_t chain_sm[];
  const int E = chain_rows(d), slab = (E + 2 * kChainPad) * kChainLd;
  uint16_t* cur = chain_sm + kChainPad * kChainLd;   // row 0 of the tile; rows [-4, 0) and [E, E + 4) stay zero
  uint16_t* nxt = cur + slab;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lrow = lane & 15, lk = lane >> 4;
  const int b = blockIdx.y, t0 = blockIdx.x * kChainTT, te = t0 - 7 * d;
  const uint16_t* xb = x + (int64_t)b * T * 1024;
  uint16_t* ob = out + (int64_t)b * T * 1024;
  // zero pad rows of both maps
  for (int q = tid; q < 2 * 2 * kChainPad * 16; q += 256) {
    const int m = q >> 7, r = (q >> 4) & 7, c8 = (q & 15) * 8;
    const int row = r < kChainPad ? r - kChainPad : E + r - kChainPad;
    *reinterpret_cast<uint4*>(cur + m * slab + row * kChainLd + c8) = make_uint4(0, 0, 0, 0);
  }
  // stage 0 input: split_0 over the tile, zeros outside the window
  for (int q = tid; q < E * 16; q += 256) {
    const int r = q >> 4, c8 = (q & 15) * 8, t = te + r;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (t >= 0 && t < T) v = *reinterpret_cast<const uint4*>(xb + (int64_t)t * 1024 + c8);
    *reinterpret_cast<uint4*>(cur + r * kChainLd + c8) = v;
  }
  // group 7 passes through
  for (int q = tid; q < kChainTT * 16; q += 256) {
    const int t = t0 + (q >> 4), c = 7 * 128 + (q & 15) * 8;
    if (t < T) *reinterpret_cast<uint4*>(ob + (int64_t)t * 1024 + c) = *reinterpret_cast<const uint4*>(xb + (int64_t)t * 1024 + c);
  }
  __syncthreads();
  for (int i = 0; i < Res2ChainW::kStages; ++i) {
    const uint16_t* w = static_cast<const uint16_t*>(W.w[i]);
    bf16x8 bfr[2][12];
    float bias[2], sc[2], sh[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int n = wv * 32 + nt * 16 + lrow;
#pragma unroll
      for (int ks = 0; ks < 12; ++ks) bfr[nt][ks] = *reinterpret_cast<const bf16x8*>(w + n * 384 + ks * 32 + lk * 8);
      bias[nt] = W.bias[i][n];
      sc[nt] = W.s[i][n];
      sh[nt] = W.h[i][n];
    }
    for (int mt = 0; mt < E / 16; ++mt) {
      floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ks = 0; ks < 12; ++ks) {
        const int r = mt * 16 + lrow + ((ks >> 2) - 1) * d;   // in [-d, E + d): the pad rows are zeros
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(cur + r * kChainLd + (ks & 3) * 32 + lk * 8);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr[0][ks], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr[1][ks], acc[1], 0, 0, 0);
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int n = wv * 32 + nt * 16 + lrow;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int row = mt * 16 + lk * 4 + rr, t = te + row;
          const bool inwin = t >= 0 && t < T;
          float v = fmaxf(acc[nt][rr] + bias[nt], 0.f);
          v = v * sc[nt] + sh[nt];
          const uint16_t vb = f2bf_bits(v);
          if (inwin && t >= t0 && t < t0 + kChainTT) ob[(int64_t)t * 1024 + i * 128 + n] = vb;
          if (i + 1 < Res2ChainW::kStages) {
            uint16_t nv = 0;
            if (inwin) nv = f2bf_bits(bf_bits2f(vb) + bf_bits2f(xb[(int64_t)t * 1024 + (i + 1) * 128 + n]));
            nxt[row * kChainLd + n] = nv;
          }
        }
      }
    }
    __syncthreads();
    uint16_t* t_ = cur;
    cur = nxt;
    nxt = t_;
  }
}

// ---------------------------------------------------------------- ASTP
// Context statistics per (window, channel), tstp_pool's two fp64 passes: ctx (B, 2 C) = [mean | sqrt(unbiased var +
// 1e-7)]; x32 (nullable): the fp32 copy of x the attention GEMMs read.
template <bool BF>
__global__ __launch_bounds__(256) void astp_context_kernel(const act_t<BF>* __restrict__ x, int T, int C,
                                                           float* __restrict__ ctx, float* __restrict__ x32) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, b = blockIdx.y;
  const int c = blockIdx.x * 64 + lane;
  const act_t<BF>* xb = x + (int64_t)b * T * C + c;
  double sum = 0.0;
  for (int t = g; t < T; t += 4) {
    const float v = ld_act(xb, (int64_t)t * C);
    sum += (double)v;
    if (x32) x32[((int64_t)b * T + t) * C + c] = v;
  }
  red[g][lane] = sum;
  __syncthreads();
  const double mean = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (double)T;
  __syncthreads();
  double ss = 0.0;
  for (int t = g; t < T; t += 4) {
    const double d = (double)ld_act(xb, (int64_t)t * C) - mean;
    ss += d * d;
  }
  red[g][lane] = ss;
  __syncthreads();
  if (g == 0) {
    const double var = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (double)(T - 1);
    ctx[(int64_t)b * 2 * C + c] = (float)mean;
    ctx[(int64_t)b * 2 * C + C + c] = (float)sqrt(var + 1e-7);
  }
}

// h[b, t, j] = tanh(h[b, t, j] + cv[b, j]), j < 128: the context half of linear1 is constant over a window's frames
__global__ __launch_bounds__(256) void astp_tanh_kernel(float* __restrict__ h, const float* __restrict__ cv, int T,
                                                        int64_t rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * 128) return;
  h[i] = tanhf(h[i] + cv[((i >> 7) / T) * 128 + (i & 127)]);
}

// Softmax over time per (window, channel) of the scores e, then the weighted statistics in fp64:
// stats (B, 2 C) = [m = sum_t a x | sqrt(max(var, clamp))], a = softmax_t(e).  ASTP: var = sum_t a x^2 - m^2, clamp 1e-7.
// ASP (CENTRED): var = sum_t a (x - m)^2 in a second pass over the (L2-resident) rows, clamp the fp32 1e-5: the
// difference of squares keeps 1e-10 absolute in fp64 at a mean of 1000, which is the whole variance of a channel of
// std 0.01 to five digits only; the centred sum is exact for a constant channel and for T == 1.
template <bool BF, bool CENTRED>
__global__ __launch_bounds__(256) void astp_softmax_stats_kernel(const act_t<BF>* __restrict__ x,
                                                                 const float* __restrict__ e, int T, int C,
                                                                 double clamp, float* __restrict__ stats) {
  __shared__ double red[3][4][64];
  __shared__ float redm[4][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, b = blockIdx.y;
  const int c = blockIdx.x * 64 + lane;
  const int64_t base = (int64_t)b * T * C + c;
  float mx = -INFINITY;
  for (int t = g; t < T; t += 4) mx = fmaxf(mx, e[base + (int64_t)t * C]);
  redm[g][lane] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(redm[0][lane], redm[1][lane]), fmaxf(redm[2][lane], redm[3][lane]));
  double sw = 0.0, s1 = 0.0, s2 = 0.0;
  for (int t = g; t < T; t += 4) {
    const double w = exp((double)(e[base + (int64_t)t * C] - mx));
    const double v = (double)ld_act(x, base + (int64_t)t * C);
    sw += w;
    s1 += w * v;
    s2 += w * v * v;
  }
  red[0][g][lane] = sw;
  red[1][g][lane] = s1;
  red[2][g][lane] = s2;
  __syncthreads();
  const double w = red[0][0][lane] + red[0][1][lane] + red[0][2][lane] + red[0][3][lane];
  const double m = (red[1][0][lane] + red[1][1][lane] + red[1][2][lane] + red[1][3][lane]) / w;
  double var = (red[2][0][lane] + red[2][1][lane] + red[2][2][lane] + red[2][3][lane]) / w - m * m;
  if constexpr (CENTRED) {
    __syncthreads();   // every wave has read the first pass's sums
    double sc = 0.0;
    for (int t = g; t < T; t += 4) {
      const double d = (double)ld_act(x, base + (int64_t)t * C) - m;
      sc += exp((double)(e[base + (int64_t)t * C] - mx)) * d * d;
    }
    red[2][g][lane] = sc;
    __syncthreads();
    var = (red[2][0][lane] + red[2][1][lane] + red[2][2][lane] + red[2][3][lane]) / w;
  }
  if (g == 0) {
    stats[(int64_t)b * 2 * C + c] = (float)m;
    // ASP keeps a NaN variance, as torch.clamp does; ASTP's expression clamps it, as it always has
    const double cl = CENTRED ? (var < clamp ? clamp : var) : (var > clamp ? var : clamp);
    stats[(int64_t)b * 2 * C + C + c] = (float)sqrt(cl);
  }
}

inline unsigned blocks(int64_t n) {
  SD_CHECK(n > 0 && (n + 255) / 256 <= 0x7fffffff, kErrInvalid, "ecapa: element count out of range");
  return (unsigned)((n + 255) / 256);
}

}  // namespace

void ecapa_im2col(const float* fbank, int B, int T, void* out, bool out_bf16, hipStream_t st) {
  const int64_t n = (int64_t)B * T * 400;
  ProfScope prof("ecapa_im2col", 0.0, n * (out_bf16 ? 2.0 : 4.0) + (double)B * T * 320.0, st);
  if (out_bf16)
    hipLaunchKernelGGL(ecapa_im2col_kernel<true>, dim3(blocks(n)), dim3(256), 0, st, fbank, B, T,
                       static_cast<uint16_t*>(out));
  else
    hipLaunchKernelGGL(ecapa_im2col_kernel<false>, dim3(blocks(n)), dim3(256), 0, st, fbank, B, T,
                       static_cast<float*>(out));
  SD_LAUNCH_CHECK();
}

void ecapa_add_slice(const void* a, int lda, const void* b, int ldb, int64_t rows, void* out, int ldo, bool bf16,
                     hipStream_t st) {
  const int64_t n = rows * 128;
  ProfScope prof("ecapa_add_slice", 0.0, n * (bf16 ? 2.0 : 4.0) * (b ? 3.0 : 2.0), st);
  if (bf16)
    hipLaunchKernelGGL(ecapa_add_slice_kernel<true>, dim3(blocks(n)), dim3(256), 0, st, static_cast<const uint16_t*>(a),
                       lda, static_cast<const uint16_t*>(b), ldb, rows, static_cast<uint16_t*>(out), ldo);
  else
    hipLaunchKernelGGL(ecapa_add_slice_kernel<false>, dim3(blocks(n)), dim3(256), 0, st, static_cast<const float*>(a),
                       lda, static_cast<const float*>(b), ldb, rows, static_cast<float*>(out), ldo);
  SD_LAUNCH_CHECK();
}

bool res2_chain_fused_supported(int dilation) { return dilation >= 1 && dilation <= kChainPad; }

void res2_chain_fused(const void* x, int B, int T, int d, const Res2ChainW& W, void* out, hipStream_t st) {
  SD_CHECK(x && out && B >= 1 && B <= 65535 && T >= 1 && res2_chain_fused_supported(d), kErrInvalid,
           "res2_chain_fused: 1 <= B <= 65535, T >= 1, dilation 1..4");
  const int bytes = 2 * (chain_rows(d) + 2 * kChainPad) * kChainLd * (int)sizeof(uint16_t);
  allow_dynamic_lds<&res2_chain_kernel>(2 * (chain_rows(kChainPad) + 2 * kChainPad) * kChainLd * (int)sizeof(uint16_t));
  const double flops = 2.0 * B * T * 128.0 * 384.0 * Res2ChainW::kStages;
  ProfScope prof("res2_chain_fused", flops, 2.0 * B * T * 1024 * 2.0 + 7.0 * 128 * 384 * 2, st);
  hipLaunchKernelGGL(res2_chain_kernel, dim3(cdiv(T, kChainTT), B), dim3(256), bytes, st,
                     static_cast<const uint16_t*>(x), T, d, W, static_cast<uint16_t*>(out));
  SD_LAUNCH_CHECK();
}

void ecapa_se_gate(const void* y, bool y_bf16, int B, int T, const float* w1t, const float* b1, const float* w2t,
                   const float* b2, float* mean, float* gate, hipStream_t st) {
  SD_CHECK(B >= 1 && B <= 65535 && T >= 1, kErrInvalid, "ecapa_se_gate: 1 <= B <= 65535, T >= 1");
  {
    ProfScope prof("ecapa_col_mean", 0.0, (double)B * T * 1024 * (y_bf16 ? 2.0 : 4.0), st);
    if (y_bf16)
      hipLaunchKernelGGL(ecapa_col_mean_kernel<true>, dim3(16, B), dim3(256), 0, st, static_cast<const uint16_t*>(y), T,
                         1024, mean);
    else
      hipLaunchKernelGGL(ecapa_col_mean_kernel<false>, dim3(16, B), dim3(256), 0, st, static_cast<const float*>(y), T,
                         1024, mean);
    SD_LAUNCH_CHECK();
  }
  ProfScope prof("ecapa_se_fc", 4.0 * B * 1024 * 128, 4.0 * B * (2.0 * 1024 * 128 + 2048), st);
  hipLaunchKernelGGL(ecapa_se_fc_kernel, dim3(B), dim3(1024), 0, st, mean, w1t, b1, w2t, b2, gate);
  SD_LAUNCH_CHECK();
}

void ecapa_se_apply(const void* x, int ldx, const void* y, const float* gate, int B, int T, void* out, int ldo,
                    bool bf16, hipStream_t st) {
  const int64_t rows = (int64_t)B * T, n = rows * 1024;
  ProfScope prof("ecapa_se_apply", 2.0 * n, n * (bf16 ? 2.0 : 4.0) * 3.0, st);
  if (bf16)
    hipLaunchKernelGGL(ecapa_se_apply_kernel<true>, dim3(blocks(n)), dim3(256), 0, st, static_cast<const uint16_t*>(x),
                       ldx, static_cast<const uint16_t*>(y), gate, T, rows, static_cast<uint16_t*>(out), ldo);
  else
    hipLaunchKernelGGL(ecapa_se_apply_kernel<false>, dim3(blocks(n)), dim3(256), 0, st, static_cast<const float*>(x),
                       ldx, static_cast<const float*>(y), gate, T, rows, static_cast<float*>(out), ldo);
  SD_LAUNCH_CHECK();
}

void astp_pool(const AstpArgs& a, hipStream_t st) {
  constexpr int H = 128;
  const int C = a.C;
  SD_CHECK(a.x && a.w1x && a.w1c && a.b1 && a.w2 && a.b2 && a.stats && a.ctx && a.cv && a.h && a.e, kErrInvalid,
           "astp_pool: null argument");
  SD_CHECK(C >= 64 && C % 64 == 0, kErrInvalid, "astp_pool: C must be a multiple of 64");
  SD_CHECK(a.B >= 1 && a.B <= 65535, kErrInvalid, "astp_pool: 1 <= B <= 65535");
  SD_CHECK(a.T >= 2, kErrShape, "ASTP needs at least 2 frames (the unbiased variance of one frame is NaN)");
  SD_CHECK(!a.x_bf16 || a.x32, kErrInvalid, "astp_pool: a bf16 map needs the fp32 scratch copy");
  const int64_t rows = (int64_t)a.B * a.T;
  const dim3 grid(C / 64, a.B);
  {
    ProfScope prof("astp_context", 0.0, (double)rows * C * (a.x_bf16 ? 4.0 : 8.0), st);
    if (a.x_bf16)
      hipLaunchKernelGGL(astp_context_kernel<true>, grid, dim3(256), 0, st, static_cast<const uint16_t*>(a.x), a.T, C,
                         a.ctx, a.x32);
    else
      hipLaunchKernelGGL(astp_context_kernel<false>, grid, dim3(256), 0, st, static_cast<const float*>(a.x), a.T, C,
                         a.ctx, static_cast<float*>(nullptr));
    SD_LAUNCH_CHECK();
  }
  // the context half of linear1, once per window: cv = W1[:, C:] [mean | std] + b1
  seg_linear(a.ctx, a.B, 2 * C, a.w1c, a.b1, H, a.cv, st);
  // the per-frame half and linear2 on the exact (or bf16x3) GEMM: fp32 in every mode
  const float* x32 = a.x_bf16 ? a.x32 : static_cast<const float*>(a.x);
  conv_gemm(linear_args(x32, (int)rows, C, C, a.w1x, H, a.h, H), false, st);
  hipLaunchKernelGGL(astp_tanh_kernel, dim3(blocks(rows * H)), dim3(256), 0, st, a.h, a.cv, a.T, rows);
  SD_LAUNCH_CHECK();
  ConvGemmArgs p = linear_args(a.h, (int)rows, H, H, a.w2, C, a.e, C);
  p.beta = a.b2;
  conv_gemm(p, false, st);
  softmax_stats(a.x, a.x_bf16, a.e, a.B, a.T, C, false, a.stats, st);
}

void softmax_stats(const void* x, bool x_bf16, const float* e, int B, int T, int C, bool asp, float* stats,
                   hipStream_t st) {
  SD_CHECK(x && e && stats && B >= 1 && B <= 65535 && T >= 1 && C >= 64 && C % 64 == 0, kErrInvalid,
           "softmax_stats: C must be a multiple of 64, 1 <= B <= 65535, T >= 1");
  const dim3 grid(C / 64, B);
  ProfScope prof("astp_softmax_stats", 0.0, (double)B * T * C * 2.0 * ((x_bf16 ? 2.0 : 4.0) + 4.0), st);
  // ASP's clamp is the fp32 constant the reference's float tensors see, so T == 1 gives its sqrt(1e-5) bit for bit
  const double clamp = asp ? (double)1e-5f : 1e-7;
  const uint16_t* xb = static_cast<const uint16_t*>(x);
  const float* xf = static_cast<const float*>(x);
  if (x_bf16 && asp)
    hipLaunchKernelGGL((astp_softmax_stats_kernel<true, true>), grid, dim3(256), 0, st, xb, e, T, C, clamp, stats);
  else if (x_bf16)
    hipLaunchKernelGGL((astp_softmax_stats_kernel<true, false>), grid, dim3(256), 0, st, xb, e, T, C, clamp, stats);
  else if (asp)
    hipLaunchKernelGGL((astp_softmax_stats_kernel<false, true>), grid, dim3(256), 0, st, xf, e, T, C, clamp, stats);
  else
    hipLaunchKernelGGL((astp_softmax_stats_kernel<false, false>), grid, dim3(256), 0, st, xf, e, T, C, clamp, stats);
  SD_LAUNCH_CHECK();
}

void asp_pool(const AspArgs& a, hipStream_t st) {
  constexpr int H = 128;
  SD_CHECK(a.x && a.w1 && a.b1 && a.bn_s && a.bn_h && a.w2 && a.b2 && a.stats && a.h && a.e, kErrInvalid,
           "asp_pool: null argument");
  SD_CHECK(a.B >= 1 && a.B <= 65535 && a.T >= 1 && a.C >= 64 && a.C % 64 == 0, kErrInvalid,
           "asp_pool: C must be a multiple of 64, 1 <= B <= 65535, T >= 1");
  SD_CHECK(!a.x_bf16 || a.x32, kErrInvalid, "asp_pool: a bf16 map needs the fp32 scratch copy");
  const int64_t rows = (int64_t)a.B * a.T;
  SD_CHECK(rows * a.C < (1ll << 31), kErrInvalid, "asp_pool: map out of range");
  const float* x32 = static_cast<const float*>(a.x);
  if (a.x_bf16) {
    bf16_to_f32(a.x, rows * a.C, a.x32, st);
    x32 = a.x32;
  }
  // attention.0 -> ReLU -> attention.2 (BatchNorm1d AFTER the ReLU: the post-activation affine, never folded)
  ConvGemmArgs p = linear_args(x32, (int)rows, a.C, a.C, a.w1, H, a.h, H);
  p.beta = a.b1; p.act = kActRelu; p.post_scale = a.bn_s; p.post_shift = a.bn_h;
  conv_gemm(p, false, st);
  // attention.3, on at least kAspMinRows rows (h and e hold that many; the surplus rows are scratch nobody reads):
  // conv_gemm hands <= 16 rows to the skinny kernel, whose sums are ordered differently, and a chunk's embedding must
  // not depend on how many chunks share the call
  ConvGemmArgs q = linear_args(a.h, (int)std::max<int64_t>(rows, kAspMinRows), H, H, a.w2, a.C, a.e, a.C);
  q.beta = a.b2;
  conv_gemm(q, false, st);
  softmax_stats(a.x, a.x_bf16, a.e, a.B, a.T, a.C, true, a.stats, st);
}

}  // namespace sd
