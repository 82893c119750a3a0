// ReDimNetB2 kernels on gfx950 (egs/magicdata-ramc/ts_vad2/redimnet_wespeaker.py): what the trunk (redimnet.cpp) runs
// besides conv_gemm, layernorm and attention.
//
//   redim_stem            Conv2d(1 -> 16, 3x3) + channels-first LayerNorm of the fbank map (:670-673)
//   redim_block2d_kernel  a whole 2-D ConvNeXt-like block in one launch, bf16 (:135-165; described at the kernel)
//   redim_gconv_kernel    the generic arm's grouped 3x3 conv + folded BatchNorm2d + erf GELU
//   redim_dwconv1d        the 1-D block's depthwise conv over time + folded BatchNorm1d + erf GELU (:586-607)
//   redim_stage_mix       the softmax-weighted sum over the earlier stage outputs (:768-772)
//
// Every map is channel-last (B, T, 1152) with channel f * c + ch, fp32 or bf16 bits; a kernel reaches a window's frames
// through its own (b, t) only, and every tap outside [0, T) x [0, f) reads as zero ("same" padding).
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "prof.h"

namespace sd {
namespace {

constexpr int kCF = kRedimCF;

__device__ __forceinline__ void ld4(const float* p, float v[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void ld4(const uint16_t* p, float v[4]) {
  const uint2 t = *reinterpret_cast<const uint2*>(p);
  v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
  v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
}
__device__ __forceinline__ void st4(float* p, const float v[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void st4(uint16_t* p, const float v[4]) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
}

// one tap of the grouped conv: 4 inputs x 4 outputs, w = [out 4][in 4]
__device__ __forceinline__ void gtap(const float xv[4], const float* __restrict__ w, float acc[4]) {
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const float4 q = *reinterpret_cast<const float4*>(w + o * 4);
    acc[o] = fmaf(xv[0], q.x, fmaf(xv[1], q.y, fmaf(xv[2], q.z, fmaf(xv[3], q.w, acc[o]))));
  }
}

// ---------------------------------------------------------------- stem
template <bool BF>
__global__ __launch_bounds__(256) void redim_stem_kernel(const float* __restrict__ fb, int T, int64_t n,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ g, const float* __restrict__ beta,
                                                         act_t<BF>* __restrict__ out) {
  constexpr int F = 72, C = 16;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (b, t, f)
  if (i >= n) return;
  const int fi = (int)(i % F);
  const int64_t bt = i / F;
  const int t = (int)(bt % T);
  float x[9];   // [df][dt]
#pragma unroll
  for (int df = 0; df < 3; ++df)
#pragma unroll
    for (int dt = 0; dt < 3; ++dt) {
      const int ff = fi + df - 1, tt = t + dt - 1;
      x[df * 3 + dt] = (ff >= 0 && ff < F && tt >= 0 && tt < T) ? fb[(bt + dt - 1) * F + ff] : 0.f;
    }
  float v[C], u = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float a = bias[c];
#pragma unroll
    for (int k = 0; k < 9; ++k) a = fmaf(x[k], w[c * 9 + k], a);
    v[c] = a;
    u += a;
  }
  u *= 1.f / C;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) s += (v[c] - u) * (v[c] - u);
  const float d = sqrtf(s * (1.f / C) + 1e-6f);
#pragma unroll
  for (int c = 0; c < C; c += 4) {
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = g[c + j] * ((v[c + j] - u) / d) + beta[c + j];
    st4(out + i * C + c, y);
  }
}

// ---------------------------------------------------------------- generic arm: grouped conv + BN + GELU
template <bool BF>
__global__ __launch_bounds__(256) void redim_gconv_kernel(const act_t<BF>* __restrict__ x, int T, int c, int64_t items,
                                                          const float* __restrict__ dw, const float* __restrict__ dw_b,
                                                          act_t<BF>* __restrict__ h) {
  extern __shared__ __attribute__((aligned(16))) float gw[];   // 36 c weights, then c biases
  const int G = c / 4, f = kCF / c;
  for (int i = threadIdx.x; i < 36 * c; i += 256) gw[i] = dw[i];
  for (int i = threadIdx.x; i < c; i += 256) gw[36 * c + i] = dw_b[i];
  __syncthreads();
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;   // (b, t, f, group)
  if (it >= items) return;
  const int g = (int)(it % G);
  const int64_t pix = it / G;
  const int fi = (int)(pix % f);
  const int64_t bt = pix / f;
  const int t = (int)(bt % T);
  float acc[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) acc[o] = gw[36 * c + 4 * g + o];
  for (int dt = 0; dt < 3; ++dt) {
    const int tt = t + dt - 1;
    if (tt < 0 || tt >= T) continue;
    for (int df = 0; df < 3; ++df) {
      const int ff = fi + df - 1;
      if (ff < 0 || ff >= f) continue;
      float xv[4];
      ld4(x + (bt + dt - 1) * kCF + ff * c + 4 * g, xv);
      gtap(xv, gw + ((df * 3 + dt) * G + g) * 16, acc);
    }
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) acc[o] = gelu_erf(acc[o]);
  st4(h + pix * c + 4 * g, acc);
}

// ---------------------------------------------------------------- fused 2-D block (bf16)
// One workgroup = kB2TT time rows of one window, all f frequency rows, all c channels.  xs: the kB2TT + 2 staged input
// rows (row 0 is frame t0 - 1; frames outside [0, T) are zeros).  Phase 1, VALU: each thread takes (pixel, group) items
// of ONE group, 9 taps x 4 x 4 FMAs from xs with the group's folded weights in registers, GELU, 4 bf16 into hs
// (pixel-major, rows of C + 8: the 16 rows of a fragment read spread over the banks).  Phase 2, MFMA: the waves share
// the (16 pixels x 16 outputs) tiles of out = hs W^T, A fragments from hs, B fragments straight from the packed (C, C)
// weight in global memory (<= 32 KB, L2-resident); K = 16 is run as a 32-deep step whose upper half is zero.
// Epilogue: + bias + the skip, written in place over the skip value in xs, then the finished rows go to global as
// 16-B stores.  The rounding points are the generic arm's: h to bf16, the sum to bf16.
constexpr int kB2TT = 8;

template <int C>
__global__ __launch_bounds__(256) void redim_block2d_kernel(const uint16_t* __restrict__ x, int T,
                                                            const float* __restrict__ dw,
                                                            const float* __restrict__ dw_b,
                                                            const uint16_t* __restrict__ pw,
                                                            const float* __restrict__ pw_b,
                                                            uint16_t* __restrict__ out) {
  constexpr int F = kCF / C, G = C / 4, NP = kB2TT * F, MT = (NP + 15) / 16, HL = C + 8, NT = C / 16, KS = (C + 31) / 32;
  __shared__ __attribute__((aligned(16))) uint16_t xs[(kB2TT + 2) * kCF];
  __shared__ __attribute__((aligned(16))) uint16_t hs[MT * 16 * HL];
  __shared__ __attribute__((aligned(16))) float gw[37 * C];
  static_assert(sizeof(uint16_t) * ((kB2TT + 2) * kCF + MT * 16 * HL) + sizeof(float) * 37 * C <= 65536, "LDS budget");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lrow = lane & 15, lk = lane >> 4;
  const int b = blockIdx.y, t0 = blockIdx.x * kB2TT;
  const uint16_t* xb = x + (int64_t)b * T * kCF;
  uint16_t* ob = out + (int64_t)b * T * kCF;
  for (int q = tid; q < (kB2TT + 2) * (kCF / 8); q += 256) {
    const int r = q / (kCF / 8), c8 = (q % (kCF / 8)) * 8, t = t0 - 1 + r;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (t >= 0 && t < T) v = *reinterpret_cast<const uint4*>(xb + (int64_t)t * kCF + c8);
    *reinterpret_cast<uint4*>(xs + r * kCF + c8) = v;
  }
  for (int i = tid; i < 36 * C; i += 256) gw[i] = dw[i];
  for (int i = tid; i < C; i += 256) gw[36 * C + i] = dw_b[i];
  __syncthreads();
  // phase 1: grouped conv + folded BN + GELU.  256 % G == 0, so a thread's items all belong to one group: its 9 x 16
  // weights and 4 biases live in registers, and only the 9 input vectors of an item come from LDS.
  {
    const int g = tid % G;
    float w[9][16], bias4[4];
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
      for (int q = 0; q < 16; q += 4) {
        const float4 v = *reinterpret_cast<const float4*>(gw + (tp * G + g) * 16 + q);
        w[tp][q] = v.x; w[tp][q + 1] = v.y; w[tp][q + 2] = v.z; w[tp][q + 3] = v.w;
      }
#pragma unroll
    for (int o = 0; o < 4; ++o) bias4[o] = gw[36 * C + 4 * g + o];
    for (int p = tid / G; p < NP; p += 256 / G) {
      const int tl = p / F, fi = p % F;
      float acc[4] = {bias4[0], bias4[1], bias4[2], bias4[3]};
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
#pragma unroll
        for (int df = 0; df < 3; ++df) {
          const int ff = fi + df - 1;
          if (ff < 0 || ff >= F) continue;
          float xv[4];
          ld4(xs + (tl + dt) * kCF + ff * C + 4 * g, xv);
#pragma unroll
          for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) acc[o] = fmaf(xv[ci], w[df * 3 + dt][o * 4 + ci], acc[o]);
        }
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) acc[o] = gelu_erf(acc[o]);
      st4(hs + p * HL + 4 * g, acc);
    }
  }
  __syncthreads();
  // phase 2: pointwise conv on MFMA + bias + skip.  A wave keeps one 16-column panel of the weight in registers (loaded
  // once from global) and walks its share of the 16-pixel row tiles: WN waves across the panels, WM across the rows.
  constexpr int WN = NT < 4 ? NT : 4, WM = 4 / WN;
  const int wn = wv % WN, wm = wv / WN;
  for (int nt = wn; nt < NT; nt += WN) {
    const int n = nt * 16 + lrow;
    bf16x8 bw[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = ks * 32 + lk * 8;
      bw[ks] = bf16x8{};
      if (k < C) bw[ks] = *reinterpret_cast<const bf16x8*>(pw + n * C + k);
    }
    const float bias = pw_b[n];
    for (int mt = wm; mt < MT; mt += WM) {
      floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int k = ks * 32 + lk * 8;
        bf16x8 a = {};
        // c = 128: rows 72 .. 79 of the last tile were never written; they feed only their own (discarded) outputs
        if (k < C) a = *reinterpret_cast<const bf16x8*>(hs + (mt * 16 + lrow) * HL + k);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bw[ks], acc, 0, 0, 0);
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int p = mt * 16 + lk * 4 + rr;
        if (p >= NP) continue;
        const int tl = p / F, fi = p % F;
        // in place over the skip value: no other lane reads or writes this element of xs after phase 1
        uint16_t* e = xs + (tl + 1) * kCF + fi * C + n;
        *e = f2bf_bits(acc[rr] + bias + bf_bits2f(*e));
      }
    }
  }
  __syncthreads();
  // the finished rows 1 .. kB2TT of xs -> global, 16 B per lane
  for (int q = tid; q < kB2TT * (kCF / 8); q += 256) {
    const int r = q / (kCF / 8), c8 = (q % (kCF / 8)) * 8, t = t0 + r;
    if (t < T) *reinterpret_cast<uint4*>(ob + (int64_t)t * kCF + c8) = *reinterpret_cast<const uint4*>(xs + (r + 1) * kCF + c8);
  }
}

// ---------------------------------------------------------------- depthwise conv over time + BN + GELU
constexpr int kDwCH = 48, kDwTT = 64, kDwMaxK = 59;

template <bool BF>
__global__ __launch_bounds__(192) void redim_dwconv1d_kernel(const float* __restrict__ x, int T, int hC, int k,
                                                             const float* __restrict__ wt,
                                                             const float* __restrict__ bias,
                                                             act_t<BF>* __restrict__ y) {
  __shared__ float xs[(kDwTT + kDwMaxK - 1) * kDwCH];
  __shared__ float ws[kDwMaxK * kDwCH];
  const int tid = threadIdx.x, c = tid % kDwCH, sub = tid / kDwCH;
  const int b = blockIdx.z, ch0 = blockIdx.y * kDwCH, t0 = blockIdx.x * kDwTT, half = k / 2;
  const int rows = kDwTT + k - 1;
  const float* xb = x + (int64_t)b * T * hC + ch0;
  for (int q = tid; q < rows * kDwCH; q += 192) {
    const int r = q / kDwCH, cc = q % kDwCH, t = t0 - half + r;
    xs[q] = (t >= 0 && t < T) ? xb[(int64_t)t * hC + cc] : 0.f;
  }
  for (int q = tid; q < k * kDwCH; q += 192) ws[q] = wt[(q / kDwCH) * hC + ch0 + q % kDwCH];
  __syncthreads();
  const float bv = bias[ch0 + c];
  for (int tl = sub; tl < kDwTT; tl += 4) {
    const int t = t0 + tl;
    if (t >= T) break;
    float acc = bv;
    for (int j = 0; j < k; ++j) acc = fmaf(xs[(tl + j) * kDwCH + c], ws[j * kDwCH + c], acc);
    st_act(y, ((int64_t)b * T + t) * hC + ch0 + c, gelu_erf(acc));
  }
}

// ---------------------------------------------------------------- stage mix
template <bool BF>
__global__ __launch_bounds__(256) void redim_stage_mix_kernel(RedimMixArgs a, int64_t n4, act_t<BF>* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // groups of 4 channels
  if (i >= n4) return;
  const int ch = (int)(i % (kCF / 4)) * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < a.n; ++k) {
    float v[4];
    ld4(static_cast<const act_t<BF>*>(a.x[k]) + i * 4, v);
    const float4 w = *reinterpret_cast<const float4*>(a.w + k * kCF + ch);
    acc[0] = fmaf(w.x, v[0], acc[0]); acc[1] = fmaf(w.y, v[1], acc[1]);
    acc[2] = fmaf(w.z, v[2], acc[2]); acc[3] = fmaf(w.w, v[3], acc[3]);
  }
  st4(y + i * 4, acc);
}

inline unsigned blocks(int64_t n) {
  SD_CHECK(n > 0 && (n + 255) / 256 <= 0x7fffffff, kErrInvalid, "redimnet: element count out of range");
  return (unsigned)((n + 255) / 256);
}

bool block_width(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }

template <int C>
void launch_block2d(const void* x, int B, int T, const RedimBlock2dW& W, void* out, hipStream_t st) {
  hipLaunchKernelGGL(redim_block2d_kernel<C>, dim3(cdiv(T, kB2TT), B), dim3(256), 0, st, static_cast<const uint16_t*>(x),
                     T, W.dw, W.dw_b, static_cast<const uint16_t*>(W.pw), W.pw_b, static_cast<uint16_t*>(out));
}

}  // namespace

void redim_pack_dw(const float* w, const float* bias, const float* s, const float* h, int c, std::vector<float>& dw,
                   std::vector<float>& dw_b) {
  const int G = c / 4;
  dw.assign((size_t)36 * c, 0.f);
  dw_b.assign(c, 0.f);
  for (int co = 0; co < c; ++co) {
    const int g = co / 4, o = co % 4;
    for (int ci = 0; ci < 4; ++ci)
      for (int df = 0; df < 3; ++df)
        for (int dt = 0; dt < 3; ++dt)
          dw[((size_t)(df * 3 + dt) * G + g) * 16 + o * 4 + ci] =
              (float)((double)w[((size_t)co * 4 + ci) * 9 + df * 3 + dt] * s[co]);
    dw_b[co] = (float)((double)bias[co] * s[co] + h[co]);
  }
}

void redim_stem(const float* fbank, int B, int T, const float* w, const float* bias, const float* g, const float* beta,
                void* out, bool out_bf16, hipStream_t st) {
  SD_CHECK(fbank && w && bias && g && beta && out && B >= 1 && T >= 1, kErrInvalid, "redim_stem: bad argument");
  const int64_t n = (int64_t)B * T * 72;
  ProfScope prof("redim_stem", 2.0 * n * 16 * 9, n * (4.0 + 16 * (out_bf16 ? 2.0 : 4.0)), st);
  if (out_bf16)
    hipLaunchKernelGGL(redim_stem_kernel<true>, dim3(blocks(n)), dim3(256), 0, st, fbank, T, n, w, bias, g, beta,
                       static_cast<uint16_t*>(out));
  else
    hipLaunchKernelGGL(redim_stem_kernel<false>, dim3(blocks(n)), dim3(256), 0, st, fbank, T, n, w, bias, g, beta,
                       static_cast<float*>(out));
  SD_LAUNCH_CHECK();
}

void redim_gconv3x3(const void* x, bool bf16, int B, int T, int c, const float* dw, const float* dw_b, void* h,
                    hipStream_t st) {
  SD_CHECK(x && dw && dw_b && h && x != h && B >= 1 && T >= 1 && block_width(c), kErrInvalid,
           "redim_gconv3x3: c must be 16, 32, 64 or 128, B >= 1, T >= 1, h apart from x");
  const int64_t items = (int64_t)B * T * (kCF / 4), el = (int64_t)B * T * kCF;
  ProfScope prof("redim_gconv3x3", 2.0 * el * 36, 2.0 * el * (bf16 ? 2.0 : 4.0), st);
  const size_t lds = (size_t)37 * c * sizeof(float);
  if (bf16)
    hipLaunchKernelGGL(redim_gconv_kernel<true>, dim3(blocks(items)), dim3(256), lds, st,
                       static_cast<const uint16_t*>(x), T, c, items, dw, dw_b, static_cast<uint16_t*>(h));
  else
    hipLaunchKernelGGL(redim_gconv_kernel<false>, dim3(blocks(items)), dim3(256), lds, st,
                       static_cast<const float*>(x), T, c, items, dw, dw_b, static_cast<float*>(h));
  SD_LAUNCH_CHECK();
}

void redim_block2d_fused(const void* x, int B, int T, int c, const RedimBlock2dW& W, void* out, hipStream_t st) {
  SD_CHECK(x && out && x != out && W.dw && W.dw_b && W.pw && W.pw_b && B >= 1 && B <= 65535 && T >= 1 && block_width(c),
           kErrInvalid, "redim_block2d_fused: c must be 16, 32, 64 or 128, 1 <= B <= 65535, T >= 1, out apart from x");
  const double el = (double)B * T * kCF;
  ProfScope prof("redim_block2d", 2.0 * el * (36 + c), 2.0 * el * 2.0, st);
  switch (c) {
    case 16: launch_block2d<16>(x, B, T, W, out, st); break;
    case 32: launch_block2d<32>(x, B, T, W, out, st); break;
    case 64: launch_block2d<64>(x, B, T, W, out, st); break;
    default: launch_block2d<128>(x, B, T, W, out, st); break;
  }
  SD_LAUNCH_CHECK();
}

void redim_block2d(const void* x, int B, int T, int c, const RedimBlock2dW& W, void* tmp, void* out, bool bf16,
                   bool generic, hipStream_t st) {
  if (!generic) {
    SD_CHECK(bf16, kErrInvalid, "redim_block2d: the fused kernel is bf16 (fp32 and bf16x3 take the generic arm)");
    redim_block2d_fused(x, B, T, c, W, out, st);
    return;
  }
  SD_CHECK(tmp && out && x != out && tmp != out && W.pw && W.pw_b, kErrInvalid, "redim_block2d: bad argument");
  SD_CHECK((int64_t)B * T * (kCF / 16) < (1ll << 31), kErrInvalid, "redim_block2d: map out of range");
  redim_gconv3x3(x, bf16, B, T, c, W.dw, W.dw_b, tmp, st);
  ConvGemmArgs p = linear_args(tmp, B * T * (kCF / c), c, c, W.pw, c, out, c);
  p.a_bf16 = bf16; p.out_bf16 = bf16;
  p.beta = W.pw_b;
  p.res = x; p.res_bf16 = bf16; p.res_ld = c;
  conv_gemm(p, bf16, st);
}

void redim_dwconv1d(const float* x, int B, int T, int hC, int k, const float* wt, const float* bias, void* y,
                    bool y_bf16, hipStream_t st) {
  SD_CHECK(x && wt && bias && y && B >= 1 && B <= 65535 && T >= 1 && hC >= kDwCH && hC % kDwCH == 0 && k >= 1 &&
               k <= kDwMaxK && k % 2 == 1,
           kErrInvalid, "redim_dwconv1d: hC must be a multiple of 48, k odd and <= 59, 1 <= B <= 65535, T >= 1");
  const double el = (double)B * T * hC;
  ProfScope prof("redim_dwconv1d", 2.0 * el * k, el * (4.0 + (y_bf16 ? 2.0 : 4.0)), st);
  const dim3 grid(cdiv(T, kDwTT), hC / kDwCH, B);
  if (y_bf16)
    hipLaunchKernelGGL(redim_dwconv1d_kernel<true>, grid, dim3(192), 0, st, x, T, hC, k, wt, bias,
                       static_cast<uint16_t*>(y));
  else
    hipLaunchKernelGGL(redim_dwconv1d_kernel<false>, grid, dim3(192), 0, st, x, T, hC, k, wt, bias,
                       static_cast<float*>(y));
  SD_LAUNCH_CHECK();
}

void redim_stage_mix(const RedimMixArgs& a, int64_t rows, void* y, bool bf16, hipStream_t st) {
  SD_CHECK(a.n >= 2 && a.n <= RedimMixArgs::kMax && a.w && y && rows >= 1, kErrInvalid,
           "redim_stage_mix: 2 to 7 inputs, rows >= 1");
  for (int k = 0; k < a.n; ++k) SD_CHECK(a.x[k] && a.x[k] != y, kErrInvalid, "redim_stage_mix: null or aliased input");
  const int64_t n4 = rows * (kCF / 4);
  ProfScope prof("redim_stage_mix", 2.0 * n4 * 4 * a.n, (double)n4 * 4 * (a.n + 1) * (bf16 ? 2.0 : 4.0), st);
  if (bf16)
    hipLaunchKernelGGL(redim_stage_mix_kernel<true>, dim3(blocks(n4)), dim3(256), 0, st, a, n4,
                       static_cast<uint16_t*>(y));
  else
    hipLaunchKernelGGL(redim_stage_mix_kernel<false>, dim3(blocks(n4)), dim3(256), 0, st, a, n4,
                       static_cast<float*>(y));
  SD_LAUNCH_CHECK();
}

}  // namespace sd
