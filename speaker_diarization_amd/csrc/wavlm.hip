// WavLM kernels for gfx950 (declarations and contracts in kernels.h): the waveform conv layer with its norm, the
// grouped 128-tap positional conv, the relative-position bias table and self-attention with the gated bias; for TS-VAD's
// WavLM speech encoders the layer-weighted sum, its projection + LayerNorm and the waveform window gather.
#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "launch.h"
#include "prof.h"

namespace sd {

namespace {

constexpr int kC = 512;            // conv front end channels
constexpr int kL0K = 10;           // layer 0 taps
constexpr int kL0S = 5;            // layer 0 stride
constexpr int kL0Block = 256;      // frames per workgroup: 64 per wave
constexpr int kL0Samples = kL0Block * kL0S + kL0K - kL0S;   // samples a workgroup's frames read
constexpr int kCPL = kC / 64;      // channels per lane: lane + 64 j

// The samples of frames [f0, f0 + 256) of one window, zeros past its end (only frames >= T0 read those).
__device__ __forceinline__ void l0_stage(const float* __restrict__ wav, int n, int f0, float* s) {
  const int64_t base = (int64_t)f0 * kL0S;
  for (int i = threadIdx.x; i < kL0Samples; i += 256) s[i] = base + i < n ? wav[base + i] : 0.f;
}

__device__ __forceinline__ void l0_weights(const float* __restrict__ w, int lane, float (&wr)[kCPL][kL0K]) {
#pragma unroll
  for (int j = 0; j < kCPL; ++j)
#pragma unroll
    for (int k = 0; k < kL0K; ++k) wr[j][k] = w[(lane + 64 * j) * kL0K + k];
}

// conv outputs of the lane's 8 channels at local frame fl (every lane reads the same 10 samples: an LDS broadcast)
__device__ __forceinline__ void l0_conv(const float* s, int fl, const float (&wr)[kCPL][kL0K], float (&v)[kCPL]) {
  float x[kL0K];
#pragma unroll
  for (int k = 0; k < kL0K; ++k) x[k] = s[fl * kL0S + k];
#pragma unroll
  for (int j = 0; j < kCPL; ++j) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < kL0K; ++k) a = fmaf(wr[j][k], x[k], a);
    v[j] = a;
  }
}

// partial[((b * parts + p) * 3 + {0, 1, 2}) * 512 + c] = (count, mean, M2) of the 64 frames of wave p % 4 of block p / 4
__global__ __launch_bounds__(256) void wavlm_l0_stats_kernel(const float* __restrict__ wav, int n, int T0,
                                                             const float* __restrict__ w, float* __restrict__ partial) {
  __shared__ float s[kL0Samples];
  const int b = blockIdx.y, f0 = blockIdx.x * kL0Block, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  l0_stage(wav + (int64_t)b * n, n, f0, s);
  float wr[kCPL][kL0K];
  l0_weights(w, lane, wr);
  __syncthreads();
  const int fl0 = wave * 64;
  const int cnt = min(64, max(0, T0 - (f0 + fl0)));
  float mean[kCPL], m2[kCPL], v[kCPL];
#pragma unroll
  for (int j = 0; j < kCPL; ++j) mean[j] = m2[j] = 0.f;
  if (cnt > 0) {
    for (int i = 0; i < cnt; ++i) {
      l0_conv(s, fl0 + i, wr, v);
#pragma unroll
      for (int j = 0; j < kCPL; ++j) mean[j] += v[j];
    }
#pragma unroll
    for (int j = 0; j < kCPL; ++j) mean[j] /= (float)cnt;
    for (int i = 0; i < cnt; ++i) {
      l0_conv(s, fl0 + i, wr, v);
#pragma unroll
      for (int j = 0; j < kCPL; ++j) {
        const float d = v[j] - mean[j];
        m2[j] = fmaf(d, d, m2[j]);
      }
    }
  }
  const int parts = gridDim.x * 4, p = blockIdx.x * 4 + wave;
  float* o = partial + ((int64_t)b * parts + p) * 3 * kC;
#pragma unroll
  for (int j = 0; j < kCPL; ++j) {
    const int c = lane + 64 * j;
    o[c] = (float)cnt;
    o[kC + c] = mean[j];
    o[2 * kC + c] = m2[j];
  }
}

// ss[(b * 2 + 0) * 512 + c] = g rstd, [(b * 2 + 1) * 512 + c] = beta - mean g rstd (biased variance, eps 1e-5)
__global__ __launch_bounds__(256) void wavlm_l0_finalize_kernel(const float* __restrict__ partial, int parts,
                                                                const float* __restrict__ g,
                                                                const float* __restrict__ beta, float* __restrict__ ss) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= kC) return;
  double cnt = 0.0, mean = 0.0, m2 = 0.0;
  for (int p = 0; p < parts; ++p) {
    const float* o = partial + ((int64_t)b * parts + p) * 3 * kC;
    const double nb = o[c];
    if (nb == 0.0) continue;
    const double mb = o[kC + c], sb = o[2 * kC + c], tot = cnt + nb, d = mb - mean;
    mean += d * nb / tot;
    m2 += sb + d * d * cnt * nb / tot;
    cnt = tot;
  }
  const double rstd = 1.0 / sqrt(m2 / cnt + 1e-5);
  const float scale = (float)(g[c] * rstd);
  ss[((int64_t)b * 2) * kC + c] = scale;
  ss[((int64_t)b * 2 + 1) * kC + c] = (float)(beta[c] - mean * g[c] * rstd);
}

// LN false: y = gelu(conv * ss_scale + ss_shift) (p0 / p1 = the window's scale / shift rows); LN true: y =
// gelu(LayerNorm_c(conv) p0 + p1) (p0 / p1 = the affine).
template <bool LN, bool BF>
__global__ __launch_bounds__(256) void wavlm_l0_norm_kernel(const float* __restrict__ wav, int n, int T0,
                                                            const float* __restrict__ w, const float* __restrict__ p0,
                                                            const float* __restrict__ p1, int64_t p_stride,
                                                            act_t<BF>* __restrict__ out) {
  __shared__ float s[kL0Samples];
  const int b = blockIdx.y, f0 = blockIdx.x * kL0Block, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  l0_stage(wav + (int64_t)b * n, n, f0, s);
  float wr[kCPL][kL0K], a0[kCPL], a1[kCPL], v[kCPL];
  l0_weights(w, lane, wr);
#pragma unroll
  for (int j = 0; j < kCPL; ++j) {
    a0[j] = p0[(int64_t)b * p_stride + lane + 64 * j];
    a1[j] = p1[(int64_t)b * p_stride + lane + 64 * j];
  }
  __syncthreads();
  const int fl0 = wave * 64;
  const int cnt = min(64, max(0, T0 - (f0 + fl0)));
  for (int i = 0; i < cnt; ++i) {
    l0_conv(s, fl0 + i, wr, v);
    if (LN) {
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < kCPL; ++j) sum += v[j];
      const float mean = warp_sum(sum) * (1.f / kC);
      float sq = 0.f;
#pragma unroll
      for (int j = 0; j < kCPL; ++j) {
        v[j] -= mean;
        sq = fmaf(v[j], v[j], sq);
      }
      const float rstd = rsqrtf(warp_sum(sq) * (1.f / kC) + 1e-5f);
#pragma unroll
      for (int j = 0; j < kCPL; ++j) v[j] *= rstd;
    }
    act_t<BF>* o = out + ((int64_t)b * T0 + f0 + fl0 + i) * kC;
#pragma unroll
    for (int j = 0; j < kCPL; ++j) st_act(o, lane + 64 * j, gelu_erf(fmaf(v[j], a0[j], a1[j])));
  }
}

template <bool BF>
__global__ __launch_bounds__(256) void wavlm_ln_gelu_kernel(act_t<BF>* __restrict__ x, int64_t rows,
                                                            const float* __restrict__ g, const float* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  act_t<BF>* r = x + row * kC;
  float v[kCPL], sum = 0.f;
#pragma unroll
  for (int j = 0; j < kCPL; ++j) {
    v[j] = ld_act(r, lane + 64 * j);
    sum += v[j];
  }
  const float mean = warp_sum(sum) * (1.f / kC);
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < kCPL; ++j) {
    v[j] -= mean;
    sq = fmaf(v[j], v[j], sq);
  }
  const float rstd = rsqrtf(warp_sum(sq) * (1.f / kC) + 1e-5f);
#pragma unroll
  for (int j = 0; j < kCPL; ++j) {
    const int c = lane + 64 * j;
    st_act(r, c, gelu_erf(fmaf(v[j] * rstd, g[c], b[c])));
  }
}

template <bool BF>
__global__ __launch_bounds__(256) void wavlm_add_kernel(float* __restrict__ x, const act_t<BF>* __restrict__ t, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] += ld_act(t, i);
}

// ---- positional conv
constexpr int kPosTaps = 128, kPosPad = 64, kPosTile = 64;
constexpr int kPosRows = kPosTile + kPosTaps - 1;   // staged frames: [t0 - 64, t0 + 64 + 63)

template <bool BF, int DG>
__global__ __launch_bounds__(256) void wavlm_pos_conv_kernel(const float* __restrict__ x, int T, int D,
                                                             const act_t<BF>* __restrict__ wt,
                                                             const float* __restrict__ bias, float* __restrict__ out) {
  using lt = act_t<BF>;
  constexpr int NT = DG / 16, K = kPosTaps * DG;
  // row j = frame t0 - 64 + j; the A row of output frame t0 + m is the K values from xs[m * DG] on (tap-major)
  __shared__ __attribute__((aligned(16))) lt xs[kPosRows * DG];
  const int t0 = blockIdx.x * kPosTile, g = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  for (int i = tid; i < kPosRows * DG; i += 256) {
    const int j = i / DG, c = i - j * DG, t = t0 - kPosPad + j;
    const float v = (t >= 0 && t < T) ? x[((int64_t)b * T + t) * D + g * DG + c] : 0.f;
    if constexpr (BF) xs[i] = f2bf_bits(v); else xs[i] = v;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, lrow = lane & 15, lk = lane >> 4;
  if (t0 + wave * 16 >= T) return;   // no barrier follows
  floatx4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
  const lt* arow = xs + (wave * 16 + lrow) * DG;
  const lt* wrow = wt + ((int64_t)g * DG + lrow) * K;
  if constexpr (BF) {
#pragma unroll 4
    for (int ks = 0; ks < K / 32; ++ks) {
      const int k = ks * 32 + lk * 8;
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(arow + k);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bf16x8 w8 = *reinterpret_cast<const bf16x8*>(wrow + (int64_t)nt * 16 * K + k);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w8, acc[nt], 0, 0, 0);
      }
    }
  } else {
    // 16 k per step as four MFMAs of 4: slot lk of MFMA j takes k = 16 s + 4 lk + j in A and B alike, so both
    // operands are one 16-byte read per lane
#pragma unroll 2
    for (int s = 0; s < K / 16; ++s) {
      const int k = s * 16 + lk * 4;
      const floatx4 a = *reinterpret_cast<const floatx4*>(arow + k);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const floatx4 w4 = *reinterpret_cast<const floatx4*>(wrow + (int64_t)nt * 16 * K + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], w4[j], acc[nt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = t0 + wave * 16 + lk * 4 + r;
      if (t >= T) continue;
      const int col = g * DG + nt * 16 + lrow;
      const int64_t o = ((int64_t)b * T + t) * D + col;
      out[o] = x[o] + gelu_erf(acc[nt][r] + bias[col]);
    }
}

__global__ void wavlm_bias_table_kernel(const float* __restrict__ emb, const int* __restrict__ bmap, int off, int T,
                                        int H, float* __restrict__ table) {
  const int i = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y, W = 2 * T - 1;
  if (i < W) table[(int64_t)h * W + i] = emb[bmap[i - (T - 1) + off] * H + h];
}

// ---- gated attention
constexpr int kAq = 16, kAk = 64, kAd = 64, kSld = 68;

template <bool BF>
__global__ __launch_bounds__(256) void wavlm_attn_kernel(WavlmAttnArgs a) {
  using lt = act_t<BF>;
  constexpr int LD = BF ? 72 : 68;   // LDS row stride: 16-byte multiples, off the 64-element bank period
  __shared__ __attribute__((aligned(16))) lt Qs[kAq * LD];
  __shared__ __attribute__((aligned(16))) lt Ks[kAk * LD];
  __shared__ __attribute__((aligned(16))) lt Vs[kAk * LD];   // bf16: transposed [dim][key]; fp32: [key][dim]
  __shared__ __attribute__((aligned(16))) lt Ps[kAq * LD];
  __shared__ float Ss[kAq * kSld];
  __shared__ float gl[kAq * 8], gate_s[kAq], rscale[kAq], rl[kAq];
  const int T = a.T, D = a.D, tid = threadIdx.x;
  const int q0 = blockIdx.x * kAq, h = blockIdx.y, b = blockIdx.z;
  const int64_t row0 = (int64_t)b * T;
  const lt* qkv = static_cast<const lt*>(a.qkv);
  for (int i = tid; i < kAq * kAd; i += 256) {
    const int r = i >> 6, d = i & 63, t = q0 + r;
    Qs[r * LD + d] = t < T ? qkv[(row0 + t) * 3 * D + h * kAd + d] : lt(0);
  }
  if (tid < kAq * 8) {
    const int r = tid >> 3, j = tid & 7, t = q0 + r;
    float s = 0.f;
    if (t < T) {
      const float* xr = a.xin + (row0 + t) * D + h * kAd;
      s = a.grep_b[j];
      for (int d = 0; d < kAd; ++d) s = fmaf(xr[d], a.grep_w[j * kAd + d], s);
    }
    gl[tid] = s;
  }
  __syncthreads();
  if (tid < kAq) {
    const float* p = gl + tid * 8;
    const float ga = 1.f / (1.f + expf(-(p[0] + p[1] + p[2] + p[3])));
    const float gb = 1.f / (1.f + expf(-(p[4] + p[5] + p[6] + p[7])));
    gate_s[tid] = ga * (gb * a.grep_a[h] - 1.f) + 2.f;
  }
  const int lane = tid & 63, wave = tid >> 6, lrow = lane & 15, lk = lane >> 4;
  const int srow = tid >> 4, scg = tid & 15;   // softmax: 16 threads per query row, 4 keys each
  float m_run = -INFINITY, l_run = 0.f;
  floatx4 oacc = {0.f, 0.f, 0.f, 0.f};
  const float* trow = a.table + (int64_t)h * (2 * T - 1) + (T - 1);
  for (int k0 = 0; k0 < T; k0 += kAk) {
    __syncthreads();   // the previous tile's readers are done; gate_s and Qs are visible
    for (int i = tid; i < kAk * kAd; i += 256) {
      const int r = i >> 6, d = i & 63, t = k0 + r;
      lt kv = lt(0), vv = lt(0);
      if (t < T) {
        const lt* p = qkv + (row0 + t) * 3 * D + h * kAd + d;
        kv = p[D];
        vv = p[2 * D];
      }
      Ks[r * LD + d] = kv;
      if constexpr (BF) Vs[d * LD + r] = vv; else Vs[r * LD + d] = vv;
    }
    __syncthreads();
    {   // scores of keys [16 wave, 16 wave + 16) against the 16 queries
      floatx4 acc = {0.f, 0.f, 0.f, 0.f};
      if constexpr (BF) {
#pragma unroll
        for (int ks = 0; ks < kAd / 32; ++ks) {
          const bf16x8 qa = *reinterpret_cast<const bf16x8*>(Qs + lrow * LD + ks * 32 + lk * 8);
          const bf16x8 kb = *reinterpret_cast<const bf16x8*>(Ks + (wave * 16 + lrow) * LD + ks * 32 + lk * 8);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, kb, acc, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < kAd / 4; ++kk)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Qs[lrow * LD + kk * 4 + lk], Ks[(wave * 16 + lrow) * LD + kk * 4 + lk],
                                                     acc, 0, 0, 0);
      }
      const int key = k0 + wave * 16 + lrow;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = lk * 4 + r, tq = q0 + q;
        float s = -INFINITY;
        if (key < T) {
          s = acc[r] * a.scale;
          if (tq < T) s = fmaf(gate_s[q], trow[key - tq], s);
        }
        Ss[q * kSld + wave * 16 + lrow] = s;
      }
    }
    __syncthreads();
    {   // running softmax of row srow over this tile (key k0 < T is always live, so the maximum is finite)
      float s[4], mx;
#pragma unroll
      for (int c = 0; c < 4; ++c) s[c] = Ss[srow * kSld + scg * 4 + c];
      mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      const float m_new = fmaxf(m_run, mx);
      const float sc = expf(m_run - m_new);
      float sum = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float p = expf(s[c] - m_new);
        sum += p;
        if constexpr (BF) Ps[srow * LD + scg * 4 + c] = f2bf_bits(p); else Ps[srow * LD + scg * 4 + c] = p;
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
      l_run = fmaf(l_run, sc, sum);
      m_run = m_new;
      if (scg == 0) rscale[srow] = sc;
    }
    __syncthreads();
    {   // O[16 queries][dims 16 wave ..] = O * rescale + P V
#pragma unroll
      for (int r = 0; r < 4; ++r) oacc[r] *= rscale[lk * 4 + r];
      if constexpr (BF) {
#pragma unroll
        for (int ks = 0; ks < kAk / 32; ++ks) {
          const bf16x8 pa = *reinterpret_cast<const bf16x8*>(Ps + lrow * LD + ks * 32 + lk * 8);
          const bf16x8 vb = *reinterpret_cast<const bf16x8*>(Vs + (wave * 16 + lrow) * LD + ks * 32 + lk * 8);
          oacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, oacc, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < kAk / 4; ++kk)
          oacc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ps[lrow * LD + kk * 4 + lk], Vs[(kk * 4 + lk) * LD + wave * 16 + lrow],
                                                      oacc, 0, 0, 0);
      }
    }
  }
  if (scg == 0) rl[srow] = l_run;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = lk * 4 + r, tq = q0 + q;
    if (tq >= T) continue;
    const float v = oacc[r] / rl[q];
    const int64_t o = (row0 + tq) * D + h * kAd + wave * 16 + lrow;
    if (a.out_bf16) static_cast<uint16_t*>(a.out)[o] = f2bf_bits(v); else static_cast<float*>(a.out)[o] = v;
  }
}

// ---- TS-VAD's WavLM_weight_sum head and the waveform window gather
__global__ __launch_bounds__(256) void wavlm_layer_mix_kernel(float4* __restrict__ acc, const float4* __restrict__ x,
                                                              float w, int first, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 v = x[i];
    float4 a;
    if (first) {
      a = float4{w * v.x, w * v.y, w * v.z, w * v.w};
    } else {
      a = acc[i];
      a = float4{fmaf(w, v.x, a.x), fmaf(w, v.y, a.y), fmaf(w, v.z, a.z), fmaf(w, v.w, a.w)};
    }
    acc[i] = a;
  }
}

constexpr int kMixRows = 16;   // rows per workgroup of wavlm_mix_proj_ln

// 16 rows x SE columns per workgroup, wave w the columns [w SE / 4, (w + 1) SE / 4) as SE / 64 MFMA tiles.  Fragment
// layout as in wavlm_pos_conv_kernel: lane (lrow, lk) holds A row lrow / B column lrow at the k slots of lk, and
// accumulator element r is (row 4 lk + r, column lrow).  Rows past `rows` read row rows - 1 and are not stored.
template <bool BF, int SE>
__global__ __launch_bounds__(256) void wavlm_mix_proj_ln_kernel(const float* __restrict__ acc, int rows, int D,
                                                                const act_t<BF>* __restrict__ wt,
                                                                const float* __restrict__ bias,
                                                                const float* __restrict__ g,
                                                                const float* __restrict__ beta,
                                                                act_t<BF>* __restrict__ out) {
  using lt = act_t<BF>;
  constexpr int NT = SE / 64;
  __shared__ float red[2][4][kMixRows];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 15, lk = lane >> 4;
  const int r0 = blockIdx.x * kMixRows;
  const float* arow = acc + (int64_t)min(r0 + lrow, rows - 1) * D;
  const int col0 = wave * (SE / 4);
  const lt* wrow = wt + (int64_t)(col0 + lrow) * D;
  floatx4 c[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) c[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
  if constexpr (BF) {
#pragma unroll 2
    for (int ks = 0; ks < D / 32; ++ks) {
      const int k = ks * 32 + lk * 8;
      const float4 a0 = *reinterpret_cast<const float4*>(arow + k);
      const float4 a1 = *reinterpret_cast<const float4*>(arow + k + 4);
      const u32x4_t pk = {pack_bf16x2(a0.x, a0.y), pack_bf16x2(a0.z, a0.w), pack_bf16x2(a1.x, a1.y),
                          pack_bf16x2(a1.z, a1.w)};
      const bf16x8 a = __builtin_bit_cast(bf16x8, pk);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bf16x8 w8 = *reinterpret_cast<const bf16x8*>(wrow + (int64_t)nt * 16 * D + k);
        c[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w8, c[nt], 0, 0, 0);
      }
    }
  } else {
    // 16 k per step as four MFMAs of 4 (slot lk of MFMA j takes k = 16 s + 4 lk + j in A and B alike)
#pragma unroll 2
    for (int s = 0; s < D / 16; ++s) {
      const int k = s * 16 + lk * 4;
      const floatx4 a = *reinterpret_cast<const floatx4*>(arow + k);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const floatx4 w4 = *reinterpret_cast<const floatx4*>(wrow + (int64_t)nt * 16 * D + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], w4[j], c[nt], 0, 0, 0);
      }
    }
  }
  // + bias, then LayerNorm over the SE columns of each row: the sum over this wave's columns (NT tiles x the 16 lanes
  // of a lk group), then over the four waves through LDS; mean first, then the centred squares
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const float bv = bias[col0 + nt * 16 + lrow];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      c[nt][r] += bv;
      s[r] += c[nt][r];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s[r] += __shfl_xor(s[r], o, 64);
    if (lrow == 0) red[0][wave][lk * 4 + r] = s[r];
  }
  __syncthreads();
  float mean[4], q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = lk * 4 + r;
    mean[r] = (red[0][0][row] + red[0][1][row] + red[0][2][row] + red[0][3][row]) * (1.f / SE);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      c[nt][r] -= mean[r];
      q[r] = fmaf(c[nt][r], c[nt][r], q[r]);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) q[r] += __shfl_xor(q[r], o, 64);
    if (lrow == 0) red[1][wave][row] = q[r];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = lk * 4 + r;
    if (r0 + row >= rows) continue;
    const float rstd = rsqrtf((red[1][0][row] + red[1][1][row] + red[1][2][row] + red[1][3][row]) * (1.f / SE) + 1e-5f);
    lt* o = out + (int64_t)(r0 + row) * SE;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = col0 + nt * 16 + lrow;
      st_act(o, col, fmaf(c[nt][r] * rstd, g[col], beta[col]));
    }
  }
}

__global__ __launch_bounds__(256) void window_wave_kernel(const float* __restrict__ wav, int64_t n_total,
                                                          const int* __restrict__ win_start,
                                                          const int* __restrict__ win_n, int n_out,
                                                          float* __restrict__ out) {
  const int w = blockIdx.y;
  const int64_t start = win_start[w];
  const int n = win_n[w];
  for (int j = blockIdx.x * 256 + threadIdx.x; j < n_out; j += gridDim.x * 256) {
    const int64_t i = start + j;
    out[(int64_t)w * n_out + j] = (j < n && i >= 0 && i < n_total) ? wav[i] : 0.f;
  }
}

}  // namespace

void wavlm_layer_mix(float* acc, const float* x, float w, bool first, int64_t n, hipStream_t st) {
  SD_CHECK(acc && x && acc != x && n >= 4 && n % 4 == 0, kErrInvalid, "wavlm_layer_mix: n must be a positive multiple of 4");
  SD_CHECK(((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(x)) & 15) == 0, kErrInvalid,
           "wavlm_layer_mix: pointers must be 16-byte aligned");
  const int64_t n4 = n / 4;
  const int64_t blocks = std::min<int64_t>((n4 + 255) / 256, (int64_t)device_cus() * 8);
  ProfScope prof("wavlm_layer_mix", 2.0 * n, (first ? 8.0 : 12.0) * n, st);
  hipLaunchKernelGGL(wavlm_layer_mix_kernel, dim3((unsigned)blocks), dim3(256), 0, st, reinterpret_cast<float4*>(acc),
                     reinterpret_cast<const float4*>(x), w, first ? 1 : 0, n4);
  SD_LAUNCH_CHECK();
}

void wavlm_mix_proj_ln(const float* acc, int rows, int D, const void* wt, bool bf16, const float* bias, const float* g,
                       const float* beta, int SE, void* out, hipStream_t st) {
  SD_CHECK(acc && wt && bias && g && beta && out && rows >= 1, kErrInvalid, "wavlm_mix_proj_ln: bad argument");
  SD_CHECK(SE == 192 || SE == 256, kErrInvalid, "wavlm_mix_proj_ln: speaker_embed_dim must be 192 or 256");
  SD_CHECK(D >= 32 && D % 32 == 0, kErrInvalid, "wavlm_mix_proj_ln: D must be a multiple of 32");
  SD_CHECK(((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(wt)) & 15) == 0, kErrInvalid,
           "wavlm_mix_proj_ln: pointers must be 16-byte aligned");
  const dim3 grid(cdiv(rows, kMixRows));
  ProfScope prof("wavlm_mix_proj_ln", 2.0 * rows * SE * (double)D,
                 4.0 * rows * D + (bf16 ? 2.0 : 4.0) * ((double)SE * D + (double)rows * SE), st);
  auto go = [&](auto kernel, auto* w, auto* o) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, acc, rows, D, w, bias, g, beta, o);
  };
  if (bf16) {
    auto* w = static_cast<const uint16_t*>(wt);
    auto* o = static_cast<uint16_t*>(out);
    if (SE == 192) go(wavlm_mix_proj_ln_kernel<true, 192>, w, o); else go(wavlm_mix_proj_ln_kernel<true, 256>, w, o);
  } else {
    auto* w = static_cast<const float*>(wt);
    auto* o = static_cast<float*>(out);
    if (SE == 192) go(wavlm_mix_proj_ln_kernel<false, 192>, w, o); else go(wavlm_mix_proj_ln_kernel<false, 256>, w, o);
  }
  SD_LAUNCH_CHECK();
}

void window_wave(const float* wav, int64_t n_total, const int* win_start, const int* win_n, int n_win, int n_out,
                 float* out, hipStream_t st) {
  SD_CHECK(wav && win_start && win_n && out && n_total >= 0 && n_win >= 1 && n_win <= 65535 && n_out >= 1, kErrInvalid,
           "window_wave: bad argument");
  hipLaunchKernelGGL(window_wave_kernel, dim3(std::min(cdiv(n_out, 256), 64), n_win), dim3(256), 0, st, wav, n_total,
                     win_start, win_n, n_out, out);
  SD_LAUNCH_CHECK();
}

int wavlm_l0_parts(int T0) { return cdiv(T0, kL0Block) * 4; }

void wavlm_layer0(const float* wav, int B, int n, const float* w, const float* g, const float* b, bool layer_norm,
                  float* partial, float* ss, void* out, bool out_bf16, hipStream_t st) {
  SD_CHECK(wav && w && g && b && out && B >= 1 && n >= kL0K, kErrInvalid, "wavlm_layer0: bad argument");
  SD_CHECK(B <= 65535, kErrInvalid, "wavlm_layer0: at most 65535 windows per launch");
  const int T0 = (n - kL0K) / kL0S + 1;
  const dim3 grid(cdiv(T0, kL0Block), B);
  if (layer_norm) {
    if (out_bf16)
      hipLaunchKernelGGL((wavlm_l0_norm_kernel<true, true>), grid, dim3(256), 0, st, wav, n, T0, w, g, b, (int64_t)0,
                         static_cast<uint16_t*>(out));
    else
      hipLaunchKernelGGL((wavlm_l0_norm_kernel<true, false>), grid, dim3(256), 0, st, wav, n, T0, w, g, b, (int64_t)0,
                         static_cast<float*>(out));
    SD_LAUNCH_CHECK();
    return;
  }
  SD_CHECK(partial && ss, kErrInvalid, "wavlm_layer0: the group norm needs its scratch");
  hipLaunchKernelGGL(wavlm_l0_stats_kernel, grid, dim3(256), 0, st, wav, n, T0, w, partial);
  hipLaunchKernelGGL(wavlm_l0_finalize_kernel, dim3(kC / 256, B), dim3(256), 0, st, partial, wavlm_l0_parts(T0), g, b,
                     ss);
  if (out_bf16)
    hipLaunchKernelGGL((wavlm_l0_norm_kernel<false, true>), grid, dim3(256), 0, st, wav, n, T0, w, ss, ss + kC,
                       (int64_t)2 * kC, static_cast<uint16_t*>(out));
  else
    hipLaunchKernelGGL((wavlm_l0_norm_kernel<false, false>), grid, dim3(256), 0, st, wav, n, T0, w, ss, ss + kC,
                       (int64_t)2 * kC, static_cast<float*>(out));
  SD_LAUNCH_CHECK();
}

void wavlm_ln_gelu(void* x, bool bf16, int64_t rows, const float* g, const float* b, hipStream_t st) {
  SD_CHECK(x && g && b && rows >= 1 && rows < (1ll << 32), kErrInvalid, "wavlm_ln_gelu: bad argument");
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (bf16)
    hipLaunchKernelGGL(wavlm_ln_gelu_kernel<true>, grid, dim3(256), 0, st, static_cast<uint16_t*>(x), rows, g, b);
  else
    hipLaunchKernelGGL(wavlm_ln_gelu_kernel<false>, grid, dim3(256), 0, st, static_cast<float*>(x), rows, g, b);
  SD_LAUNCH_CHECK();
}

void wavlm_add(float* x, const void* t, bool t_bf16, int64_t n, hipStream_t st) {
  SD_CHECK(x && t && n >= 1 && n < (1ll << 39), kErrInvalid, "wavlm_add: bad argument");
  const dim3 grid((unsigned)((n + 255) / 256));
  if (t_bf16)
    hipLaunchKernelGGL(wavlm_add_kernel<true>, grid, dim3(256), 0, st, x, static_cast<const uint16_t*>(t), n);
  else
    hipLaunchKernelGGL(wavlm_add_kernel<false>, grid, dim3(256), 0, st, x, static_cast<const float*>(t), n);
  SD_LAUNCH_CHECK();
}

void wavlm_pos_conv(const float* x, int B, int T, int D, const void* wt, bool bf16, const float* bias, float* out,
                    hipStream_t st) {
  SD_CHECK(x && wt && bias && out && x != out && B >= 1 && T >= 1, kErrInvalid, "wavlm_pos_conv: bad argument");
  SD_CHECK(D == 768 || D == 1024, kErrInvalid, "wavlm_pos_conv: D must be 768 or 1024 (16 groups of 48 or 64)");
  SD_CHECK(B <= 65535, kErrInvalid, "wavlm_pos_conv: at most 65535 windows per launch");
  const dim3 grid(cdiv(T, kPosTile), 16, B);
  if (D == 768) {
    if (bf16)
      hipLaunchKernelGGL((wavlm_pos_conv_kernel<true, 48>), grid, dim3(256), 0, st, x, T, D,
                         static_cast<const uint16_t*>(wt), bias, out);
    else
      hipLaunchKernelGGL((wavlm_pos_conv_kernel<false, 48>), grid, dim3(256), 0, st, x, T, D,
                         static_cast<const float*>(wt), bias, out);
  } else {
    if (bf16)
      hipLaunchKernelGGL((wavlm_pos_conv_kernel<true, 64>), grid, dim3(256), 0, st, x, T, D,
                         static_cast<const uint16_t*>(wt), bias, out);
    else
      hipLaunchKernelGGL((wavlm_pos_conv_kernel<false, 64>), grid, dim3(256), 0, st, x, T, D,
                         static_cast<const float*>(wt), bias, out);
  }
  SD_LAUNCH_CHECK();
}

void wavlm_bias_table(const float* emb, const int* bmap, int off, int T, int H, float* table, hipStream_t st) {
  SD_CHECK(emb && bmap && table && T >= 1 && H >= 1 && off >= T - 1, kErrInvalid, "wavlm_bias_table: bad argument");
  hipLaunchKernelGGL(wavlm_bias_table_kernel, dim3(cdiv(2 * T - 1, 256), H), dim3(256), 0, st, emb, bmap, off, T, H,
                     table);
  SD_LAUNCH_CHECK();
}

void wavlm_attention(const WavlmAttnArgs& a, hipStream_t st) {
  SD_CHECK(a.qkv && a.xin && a.grep_w && a.grep_b && a.grep_a && a.table && a.out, kErrInvalid,
           "wavlm_attention: null argument");
  SD_CHECK(a.B >= 1 && a.B <= 65535 && a.T >= 1 && a.H >= 1 && a.H <= 65535 && a.D == a.H * kAd, kErrInvalid,
           "wavlm_attention: head size must be 64");
  const dim3 grid(cdiv(a.T, kAq), a.H, a.B);
  if (a.bf16)
    hipLaunchKernelGGL(wavlm_attn_kernel<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(wavlm_attn_kernel<false>, grid, dim3(256), 0, st, a);
  SD_LAUNCH_CHECK();
}

}  // namespace sd
