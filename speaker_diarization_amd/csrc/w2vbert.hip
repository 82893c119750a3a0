// w2v-BERT 2.0 kernels for gfx950 (declarations and contracts in kernels.h): self-attention with the relative_key
// distance embedding, and the conv module's middle (GLU, causal depthwise conv, LayerNorm over channels, swish).
#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "launch.h"
#include "prof.h"

namespace sd {

namespace {

// ---- relative-key attention
constexpr int kAq = 16, kAk = 64, kAd = 64, kSld = 68;
constexpr int kLeft = 64, kRight = 8, kRcols = kW2vDistRows;   // 73 distances padded to 80 columns (5 MFMA tiles)
constexpr int kRld = 84;                                        // row stride of R in LDS, off the bank period

template <bool BF>
__global__ __launch_bounds__(256) void w2vbert_attn_kernel(W2vAttnArgs a) {
  using lt = act_t<BF>;
  constexpr int LD = BF ? 72 : 68;   // LDS row stride: 16-byte multiples, off the 64-element bank period
  __shared__ __attribute__((aligned(16))) lt Qs[kAq * LD];
  __shared__ __attribute__((aligned(16))) lt Ks[kAk * LD];
  __shared__ __attribute__((aligned(16))) lt Vs[kAk * LD];   // bf16: transposed [dim][key]; fp32: [key][dim]
  __shared__ __attribute__((aligned(16))) lt Ps[kAq * LD];
  __shared__ float Ss[kAq * kSld];
  __shared__ float Rs[kAq * kRld];   // R[q][j] = q . E[j], j = clamp(key - query, -64, 8) + 64
  __shared__ float rscale[kAq], rl[kAq];
  const int T = a.T, D = a.D, tid = threadIdx.x;
  const int q0 = blockIdx.x * kAq, h = blockIdx.y, b = blockIdx.z;
  const int64_t row0 = (int64_t)b * T;
  const lt* qkv = static_cast<const lt*>(a.qkv);
  const lt* E = static_cast<const lt*>(a.dist);   // (80, 64), rows 73 .. 79 zero
  for (int i = tid; i < kAq * kAd; i += 256) {
    const int r = i >> 6, d = i & 63, t = q0 + r;
    Qs[r * LD + d] = t < T ? qkv[(row0 + t) * 3 * D + h * kAd + d] : lt(0);
  }
  const int lane = tid & 63, wave = tid >> 6, lrow = lane & 15, lk = lane >> 4;
  const int srow = tid >> 4, scg = tid & 15;   // softmax: 16 threads per query row, 4 keys each
  __syncthreads();
  // R = Q E^T once per query tile: wave w the distance columns [16 w, 16 w + 16), wave 0 also [64, 80)
  for (int ct = wave; ct < kRcols / 16; ct += 4) {
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    const lt* erow = E + (ct * 16 + lrow) * kAd;
    if constexpr (BF) {
#pragma unroll
      for (int ks = 0; ks < kAd / 32; ++ks) {
        const bf16x8 qa = *reinterpret_cast<const bf16x8*>(Qs + lrow * LD + ks * 32 + lk * 8);
        const bf16x8 eb = *reinterpret_cast<const bf16x8*>(erow + ks * 32 + lk * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, eb, acc, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int kk = 0; kk < kAd / 4; ++kk)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Qs[lrow * LD + kk * 4 + lk], erow[kk * 4 + lk], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Rs[(lk * 4 + r) * kRld + ct * 16 + lrow] = acc[r];
  }
  float m_run = -INFINITY, l_run = 0.f;
  floatx4 oacc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < T; k0 += kAk) {
    __syncthreads();   // the previous tile's readers are done; Rs is visible
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
        const int q = lk * 4 + r;
        float s = -INFINITY;
        if (key < T) {
          const int dist = min(max(key - (q0 + q), -kLeft), kRight) + kLeft;
          s = (acc[r] + Rs[q * kRld + dist]) * a.scale;
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

// ---- conv mix: GLU on load, causal depthwise k31, LayerNorm over the 1024 channels, swish
constexpr int kMC = kW2vConvC, kMK = kW2vConvK, kMT = kW2vConvTile;
constexpr int kMRows = kMT + kMK - 1;   // frames a tile reads: [t0 - 30, t0 + 16)
constexpr int kMChunk = 256;            // thread tid owns the channels tid + 256 j over the tile's frames

// A thread owns its channels over time, so nothing is shared between threads before the LayerNorm and the input needs no
// LDS staging: each frame row is two coalesced reads (the value and gate halves) of 256 consecutive channels.  The conv
// results of the tile (16 frames x 1024 channels, fp32) wait in LDS for the LayerNorm statistics; each thread reads
// back only what it wrote.
constexpr int kMixLds = (kMT * kMC + 2 * 4 * kMT) * 4;   // 66,048 bytes of dynamic LDS

template <bool BF>
__global__ __launch_bounds__(256) void w2vbert_conv_mix_kernel(const act_t<BF>* __restrict__ x, int T,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ g,
                                                               const float* __restrict__ beta,
                                                               act_t<BF>* __restrict__ out) {
  extern __shared__ float mix_lds[];
  float* ys = mix_lds;                 // [frame][channel]
  float* red = mix_lds + kMT * kMC;    // [2][wave][frame]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = blockIdx.x * kMT, b = blockIdx.y;
  const act_t<BF>* xb = x + (int64_t)b * T * 2 * kMC;
  float sum[kMT];
#pragma unroll
  for (int t = 0; t < kMT; ++t) sum[t] = 0.f;
#pragma unroll 1
  for (int j = 0; j < kMC / kMChunk; ++j) {
    const int c = j * kMChunk + tid;
    float wr[kMK], acc[kMT];
#pragma unroll
    for (int k = 0; k < kMK; ++k) wr[k] = w[c * kMK + k];
#pragma unroll
    for (int t = 0; t < kMT; ++t) acc[t] = 0.f;
    // value * sigmoid(gate) of frames [t0 - 30, t0 + 16) of this window; zeros before its first frame and past its last
#pragma unroll
    for (int i = 0; i < kMRows; ++i) {
      const int t = t0 - (kMK - 1) + i;
      float v = 0.f;
      if (t >= 0 && t < T) {
        const act_t<BF>* r = xb + (int64_t)t * 2 * kMC;
        v = ld_act(r, c) * sigmoidf_(ld_act(r, kMC + c));
      }
#pragma unroll
      for (int tt = 0; tt < kMT; ++tt)
        if (i - tt >= 0 && i - tt < kMK) acc[tt] = fmaf(wr[i - tt], v, acc[tt]);
    }
#pragma unroll
    for (int t = 0; t < kMT; ++t) {
      ys[t * kMC + c] = acc[t];
      sum[t] += acc[t];
    }
  }
  // LayerNorm over the 1024 channels of each of the 16 frames: mean, then the centred squares (fp32)
#pragma unroll
  for (int t = 0; t < kMT; ++t) {
    const float s = warp_sum(sum[t]);
    if (lane == 0) red[wave * kMT + t] = s;
  }
  __syncthreads();
  float mean[kMT], rstd[kMT];
#pragma unroll
  for (int t = 0; t < kMT; ++t) {
    mean[t] = (red[t] + red[kMT + t] + red[2 * kMT + t] + red[3 * kMT + t]) * (1.f / kMC);
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < kMC / kMChunk; ++j) {
      const float d = ys[t * kMC + j * kMChunk + tid] - mean[t];
      sq = fmaf(d, d, sq);
    }
    sq = warp_sum(sq);
    if (lane == 0) red[(4 + wave) * kMT + t] = sq;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < kMT; ++t)
    rstd[t] = rsqrtf((red[4 * kMT + t] + red[5 * kMT + t] + red[6 * kMT + t] + red[7 * kMT + t]) * (1.f / kMC) + 1e-5f);
#pragma unroll 1
  for (int j = 0; j < kMC / kMChunk; ++j) {
    const int c = j * kMChunk + tid;
    const float gc = g[c], bc = beta[c];
#pragma unroll
    for (int t = 0; t < kMT; ++t) {
      if (t0 + t >= T) continue;
      const float v = fmaf((ys[t * kMC + c] - mean[t]) * rstd[t], gc, bc);
      st_act(out, ((int64_t)b * T + t0 + t) * kMC + c, v * sigmoidf_(v));
    }
  }
}

}  // namespace

void w2vbert_attention(const W2vAttnArgs& a, hipStream_t st) {
  SD_CHECK(a.qkv && a.dist && a.out, kErrInvalid, "w2vbert_attention: null argument");
  SD_CHECK(a.B >= 1 && a.B <= 65535 && a.T >= 1 && a.H >= 1 && a.H <= 65535 && a.D == a.H * kAd, kErrInvalid,
           "w2vbert_attention: head size must be 64");
  SD_CHECK(((reinterpret_cast<uintptr_t>(a.qkv) | reinterpret_cast<uintptr_t>(a.dist)) & 15) == 0, kErrInvalid,
           "w2vbert_attention: pointers must be 16-byte aligned");
  const dim3 grid(cdiv(a.T, kAq), a.H, a.B);
  ProfScope prof("w2vbert_attention", 4.0 * a.B * a.H * (double)a.T * a.T * kAd + 2.0 * a.B * a.H * a.T * kRcols * kAd,
                 (a.bf16 ? 2.0 : 4.0) * 4.0 * a.B * a.T * a.D, st);
  if (a.bf16)
    hipLaunchKernelGGL(w2vbert_attn_kernel<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(w2vbert_attn_kernel<false>, grid, dim3(256), 0, st, a);
  SD_LAUNCH_CHECK();
}

void w2vbert_conv_mix(const void* x, int B, int T, const float* w, const float* g, const float* beta, void* out,
                      bool bf16, hipStream_t st) {
  SD_CHECK(x && w && g && beta && out && x != out, kErrInvalid, "w2vbert_conv_mix: bad argument");
  SD_CHECK(B >= 1 && B <= 65535 && T >= 1, kErrInvalid, "w2vbert_conv_mix: 1 .. 65535 windows of at least one frame");
  const dim3 grid(cdiv(T, kMT), B);
  ProfScope prof("w2vbert_conv_mix", 2.0 * B * T * (double)kMC * kMK, (bf16 ? 2.0 : 4.0) * 3.0 * B * T * kMC, st);
  allow_dynamic_lds<&w2vbert_conv_mix_kernel<true>, &w2vbert_conv_mix_kernel<false>>(kMixLds);
  if (bf16)
    hipLaunchKernelGGL(w2vbert_conv_mix_kernel<true>, grid, dim3(256), kMixLds, st, static_cast<const uint16_t*>(x), T, w, g,
                       beta, static_cast<uint16_t*>(out));
  else
    hipLaunchKernelGGL(w2vbert_conv_mix_kernel<false>, grid, dim3(256), kMixLds, st, static_cast<const float*>(x), T, w, g,
                       beta, static_cast<float*>(out));
  SD_LAUNCH_CHECK();
}

}  // namespace sd
