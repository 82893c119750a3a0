// SimAM gate of the SimAM-ResNet34 BasicBlock (egs/alimeeting/ts_vad2/samresnet_wespeaker.py:57-70) for gfx950, on
// NHWC maps (B, H, W, C), bf16 or fp32, C % 64 == 0.  Per (b, c) over the H x W map Y = bn2(conv2(.)), n = H W - 1:
//   d = (Y - mean)^2,  v = sum d / n,  out = relu(Y * sigmoid(d / (4 (v + 1e-4)) + 0.5) + shortcut)
//
// Three launches; the map is read twice and written once:
//   simam_partial   a workgroup owns a tile of kPix pixels x 64 channels.  A thread reads 8 channels of every 32nd
//                   pixel (16 B of bf16 per load; the 8 lanes of a pixel read 128 contiguous bytes) and keeps fp64 sums
//                   of (y - K) and (y - K)^2 with K its first value, so a channel at mean 1000 / std 0.01 loses nothing
//                   and a constant channel has M2 == 0 exactly.  The 32 pixel slots are merged with Chan's formula in
//                   slot order -> one (n, mean, M2) per (tile, channel).
//   simam_finalize  merges a channel's tile partials in tile order (n_tiles x 24 B per channel: 6.9 MB against the
//                   590 MB stage-1 map of a 96 x 598 batch) -> stat (b, c) = (mean, 1 / (4 (v + 1e-4))).
//   simam_apply     the gate, the shortcut, the ReLU (NaN kept) and the block's output in one pass, fp64 up to the one
//                   rounding to the output type; NHWC as 16-B stores (in place on Y allowed), or any element strides
//                   (the stage-4 map leaves as (B, T', C F)).
// No floating-point atomics, every order fixed by (H W, C) alone: an item's result does not depend on the batch it
// runs in, and a NaN stays in its (b, c) channel.  Statistics are taken on the values the gate reads (the bf16-rounded
// map in bf16 mode).  Scratch is indexed by the item, so disjoint window slices share nothing.
#include "common.h"
#include "kernels.h"
#include "prof.h"

namespace sd {
namespace {

constexpr int kPix = 1024;    // pixels per tile
constexpr int kSlots = 32;    // pixel slots of a workgroup: 256 threads / 8 lanes per 64-channel pixel

struct Moments {   // count, mean, sum of squared deviations
  double n, mean, m2;
};

// Chan et al.: b appended to a (an empty side leaves the other unchanged)
__device__ __forceinline__ Moments merge(const Moments& a, const Moments& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double n = a.n + b.n, delta = b.mean - a.mean;
  return Moments{n, a.mean + delta * (b.n / n), a.m2 + b.m2 + delta * delta * (a.n * b.n / n)};
}

__device__ __forceinline__ void load8(const uint16_t* p, float v[8]) {
  const uint4 r = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    v[2 * u] = __uint_as_float(w[u] << 16);
    v[2 * u + 1] = __uint_as_float(w[u] & 0xffff0000u);
  }
}
__device__ __forceinline__ void load8(const float* p, float v[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(uint16_t* p, const float v[8]) {
  *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                            pack_bf16x2(v[6], v[7]));
}
__device__ __forceinline__ void store8(float* p, const float v[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// pixels of slot s in a tile of tile_n pixels (pixel i of the tile belongs to slot i % kSlots)
__device__ __forceinline__ int slot_count(int tile_n, int s) { return s < tile_n ? (tile_n - s + kSlots - 1) / kSlots : 0; }

// grid (n_tiles, C / 64, B) -> partial[((b * n_tiles + tile) * C + c)] = (n, mean, M2) of the tile's pixels
template <bool BF>
__global__ __launch_bounds__(256) void simam_partial_kernel(const act_t<BF>* __restrict__ y, int HW, int C,
                                                            double* __restrict__ partial) {
  __shared__ double sm[kSlots][64], sq[kSlots][64];
  const int tid = threadIdx.x, cg = tid & 7, slot = tid >> 3;
  const int tile = blockIdx.x, c0 = blockIdx.y * 64, b = blockIdx.z;
  const int p0 = tile * kPix, tile_n = min(kPix, HW - p0);
  const act_t<BF>* src = y + ((int64_t)b * HW + p0) * C + c0 + cg * 8;
  double k[8], s1[8], s2[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) k[u] = s1[u] = s2[u] = 0.0;
  for (int i = slot; i < tile_n; i += kSlots) {
    float v[8];
    load8(src + (int64_t)i * C, v);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (i == slot) k[u] = (double)v[u];
      const double d = (double)v[u] - k[u];
      s1[u] += d;
      s2[u] = fma(d, d, s2[u]);
    }
  }
  const double n = (double)slot_count(tile_n, slot);
#pragma unroll
  for (int u = 0; u < 8; ++u) {   // n == 0: never read (merge skips an empty side)
    sm[slot][cg * 8 + u] = k[u] + s1[u] / n;
    sq[slot][cg * 8 + u] = s2[u] - s1[u] * s1[u] / n;
  }
  __syncthreads();
  // wave `part` merges slots 8 part .. 8 part + 7 of channel ch in slot order, then wave 0 the four parts in order
  const int ch = tid & 63, part = tid >> 6;
  Moments m{0.0, 0.0, 0.0};
#pragma unroll
  for (int s = part * 8; s < part * 8 + 8; ++s)
    m = merge(m, Moments{(double)slot_count(tile_n, s), sm[s][ch], sq[s][ch]});
  __syncthreads();
  sm[part][ch] = m.mean;
  sq[part][ch] = m.m2;
  sm[4 + part][ch] = m.n;
  __syncthreads();
  if (part == 0) {
    Moments t{sm[4][ch], sm[0][ch], sq[0][ch]};
#pragma unroll
    for (int g = 1; g < 4; ++g) t = merge(t, Moments{sm[4 + g][ch], sm[g][ch], sq[g][ch]});
    double* dst = partial + (((int64_t)b * gridDim.x + tile) * C + c0 + ch) * 3;
    dst[0] = t.n;
    dst[1] = t.mean;
    dst[2] = t.m2;
  }
}

// grid (C / 64, B): stat[b * C + c] = (mean, 1 / (4 (M2 / (HW - 1) + 1e-4))) from the n_tiles records in record order
__global__ __launch_bounds__(256) void simam_finalize_kernel(const double* __restrict__ partial, int HW, int C,
                                                             int n_tiles, double2* __restrict__ stat) {
  __shared__ double sn[4][64], sm[4][64], sq[4][64];
  const int ch = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + ch, b = blockIdx.y;
  const int per = (n_tiles + 3) / 4;
  Moments m{0.0, 0.0, 0.0};
  for (int t = part * per; t < min(n_tiles, (part + 1) * per); ++t) {
    const double* p = partial + (((int64_t)b * n_tiles + t) * C + c) * 3;
    m = merge(m, Moments{p[0], p[1], p[2]});
  }
  sn[part][ch] = m.n;
  sm[part][ch] = m.mean;
  sq[part][ch] = m.m2;
  __syncthreads();
  if (part == 0) {
    Moments t{sn[0][ch], sm[0][ch], sq[0][ch]};
#pragma unroll
    for (int g = 1; g < 4; ++g) t = merge(t, Moments{sn[g][ch], sm[g][ch], sq[g][ch]});
    const double v = t.m2 / (double)(HW - 1);   // H W == 1: 0 / 0 = NaN like the reference
    stat[(int64_t)b * C + c] = make_double2(t.mean, 1.0 / (4.0 * (v + 1e-4)));
  }
}

struct OutMap {
  int64_t sb, sp_h, sp_w, sn;   // element strides of (b, h, w, c)
  int W;
  bool nhwc;
};

// grid (n_tiles, C / 64, B).  y and out may be the same NHWC buffer: a thread reads its 8 values before it writes them.
template <bool BF>
__global__ __launch_bounds__(256) void simam_apply_kernel(const act_t<BF>* y, const act_t<BF>* __restrict__ res, int HW,
                                                          int C, const double2* __restrict__ stat, act_t<BF>* out,
                                                          OutMap o) {
  const int tid = threadIdx.x, cg = tid & 7, slot = tid >> 3;
  const int tile = blockIdx.x, c0 = blockIdx.y * 64 + cg * 8, b = blockIdx.z;
  const int p0 = tile * kPix, tile_n = min(kPix, HW - p0);
  double mean[8], inv[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const double2 s = stat[(int64_t)b * C + c0 + u];
    mean[u] = s.x;
    inv[u] = s.y;
  }
  for (int i = slot; i < tile_n; i += kSlots) {
    const int64_t e = ((int64_t)b * HW + p0 + i) * C + c0;
    float v[8], r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    load8(y + e, v);
    if (res) load8(res + e, r);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double x = (double)v[u], d = x - mean[u];
      const double g = 1.0 / (1.0 + exp(-fma(d * d, inv[u], 0.5)));
      v[u] = relu_keep_nan((float)fma(x, g, (double)r[u]));
    }
    if (o.nhwc) {
      store8(out + e, v);
    } else {
      const int p = p0 + i, h = p / o.W, w = p - h * o.W;
      const int64_t ob = (int64_t)b * o.sb + (int64_t)h * o.sp_h + (int64_t)w * o.sp_w;
#pragma unroll
      for (int u = 0; u < 8; ++u) st_act(out, ob + (int64_t)(c0 + u) * o.sn, v[u]);
    }
  }
}

}  // namespace

int simam_tiles(int HW) { return cdiv(HW, kPix); }

void simam_gate(const SimamArgs& a, hipStream_t st) {
  SD_CHECK(a.y && a.out && a.partial && a.stat, kErrInvalid, "simam: null argument");
  SD_CHECK(a.B >= 1 && a.B <= 65535 && a.H >= 1 && a.W >= 1 && a.C >= 64 && a.C % 64 == 0 && a.C / 64 <= 65535,
           kErrInvalid, "simam: 1 <= B <= 65535, C a multiple of 64");
  SD_CHECK((int64_t)a.H * a.W < (1ll << 31), kErrInvalid, "simam: map out of range");
  const int HW = a.H * a.W, C = a.C, n_tiles = simam_tiles(HW);
  const double esz = a.bf16 ? 2.0 : 4.0, elems = (double)a.B * HW * C;
  const bool nhwc = a.o_sn == 1 && a.o_sw == C && a.o_sh == (int64_t)a.W * C && a.o_sb == (int64_t)HW * C;
  SD_CHECK(nhwc || a.out != a.y, kErrInvalid, "simam: only an NHWC output may alias the input");
  const OutMap o{a.o_sb, a.o_sh, a.o_sw, a.o_sn, a.W, nhwc};
  const dim3 grid(n_tiles, C / 64, a.B);
  double* const partial = reinterpret_cast<double*>(a.partial);
  double2* const stat = reinterpret_cast<double2*>(a.stat);
  {
    ProfScope prof("simam_stats", 0.0, elems * esz + 2.0 * 24.0 * a.B * n_tiles * C, st);
    if (a.bf16)
      hipLaunchKernelGGL(simam_partial_kernel<true>, grid, dim3(256), 0, st, static_cast<const uint16_t*>(a.y), HW, C,
                         partial);
    else
      hipLaunchKernelGGL(simam_partial_kernel<false>, grid, dim3(256), 0, st, static_cast<const float*>(a.y), HW, C,
                         partial);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(simam_finalize_kernel, dim3(C / 64, a.B), dim3(256), 0, st, partial, HW, C, n_tiles, stat);
    SD_LAUNCH_CHECK();
  }
  ProfScope prof("simam_apply", 0.0, elems * esz * (a.res ? 3.0 : 2.0), st);
  if (a.bf16)
    hipLaunchKernelGGL(simam_apply_kernel<true>, grid, dim3(256), 0, st, static_cast<const uint16_t*>(a.y),
                       static_cast<const uint16_t*>(a.res), HW, C, stat, static_cast<uint16_t*>(a.out), o);
  else
    hipLaunchKernelGGL(simam_apply_kernel<false>, grid, dim3(256), 0, st, static_cast<const float*>(a.y),
                       static_cast<const float*>(a.res), HW, C, stat, static_cast<float*>(a.out), o);
  SD_LAUNCH_CHECK();
}

}  // namespace sd
