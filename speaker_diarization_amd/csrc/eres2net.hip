// ERes2NetV2 kernels for gfx950 (egs/alimeeting/ts_vad2/ERes2NetV2.py, fusion.py): what conv_gemm, res_conv.hip and
// fcm_conv.hip do not cover.
//
// res2_conv3x3: the 3x3 slice conv of a Res2Net block (ERes2NetV2.py:73-83, 140-151) on v_mfma_f32_16x16x32_bf16.  It
//   reads `width` channels at a channel offset of the conv1 map, optionally adds the previous slice's output on load
//   (sp = sp + spx[i]), and writes bn + Hardtanh(0, 20) to a channel offset of the concat map.  A workgroup owns an
//   output patch of <= 128 pixels times 32 output channels and walks the input in 32-channel slabs: the slab's halo and
//   its 9 x 32 x 32 weights are staged in LDS (80-B rows: 16-B fragment reads of 16 consecutive rows fall on distinct
//   bank slots), each wave computes 32 pixels x 32 channels per tap with 4 MFMAs.  Channels >= width read as zeros
//   and are not stored, so any even width works; slices whose offsets are 16-B aligned load 16 B per lane, the others
//   (width 26 / 52 in an unpadded map) 4 B per lane.
// aff_gate: the in-block AFF (fusion.py:10-30) in one pass.  A workgroup owns 64 pixels (one per lane); wave g owns the
//   hidden units and the channels congruent to g modulo 4.  x and y are staged once in LDS (odd word stride: the 64
//   lanes of a wave fall on 64 banks), the weights are wave-uniform and come through the scalar cache (the fp32 stage-4
//   weights, 139 KB, do not fit LDS next to the tile), hidden units stay in registers.  SiLU and tanh are fp32.
// aff_blend / slice_add / nhwc_to_frames: element-wise pieces (fuse34's blend, the fp32 path's sp + spx[i], and the
//   frame-level output order f * C + c).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "kernels.h"
#include "launch.h"
#include "prof.h"

namespace sd {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 128;       // output pixels per workgroup
constexpr int kMaxPos = 400;     // halo positions: (TH + 2) (TW + 2) over the patches res2_geom picks is <= 390
constexpr int kRow = 80;         // LDS bytes per staged row of 32 bf16 channels (64 B + 16 B pad)

__device__ __forceinline__ float clamp20(float v) { return v < 0.f ? 0.f : (v > 20.f ? 20.f : v); }   // NaN stays

struct Res2Geom {
  int TH, TW, n_th, n_tw, n_ct;
};

template <int VEC>
__device__ __forceinline__ void res2_load(const uint16_t* p, uint32_t (&w)[VEC / 2]) {
  if constexpr (VEC == 8) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
    w[0] = *reinterpret_cast<const uint32_t*>(p);
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void res2_conv_kernel(Res2ConvArgs a, Res2Geom g) {
  __shared__ __attribute__((aligned(16))) uint8_t xs[kMaxPos * kRow];
  __shared__ __attribute__((aligned(16))) uint8_t wsm[9 * 32 * kRow];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int Cp = res2_padded(a.width);
  const uint16_t* X = reinterpret_cast<const uint16_t*>(a.x);
  const uint16_t* Ad = reinterpret_cast<const uint16_t*>(a.add);
  const uint16_t* Wt = reinterpret_cast<const uint16_t*>(a.w);

  const int ct = blockIdx.x % g.n_ct;
  int tile = blockIdx.x / g.n_ct;
  const int tw = tile % g.n_tw;
  tile /= g.n_tw;
  const int th = tile % g.n_th, b = tile / g.n_th;
  const int ho0 = th * g.TH, wo0 = tw * g.TW, n0 = ct * 32;
  const int HC = g.TW + 2, n_pos = (g.TH + 2) * HC;

  int base[2];
  bool pvalid[2];
#pragma unroll
  for (int pb = 0; pb < 2; ++pb) {
    const int pp = (wv * 2 + pb) * 16 + l15;
    const int r = pp / g.TW, c = pp - r * g.TW;
    const bool in_tile = pp < g.TH * g.TW;
    pvalid[pb] = in_tile && ho0 + r < a.H && wo0 + c < a.W;
    base[pb] = in_tile ? r * HC + c : 0;
  }
  floatx4 acc[2][2];
#pragma unroll
  for (int pb = 0; pb < 2; ++pb)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[pb][nt] = floatx4{0.f, 0.f, 0.f, 0.f};

  constexpr int UPP = 32 / VEC;   // load units per staged position
  const int n_slab = Cp / 32;
  for (int slab = 0; slab < n_slab; ++slab) {
    for (int u = tid; u < n_pos * UPP; u += kThreads) {
      const int pos = u / UPP, cu = (u - pos * UPP) * VEC;
      const int row = pos / HC, col = pos - row * HC;
      const int hi = ho0 - 1 + row, wi = wo0 - 1 + col, ch = slab * 32 + cu;
      uint32_t w[VEC / 2];
#pragma unroll
      for (int k = 0; k < VEC / 2; ++k) w[k] = 0u;
      if ((unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W && ch < a.width) {
        const int64_t pix = ((int64_t)b * a.H + hi) * a.W + wi;
        res2_load<VEC>(X + pix * a.ldx + a.x_coff + ch, w);
        if (Ad) {
          uint32_t s[VEC / 2];
          res2_load<VEC>(Ad + pix * a.ld_add + a.add_coff + ch, s);
#pragma unroll
          for (int k = 0; k < VEC / 2; ++k)
            w[k] = pack_bf16x2(__uint_as_float(w[k] << 16) + __uint_as_float(s[k] << 16),
                               __uint_as_float(w[k] & 0xffff0000u) + __uint_as_float(s[k] & 0xffff0000u));
        }
      }
      uint32_t* d = reinterpret_cast<uint32_t*>(xs + pos * kRow + cu * 2);
#pragma unroll
      for (int k = 0; k < VEC / 2; ++k) d[k] = w[k];
    }
    for (int u = tid; u < 9 * 32 * 4; u += kThreads) {
      const int rowid = u >> 2, ck = u & 3;          // rowid = t * 32 + j
      const int t = rowid >> 5, n = n0 + (rowid & 31);
      *reinterpret_cast<uint4*>(wsm + rowid * kRow + ck * 16) =
          *reinterpret_cast<const uint4*>(Wt + ((int64_t)n * 9 + t) * Cp + slab * 32 + ck * 8);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int toff = (t / 3) * HC + (t % 3);
      bf16x8 wf[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        wf[nt] = *reinterpret_cast<const bf16x8*>(wsm + (t * 32 + nt * 16 + l15) * kRow + q * 16);
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(xs + (base[pb] + toff) * kRow + q * 16);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          acc[pb][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], af, acc[pb][nt], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // lane (l15, q) holds channels n0 + 16 nt + 4 q + (0..3) of pixel l15 of its two pixel blocks
  uint16_t* const out = reinterpret_cast<uint16_t*>(a.out);
#pragma unroll
  for (int pb = 0; pb < 2; ++pb) {
    if (!pvalid[pb]) continue;
    const int pp = (wv * 2 + pb) * 16 + l15;
    const int r = pp / g.TW, c = pp - r * g.TW;
    const int64_t pix = ((int64_t)b * a.H + ho0 + r) * a.W + wo0 + c;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int c0 = n0 + nt * 16 + q * 4;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = clamp20(fmaf(acc[pb][nt][i], a.alpha[c0 + i], a.beta[c0 + i]));
      uint32_t* o = reinterpret_cast<uint32_t*>(out + pix * a.ldo + a.o_coff + c0);
      if (c0 < a.width) o[0] = pack_bf16x2(v[0], v[1]);        // width is even: a pair is whole or absent
      if (c0 + 2 < a.width) o[1] = pack_bf16x2(v[2], v[3]);
    }
  }
}

// The patch TH x TW <= 128 pixels: rows of up to 16 pixels, as many rows as fit.
Res2Geom res2_geom(const Res2ConvArgs& a) {
  Res2Geom g;
  g.TW = std::min(a.W, 16);
  g.TH = std::min(a.H, kTile / g.TW);
  g.n_th = cdiv(a.H, g.TH);
  g.n_tw = cdiv(a.W, g.TW);
  g.n_ct = res2_padded(a.width) / 32;
  return g;
}

// ------------------------------------------------------------------------------------------------ aff_gate
constexpr int kAffPix = 64;

__device__ __forceinline__ float silu_f32(float v) { return v / (1.f + expf(-v)); }

template <bool BF>
__device__ __forceinline__ float aff_tile_get(const uint32_t* row, int k) {
  if constexpr (BF) {
    const uint32_t w = row[k >> 1];
    return (k & 1) ? __uint_as_float(w & 0xffff0000u) : __uint_as_float(w << 16);
  } else {
    return __uint_as_float(row[k]);
  }
}

template <bool BF, int IPT>
__global__ __launch_bounds__(kThreads) void aff_gate_kernel(AffGateArgs a, int SW) {
  constexpr int IH = 4 * IPT;
  extern __shared__ __attribute__((aligned(16))) uint32_t aff_smem[];
  uint32_t* const tile = aff_smem;                                     // [64][SW]: x words then y words
  float* const hs = reinterpret_cast<float*>(aff_smem + kAffPix * SW);  // [64][IH + 1]
  const int tid = threadIdx.x, lane = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = a.C;
  const int RW = BF ? C / 2 : C;           // words per slice row
  const int EPW = BF ? 2 : 1;              // elements per word
  const int64_t p0 = (int64_t)blockIdx.x * kAffPix;
  const int np = a.P - p0 < kAffPix ? (int)(a.P - p0) : kAffPix;
  using T = act_t<BF>;
  const T* X = reinterpret_cast<const T*>(a.x);
  const T* Y = reinterpret_cast<const T*>(a.y);

  for (int u = tid; u < kAffPix * RW; u += kThreads) {
    const int p = u / RW, wd = u - p * RW;
    uint32_t vx = 0u, vy = 0u;
    if (p < np) {
      vx = *reinterpret_cast<const uint32_t*>(X + (p0 + p) * a.ldx + a.x_coff + wd * EPW);
      vy = *reinterpret_cast<const uint32_t*>(Y + (p0 + p) * a.ldy + a.y_coff + wd * EPW);
    }
    tile[p * SW + wd] = vx;
    tile[p * SW + RW + wd] = vy;
  }
  __syncthreads();

  // ---- hidden units g, g + 4, ...: h = SiLU(a1 (W1 [x | y]) + c1)
  const uint32_t* row = tile + lane * SW;
  {
    float acc[IPT];
#pragma unroll
    for (int j = 0; j < IPT; ++j) acc[j] = 0.f;
    const float* w1 = a.w1 + (size_t)g * IPT;
    for (int k = 0; k < C; ++k) {        // x then y, the order of torch.cat((x, ds_y), 1)
      const float v = aff_tile_get<BF>(row, k);
#pragma unroll
      for (int j = 0; j < IPT; ++j) acc[j] = fmaf(w1[(size_t)k * IH + j], v, acc[j]);
    }
    const uint32_t* rowy = row + RW;
    for (int k = 0; k < C; ++k) {
      const float v = aff_tile_get<BF>(rowy, k);
#pragma unroll
      for (int j = 0; j < IPT; ++j) acc[j] = fmaf(w1[(size_t)(C + k) * IH + j], v, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < IPT; ++j)
      hs[lane * (IH + 1) + g + 4 * j] = silu_f32(fmaf(acc[j], a.a1[g * IPT + j], a.c1[g * IPT + j]));
  }
  __syncthreads();

  // ---- channels g, g + 4, ...: att = a2 (W2 h) + c2, out = x (1 + tanh att) + y (1 - tanh att)
  float h[IH];
#pragma unroll
  for (int i = 0; i < IH; ++i) h[i] = hs[lane * (IH + 1) + i];
  for (int c = g; c < C; c += 4) {
    const float* w2 = a.w2 + (size_t)c * IH;
    float att = 0.f;
#pragma unroll
    for (int i = 0; i < IH; ++i) att = fmaf(w2[i], h[i], att);
    const float xa = 1.f + tanhf(fmaf(att, a.a2[c], a.c2[c]));
    const float xv = aff_tile_get<BF>(row, c), yv = aff_tile_get<BF>(row + RW, c);
    const float o = xv * xa + yv * (2.f - xa);
    if constexpr (BF) reinterpret_cast<uint16_t*>(tile + lane * SW)[c] = f2bf_bits(o);   // own channel's half word
    else tile[lane * SW + c] = __float_as_uint(o);
  }
  __syncthreads();

  T* O = reinterpret_cast<T*>(a.out);
  for (int u = tid; u < np * RW; u += kThreads) {
    const int p = u / RW, wd = u - p * RW;
    *reinterpret_cast<uint32_t*>(O + (p0 + p) * a.ldo + a.o_coff + wd * EPW) = tile[p * SW + wd];
  }
}

template <bool BF, int IPT>
void launch_aff(const AffGateArgs& a, hipStream_t st) {
  const int RW = BF ? a.C / 2 : a.C;
  const int SW = (2 * RW) | 1;
  const size_t smem = ((size_t)kAffPix * SW + (size_t)kAffPix * (4 * IPT + 1)) * 4;
  SD_CHECK(smem <= 160 * 1024, kErrInvalid, "aff_gate: LDS budget");
  allow_dynamic_lds<&aff_gate_kernel<BF, IPT>>(160 * 1024);
  const int64_t blocks = (a.P + kAffPix - 1) / kAffPix;
  SD_CHECK(blocks < (1ll << 31), kErrInvalid, "aff_gate: too many pixels");
  hipLaunchKernelGGL((aff_gate_kernel<BF, IPT>), dim3((unsigned)blocks), dim3(kThreads), smem, st, a, SW);
}

template <bool BF>
void launch_aff_ipt(const AffGateArgs& a, hipStream_t st) {
  switch (aff_ipt(a.I)) {
    case 2: launch_aff<BF, 2>(a, st); break;
    case 4: launch_aff<BF, 4>(a, st); break;
    case 7: launch_aff<BF, 7>(a, st); break;
    default: launch_aff<BF, 13>(a, st); break;
  }
}

// ------------------------------------------------------------------------------------------------ element-wise
template <bool BF>
__global__ __launch_bounds__(kThreads) void aff_blend_kernel(const act_t<BF>* __restrict__ x, int ldx,
                                                             const act_t<BF>* __restrict__ y, int ldy,
                                                             const float* __restrict__ att, int B, int H, int W, int C,
                                                             float* __restrict__ out, int64_t o_sb, int64_t o_sh,
                                                             int64_t o_sw, int64_t o_sn) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)B * H * W * C) return;
  const int c = (int)(i % C);
  const int64_t m = i / C;
  const int w = (int)(m % W);
  const int64_t t = m / W;
  const int h = (int)(t % H), b = (int)(t / H);
  const float xa = 1.f + tanhf(att[i]);
  const float xv = ld_act(x, m * ldx + c), yv = ld_act(y, m * ldy + c);
  out[b * o_sb + h * o_sh + w * o_sw + c * o_sn] = xv * xa + yv * (2.f - xa);
}

template <bool BF>
__global__ __launch_bounds__(kThreads) void slice_add_kernel(act_t<BF>* __restrict__ x, int ldx,
                                                             const act_t<BF>* __restrict__ y, int ldy, int64_t P,
                                                             int C) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= P * C) return;
  const int c = (int)(i % C);
  const int64_t p = i / C;
  st_act(x, p * ldx + c, ld_act(x, p * ldx + c) + ld_act(y, p * ldy + c));
}

template <bool BF>
__global__ __launch_bounds__(kThreads) void nhwc_to_frames_kernel(const act_t<BF>* __restrict__ x, int B, int H, int W,
                                                                  int C, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;   // over the output: c fastest, then h
  if (i >= (int64_t)B * H * W * C) return;
  const int c = (int)(i % C);
  int64_t t = i / C;
  const int h = (int)(t % H);
  t /= H;
  const int w = (int)(t % W), b = (int)(t / W);
  out[i] = ld_act(x, (((int64_t)b * H + h) * W + w) * C + c);
}

unsigned ew_blocks(int64_t n) {
  const int64_t blocks = (n + kThreads - 1) / kThreads;
  SD_CHECK(blocks >= 1 && blocks < (1ll << 31), kErrInvalid, "eres2net: element-wise launch size");
  return (unsigned)blocks;
}

}  // namespace

bool res2_conv_supported(const Res2ConvArgs& a) {
  return a.x && a.w && a.alpha && a.beta && a.out && a.B >= 1 && a.H >= 1 && a.W >= 1 && a.width >= 2 &&
         a.width % 2 == 0 && a.width <= 512 && a.ldx % 2 == 0 && a.x_coff % 2 == 0 && a.x_coff >= 0 &&
         a.x_coff + a.width <= a.ldx && a.ldo % 2 == 0 && a.o_coff % 2 == 0 && a.o_coff >= 0 &&
         a.o_coff + a.width <= a.ldo &&
         (!a.add || (a.ld_add % 2 == 0 && a.add_coff % 2 == 0 && a.add_coff >= 0 && a.add_coff + a.width <= a.ld_add));
}

void res2_conv3x3(const Res2ConvArgs& a, hipStream_t st) {
  SD_CHECK(res2_conv_supported(a), kErrInvalid, "res2_conv3x3: unsupported arguments");
  const Res2Geom g = res2_geom(a);
  SD_CHECK((g.TH + 2) * (g.TW + 2) <= kMaxPos && g.TH * g.TW <= kTile, kErrInvalid, "res2_conv3x3: no tile fits");
  const int64_t blocks = (int64_t)a.B * g.n_th * g.n_tw * g.n_ct;
  SD_CHECK(blocks < (1ll << 31), kErrInvalid, "res2_conv3x3: too many tiles");
  const double px = (double)a.B * a.H * a.W;
  ProfScope prof("res2_conv3x3", 2.0 * px * 9.0 * a.width * a.width,
                 2.0 * px * a.width * (a.add ? 3.0 : 2.0) + 2.0 * 9.0 * a.width * a.width, st);
  auto al16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  const bool vec = a.width % 8 == 0 && a.ldx % 8 == 0 && a.x_coff % 8 == 0 && al16(a.x) &&
                   (!a.add || (a.ld_add % 8 == 0 && a.add_coff % 8 == 0 && al16(a.add)));
  if (vec) hipLaunchKernelGGL(res2_conv_kernel<8>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a, g);
  else hipLaunchKernelGGL(res2_conv_kernel<2>, dim3((unsigned)blocks), dim3(kThreads), 0, st, a, g);
  SD_LAUNCH_CHECK();
}

int aff_ipt(int I) {
  const int n = (I + 3) / 4;
  return n <= 2 ? 2 : n <= 4 ? 4 : n <= 7 ? 7 : 13;
}

AffPacked aff_pack(const float* w1, const float* a1, const float* c1, const float* w2, const float* a2,
                   const float* c2, int C, int I, int Cp) {
  SD_CHECK(I >= 1 && I <= 52 && C >= 2 && Cp >= C, kErrInvalid, "aff_pack: inter channels 1 .. 52");
  const int IPT = aff_ipt(I), IH = 4 * IPT;
  AffPacked p;
  p.w1.assign((size_t)2 * Cp * IH, 0.f);
  p.a1.assign(IH, 0.f);
  p.c1.assign(IH, 0.f);
  p.w2.assign((size_t)Cp * IH, 0.f);
  p.a2.assign(Cp, 0.f);
  p.c2.assign(Cp, 0.f);
  for (int i = 0; i < I; ++i) {
    const int g = i % 4, j = i / 4;   // hidden unit i = g + 4 j sits in register j of wave g
    for (int half = 0; half < 2; ++half)
      for (int c = 0; c < C; ++c)
        p.w1[((size_t)(half * Cp + c) * 4 + g) * IPT + j] = w1[(size_t)i * 2 * C + half * C + c];
    p.a1[g * IPT + j] = a1[i];
    p.c1[g * IPT + j] = c1[i];
  }
  for (int c = 0; c < C; ++c) {
    for (int i = 0; i < I; ++i) p.w2[(size_t)c * IH + i] = w2[(size_t)c * I + i];
    p.a2[c] = a2[c];
    p.c2[c] = c2[c];
  }
  return p;
}

void aff_gate(const AffGateArgs& a, hipStream_t st) {
  const int unit = a.bf16 ? 2 : 1;   // 4-byte accesses
  SD_CHECK(a.x && a.y && a.out && a.w1 && a.a1 && a.c1 && a.w2 && a.a2 && a.c2 && a.P >= 1 && a.C >= 2 &&
               a.C % 2 == 0 && a.C <= 224 && a.I >= 1 && a.I <= 52,
           kErrInvalid, "aff_gate: bad argument");
  SD_CHECK(a.ldx % unit == 0 && a.x_coff % unit == 0 && a.ldy % unit == 0 && a.y_coff % unit == 0 &&
               a.ldo % unit == 0 && a.o_coff % unit == 0 && a.x_coff + a.C <= a.ldx && a.y_coff + a.C <= a.ldy &&
               a.o_coff + a.C <= a.ldo && a.x_coff >= 0 && a.y_coff >= 0 && a.o_coff >= 0,
           kErrInvalid, "aff_gate: slices must be 4-byte aligned and inside their rows");
  const double esz = a.bf16 ? 2.0 : 4.0;
  ProfScope prof("aff_gate", 2.0 * a.P * 3.0 * a.C * a.I, esz * 3.0 * a.P * a.C, st);
  if (a.bf16) launch_aff_ipt<true>(a, st);
  else launch_aff_ipt<false>(a, st);
  SD_LAUNCH_CHECK();
}

void aff_blend(const void* x, int ldx, const void* y, int ldy, bool bf16, const float* att, int B, int H, int W, int C,
               float* out, int64_t o_sb, int64_t o_sh, int64_t o_sw, int64_t o_sn, hipStream_t st) {
  SD_CHECK(x && y && att && out && B >= 1 && H >= 1 && W >= 1 && C >= 1, kErrInvalid, "aff_blend: bad argument");
  const int64_t n = (int64_t)B * H * W * C;
  ProfScope prof("aff_blend", 0.0, n * ((bf16 ? 4.0 : 8.0) + 8.0), st);
  if (bf16)
    hipLaunchKernelGGL(aff_blend_kernel<true>, dim3(ew_blocks(n)), dim3(kThreads), 0, st,
                       static_cast<const uint16_t*>(x), ldx, static_cast<const uint16_t*>(y), ldy, att, B, H, W, C, out,
                       o_sb, o_sh, o_sw, o_sn);
  else
    hipLaunchKernelGGL(aff_blend_kernel<false>, dim3(ew_blocks(n)), dim3(kThreads), 0, st,
                       static_cast<const float*>(x), ldx, static_cast<const float*>(y), ldy, att, B, H, W, C, out, o_sb,
                       o_sh, o_sw, o_sn);
  SD_LAUNCH_CHECK();
}

void slice_add(void* x, int ldx, const void* y, int ldy, bool bf16, int64_t P, int C, hipStream_t st) {
  SD_CHECK(x && y && P >= 1 && C >= 1, kErrInvalid, "slice_add: bad argument");
  ProfScope prof("slice_add", 0.0, (bf16 ? 2.0 : 4.0) * 3.0 * P * C, st);
  if (bf16)
    hipLaunchKernelGGL(slice_add_kernel<true>, dim3(ew_blocks(P * C)), dim3(kThreads), 0, st,
                       static_cast<uint16_t*>(x), ldx, static_cast<const uint16_t*>(y), ldy, P, C);
  else
    hipLaunchKernelGGL(slice_add_kernel<false>, dim3(ew_blocks(P * C)), dim3(kThreads), 0, st, static_cast<float*>(x),
                       ldx, static_cast<const float*>(y), ldy, P, C);
  SD_LAUNCH_CHECK();
}

void nhwc_to_frames(const void* x, bool bf16, int B, int H, int W, int C, float* out, hipStream_t st) {
  SD_CHECK(x && out && B >= 1 && H >= 1 && W >= 1 && C >= 1, kErrInvalid, "nhwc_to_frames: bad argument");
  const int64_t n = (int64_t)B * H * W * C;
  ProfScope prof("nhwc_to_frames", 0.0, n * ((bf16 ? 2.0 : 4.0) + 4.0), st);
  if (bf16)
    hipLaunchKernelGGL(nhwc_to_frames_kernel<true>, dim3(ew_blocks(n)), dim3(kThreads), 0, st,
                       static_cast<const uint16_t*>(x), B, H, W, C, out);
  else
    hipLaunchKernelGGL(nhwc_to_frames_kernel<false>, dim3(ew_blocks(n)), dim3(kThreads), 0, st,
                       static_cast<const float*>(x), B, H, W, C, out);
  SD_LAUNCH_CHECK();
}

}  // namespace sd
