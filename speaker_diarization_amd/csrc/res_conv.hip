// ResNet34 trunk 3x3 convolutions (resnet_wespeaker.py BasicBlock) for gfx950: bf16 NHWC maps, pad 1, stride 1
// or 2 in BOTH axes, Cin / Cout in {32, 64, 128, 256, 512}, fp32 accumulation on v_mfma_f32_16x16x32_bf16.
//
// A workgroup (4 waves) owns an output patch of TH x TW <= 128 pixels (chosen per map so that narrow maps still
// fill their tiles, res_geom below) times NT = 32 or 64 output channels, and walks Cin in slabs of 32 channels:
//   - the slab's input halo ((TH-1)s+3) x ((TW-1)s+3) pixels x 64 B is staged in LDS once (every input pixel is
//     read from memory once per tile and slab, not nine times), the slab's 9 x NT x 32 weights next to it (streamed
//     per slab from the packed Wt[N][K]: nothing holds all 9 Cin Cout weights);
//   - the NEXT slab's halo and weights are loaded into registers while the current slab computes;
//   - per tap a wave reads 2 weight fragments + PB pixel fragments (16 B per lane each) for 2 PB MFMAs, weights as
//     the A operand so a lane ends with 8 contiguous channels of one pixel (band_channel order, as fcm_conv.hip).
// LDS images are chunk planes: the q-th 16-B chunk (channels 8q..8q+7 of the slab) of every pixel / weight row is
// contiguous at 16 B per pixel, plane sizes multiples of 256 B, so the 16 lanes of a ds_read_b128 lane group
// (8 lanes of one q, 8 of another, consecutive pixels) hit 16 distinct 16-B bank slots.  With stride 2 the halo
// columns are staged even columns first, then odd ones: a tap's 16 pixels are again consecutive.  The staging
// stores put 8 consecutive pixels of one chunk on the 8 lanes of a ds_write_b128 lane group (128 contiguous bytes).
// The 1x1 stride-2 shortcut of a block opener is two more MFMAs per pixel block on the centre tap's fragment
// (ResFuse), stored to a second output.  Epilogue: folded BN, bf16 residual, ReLU that keeps NaN, 16-B bf16 stores.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "launch.h"
#include "prof.h"

namespace sd {
namespace {

constexpr int kThreads = 256;
constexpr int kTileM = 128;                       // output pixels per workgroup
constexpr uint32_t kNoPix = 0xffffffffu;

// Output channel (within a 32-channel group) of accumulator row i of MFMA tile nt: lane group q owns the 8
// contiguous channels 8q .. 8q+7 over its two tiles (fcm_conv.hip band_channel).
__host__ __device__ inline int res_channel(int i, int nt) { return 8 * (i >> 2) + 4 * nt + (i & 3); }

struct ResGeom {
  int TH, TW;      // output patch
  int HR, HC;      // halo rows / columns
  int HCh;         // stride 2: even halo columns, (HC + 1) / 2
  int HCp;         // staged positions per halo row: HC, or 2 * HCh
  int plane;       // bytes per chunk plane (multiple of 256)
  int n_th, n_tw;  // tiles over Ho / Wo
  int n_ct;        // output-channel tiles
};

// staged halo positions a thread can hold in its prefetch registers (4 chunks per position, 256 threads)
template <int S>
constexpr int res_xper() { return S == 1 ? 4 : 10; }
template <int S>
constexpr int res_max_pos() { return res_xper<S>() * kThreads / 4; }

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int WM, int WN, int PB, int S, bool SC>
__global__ __launch_bounds__(kThreads) void res_conv_kernel(ConvGemmArgs p, ResFuse f, ResGeom g) {
  static_assert(WM * WN == 4 && 16 * PB * WM == kTileM, "4 waves cover the 128-pixel tile");
  constexpr int NT = 32 * WN;
  constexpr int kXPer = res_xper<S>();
  constexpr int kWVec = 9 * NT * 4;                              // 16-B chunks of a weight slab
  constexpr int kWPer = (kWVec + kThreads - 1) / kThreads;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];   // [4 planes of halo][9 taps x 4 planes x NT rows]
  uint8_t* const xs = smem;
  uint8_t* const wsm = smem + 4 * g.plane;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int wm = wv / WN, wn = wv % WN;
  const uint16_t* A = reinterpret_cast<const uint16_t*>(p.A);
  const uint16_t* Wt = reinterpret_cast<const uint16_t*>(p.Wt);

  const int ct = blockIdx.x % g.n_ct;
  int tile = blockIdx.x / g.n_ct;
  const int tw = tile % g.n_tw;
  tile /= g.n_tw;
  const int th = tile % g.n_th, b = tile / g.n_th;
  const int ho0 = th * g.TH, wo0 = tw * g.TW, n0 = ct * NT;

  // ---- staging maps (slab-invariant).  A wave-instruction covers 16 consecutive positions x 4 chunks; lane l
  // takes position (l & 7) + 8 (l >> 5), chunk (l >> 3) & 3: 8-lane groups write 128 contiguous bytes
  const int s_pos = (lane & 7) + 8 * (lane >> 5), s_q = (lane >> 3) & 3;
  uint32_t x_src[kXPer];   // element offset of the position's pixel (slab 0, chunk s_q) in A, kNoPix = zeros
  int x_dst[kXPer];        // byte offset in xs, -1 = nothing to stage
  const int n_pos = g.HR * g.HCp;
#pragma unroll
  for (int k = 0; k < kXPer; ++k) {
    const int pos = (wv + 4 * k) * 16 + s_pos;
    x_src[k] = kNoPix;
    x_dst[k] = -1;
    if (pos < n_pos) {
      const int row = pos / g.HCp, cp = pos - row * g.HCp;
      const int c = S == 1 ? cp : (cp < g.HCh ? 2 * cp : 2 * (cp - g.HCh) + 1);
      const int hi = ho0 * S - 1 + row, wi = wo0 * S - 1 + c;
      x_dst[k] = s_q * g.plane + pos * 16;
      if (c < g.HC && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
        x_src[k] = (uint32_t)((((int64_t)b * p.H + hi) * p.W + wi) * p.lda + p.a_coff + s_q * 8);
    }
  }
  // weights: LDS row j of tap t, chunk q at ((t * 4 + q) * NT + j) * 16 holds channel n0 + 32 (j >> 5) +
  // res_channel(j & 15, (j >> 4) & 1), so fragment reads take consecutive rows
  uint32_t w_src[kWPer];
  int w_dst[kWPer];
#pragma unroll
  for (int k = 0; k < kWPer; ++k) {
    const int grp = wv + 4 * k;                      // 16 rows x 4 chunks
    const int t = grp / (NT / 16), j = (grp % (NT / 16)) * 16 + s_pos;
    w_dst[k] = -1;
    w_src[k] = 0;
    if (grp < 9 * (NT / 16)) {
      const int n = n0 + 32 * (j >> 5) + res_channel(j & 15, (j >> 4) & 1);
      w_dst[k] = ((t * 4 + s_q) * NT + j) * 16;
      w_src[k] = (uint32_t)(n * p.K + t * p.Cin + s_q * 8);
    }
  }
  // ---- this lane's pixels: p = (wm * PB + pb) * 16 + l15 of the patch, row-major over TH x TW
  int base[PB];        // staged position of the pixel's tap (0, 0)
  bool pvalid[PB];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {
    const int pp = (wm * PB + pb) * 16 + l15;
    const int r = pp / g.TW, c = pp - r * g.TW;
    pvalid[pb] = pp < g.TH * g.TW && ho0 + r < p.Ho && wo0 + c < p.Wo;
    base[pb] = pp < g.TH * g.TW ? r * S * g.HCp + c : 0;
  }
  const int tapcol[3] = {0, S == 1 ? 1 : g.HCh, S == 1 ? 2 : 1};
  const int sc_row = n0 + wn * 32;   // first channel of this wave's 32-channel group

  u32x4_t xv[kXPer], wvv[kWPer];
  u32x4_t scv[2];
  auto load_slab = [&](int slab) {
#pragma unroll
    for (int k = 0; k < kXPer; ++k) {
      xv[k] = u32x4_t{0u, 0u, 0u, 0u};
      if (x_src[k] != kNoPix) xv[k] = *reinterpret_cast<const u32x4_t*>(A + (size_t)x_src[k] + slab * 32);
    }
#pragma unroll
    for (int k = 0; k < kWPer; ++k)   // unconditional (a lane with nothing to stage re-reads row 0): stays in registers
      wvv[k] = *reinterpret_cast<const u32x4_t*>(Wt + (size_t)w_src[k] + slab * 32);
    if constexpr (SC) {
      const uint16_t* Ws = reinterpret_cast<const uint16_t*>(f.sc_w);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        scv[nt] = *reinterpret_cast<const u32x4_t*>(Ws + (size_t)(sc_row + res_channel(l15, nt)) * p.Cin + slab * 32 + q * 8);
    }
  };

  floatx4 acc[PB][2], sacc[SC ? PB : 1][2];
#pragma unroll
  for (int pb = 0; pb < PB; ++pb)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      acc[pb][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
      if constexpr (SC) sacc[pb][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
    }

  const int n_slab = p.Cin / 32;
  load_slab(0);
  for (int slab = 0; slab < n_slab; ++slab) {
#pragma unroll
    for (int k = 0; k < kXPer; ++k)
      if (x_dst[k] >= 0) *reinterpret_cast<u32x4_t*>(xs + x_dst[k]) = xv[k];
#pragma unroll
    for (int k = 0; k < kWPer; ++k)
      if (w_dst[k] >= 0) *reinterpret_cast<u32x4_t*>(wsm + w_dst[k]) = wvv[k];
    bf16x8 wsc[2];
    if constexpr (SC) {
      wsc[0] = __builtin_bit_cast(bf16x8, scv[0]);
      wsc[1] = __builtin_bit_cast(bf16x8, scv[1]);
    }
    lds_barrier();   // the slab is staged
    if (slab + 1 < n_slab) load_slab(slab + 1);   // in flight while this slab computes
    const uint8_t* xq = xs + q * g.plane;
#pragma unroll
    for (int dh = 0; dh < 3; ++dh)
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) {
        const int t = dh * 3 + dw;
        const int toff = dh * g.HCp + tapcol[dw];
        bf16x8 wf[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          wf[nt] = *reinterpret_cast<const bf16x8*>(wsm + ((t * 4 + q) * NT + wn * 32 + nt * 16 + l15) * 16);
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(xq + (base[pb] + toff) * 16);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            acc[pb][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], af, acc[pb][nt], 0, 0, 0);
          if constexpr (SC) {
            if (t == 4)   // input pixel (S ho, S wo): the 1x1 shortcut's operand
#pragma unroll
              for (int nt = 0; nt < 2; ++nt)
                sacc[pb][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wsc[nt], af, sacc[pb][nt], 0, 0, 0);
          }
        }
      }
    lds_barrier();   // every wave is done with the slab's LDS image
  }

  // ---- epilogue: this lane holds channels c0 .. c0 + 7 of its PB pixels
  const int c0 = n0 + wn * 32 + q * 8;
  float al[8], be[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    al[u] = p.alpha ? p.alpha[c0 + u] : 1.f;
    be[u] = p.beta ? p.beta[c0 + u] : 0.f;
  }
  const bool nhwc = p.o_sn == 1 && p.o_sw == p.N && p.o_sh == (int64_t)p.Wo * p.N &&
                    p.o_sb == (int64_t)p.Ho * p.Wo * p.N;
  uint16_t* const out = reinterpret_cast<uint16_t*>(p.out);
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {
    if (!pvalid[pb]) continue;
    const int pp = (wm * PB + pb) * 16 + l15;
    const int r = pp / g.TW, c = pp - r * g.TW;
    const int ho = ho0 + r, wo = wo0 + c;
    const int64_t pix = ((int64_t)b * p.Ho + ho) * p.Wo + wo;
    if constexpr (SC) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = fmaf(sacc[pb][u >> 2][u & 3], f.sc_alpha[c0 + u], f.sc_beta[c0 + u]);
      *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(f.sc_out) + pix * p.N + c0) =
          make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                     pack_bf16x2(v[6], v[7]));
    }
    float rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (p.res) {
      const uint4 r4 = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(p.res) + pix * p.res_ld + c0);
      const uint32_t rw[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        rv[2 * u] = __uint_as_float(rw[u] << 16);
        rv[2 * u + 1] = __uint_as_float(rw[u] & 0xffff0000u);
      }
    }
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      v[u] = fmaf(acc[pb][u >> 2][u & 3], al[u], be[u]) + rv[u];
      if (p.act == kActRelu) v[u] = relu_keep_nan(v[u]);
    }
    if (nhwc) {
      *reinterpret_cast<uint4*>(out + pix * p.N + c0) =
          make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                     pack_bf16x2(v[6], v[7]));
    } else {
      const int64_t ob = (int64_t)b * p.o_sb + (int64_t)ho * p.o_sh + (int64_t)wo * p.o_sw;
#pragma unroll
      for (int u = 0; u < 8; ++u) out[ob + (int64_t)(c0 + u) * p.o_sn] = f2bf_bits(v[u]);
    }
  }
}

// The patch TH x TW <= 128 pixels with the fewest tiles over the Ho x Wo map (then the smallest halo) whose halo
// fits the prefetch registers: 8 x 16 on the wide stage-1 / stage-2 maps, 5 x 25 on the 20 x 100 and 10 x 50
// maps of stages 3 and 4 (2 x 2 tiles of a 10 x 50 map with 2 % of the lanes idle; 16-frame row strips would
// leave 22 %).
ResGeom res_geom(const ConvGemmArgs& p, int NT) {
  const int s = p.sh, max_pos = s == 1 ? res_max_pos<1>() : res_max_pos<2>();
  ResGeom best{};
  int64_t best_tiles = -1, best_halo = 0;
  for (int th = 1; th <= std::min(p.Ho, kTileM); ++th) {
    const int tw = std::min(p.Wo, kTileM / th);
    const int hr = (th - 1) * s + 3, hc = (tw - 1) * s + 3;
    const int hch = (hc + 1) / 2, hcp = s == 1 ? hc : 2 * hch;
    if (hr * hcp > max_pos) continue;
    const int64_t tiles = (int64_t)cdiv(p.Ho, th) * cdiv(p.Wo, tw), halo = (int64_t)hr * hcp;
    if (best_tiles < 0 || tiles < best_tiles || (tiles == best_tiles && halo < best_halo)) {
      best_tiles = tiles;
      best_halo = halo;
      best.TH = th; best.TW = tw; best.HR = hr; best.HC = hc; best.HCh = hch; best.HCp = hcp;
      best.plane = (hr * hcp * 16 + 255) / 256 * 256;
      best.n_th = cdiv(p.Ho, th); best.n_tw = cdiv(p.Wo, tw);
    }
  }
  best.n_ct = p.N / NT;
  return best;
}

template <int WM, int WN, int PB, int S, bool SC>
void launch_res(const ConvGemmArgs& p, const ResFuse& f, hipStream_t st) {
  constexpr int NT = 32 * WN;
  const ResGeom g = res_geom(p, NT);
  SD_CHECK(g.TH > 0, kErrInvalid, "res_conv: no tile fits");
  const int64_t blocks = (int64_t)p.B * g.n_th * g.n_tw * g.n_ct;
  SD_CHECK(blocks < (1ll << 31), kErrInvalid, "res_conv: too many tiles");
  const size_t smem = (size_t)4 * g.plane + (size_t)9 * 4 * NT * 16;
  allow_dynamic_lds<&res_conv_kernel<WM, WN, PB, S, SC>>(96 * 1024);
  SD_CHECK(smem <= 96 * 1024, kErrInvalid, "res_conv: LDS budget");
  hipLaunchKernelGGL((res_conv_kernel<WM, WN, PB, S, SC>), dim3((unsigned)blocks), dim3(kThreads), smem, st, p, f, g);
}

// The kernel streams the weights per 32-channel slab, so the width is bounded only by what has been tested.
bool res_chan_ok(int c) { return c == 32 || c == 64 || c == 128 || c == 256 || c == 512; }

}  // namespace

bool res_conv_runs(const ConvGemmArgs& p) {
  return p.a_bf16 && p.out_bf16 && !p.pre_scale && !p.gate && !p.glu && !p.a_tiled && p.kh == 3 && p.kw == 3 &&
         p.ph == 1 && p.pw == 1 && p.dh == 1 && p.dw == 1 && p.sh == p.sw && (p.sh == 1 || p.sh == 2) &&
         res_chan_ok(p.Cin) && res_chan_ok(p.N) && p.K == 9 * p.Cin && p.lda % 8 == 0 && p.a_coff % 8 == 0 &&
         p.a_coff + p.Cin <= p.lda && (p.act == kActNone || p.act == kActRelu) &&
         (!p.res || (p.res_bf16 && p.res_ld % 8 == 0)) && p.Ho == (p.H - 1) / p.sh + 1 &&
         p.Wo == (p.W - 1) / p.sw + 1 && (int64_t)p.B * p.H * p.W * p.lda < (1ll << 31) &&
         (int64_t)p.N * p.K < (1ll << 31);
}

// The shape classes on which the kernel measured faster than conv_gemm by more than the run-to-run spread
// (tools/res_conv_probe.py at B = 64): the stride-1 convs of stages 2-4 and the stage-2
// opener.  Refused, so conv_gemm serves them: 32 -> 32 stride 1 (fcm_conv.hip's ring kernel is 1.4x faster), the
// stage-3 / stage-4 openers 64 -> 128 and 128 -> 256 at stride 2 (gemm_dma + a separate shortcut launch is 1.3x
// faster), and every class that was not measured.  The base-64 trunk's classes (SimAM-ResNet34: 64 -> 64 on the 80-row
// map, 512 -> 512, the 64 -> 128 / 128 -> 256 / 256 -> 512 openers) were measured on their own at B = 96, 598 frames
//  and the same rule matches that table: every stride-1 class here, every opener to conv_gemm.
bool res_conv_supported(const ConvGemmArgs& p) {
  if (!res_conv_runs(p)) return false;
  if (p.sh == 1) return p.Cin == p.N && p.Cin >= 64;
  return p.Cin == 32 && p.N == 64;
}

void res_conv3x3(const ConvGemmArgs& p, const ResFuse& f, hipStream_t st) {
  SD_CHECK(res_conv_runs(p), kErrInvalid, "res_conv: unsupported arguments");
  SD_CHECK(!f.sc_w || (f.sc_alpha && f.sc_beta && f.sc_out), kErrInvalid, "res_conv: incomplete shortcut");
  const double px = (double)p.B * p.Ho * p.Wo;
  const double flops = 2.0 * px * p.N * p.K + (f.sc_w ? 2.0 * px * p.N * p.Cin : 0.0);
  const double bytes = 2.0 * p.B * p.H * p.W * p.Cin + 2.0 * p.N * (p.K + (f.sc_w ? p.Cin : 0)) +
                       2.0 * px * p.N * (1 + (p.res ? 1 : 0) + (f.sc_w ? 1 : 0));
  ProfScope prof("res_conv3x3", flops, bytes, st);
  const bool sc = f.sc_w != nullptr, n32 = p.N == 32;
  if (p.sh == 1) {
    if (n32) sc ? launch_res<4, 1, 2, 1, true>(p, f, st) : launch_res<4, 1, 2, 1, false>(p, f, st);
    else sc ? launch_res<2, 2, 4, 1, true>(p, f, st) : launch_res<2, 2, 4, 1, false>(p, f, st);
  } else {
    if (n32) sc ? launch_res<4, 1, 2, 2, true>(p, f, st) : launch_res<4, 1, 2, 2, false>(p, f, st);
    else sc ? launch_res<2, 2, 4, 2, true>(p, f, st) : launch_res<2, 2, 4, 2, false>(p, f, st);
  }
  SD_LAUNCH_CHECK();
}

}  // namespace sd
