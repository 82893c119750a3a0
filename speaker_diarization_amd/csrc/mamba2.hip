// Mamba2 (SSD) kernels of the bidirectional Mamba2BlockV2 back end on gfx950 (kernels.h, mamba2.h).
//
// The mixer of mamba_ssm's Mamba2 (headdim 64, ngroups 1, rmsnorm, norm_before_gate False, D per head) between its two
// projections, which stay on conv_gemm:
//   zxbcdt = in_proj(rmsnorm(r))                      mamba2_norm + conv_gemm (dt_raw: fp32 dot products in mamba2_norm)
//   xBC = silu(causal_conv1d(xBC) + bias)             mamba2_scan
//   S_l = exp(dt_l A) S_{l-1} + dt_l x_l (x) Bm_l     mamba2_scan, state in registers
//   y_l = S_l Cm_l + D x_l, g = y * silu(z)           mamba2_scan (+ the head's sum of g^2 per row)
//   h = out_proj(g * rstd * norm.weight)              conv_gemm with norm.weight folded into the columns; rstd applied
//                                                     with the residual sum by the next mamba2_norm / mamba2_finish
// Both directions of a layer run in the same launches (direction is a grid dimension); the backward chain walks its
// sequence with reversed indices.
#include "kernels.h"
#include "prof.h"

#include <algorithm>

namespace sd {
namespace {

constexpr int kP = kMamba2HeadDim;   // channels of a head
constexpr int kTL = 16;              // steps staged in LDS at a time

__device__ __forceinline__ float silu_f(float v) { return v / (1.f + __expf(-v)); }

// rstd of the gated RMSNorm of row r: the heads' partial sums in head order (no atomics: bit-identical runs)
__device__ __forceinline__ float gated_rstd(const float* ssq, int64_t r, int nh, int d_inner) {
  float s = 0.f;
  for (int h = 0; h < nh; ++h) s += ssq[r * nh + h];
  return rsqrtf(s / (float)d_inner + kMamba2Eps);
}

// One wave per (row, direction).
template <bool BF>
__global__ __launch_bounds__(256) void mamba2_norm_kernel(Mamba2NormArgs a) {
  const int lane = threadIdx.x & 63, dir = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.rows) return;
  const int E = a.E;
  const int64_t dr = (int64_t)dir * a.rows + r;
  const float* rin = a.r_in + (int64_t)dir * a.r_in_dir + r * E;
  float ss = 0.f;
  if (a.t) {
    const float gs = gated_rstd(a.ssq, dr, a.nh, a.d_inner);
    const float* t = a.t + dr * E;
    float* ro = a.r_out + dr * E;
    for (int e = lane; e < E; e += 64) {
      const float v = fmaf(t[e], gs, rin[e]);
      ro[e] = v;
      ss = fmaf(v, v, ss);
    }
    rin = ro;   // the second pass reads what this lane stored
  } else {
    for (int e = lane; e < E; e += 64) ss = fmaf(rin[e], rin[e], ss);
  }
  const float rstd = rsqrtf(warp_sum(ss) / (float)E + kMamba2Eps);
  act_t<BF>* y = reinterpret_cast<act_t<BF>*>(a.y) + dr * E;
  const float* w = a.w + (int64_t)dir * E;
  for (int e = lane; e < E; e += 64) st_act(y, e, rin[e] * rstd * w[e]);
  // dt_raw = the normalised row times in_proj's dt rows, in fp32 from the unrounded row whatever the GEMMs' precision
  const float* wd = a.w_dt + (int64_t)dir * a.nh * E;
  float* dt = a.dt_raw + dr * a.nh;
  for (int h = 0; h < a.nh; ++h) {
    float s = 0.f;
    for (int e = lane; e < E; e += 64) s = fmaf(rin[e] * rstd * w[e], wd[(int64_t)h * E + e], s);
    s = warp_sum(s);
    if (lane == 0) dt[h] = s;
  }
}

template <bool BF>
__global__ __launch_bounds__(256) void mamba2_finish_kernel(Mamba2FinishArgs a) {
  const int lane = threadIdx.x & 63, dir = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.rows) return;
  const int E = a.E;
  const int64_t dr = (int64_t)dir * a.rows + r;
  const float* rin = a.r_in + (int64_t)dir * a.r_in_dir + r * E;
  const float* t = a.t + dr * E;
  const float gs = gated_rstd(a.ssq, dr, a.nh, a.d_inner);
  const int64_t seq = r / a.T, tt = r % a.T, b = seq / a.NS, spk = seq % a.NS;
  act_t<BF>* o = reinterpret_cast<act_t<BF>*>(a.out) + (b * a.T + tt) * ((int64_t)a.NS * 2 * E) + (spk * 2 + dir) * E;
  for (int e = lane; e < E; e += 64) st_act(o, e, fmaf(t[e], gs, rin[e]));
}

// NJ: states per thread; thread (p = tid / 4, q = tid % 4) owns states [q * NJ, (q + 1) * NJ) of channel p, so
// d_state <= 4 * NJ (states past d_state read zero Bm / Cm and stay zero).
template <bool BF, int NJ>
__global__ __launch_bounds__(256) void mamba2_scan_kernel(Mamba2ScanArgs a) {
  constexpr int NP = NJ + 4;        // a quarter row padded by 4 floats: the four quarters' 16-B reads hit disjoint banks
  constexpr int NROW = 4 * NP;
  constexpr int W = kP + 8 * NJ;    // staged values per step: x | Bm | Cm
  constexpr int V = BF ? 8 : 4;     // elements per 16-byte load
  constexpr int U = W / V;          // loads per step
  // rows 0 .. 2: the three steps before the chunk (the conv's history); row l + 3: step l of the chunk
  __shared__ __attribute__((aligned(16))) float sB[kTL + 3][NROW];
  __shared__ __attribute__((aligned(16))) float sC[kTL + 3][NROW];
  __shared__ __attribute__((aligned(16))) float sX[kTL + 3][kP];
  __shared__ float sY[kTL][kP], sDt[kTL], sDa[kTL];
  using T = act_t<BF>;
  const int tid = threadIdx.x;
  const int seq = blockIdx.x, h = blockIdx.y, dir = blockIdx.z;
  const int grp = seq / a.I, inner = seq % a.I;
  const int w0 = grp * a.G;
  const int L = min(a.G, a.B - w0);
  const int N = a.d_state, DI = a.d_inner, H = DI / kP, CD = DI + 2 * N;
  const T* zx = reinterpret_cast<const T*>(a.zx) + (int64_t)dir * a.rows * a.ldz;
  T* gout = reinterpret_cast<T*>(a.g) + (int64_t)dir * a.rows * DI;
  float* ssq = a.ssq + (int64_t)dir * a.rows * H;
  const float* cw = a.conv_w + (int64_t)dir * CD * 4;
  const float* cb = a.conv_b + (int64_t)dir * CD;
  const float dtb = a.dt_bias[dir * H + h], A = a.A[dir * H + h], Dh = a.D[dir * H + h];
  // token row of step l: the backward chain reads its windows last to first
  auto row = [&](int l) -> int64_t { return (int64_t)(w0 + (dir ? L - 1 - l : l)) * a.I + inner; };
  const int p = tid >> 2, q = tid & 3;
  float S[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) S[j] = 0.f;

  for (int l0 = 0; l0 < L; l0 += kTL) {
    const int tl = min(kTL, L - l0);
    // ---- the raw xBC values of this head's x and of Bm / Cm for steps l0 - 3 .. l0 + tl - 1 into LDS rows 0 .. tl + 2
    // (zeros before the sequence's start and for the states past d_state), 16 bytes per load
    for (int idx = tid; idx < (tl + 3) * U; idx += 256) {
      const int j = idx / U, u = idx % U;
      const int ls = l0 - 3 + j;
      int col = 0;
      float* dst;
      bool live = ls >= 0;
      if (u < kP / V) {
        col = h * kP + u * V;
        dst = &sX[j][u * V];
      } else {
        const int v = u - kP / V;
        const bool is_c = v >= 4 * NJ / V;
        const int n0 = (v % (4 * NJ / V)) * V;
        dst = (is_c ? sC[j] : sB[j]) + (n0 / NJ) * NP + n0 % NJ;
        live = live && n0 < N;   // d_state is a multiple of 16: a vector never straddles it
        col = DI + (is_c ? N : 0) + n0;
      }
      float f[V];
#pragma unroll
      for (int i = 0; i < V; ++i) f[i] = 0.f;
      if (live) {
        const T* src = zx + row(ls) * a.ldz + DI + col;
        if constexpr (BF) {
          const uint4 raw = *reinterpret_cast<const uint4*>(src);
          const uint32_t wds[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            f[2 * i] = __uint_as_float(wds[i] << 16);
            f[2 * i + 1] = __uint_as_float(wds[i] & 0xffff0000u);
          }
        } else {
          const float4 raw = *reinterpret_cast<const float4*>(src);
          f[0] = raw.x; f[1] = raw.y; f[2] = raw.z; f[3] = raw.w;
        }
      }
#pragma unroll
      for (int i = 0; i < V; i += 4) *reinterpret_cast<float4*>(dst + i) = make_float4(f[i], f[i + 1], f[i + 2], f[i + 3]);
    }
    __syncthreads();
    // ---- causal conv + bias + SiLU in place, one thread per channel walking its steps last to first (row j = l + 3
    // is overwritten once rows j - 3 .. j have been read)
    for (int c = tid; c < W; c += 256) {
      int ch, stride;
      float* pc;
      if (c < kP) {
        ch = h * kP + c;
        pc = &sX[0][c];
        stride = kP;
      } else {
        const bool is_c = c - kP >= 4 * NJ;
        const int n = (c - kP) % (4 * NJ);
        if (n >= N) continue;   // stays zero
        ch = DI + (is_c ? N : 0) + n;
        pc = (is_c ? sC[0] : sB[0]) + (n / NJ) * NP + n % NJ;
        stride = NROW;
      }
      const float w0c = cw[ch * 4], w1c = cw[ch * 4 + 1], w2c = cw[ch * 4 + 2], w3c = cw[ch * 4 + 3], bc = cb[ch];
      for (int j = tl + 2; j >= 3; --j) {
        float acc = fmaf(w0c, pc[(j - 3) * stride], bc);
        acc = fmaf(w1c, pc[(j - 2) * stride], acc);
        acc = fmaf(w2c, pc[(j - 1) * stride], acc);
        acc = fmaf(w3c, pc[j * stride], acc);
        pc[j * stride] = silu_f(acc);
      }
    }
    if (tid < tl) {
      const int64_t r = row(l0 + tid);
      const float v = a.dt_raw[((int64_t)dir * a.rows + r) * H + h] + dtb;
      const float dt = v > 20.f ? v : log1pf(expf(v));   // F.softplus (threshold 20)
      sDt[tid] = dt;
      sDa[tid] = expf(dt * A);
    }
    __syncthreads();
    // ---- the recurrence
    for (int ll = 0; ll < tl; ++ll) {
      const float da = sDa[ll], dtx = sDt[ll] * sX[ll + 3][p];
      const float4* bq = reinterpret_cast<const float4*>(sB[ll + 3] + q * NP);
      const float4* cq = reinterpret_cast<const float4*>(sC[ll + 3] + q * NP);
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < NJ / 4; ++j) {
        const float4 bv = bq[j], cv = cq[j];
        S[4 * j + 0] = fmaf(da, S[4 * j + 0], dtx * bv.x);
        S[4 * j + 1] = fmaf(da, S[4 * j + 1], dtx * bv.y);
        S[4 * j + 2] = fmaf(da, S[4 * j + 2], dtx * bv.z);
        S[4 * j + 3] = fmaf(da, S[4 * j + 3], dtx * bv.w);
        acc = fmaf(S[4 * j + 0], cv.x, acc);
        acc = fmaf(S[4 * j + 1], cv.y, acc);
        acc = fmaf(S[4 * j + 2], cv.z, acc);
        acc = fmaf(S[4 * j + 3], cv.w, acc);
      }
      acc += __shfl_xor(acc, 1, 64);
      acc += __shfl_xor(acc, 2, 64);
      if (q == 0) sY[ll][p] = acc;
    }
    __syncthreads();
    // ---- skip term, gate, store, the head's share of the row's sum of g^2: one wave per step
    const int lane = tid & 63;
    for (int ll = tid >> 6; ll < tl; ll += 4) {
      const int64_t r = row(l0 + ll);
      const float x = sX[ll + 3][lane];
      const float y = fmaf(Dh, x, sY[ll][lane]);
      const float g = y * silu_f(ld_act(zx, r * a.ldz + h * kP + lane));
      st_act(gout, r * DI + h * kP + lane, g);
      const float s = warp_sum(g * g);
      if (lane == 0) ssq[r * H + h] = s;
    }
    __syncthreads();
  }
}

template <bool BF>
void launch_scan(const Mamba2ScanArgs& a, dim3 grid, hipStream_t st) {
  if (a.d_state <= 64) hipLaunchKernelGGL((mamba2_scan_kernel<BF, 16>), grid, dim3(256), 0, st, a);
  else if (a.d_state <= 128) hipLaunchKernelGGL((mamba2_scan_kernel<BF, 32>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((mamba2_scan_kernel<BF, 64>), grid, dim3(256), 0, st, a);
}

__global__ __launch_bounds__(256) void poison_groups_kernel(float* x, int64_t per_win, const int* grp, int group) {
  const int w = blockIdx.x;
  if (!grp[w / group]) return;
  float* xr = x + (int64_t)w * per_win;
  for (int64_t i = threadIdx.x; i < per_win; i += blockDim.x) xr[i] = __uint_as_float(0x7fc00000u);
}

}  // namespace

void mamba2_norm(const Mamba2NormArgs& a, hipStream_t st) {
  SD_CHECK(a.rows > 0 && a.E > 0 && a.r_in && a.w && a.y && a.w_dt && a.dt_raw && a.nh > 0, kErrInvalid,
           "mamba2_norm: bad argument");
  SD_CHECK(!a.t || (a.ssq && a.r_out && a.d_inner > 0), kErrInvalid, "mamba2_norm: t needs ssq and r_out");
  ProfScope prof("mamba2_norm", 0.0, (double)a.rows * a.E * 2 * (a.t ? 16.0 : 4.0 + (a.y_bf16 ? 2.0 : 4.0)), st);
  const dim3 grid((unsigned)((a.rows + 3) / 4), 2);
  if (a.y_bf16) hipLaunchKernelGGL(mamba2_norm_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(mamba2_norm_kernel<false>, grid, dim3(256), 0, st, a);
  SD_LAUNCH_CHECK();
}

void mamba2_finish(const Mamba2FinishArgs& a, hipStream_t st) {
  SD_CHECK(a.rows > 0 && a.E > 0 && a.r_in && a.t && a.ssq && a.out && a.nh > 0 && a.d_inner > 0, kErrInvalid,
           "mamba2_finish: bad argument");
  SD_CHECK(a.NS >= 1 && a.T >= 1 && a.rows % ((int64_t)a.NS * a.T) == 0, kErrInvalid,
           "mamba2_finish: rows must be whole (window, speaker) blocks of T frames");
  ProfScope prof("mamba2_finish", 0.0, (double)a.rows * a.E * 2 * (8.0 + (a.out_bf16 ? 2.0 : 4.0)), st);
  const dim3 grid((unsigned)((a.rows + 3) / 4), 2);
  if (a.out_bf16) hipLaunchKernelGGL(mamba2_finish_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(mamba2_finish_kernel<false>, grid, dim3(256), 0, st, a);
  SD_LAUNCH_CHECK();
}

void mamba2_scan(const Mamba2ScanArgs& a, hipStream_t st) {
  SD_CHECK(a.zx && a.dt_raw && a.g && a.ssq && a.conv_w && a.conv_b && a.dt_bias && a.A && a.D, kErrInvalid,
           "mamba2_scan: null argument");
  SD_CHECK(a.B >= 1 && a.G >= 1 && a.I >= 1 && a.rows == (int64_t)a.B * a.I, kErrInvalid,
           "mamba2_scan: rows must be B * I");
  SD_CHECK(a.d_inner >= kMamba2HeadDim && a.d_inner % kMamba2HeadDim == 0 && a.d_inner / kMamba2HeadDim <= 65535,
           kErrInvalid, "mamba2_scan: d_inner must be a multiple of 64");
  SD_CHECK(a.d_state >= 1 && a.d_state <= kMamba2MaxState, kErrInvalid, "mamba2_scan: d_state must be 1 .. 256");
  const int heads = a.d_inner / kMamba2HeadDim;
  SD_CHECK(a.ldz >= 2 * a.d_inner + 2 * a.d_state + heads, kErrInvalid, "mamba2_scan: ldz below d_in_proj");
  const int64_t nseq = (int64_t)cdiv(a.B, a.G) * a.I;
  SD_CHECK(nseq <= 0x7fffffff, kErrInvalid, "mamba2_scan: too many sequences");
  const double el = a.bf16 ? 2.0 : 4.0;
  // zxbcdt read once, g written once; 2 * (2 flops per state update + 2 per output term) per (row, channel, state)
  ProfScope prof("mamba2_scan", 2.0 * a.rows * a.d_inner * (4.0 * a.d_state),
                 2.0 * a.rows * (el * (a.ldz + a.d_inner) + 4.0 * heads), st);
  prof.set_steps((double)std::min(a.G, a.B));
  const dim3 grid((unsigned)nseq, heads, 2);
  if (a.bf16) launch_scan<true>(a, grid, st);
  else launch_scan<false>(a, grid, st);
  SD_LAUNCH_CHECK();
}

void poison_groups(float* x, int B, int64_t per_win, const int* grp, int group, hipStream_t st) {
  SD_CHECK(x && grp && B >= 1 && group >= 1, kErrInvalid, "poison_groups: bad argument");
  hipLaunchKernelGGL(poison_groups_kernel, dim3(B), dim3(256), 0, st, x, per_win, grp, group);
  SD_LAUNCH_CHECK();
}

}  // namespace sd
