// ResNet34 pooled head prologue: TSTP (temporal statistics pooling, egs/alimeeting/ts_vad2/
// pooling_layers_wespeaker.py:66-88): stats = [mean_t x | sqrt(var_t x (unbiased) + 1e-7)] over the stage-4 map
// x (B, T', C) channel-last (C = 2560, channel c * 10 + f: TSTP flattens (C, F) the same way), plus the fp32
// time-out map when asked for.  The epsilon is an argument: 3D-Speaker's TSTP (pooling_layers_3d_speaker.py:52, ERes2NetV2)
// adds 1e-8.
//
// stats_pool's layout: one workgroup owns 64 channels of one batch row, its 4 waves split the time axis, so every
// wave load is 64 consecutive channels of one frame (128 B bf16 / 256 B fp32).  Two passes over the (small,
// L2-resident) rows, both accumulated in fp64: a channel that is constant over time (a dead ReLU channel) has a
// mean equal to its value, every deviation exactly 0 and std = sqrt(1e-7) exactly -- E[x^2] - mean^2 would leave
// rounding noise of the order of 1e-7 itself there.  Nothing clamps: a NaN frame makes its channel's mean and std
// NaN and no other, and T' == 1 gives var = 0 / 0 = NaN like torch.var(unbiased).
#include "common.h"
#include "kernels.h"
#include "prof.h"

namespace sd {
namespace {

constexpr int kGroups = 4;

template <bool BF>
__global__ __launch_bounds__(256) void tstp_pool_kernel(const act_t<BF>* __restrict__ x, int T, int C,
                                                        float* __restrict__ stats, float* __restrict__ tout,
                                                        double eps) {
  __shared__ double red[kGroups][64];
  const int lane = threadIdx.x & 63;
  const int g = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int c = blockIdx.x * 64 + lane;   // C % 64 == 0: always in range
  const act_t<BF>* xb = x + (int64_t)b * T * C + c;
  double sum = 0.0;
  for (int t = g; t < T; t += kGroups) {
    const float v = ld_act(xb, (int64_t)t * C);
    sum += (double)v;
    if (tout) tout[((int64_t)b * T + t) * C + c] = v;
  }
  if (!stats) return;
  red[g][lane] = sum;
  __syncthreads();
  const double mean = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (double)T;
  __syncthreads();
  double ss = 0.0;
  for (int t = g; t < T; t += kGroups) {
    const double d = (double)ld_act(xb, (int64_t)t * C) - mean;
    ss += d * d;
  }
  red[g][lane] = ss;
  __syncthreads();
  if (g == 0) {
    const double var = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (double)(T - 1);
    stats[(int64_t)b * 2 * C + c] = (float)mean;
    stats[(int64_t)b * 2 * C + C + c] = (float)sqrt(var + eps);
  }
}

// y = relu(x) that keeps NaN (torch's F.relu; v_max_f32 would return 0 for it)
__global__ __launch_bounds__(256) void relu_keep_nan_kernel(const float* __restrict__ x, int64_t n,
                                                            float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float v = x[i];
    y[i] = v < 0.f ? 0.f : v;
  }
}

// The pooled head's Linear layers (seg_1: 5120 -> E on the statistics, seg_2: E -> E), fp32 FMA.  A workgroup owns
// kRows batch rows x 16 outputs; each wave 4 outputs, its lanes striding K in float4 units with one accumulator per
// (row, output), then a butterfly sum.  Every output's sum order is fixed by K alone, so a row's result does not
// depend on the batch it runs in (conv_gemm would pick a different kernel for <= 16 rows), and a NaN stays in its
// row.  The weights are read once per kRows rows (5 MB for seg_1; the statistics rows come from L2).
constexpr int kRows = 8, kOuts = 4;

__global__ __launch_bounds__(256) void seg_linear_kernel(const float* __restrict__ x, int B, int K,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         int N, float* __restrict__ y) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wv) * kOuts;
  const int b0 = blockIdx.y * kRows;
  if (n0 >= N) return;   // whole waves leave; no barrier below
  float acc[kRows][kOuts];
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int o = 0; o < kOuts; ++o) acc[r][o] = 0.f;
  const int K4 = K / 4;
  for (int k4 = lane; k4 < K4; k4 += 64) {
    float4 wf[kOuts];
#pragma unroll
    for (int o = 0; o < kOuts; ++o)   // n clamped: the surplus outputs of the last wave are computed and dropped
      wf[o] = *reinterpret_cast<const float4*>(w + (int64_t)min(n0 + o, N - 1) * K + 4 * k4);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const float4 xf = *reinterpret_cast<const float4*>(x + (int64_t)min(b0 + r, B - 1) * K + 4 * k4);
#pragma unroll
      for (int o = 0; o < kOuts; ++o)
        acc[r][o] = fmaf(xf.w, wf[o].w, fmaf(xf.z, wf[o].z, fmaf(xf.y, wf[o].y, fmaf(xf.x, wf[o].x, acc[r][o]))));
    }
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int o = 0; o < kOuts; ++o) {
      const float s = warp_sum(acc[r][o]);
      if (lane == 0 && b0 + r < B && n0 + o < N) y[(int64_t)(b0 + r) * N + n0 + o] = s + bias[n0 + o];
    }
}

}  // namespace

void seg_linear(const float* x, int B, int K, const float* w, const float* bias, int N, float* y, hipStream_t st) {
  SD_CHECK(x && w && bias && y && B >= 1 && N >= 1 && K >= 4 && K % 4 == 0, kErrInvalid,
           "seg_linear: K must be a multiple of 4");
  SD_CHECK(cdiv(B, kRows) <= 65535, kErrInvalid, "seg_linear: too many rows");
  ProfScope prof("seg_linear", 2.0 * B * N * (double)K, 4.0 * ((double)cdiv(B, kRows) * N * K + (double)B * (K + N)),
                 st);
  hipLaunchKernelGGL(seg_linear_kernel, dim3(cdiv(N, 4 * kOuts), cdiv(B, kRows)), dim3(256), 0, st, x, B, K, w, bias, N,
                     y);
  SD_LAUNCH_CHECK();
}

void tstp_pool(const void* x, bool x_bf16, int B, int T, int C, float* stats, float* tout, hipStream_t st,
               double eps) {
  SD_CHECK(x && C >= 64 && C % 64 == 0 && B >= 1 && B <= 65535 && T >= 1, kErrInvalid,
           "tstp_pool: C must be a multiple of 64, 1 <= B <= 65535, T >= 1");
  if (!stats && !tout) return;
  const double elems = (double)B * T * C;
  ProfScope prof("tstp_pool", 0.0, elems * (x_bf16 ? 2.0 : 4.0) * (stats ? 2.0 : 1.0) + (tout ? elems * 4.0 : 0.0),
                 st);
  const dim3 grid(C / 64, B);
  if (x_bf16)
    hipLaunchKernelGGL(tstp_pool_kernel<true>, grid, dim3(256), 0, st, static_cast<const uint16_t*>(x), T, C, stats,
                       tout, eps);
  else
    hipLaunchKernelGGL(tstp_pool_kernel<false>, grid, dim3(256), 0, st, static_cast<const float*>(x), T, C, stats,
                       tout, eps);
  SD_LAUNCH_CHECK();
}

void relu_keep_nan(const float* x, int64_t n, float* y, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(relu_keep_nan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n, y);
  SD_LAUNCH_CHECK();
}

}  // namespace sd
