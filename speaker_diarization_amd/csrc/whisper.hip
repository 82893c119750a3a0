// Whisper-PMFA speech encoder kernels for gfx950 (launchers: kernels.h, "whisper"; the trunk: whisper.h).
//
// Front end, whisper.log_mel_spectrogram(wav, n_mels) per window without the 30-s padding, all fp32:
//   whisper_frames   the F = n / 160 frames of 400 samples each, reflect-padded by 200 at both ends (torch.stft,
//                    center=True) and multiplied by the periodic Hann window: the A rows of the DFT GEMM
//   (conv_gemm)      the 400-point DFT as an exact-f32 MFMA GEMM against the (402 x 400) [cos | sin] basis
//   whisper_mel      |X|^2 over 201 bins, the (n_mels, 201) mel matrix, log10(max(., 1e-10)); the window's maximum
//                    through an order-independent unsigned atomic max on an order-preserving key in which NaN ranks top
//   whisper_clamp    max(x, window max - 8), (x + 4) / 4; a NaN maximum makes every feature of the window NaN
// PMFA tail: whisper_add (the residual add from one column slice of the wide buffer into the next) and
// whisper_ln_wide (ln_post2 over up to 16384 columns, the row held in registers, two-pass fp32 statistics).
#include <algorithm>
#include <cmath>

#include "common.h"
#include "kernels.h"
#include "launch.h"
#include "prof.h"

namespace sd {
namespace {

constexpr int kNfft = kWhisperNfft, kHop = kWhisperHop, kBins = kWhisperBins, kSpec = 2 * kWhisperBins;

// frames[(b F + f) * 400 + j] = hann[j] * wav[b][reflect(f * 160 + j - 200)]
__global__ __launch_bounds__(256) void whisper_frames_kernel(const float* __restrict__ wav, int n, int F,
                                                             const float* __restrict__ hann, float* __restrict__ frames) {
  const int f = blockIdx.x, b = blockIdx.y;
  const float* w = wav + (int64_t)b * n;
  float* o = frames + ((int64_t)b * F + f) * kNfft;
  for (int j = threadIdx.x; j < kNfft; j += 256) {
    int i = f * kHop + j - kNfft / 2;
    if (i < 0) i = -i;                        // one reflection each side: n >= 400 > 200
    if (i >= n) i = 2 * (n - 1) - i;
    o[j] = hann[j] * w[i];
  }
}

// Order-preserving key of a float for an unsigned max; every NaN maps to the top key.
__device__ __forceinline__ uint32_t max_key(float v) {
  const uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);   // 0xffffffff -> 0x7fffffff, a NaN
}

constexpr int kMelRows = 8;   // frames per workgroup, all of one window

// spec (B F, 402) = [re 0..200 | im 0..200]; melT (201, n_mels); raw (B F, n_mels) = log10(max(mel . |X|^2, 1e-10));
// wmax[b] = max key over the window.  A non-finite power (a NaN or Inf sample in the frame) gives NaN.
__global__ __launch_bounds__(256) void whisper_mel_kernel(const float* __restrict__ spec, int F, int n_mels,
                                                          const float* __restrict__ melT, float* __restrict__ raw,
                                                          uint32_t* __restrict__ wmax) {
  __shared__ float pw[kMelRows][kBins + 3];
  __shared__ uint32_t smax;
  const int b = blockIdx.y, f0 = blockIdx.x * kMelRows, tid = threadIdx.x;
  const int nr = min(kMelRows, F - f0);
  if (tid == 0) smax = 0u;
  for (int i = tid; i < nr * kBins; i += 256) {
    const int r = i / kBins, k = i % kBins;
    const float* s = spec + ((int64_t)b * F + f0 + r) * kSpec;
    const float re = s[k], im = s[kBins + k];
    pw[r][k] = re * re + im * im;
  }
  __syncthreads();
  uint32_t mk = 0u;
  for (int i = tid; i < nr * n_mels; i += 256) {
    const int r = i / n_mels, m = i % n_mels;
    float acc = 0.f;
    bool bad = false;
    for (int k = 0; k < kBins; ++k) {
      const float p = pw[r][k];
      bad |= !(fabsf(p) <= 3.4028234664e38f);
      acc = fmaf(melT[k * n_mels + m], p, acc);
    }
    const float v = bad ? __uint_as_float(0x7fc00000u) : log10f(fmaxf(acc, 1e-10f));
    raw[((int64_t)b * F + f0 + r) * n_mels + m] = v;
    mk = max(mk, max_key(v));
  }
  atomicMax(&smax, mk);
  __syncthreads();
  if (tid == 0) atomicMax(wmax + b, smax);
}

// out (B F, ldo): columns < n_mels = (max(raw, window max - 8) + 4) / 4, columns n_mels .. ldo - 1 zero
template <bool BF>
__global__ __launch_bounds__(256) void whisper_clamp_kernel(const float* __restrict__ raw, int F, int n_mels,
                                                            const uint32_t* __restrict__ wmax, act_t<BF>* __restrict__ out,
                                                            int ldo, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t row = i / ldo;
  const int c = (int)(i % ldo);
  float v = 0.f;
  if (c < n_mels) {
    const float mx = key_value(wmax[row / F]);
    const float x = raw[row * n_mels + c];
    v = (mx != mx) ? mx : (fmaxf(x, mx - 8.f) + 4.f) * 0.25f;   // torch.maximum keeps the NaN that fmaxf would drop
  }
  st_act(out, i, v);
}

// out[r, 0..D) = x[r, 0..D) + t[r, 0..D), rows of strides ldx / D / ldo; out may alias x.
__global__ __launch_bounds__(256) void whisper_add_kernel(const float* x, int ldx, const float* __restrict__ t, float* out,
                                                          int ldo, int D4, int64_t total4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int64_t r = i / D4;
  const int c = (int)(i % D4) * 4;
  const float4 a = *reinterpret_cast<const float4*>(x + r * ldx + c);
  const float4 b = *reinterpret_cast<const float4*>(t + r * (int64_t)D4 * 4 + c);
  *reinterpret_cast<float4*>(out + r * ldo + c) = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = warp_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// One workgroup per row of W <= 1024 NV floats, the row in registers (NV float4 per thread).
template <bool BF, int NV>
__global__ __launch_bounds__(256) void whisper_ln_wide_kernel(const float* __restrict__ x, int64_t ldx, int W,
                                                              const float* __restrict__ g, const float* __restrict__ b,
                                                              float eps, act_t<BF>* __restrict__ y, int64_t ldy) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const float* xr = x + row * ldx;
  float4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = (j * 256 + threadIdx.x) * 4;
    v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < W) v[j] = *reinterpret_cast<const float4*>(xr + c);
    s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  }
  const float mean = block_sum(s, red) / W;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = (j * 256 + threadIdx.x) * 4;
    if (c < W) {
      const float dx = v[j].x - mean, dy = v[j].y - mean, dz = v[j].z - mean, dw = v[j].w - mean;
      q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  const float rstd = rsqrtf(block_sum(q, red) / W + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = (j * 256 + threadIdx.x) * 4;
    if (c < W) {
      const float4 gg = *reinterpret_cast<const float4*>(g + c), bb = *reinterpret_cast<const float4*>(b + c);
      const float o0 = fmaf((v[j].x - mean) * rstd, gg.x, bb.x), o1 = fmaf((v[j].y - mean) * rstd, gg.y, bb.y);
      const float o2 = fmaf((v[j].z - mean) * rstd, gg.z, bb.z), o3 = fmaf((v[j].w - mean) * rstd, gg.w, bb.w);
      if constexpr (BF)
        *reinterpret_cast<uint2*>(y + row * ldy + c) = make_uint2(pack_bf16x2(o0, o1), pack_bf16x2(o2, o3));
      else
        *reinterpret_cast<float4*>(y + row * ldy + c) = make_float4(o0, o1, o2, o3);
    }
  }
}

template <bool BF>
void launch_ln_wide(const float* x, int64_t ldx, int64_t rows, int W, const float* g, const float* b, float eps,
                    act_t<BF>* y, int64_t ldy, hipStream_t st) {
  const dim3 grid((unsigned)rows);
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, x, ldx, W, g, b, eps, y, ldy); };
  if (W <= 2048) go(whisper_ln_wide_kernel<BF, 2>);
  else if (W <= 4096) go(whisper_ln_wide_kernel<BF, 4>);
  else if (W <= 8192) go(whisper_ln_wide_kernel<BF, 8>);
  else go(whisper_ln_wide_kernel<BF, 16>);
}

}  // namespace

void whisper_dft_basis(std::vector<float>& basis, std::vector<float>& hann) {
  const double two_pi = 6.283185307179586476925286766559;
  basis.assign((size_t)kSpec * kNfft, 0.f);
  hann.resize(kNfft);
  for (int j = 0; j < kNfft; ++j) hann[j] = (float)(0.5 - 0.5 * std::cos(two_pi * j / kNfft));
  for (int k = 0; k < kBins; ++k)
    for (int j = 0; j < kNfft; ++j) {
      const double a = two_pi * (double)(((int64_t)k * j) % kNfft) / kNfft;   // the angle reduced exactly
      basis[(size_t)k * kNfft + j] = (float)std::cos(a);
      basis[(size_t)(kBins + k) * kNfft + j] = (float)-std::sin(a);
    }
}

void whisper_logmel(const WhisperLogmelArgs& a, hipStream_t st) {
  SD_CHECK(a.wav && a.hann && a.basis && a.melT && a.frames && a.spec && a.raw && a.wmax && a.out, kErrInvalid,
           "whisper_logmel: null argument");
  SD_CHECK(a.B >= 1 && a.B <= 65535 && a.n >= kNfft, kErrInvalid, "whisper_logmel: n_samples must be at least 400");
  SD_CHECK(a.n_mels == 80 || a.n_mels == 128, kErrInvalid, "whisper_logmel: n_mels must be 80 or 128");
  SD_CHECK(a.ldo >= a.n_mels, kErrInvalid, "whisper_logmel: ldo below n_mels");
  const int F = a.n / kHop;
  const int64_t rows = (int64_t)a.B * F;
  SD_CHECK(rows * kSpec < (1ll << 31), kErrInvalid, "whisper_logmel: B * frames * 402 must be below 2^31");
  fill_u32(a.wmax, (size_t)a.B * 4, 0u, st);   // inside the stream, so a captured forward re-initialises it
  {
    ProfScope prof("whisper_frames", 1.0 * rows * kNfft, 8.0 * rows * kNfft, st);
    hipLaunchKernelGGL(whisper_frames_kernel, dim3(F, a.B), dim3(256), 0, st, a.wav, a.n, F, a.hann, a.frames);
    SD_LAUNCH_CHECK();
  }
  {
    // always the exact-f32 MFMA, whatever the model's precision
    ConvGemmArgs p = linear_args(a.frames, (int)rows, kNfft, kNfft, a.basis, kSpec, a.spec, kSpec);
    conv_gemm(p, false, st);
  }
  {
    ProfScope prof("whisper_mel", 2.0 * rows * a.n_mels * kBins, 4.0 * rows * (kSpec + a.n_mels), st);
    hipLaunchKernelGGL(whisper_mel_kernel, dim3(cdiv(F, kMelRows), a.B), dim3(256), 0, st, a.spec, F, a.n_mels, a.melT,
                       a.raw, a.wmax);
    SD_LAUNCH_CHECK();
  }
  {
    const int64_t total = rows * a.ldo;
    const dim3 grid((unsigned)((total + 255) / 256));
    ProfScope prof("whisper_clamp", 3.0 * total, 4.0 * rows * a.n_mels + (a.out_bf16 ? 2.0 : 4.0) * total, st);
    if (a.out_bf16)
      hipLaunchKernelGGL(whisper_clamp_kernel<true>, grid, dim3(256), 0, st, a.raw, F, a.n_mels, a.wmax,
                         static_cast<uint16_t*>(a.out), a.ldo, total);
    else
      hipLaunchKernelGGL(whisper_clamp_kernel<false>, grid, dim3(256), 0, st, a.raw, F, a.n_mels, a.wmax,
                         static_cast<float*>(a.out), a.ldo, total);
    SD_LAUNCH_CHECK();
  }
}

void whisper_add(const float* x, int ldx, const float* t, float* out, int ldo, int64_t rows, int D, hipStream_t st) {
  SD_CHECK(x && t && out && rows >= 1 && D >= 4 && D % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && ldx >= D && ldo >= D,
           kErrInvalid, "whisper_add: D and the row strides must be multiples of 4");
  SD_CHECK(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
           kErrInvalid, "whisper_add: pointers must be 16-byte aligned");
  const int64_t total4 = rows * (D / 4);
  SD_CHECK(total4 < (1ll << 39), kErrInvalid, "whisper_add: too many elements");
  ProfScope prof("whisper_add", 1.0 * rows * D, 12.0 * rows * D, st);
  hipLaunchKernelGGL(whisper_add_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, x, ldx, t, out, ldo,
                     D / 4, total4);
  SD_LAUNCH_CHECK();
}

void whisper_ln_wide(const float* x, int64_t ldx, int64_t rows, int W, const float* g, const float* b, float eps,
                     void* y, int64_t ldy, bool y_bf16, hipStream_t st) {
  SD_CHECK(x && g && b && y && rows >= 1 && rows < (1ll << 31), kErrInvalid, "whisper_ln_wide: bad argument");
  SD_CHECK(W >= 4 && W % 4 == 0 && W <= kWhisperMaxWide, kErrInvalid,
           "whisper_ln_wide: the width must be a multiple of 4, at most 16384");
  SD_CHECK(ldx >= W && ldy >= W && ldx % 4 == 0 && ldy % 4 == 0, kErrInvalid,
           "whisper_ln_wide: row strides must be multiples of 4, at least the width");
  SD_CHECK(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(b) |
             reinterpret_cast<uintptr_t>(y)) & 15) == 0, kErrInvalid, "whisper_ln_wide: pointers must be 16-byte aligned");
  ProfScope prof("whisper_ln_wide", 8.0 * rows * W, (y_bf16 ? 6.0 : 8.0) * rows * W, st);
  if (y_bf16)
    launch_ln_wide<true>(x, ldx, rows, W, g, b, eps, static_cast<uint16_t*>(y), ldy, st);
  else
    launch_ln_wide<false>(x, ldx, rows, W, g, b, eps, static_cast<float*>(y), ldy, st);
  SD_LAUNCH_CHECK();
}

}  // namespace sd
