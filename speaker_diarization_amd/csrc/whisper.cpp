// Whisper-PMFA speech encoder on gfx950 (see whisper.h).
#include "whisper.h"

#include <algorithm>

namespace sd {

void whisper_stem(const WhisperStemW& w, const void* feat, int B, int F, bool bf, void* c1, float* X, hipStream_t st) {
  const int D = w.D, T = (F - 1) / 2 + 1;
  // x = gelu(conv1(x)); x = gelu(conv2(x)) (:216-217): channel-last, each a multi-tap conv_gemm with the GELU epilogue
  ConvGemmArgs p;
  p.A = feat; p.a_bf16 = bf; p.B = B; p.H = 1; p.W = F; p.Cin = w.mel_ld; p.lda = w.mel_ld;
  p.kh = 1; p.kw = 3; p.sh = 1; p.sw = 1; p.pw = 1; p.Ho = 1; p.Wo = F;
  p.Wt = w.conv1; p.N = D; p.K = 3 * w.mel_ld; p.beta = w.b1; p.act = kActGelu;
  p.out = c1; p.out_bf16 = bf; p.o_sb = (int64_t)F * D; p.o_sw = D; p.o_sn = 1;
  conv_gemm(p, bf, st);
  ConvGemmArgs q;
  q.A = c1; q.a_bf16 = bf; q.B = B; q.H = 1; q.W = F; q.Cin = D; q.lda = D;
  q.kh = 1; q.kw = 3; q.sh = 1; q.sw = 2; q.pw = 1; q.Ho = 1; q.Wo = T;
  q.Wt = w.conv2; q.N = D; q.K = 3 * D; q.beta = w.b2; q.act = kActGelu;
  q.out = X; q.out_bf16 = false; q.o_sb = (int64_t)T * D; q.o_sw = D; q.o_sn = 1;
  conv_gemm(q, bf, st);
  // the positions follow the GELU (:231), so they cannot ride in conv2's epilogue, which adds before the activation
  add_pe(X, B * T, T, D, D, w.pe, st);
}

void WhisperTrunk::load(ParamStore& ps_, DeviceArena& arena_, const std::string& pre) {
  const int D = cfg_.state, M = cfg_.n_mels, W = wide();
  const bool bf = cfg_.bf16;
  LayerLoader ld{ps_, arena_, bf};
  auto vec = [&](const std::string& key, int64_t n) {
    SD_CHECK(ps_.get(key).numel() == n, kErrParam, key + " must hold " + std::to_string(n) + " values");
    return ld.up(key);
  };
  auto linear = [&](const std::string& p, int n, int k, PackedW& w, const float*& b) {
    const HostTensor& wt = ps_.get(p + ".weight");
    SD_CHECK(wt.shape.size() == 2 && wt.shape[0] == n && wt.shape[1] == k && ps_.get(p + ".bias").numel() == n, kErrParam,
             p + ".weight must be (" + std::to_string(n) + "," + std::to_string(k) + ") with a bias");
    const ConvL l = ld.linear(p);
    w = l.w;
    b = l.beta;
  };
  mel_ld_ = (M + 31) / 32 * 32;
  {
    // the front end's constants: the DFT basis and the Hann window (whisper.hip), the caller's mel matrix transposed
    std::vector<float> basis, hann;
    whisper_dft_basis(basis, hann);
    basis_ = arena_.upload(basis);
    hann_ = arena_.upload(hann);
    const HostTensor& mf = ps_.get(pre + "mel_filters");
    SD_CHECK(mf.shape.size() == 2 && mf.shape[0] == M && mf.shape[1] == kWhisperBins, kErrParam,
             pre + "mel_filters must be (n_mels,201)");
    std::vector<float> t((size_t)kWhisperBins * M);
    for (int m = 0; m < M; ++m)
      for (int k = 0; k < kWhisperBins; ++k) t[(size_t)k * M + m] = mf.data[(size_t)m * kWhisperBins + k];
    melT_ = arena_.upload(t);
  }
  {
    // conv1 (D, n_mels, 3) -> Wt[D][tap * mel_ld + c], zero weights on the pad channels of the log-mel rows
    const HostTensor& w = ps_.get(pre + "conv1.weight");
    SD_CHECK(w.shape.size() == 3 && w.shape[0] == D && w.shape[1] == M && w.shape[2] == 3, kErrParam,
             pre + "conv1.weight must be (n_audio_state,n_mels,3)");
    std::vector<float> p((size_t)D * 3 * mel_ld_, 0.f);
    for (int n = 0; n < D; ++n)
      for (int c = 0; c < M; ++c)
        for (int t = 0; t < 3; ++t) p[((size_t)n * 3 + t) * mel_ld_ + c] = w.data[((size_t)n * M + c) * 3 + t];
    conv1_ = upload_packed(arena_, p, D, mel_ld_, 1, 3, bf);
    c1_b_ = vec(pre + "conv1.bias", D);
    conv2_ = ld.packed(pre + "conv2.weight");
    SD_CHECK(conv2_.N == D && conv2_.Cin == D && conv2_.kw == 3 && conv2_.kh == 1, kErrParam,
             pre + "conv2.weight must be (n_audio_state,n_audio_state,3)");
    c2_b_ = vec(pre + "conv2.bias", D);
  }
  {
    // the buffer as loaded, not recomputed (whisper_encoder.py:180)
    const HostTensor& pe = ps_.get(pre + "positional_embedding");
    SD_CHECK(pe.shape.size() == 2 && pe.shape[0] == cfg_.n_ctx && pe.shape[1] == D, kErrParam,
             pre + "positional_embedding must be (n_audio_ctx,n_audio_state)");
    pe_ = arena_.upload(pe.data);
  }
  for (int i = 0; i < cfg_.layers; ++i) {
    const std::string p = pre + "layers." + std::to_string(i) + ".", a = p + "attn.";
    Layer L;
    ps_.require_absent(a + "key.bias");   // Linear(n_state, n_state, bias=False) (:66)
    std::vector<float> w, b;
    for (const char* nm : {"query", "key", "value"}) {
      const HostTensor& wi = ps_.get(a + nm + ".weight");
      SD_CHECK(wi.shape.size() == 2 && wi.shape[0] == D && wi.shape[1] == D, kErrParam,
               a + nm + ".weight must be (n_audio_state,n_audio_state)");
      w.insert(w.end(), wi.data.begin(), wi.data.end());
      if (std::string(nm) == "key") {
        b.insert(b.end(), (size_t)D, 0.f);
      } else {
        const HostTensor& bi = ps_.get(a + nm + ".bias");
        SD_CHECK(bi.numel() == D, kErrParam, a + nm + ".bias size");
        b.insert(b.end(), bi.data.begin(), bi.data.end());
      }
    }
    L.in_proj = upload_packed(arena_, w, 3 * D, D, 1, 1, bf);
    L.in_b = arena_.upload(b);
    linear(a + "out", D, D, L.out_proj, L.out_b);
    L.ag = vec(p + "attn_ln.weight", D);
    L.ab = vec(p + "attn_ln.bias", D);
    linear(p + "mlp.0", 4 * D, D, L.fc1, L.b1);
    linear(p + "mlp.2", D, 4 * D, L.fc2, L.b2);
    L.mg = vec(p + "mlp_ln.weight", D);
    L.mb = vec(p + "mlp_ln.bias", D);
    layers_.push_back(L);
  }
  post_g_ = vec(pre + "ln_post2.weight", W);
  post_b_ = vec(pre + "ln_post2.bias", W);
}

void WhisperTrunk::alloc(DeviceArena& arena_, bool with_encode_out) {
  const bool bf = cfg_.bf16;
  const int D = cfg_.state;
  SD_CHECK(cfg_.max_samples >= kMinSamples, kErrInvalid, "max_samples must be at least 400");
  const size_t esz = bf ? 2 : 4;
  const size_t rf = (size_t)cfg_.max_batch * mel_frames(cfg_.max_samples);
  const size_t rows = (size_t)cfg_.max_batch * std::min(frames(cfg_.max_samples), cfg_.n_ctx);
  auto ws = [&](size_t n) { return static_cast<float*>(arena_.alloc(n * sizeof(float))); };
  frames_ = ws(rf * kWhisperNfft);
  spec_ = ws(rf * 2 * kWhisperBins);
  raw_ = ws(rf * cfg_.n_mels);
  wmax_ = static_cast<uint32_t*>(arena_.alloc((size_t)cfg_.max_batch * 4));
  feat_ = arena_.alloc(rf * mel_ld_ * esz);
  c1_ = arena_.alloc(rf * D * esz);
  X_ = ws(rows * D);
  Wide_ = ws(rows * wide());
  T_ = ws(rows * D);
  Y_ = arena_.alloc(rows * D * esz);
  QKV_ = arena_.alloc(rows * 3 * D * esz);
  AO_ = arena_.alloc(rows * D * esz);
  H_ = arena_.alloc(rows * 4 * D * esz);
  if (with_encode_out) Out_ = arena_.alloc(rows * wide() * esz);
}

void WhisperTrunk::check_input(int B, int n_samples) const {
  SD_CHECK(B >= 1 && B <= cfg_.max_batch, kErrInvalid, "batch exceeds max_batch");
  SD_CHECK(n_samples >= kMinSamples, kErrInvalid, "n_samples must be at least 400");
  SD_CHECK(n_samples <= cfg_.max_samples, kErrInvalid, "n_samples exceeds max_samples");
  SD_CHECK(frames(n_samples) <= cfg_.n_ctx, kErrInvalid,
           "the window gives more frames than n_audio_ctx: the reference truncates there (whisper_encoder.py:225-227) and "
           "TS-VAD's label-length assertion then fails");
  SD_CHECK(!gemm_x3(), kErrInvalid, "the Whisper trunk does not build bf16x3: it runs in fp32 or bf16");
}

void WhisperTrunk::stem(const float* wavs, int B, int n_samples, hipStream_t st) {
  const bool bf = cfg_.bf16;
  const int D = cfg_.state, F = mel_frames(n_samples);
  WhisperLogmelArgs m;
  m.wav = wavs; m.B = B; m.n = n_samples; m.n_mels = cfg_.n_mels;
  m.hann = hann_; m.basis = basis_; m.melT = melT_;
  m.frames = frames_; m.spec = spec_; m.raw = raw_; m.wmax = wmax_;
  m.out = feat_; m.ldo = mel_ld_; m.out_bf16 = bf;
  whisper_logmel(m, st);
  WhisperStemW w;
  w.conv1 = conv1_.w; w.conv2 = conv2_.w; w.b1 = c1_b_; w.b2 = c2_b_; w.pe = pe_; w.mel_ld = mel_ld_; w.D = D;
  whisper_stem(w, feat_, B, F, bf, c1_, X_, st);
}

void WhisperTrunk::ln(const float* x, int ldx, int rows, const float* g, const float* b, hipStream_t st) {
  // layernorm() holds rows of up to 1024 values; the published state is 1280
  if (cfg_.state <= 1024)
    layernorm(x, rows, cfg_.state, ldx, g, b, 1e-5f, Y_, cfg_.state, cfg_.bf16, st);
  else
    whisper_ln_wide(x, ldx, rows, cfg_.state, g, b, 1e-5f, Y_, cfg_.state, cfg_.bf16, st);
}

void WhisperTrunk::run_layer(const Layer& L, const float* x, int ldx, float* out, int ldo, int B, int T,
                             hipStream_t st) {
  const bool bf = cfg_.bf16;
  const int D = cfg_.state, rows = B * T;
  const Tens y{Y_, bf}, qkv{QKV_, bf}, ao{AO_, bf}, h{H_, bf}, t{T_, false};
  // x = x + attn(attn_ln(x)) (:142)
  ln(x, ldx, rows, L.ag, L.ab, st);
  conv_gemm(lin(y, rows, D, L.in_proj, L.in_b, qkv, 3 * D), bf, st);
  AttnArgs a;
  a.qkv = QKV_; a.io_bf16 = bf; a.S = B; a.T = T; a.D = D; a.nh = cfg_.heads; a.ld_qkv = 3 * D;
  a.out = AO_; a.ldo = D;
  a.scale = 0.125f;   // (64^-0.25)^2: the reference scales q and k each (:102-104)
  attention(a, bf, st);
  conv_gemm(lin(ao, rows, D, L.out_proj, L.out_b, t, D), bf, st);
  whisper_add(x, ldx, T_, out, ldo, rows, D, st);
  // x = x + mlp(mlp_ln(x)) (:146)
  ln(out, ldo, rows, L.mg, L.mb, st);
  ConvGemmArgs p = lin(y, rows, D, L.fc1, L.b1, h, 4 * D);
  p.act = kActGelu;
  conv_gemm(p, bf, st);
  conv_gemm(lin(h, rows, 4 * D, L.fc2, L.b2, t, D), bf, st);
  whisper_add(out, ldo, T_, out, ldo, rows, D, st);
}

void WhisperTrunk::run(const float* wavs, int B, int n_samples, hipStream_t st) {
  check_input(B, n_samples);
  const int D = cfg_.state, T = frames(n_samples), W = wide();
  stem(wavs, B, n_samples, st);
  const float* cur = X_;
  int ldc = D;
  for (int i = 0; i <= cfg_.layer_ed; ++i) {   // the blocks after layer_ed do not reach the output
    float* dst = i >= cfg_.layer_st ? Wide_ + (size_t)(i - cfg_.layer_st) * D : X_;
    const int ldd = i >= cfg_.layer_st ? W : D;
    run_layer(layers_[i], cur, ldc, dst, ldd, B, T, st);
    cur = dst;
    ldc = ldd;
  }
}

void WhisperTrunk::forward(const float* wavs, int B, int n_samples, float* out, hipStream_t st) {
  run(wavs, B, n_samples, st);
  const int W = wide();
  whisper_ln_wide(Wide_, W, (int64_t)B * frames(n_samples), W, post_g_, post_b_, 1e-5f, out, W, false, st);
}

Tens WhisperTrunk::encode(const float* wavs, int B, int n_samples, hipStream_t st) {
  SD_CHECK(Out_, kErrState, "the Whisper trunk was allocated without encode()'s output map");
  run(wavs, B, n_samples, st);
  const int W = wide();
  whisper_ln_wide(Wide_, W, (int64_t)B * frames(n_samples), W, post_g_, post_b_, 1e-5f, Out_, W, cfg_.bf16, st);
  return Tens{Out_, cfg_.bf16};
}

}  // namespace sd
