// ERes2NetV2 embedding extractor on gfx950 (see eres2net.h).
#include "eres2net.h"

#include <algorithm>

namespace sd {

namespace {

constexpr int kF = 80;
const int kBlocks[4] = {3, 4, 6, 3};

std::vector<int> identity_map(int n) {
  std::vector<int> m(n);
  for (int i = 0; i < n; ++i) m[i] = i;
  return m;
}

// `slices` slices of `width` channels, each padded to wp: padded index -> source channel, -1 for a pad channel
std::vector<int> slice_map(int slices, int width, int wp) {
  std::vector<int> m((size_t)slices * wp, -1);
  for (int i = 0; i < slices; ++i)
    for (int j = 0; j < width; ++j) m[(size_t)i * wp + j] = i * width + j;
  return m;
}

// Conv2d weight `wname` of shape (N0, C0, k, k) + its BatchNorm `bn`, with the output / input channels laid out by
// omap / imap (padded index -> source index or -1): zero weights, alpha = beta = 0 at the pads.
ConvL load_mapped(ParamStore& ps, DeviceArena& arena, bool bf16, const std::string& wname, const std::string& bn,
                  int N0, int C0, int k, const std::vector<int>& omap, const std::vector<int>& imap) {
  const HostTensor& t = ps.get(wname);
  SD_CHECK(t.shape.size() == 4 && t.shape[0] == N0 && t.shape[1] == C0 && t.shape[2] == k && t.shape[3] == k, kErrParam,
           wname + " must be (" + std::to_string(N0) + "," + std::to_string(C0) + "," + std::to_string(k) + "," +
               std::to_string(k) + ")");
  const int N = (int)omap.size(), Cin = (int)imap.size(), taps = k * k;
  std::vector<float> w((size_t)N * taps * Cin, 0.f);
  for (int n = 0; n < N; ++n) {
    if (omap[n] < 0) continue;
    for (int c = 0; c < Cin; ++c) {
      if (imap[c] < 0) continue;
      for (int tp = 0; tp < taps; ++tp)
        w[((size_t)n * taps + tp) * Cin + c] = t.data[((size_t)omap[n] * C0 + imap[c]) * taps + tp];
    }
  }
  ConvL L;
  L.w = upload_packed(arena, w, N, Cin, k, k, bf16);
  std::vector<float> s, h;
  ps.bn_fold(bn, s, h);
  SD_CHECK((int)s.size() == N0, kErrParam, bn + " size");
  std::vector<float> al(N, 0.f), be(N, 0.f);
  for (int n = 0; n < N; ++n)
    if (omap[n] >= 0) { al[n] = s[omap[n]]; be[n] = h[omap[n]]; }
  L.alpha = arena.upload(al);
  L.beta = arena.upload(be);
  return L;
}

// AFF(channels C, r 4).local_att at `p`: Conv2d(2C, C/4, 1) + BN + SiLU + Conv2d(C/4, C, 1) + BN (fusion.py:16-22)
AffL load_aff(ParamStore& ps, DeviceArena& arena, const std::string& p, int C, int Cp) {
  const int I = C / 4;
  const HostTensor& w1 = ps.get(p + "0.weight");
  const HostTensor& w2 = ps.get(p + "3.weight");
  SD_CHECK(w1.numel() == (int64_t)I * 2 * C && w1.shape.size() == 4 && w1.shape[0] == I, kErrParam,
           p + "0.weight must be (" + std::to_string(I) + "," + std::to_string(2 * C) + ",1,1)");
  SD_CHECK(w2.numel() == (int64_t)C * I && w2.shape.size() == 4 && w2.shape[0] == C, kErrParam,
           p + "3.weight must be (" + std::to_string(C) + "," + std::to_string(I) + ",1,1)");
  std::vector<float> a1, c1, a2, c2;
  ps.bn_fold(p + "1", a1, c1, p + "0.bias");
  ps.bn_fold(p + "4", a2, c2, p + "3.bias");
  SD_CHECK((int)a1.size() == I && (int)a2.size() == C, kErrParam, p + "{1,4} size");
  const AffPacked k = aff_pack(w1.data.data(), a1.data(), c1.data(), w2.data.data(), a2.data(), c2.data(), C, I, Cp);
  AffL L;
  L.I = I;
  L.w1 = arena.upload(k.w1); L.a1 = arena.upload(k.a1); L.c1 = arena.upload(k.c1);
  L.w2 = arena.upload(k.w2); L.a2 = arena.upload(k.a2); L.c2 = arena.upload(k.c2);
  return L;
}

void set_out(ConvGemmArgs& p, void* out, int64_t ld) {
  p.out = out;
  p.o_sn = 1; p.o_sw = ld; p.o_sh = (int64_t)p.Wo * ld; p.o_sb = (int64_t)p.Ho * p.Wo * ld;
}

}  // namespace

void ERes2Trunk::load(ParamStore& ps, DeviceArena& arena, bool bf16, int base_width, int scale, int expansion) {
  bf16_ = bf16;
  scale_ = scale;
  expansion_ = expansion;
  {
    const HostTensor& w = ps.get("conv1.weight");
    SD_CHECK(w.numel() == 64 * 9, kErrParam, "conv1.weight must be (64,1,3,3)");
    stem_.pre_s = arena.upload(w.data);
    std::vector<float> s, h;
    ps.bn_fold("bn1", s, h);
    SD_CHECK(s.size() == 64, kErrParam, "bn1 size");
    stem_.alpha = arena.upload(s);
    stem_.beta = arena.upload(h);
  }
  int cin = 64;
  for (int layer = 0; layer < 4; ++layer) {
    const int planes = 64 << layer;
    for (int blk = 0; blk < kBlocks[layer]; ++blk) {
      const std::string p = "layer" + std::to_string(layer + 1) + "." + std::to_string(blk) + ".";
      Res2BlockL rb;
      rb.stride = (blk == 0 && layer > 0) ? 2 : 1;
      rb.width = planes * base_width / 64;       // floor(planes * (baseWidth / 64.0)), :36
      rb.wp = res2_padded(rb.width);
      rb.planes_out = planes * expansion;
      const std::vector<int> slices = slice_map(scale, rb.width, rb.wp), pad = slice_map(1, rb.width, rb.wp);
      rb.c1 = load_mapped(ps, arena, bf16, p + "conv1.weight", p + "bn1", rb.width * scale, cin, 1, slices,
                          identity_map(cin));
      for (int i = 0; i < scale; ++i)
        rb.convs.push_back(load_mapped(ps, arena, bf16, p + "convs." + std::to_string(i) + ".weight",
                                       p + "bns." + std::to_string(i), rb.width, rb.width, 3, pad, pad));
      if (layer >= 2)   // BasicBlockERes2NetV2AFF (:94-160)
        for (int j = 0; j + 1 < scale; ++j)
          rb.aff.push_back(load_aff(ps, arena, p + "fuse_models." + std::to_string(j) + ".local_att.", rb.width, rb.wp));
      rb.c3 = load_mapped(ps, arena, bf16, p + "conv3.weight", p + "bn3", rb.planes_out, rb.width * scale, 1,
                          identity_map(rb.planes_out), slices);
      rb.has_sc = rb.stride != 1 || cin != rb.planes_out;
      if (rb.has_sc) {
        rb.sc = load_conv_bn(ps, arena, bf16, p + "shortcut.0.weight", p + "shortcut.1");
        SD_CHECK(rb.sc.w.N == rb.planes_out && rb.sc.w.Cin == cin && rb.sc.w.kh == 1 && rb.sc.w.kw == 1, kErrParam,
                 p + "shortcut.0.weight shape");
      }
      cin = rb.planes_out;
      blocks_.push_back(rb);
    }
  }
  ds_ = load_conv_bn(ps, arena, bf16, "layer3_ds.weight", "");   // :210, no BN, no bias
  SD_CHECK(ds_.w.N == c4() && ds_.w.Cin == c3() && ds_.w.kh == 3 && ds_.w.kw == 3, kErrParam, "layer3_ds.weight shape");
}

void ERes2Trunk::alloc(DeviceArena& a, int max_batch, int max_frames) {
  const size_t esz = bf16_ ? 2 : 4;
  // the stage-1 maps are the largest: every stride-2 stage halves the bytes
  const size_t px = (size_t)max_batch * kF * max_frames;
  const size_t io = px * 64 * expansion_, uv = px * scale_ * blocks_.front().wp;
  for (float*& b : io_) b = static_cast<float*>(a.alloc(io * esz));
  r_ = static_cast<float*>(a.alloc(io * esz));
  u_ = static_cast<float*>(a.alloc(uv * esz));
  v_ = static_cast<float*>(a.alloc(uv * esz));
  out3_ = static_cast<float*>(a.alloc((size_t)max_batch * 20 * frames25(max_frames) * c3() * esz));
  // fuse34's GEMMs read at least kMinRows rows: the rows past the batch's stay zero
  const size_t cat = std::max<size_t>((size_t)max_batch * 10 * out_frames(max_frames), kMinRows) * 2 * c4() * esz;
  cat_ = static_cast<float*>(a.alloc(cat));
  SD_HIP(hipMemset(cat_, 0, cat));
}

void ERes2Trunk::run_block(const Res2BlockL& rb, const float* cur, int B, int& H, int& W, float* out, int64_t o_ld,
                           hipStream_t st) const {
  const bool bf = bf16_;
  const int S = scale_, wp = rb.wp, SW = S * wp;
  Tens x{const_cast<float*>(cur), bf}, u{u_, bf}, v{v_, bf};
  // conv1 1x1 (stride 2 at a stage's opener) + bn1 + Hardtanh(0, 20), :69-71
  ConvGemmArgs p = conv2d(x, B, H, W, rb.c1, rb.stride, rb.stride, 0, 0, u);
  p.act = kActClamp20;
  conv_gemm(p, bf, st);
  const int Ho = p.Ho, Wo = p.Wo;
  const int64_t P = (int64_t)B * Ho * Wo;
  for (int i = 0; i < S; ++i) {
    const bool fuse = i > 0 && !rb.aff.empty(), add = i > 0 && rb.aff.empty();
    if (fuse) {   // sp = AFF(sp, spx[i]), :144, written over spx[i]
      const AffL& f = rb.aff[i - 1];
      AffGateArgs g;
      g.x = v_; g.ldx = SW; g.x_coff = (i - 1) * wp;
      g.y = u_; g.ldy = SW; g.y_coff = i * wp;
      g.out = u_; g.ldo = SW; g.o_coff = i * wp;
      g.bf16 = bf; g.P = P; g.C = wp; g.I = f.I;
      g.w1 = f.w1; g.a1 = f.a1; g.c1 = f.c1; g.w2 = f.w2; g.a2 = f.a2; g.c2 = f.c2;
      aff_gate(g, st);
    }
    const ConvL& L = rb.convs[i];
    if (bf) {
      Res2ConvArgs c;
      c.x = u_; c.ldx = SW; c.x_coff = i * wp;
      if (add) { c.add = v_; c.ld_add = SW; c.add_coff = (i - 1) * wp; }   // sp = sp + spx[i], :77
      c.B = B; c.H = Ho; c.W = Wo; c.width = wp;
      c.w = L.w.w; c.alpha = L.alpha; c.beta = L.beta;
      c.out = v_; c.ldo = SW; c.o_coff = i * wp;
      res2_conv3x3(c, st);
    } else {
      if (add) slice_add(act_at(u, i * wp).p, SW, act_at(v, (i - 1) * wp).p, SW, false, P, wp, st);
      ConvGemmArgs q = conv2d(u, B, Ho, Wo, L, 1, 1, 1, 1, v);
      q.lda = SW; q.a_coff = i * wp;
      set_out(q, act_at(v, i * wp).p, SW);
      q.act = kActClamp20;
      conv_gemm(q, false, st);
    }
  }
  const void* res = cur;
  if (rb.has_sc) {
    conv_gemm(conv2d(x, B, H, W, rb.sc, rb.stride, rb.stride, 0, 0, Tens{r_, bf}), bf, st);
    res = r_;
  }
  // conv3 1x1 + bn3 + shortcut + Hardtanh(0, 20), :85-90
  ConvGemmArgs q = conv2d(v, B, Ho, Wo, rb.c3, 1, 1, 0, 0, Tens{out, bf});
  set_out(q, out, o_ld);
  q.res = res; q.res_bf16 = bf; q.res_ld = rb.planes_out;
  q.act = kActClamp20;
  conv_gemm(q, bf, st);
  H = Ho;
  W = Wo;
}

void ERes2Trunk::forward(const float* fbank, int B, int Tf, hipStream_t st) const {
  const bool bf = bf16_;
  fcm_conv1(fbank, B, Tf, kF, stem_.pre_s, stem_.alpha, stem_.beta, io_[0], bf, st, 64);   // F.relu, no clamp (:239)
  const float* cur = io_[0];
  int H = kF, W = Tf;
  const size_t n3 = kBlocks[0] + kBlocks[1] + kBlocks[2];
  for (size_t i = 0; i < blocks_.size(); ++i) {
    const Res2BlockL& rb = blocks_[i];
    const bool last3 = i + 1 == n3, last4 = i + 1 == blocks_.size();
    float* out = last3 ? out3_ : last4 ? cat_ : (cur == io_[0] ? io_[1] : io_[0]);
    run_block(rb, cur, B, H, W, out, last4 ? 2 * c4() : rb.planes_out, st);
    cur = out;
  }
  SD_CHECK(H == 10 && W == out_frames(Tf), kErrShape, "ERes2NetV2 output map mismatch");
  // layer3_ds: 3x3 stride 2 of out3 into the second half of cat (:244)
  ConvGemmArgs p = conv2d(out3(), B, 20, frames25(Tf), ds_, 2, 2, 1, 1, cat());
  SD_CHECK(p.Ho == H && p.Wo == W, kErrShape, "layer3_ds output map mismatch");
  set_out(p, act_at(cat(), c4()).p, 2 * c4());
  conv_gemm(p, bf, st);
}

void ERes2NetV2Model::build() {
  SD_CHECK(cfg_.feat_dim == 80 && cfg_.m_channels == 64, kErrInvalid,
           "ERes2NetV2 (MI355X backend) supports feat_dim 80 and m_channels 64 only");
  const bool base = cfg_.base_width == 26 && cfg_.scale == 2 && cfg_.expansion == 2;
  const bool w24 = cfg_.base_width == 24 && cfg_.scale == 4 && cfg_.expansion == 4;
  SD_CHECK(base || w24, kErrInvalid,
           "ERes2NetV2 (MI355X backend) builds (baseWidth, scale, expansion) = (26, 2, 2) or (24, 4, 4) only");
  const bool bf = cfg_.bf16;
  const int E = cfg_.embedding_size;
  trunk_.load(ps_, arena_, bf, cfg_.base_width, cfg_.scale, cfg_.expansion);
  const int C = trunk_.c4();
  const std::string a = "fuse34.local_att.";   // :214, AFF(channels 512 e, r 4)
  f1_ = load_conv_bn(ps_, arena_, bf, a + "0.weight", a + "1", a + "0.bias");
  SD_CHECK(f1_.w.N == C / 4 && f1_.w.Cin == 2 * C && f1_.w.K == 2 * C, kErrParam, a + "0.weight shape");
  f2_ = load_conv_bn(ps_, arena_, bf, a + "3.weight", a + "4", a + "3.bias");
  SD_CHECK(f2_.w.N == C && f2_.w.K == C / 4, kErrParam, a + "3.weight shape");
  LayerLoader fp32{ps_, arena_, false};
  seg1_ = fp32.linear("seg_1");   // :219
  SD_CHECK(seg1_.w.N == E && seg1_.w.K == 2 * 10 * C, kErrParam, "seg_1.weight must be (embedding_size, 20 * 512 e)");
  SD_CHECK(ps_.get("seg_1.bias").numel() == E, kErrParam, "seg_1.bias size");
  ps_.require_all_used();
  trunk_.alloc(arena_, cfg_.max_batch, cfg_.max_frames);
  const size_t Bm = cfg_.max_batch, px = Bm * 10 * ERes2Trunk::out_frames(cfg_.max_frames);
  const size_t rows = std::max<size_t>(px, ERes2Trunk::kMinRows);
  h_ = ws(rows * (C / 4));
  att_ = ws(rows * C);
  fuse_ = ws(px * C);
  stats_ = ws(Bm * 2 * 10 * C);
}

void ERes2NetV2Model::forward(const float* fbank, int B, int Tf, float* emb, float* frame_out, float* frame25_out,
                              hipStream_t st) {
  require_finalized();
  SD_CHECK(B >= 1 && B <= cfg_.max_batch, kErrInvalid, "batch exceeds max_batch");
  SD_CHECK(Tf >= 1 && Tf <= cfg_.max_frames, kErrInvalid, "fbank frames exceed max_frames");
  SD_CHECK(Tf >= kMinFrames, kErrShape, "ERes2NetV2 needs at least 8 fbank frames");
  const bool bf = cfg_.bf16;
  const int C = trunk_.c4(), T3 = ERes2Trunk::frames25(Tf), T4 = ERes2Trunk::out_frames(Tf), C4 = 10 * C;
  trunk_.forward(fbank, B, Tf, st);
  if (frame25_out) nhwc_to_frames(trunk_.out3().p, bf, B, 20, T3, trunk_.c3(), frame25_out, st);
  if (!emb && !frame_out) return;
  // fuse34 = AFF(out4, layer3_ds(out3)) (:245): two GEMMs over the pixels of cat, then the blend
  const Tens cat = trunk_.cat();
  const int M = B * 10 * T4, Mg = std::max(M, ERes2Trunk::kMinRows);
  ConvGemmArgs g1 = lin(cat, Mg, 2 * C, f1_.w, nullptr, Tens{h_, bf}, C / 4);
  g1.alpha = f1_.alpha; g1.beta = f1_.beta; g1.act = kActSilu;
  conv_gemm(g1, bf, st);
  ConvGemmArgs g2 = lin(Tens{h_, bf}, Mg, C / 4, f2_.w, nullptr, Tens{att_, false}, C);
  g2.alpha = f2_.alpha; g2.beta = f2_.beta;
  conv_gemm(g2, bf, st);
  // written as (B, T', C * 10), channel c * 10 + f: TSTP flattens (C, F) that way (pooling_layers_3d_speaker.py:51-56)
  // get_frame_level_feat's order is (B, T', F * C), channel f * C + c
  if (frame_out)
    aff_blend(cat.p, 2 * C, act_at(cat, C).p, 2 * C, bf, att_, B, 10, T4, C, frame_out, (int64_t)T4 * C4, C, C4, 1, st);
  if (!emb) return;
  aff_blend(cat.p, 2 * C, act_at(cat, C).p, 2 * C, bf, att_, B, 10, T4, C, fuse_, (int64_t)T4 * C4, 1, C4, 10, st);
  tstp_pool(fuse_, false, B, T4, C4, stats_, nullptr, st, 1e-8);   // :246
  seg_linear(stats_, B, 2 * C4, static_cast<const float*>(seg1_.w.w), seg1_.beta, cfg_.embedding_size, emb, st);   // :248
}

}  // namespace sd
