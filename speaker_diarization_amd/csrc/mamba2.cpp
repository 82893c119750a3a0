// Host side of the Mamba2BlockV2 stage (mamba2.h): weight folding / upload and the per-layer launch sequence.
#include "mamba2.h"

#include <cmath>

namespace sd {

void Mamba2Stack::validate(int E, int d_state, int expand) {
  SD_CHECK(d_state >= 16 && d_state <= kMamba2MaxState && d_state % 16 == 0, kErrInvalid,
           "d_state must be a multiple of 16 up to 256 (Mamba2 back end)");
  SD_CHECK(expand >= 1 && ((int64_t)expand * E) % kMamba2HeadDim == 0, kErrInvalid,
           "expand * transformer_embed_dim must be a multiple of 64 (Mamba2 headdim)");
  SD_CHECK(E % 8 == 0, kErrInvalid, "transformer_embed_dim must be a multiple of 8 (Mamba2 back end)");
}

namespace {
const HostTensor& shaped(ParamStore& ps, const std::string& key, std::vector<int64_t> shape) {
  const HostTensor& t = ps.get(key);
  if (t.shape != shape) {
    std::string want;
    for (int64_t d : shape) want += (want.empty() ? "" : ", ") + std::to_string(d);
    throw Error{kErrParam, "size mismatch for " + key + ": expected (" + want + ")"};
  }
  return t;
}
}  // namespace

void Mamba2Stack::load(ParamStore& ps, DeviceArena& arena, const std::string& prefix, int E, int n_layer, int d_state,
                       int expand, bool bf16) {
  validate(E, d_state, expand);
  SD_CHECK(n_layer >= 1, kErrInvalid, "Mamba2 back end: n_layer < 1");
  E_ = E;
  N_ = d_state;
  d_inner_ = expand * E;
  heads_ = d_inner_ / kMamba2HeadDim;
  bf16_ = bf16;
  const int CD = d_inner_ + 2 * N_, dip = d_in_proj();
  // in_proj's rows padded with zeros to a multiple of 64: every GEMM path's column tiling and vector stores hold, and
  // each row of zxbcdt starts 16-byte aligned
  ldz_ = (dip + 63) / 64 * 64;
  layers_.clear();
  for (int i = 0; i < n_layer; ++i) {
    Layer L;
    std::vector<float> nw, wdt, cw, cb, dtb, A, D;
    for (int dir = 0; dir < 2; ++dir) {
      const std::string p = prefix + (dir ? "backward_blocks." : "forward_blocks.") + std::to_string(i) + ".";
      const HostTensor& n = shaped(ps, p + "norm.weight", {E});
      nw.insert(nw.end(), n.data.begin(), n.data.end());
      const HostTensor& wi = shaped(ps, p + "mixer.in_proj.weight", {dip, E});
      std::vector<float> wip((size_t)ldz_ * E, 0.f);
      std::copy(wi.data.begin(), wi.data.end(), wip.begin());
      L.in_proj[dir] = upload_packed(arena, wip, ldz_, E, 1, 1, bf16);
      // dt_raw feeds exp(softplus(.) A): its rows stay fp32 for mamba2_norm (the GEMM's dt columns are not read)
      wdt.insert(wdt.end(), wi.data.begin() + (size_t)(dip - heads_) * E, wi.data.end());
      const HostTensor& c = shaped(ps, p + "mixer.conv1d.weight", {CD, 1, 4});
      cw.insert(cw.end(), c.data.begin(), c.data.end());
      const HostTensor& b = shaped(ps, p + "mixer.conv1d.bias", {CD});
      cb.insert(cb.end(), b.data.begin(), b.data.end());
      const HostTensor& db = shaped(ps, p + "mixer.dt_bias", {heads_});
      dtb.insert(dtb.end(), db.data.begin(), db.data.end());
      const HostTensor& al = shaped(ps, p + "mixer.A_log", {heads_});
      for (float v : al.data) A.push_back(-std::exp(v));
      const HostTensor& d = shaped(ps, p + "mixer.D", {heads_});
      D.insert(D.end(), d.data.begin(), d.data.end());
      // RMSNormGated's weight folded into out_proj's input columns; its per-row rstd is applied after the GEMM
      const HostTensor& gw = shaped(ps, p + "mixer.norm.weight", {d_inner_});
      const HostTensor& wo = shaped(ps, p + "mixer.out_proj.weight", {E, d_inner_});
      std::vector<float> wop(wo.data);
      for (int e = 0; e < E; ++e)
        for (int k = 0; k < d_inner_; ++k) wop[(size_t)e * d_inner_ + k] *= gw.data[k];
      L.out_proj[dir] = upload_packed(arena, wop, E, d_inner_, 1, 1, bf16);
    }
    L.norm_w = arena.upload(nw);
    L.w_dt = arena.upload(wdt);
    L.conv_w = arena.upload(cw);
    L.conv_b = arena.upload(cb);
    L.dt_bias = arena.upload(dtb);
    L.A = arena.upload(A);
    L.D = arena.upload(D);
    layers_.push_back(L);
  }
}

void Mamba2Stack::alloc(DeviceArena& arena, int64_t max_rows) {
  max_rows_ = max_rows;
  const size_t el = bf16_ ? 2 : 4, r2 = 2 * (size_t)max_rows;
  xn_ = arena.alloc(r2 * E_ * el);
  zx_ = arena.alloc(r2 * ldz_ * el);
  g_ = arena.alloc(r2 * d_inner_ * el);
  t_ = static_cast<float*>(arena.alloc(r2 * E_ * 4));
  res_ = layers_.size() > 1 ? static_cast<float*>(arena.alloc(r2 * E_ * 4)) : nullptr;
  ssq_ = static_cast<float*>(arena.alloc(r2 * heads_ * 4));
  dt_ = static_cast<float*>(arena.alloc(r2 * heads_ * 4));
}

void Mamba2Stack::forward(const float* x, int B, int G, int I, void* out, bool out_bf16, int NS, int T,
                          hipStream_t st) const {
  const int64_t rows = (int64_t)B * I;
  SD_CHECK(!layers_.empty() && rows >= 1 && rows <= max_rows_, kErrInvalid, "Mamba2 stage: rows exceed the workspace");
  SD_CHECK(rows <= 0x7fffffff / 2, kErrInvalid, "Mamba2 stage: too many rows");
  const bool bf = bf16_;
  const int E = E_;
  auto dir_at = [&](void* p, int dir, int64_t ld) {
    return Tens{static_cast<char*>(p) + (size_t)dir * rows * ld * (bf ? 2 : 4), bf};
  };
  const float* r_in = x;
  int64_t r_in_dir = 0;
  for (size_t i = 0; i < layers_.size(); ++i) {
    const Layer& L = layers_[i];
    Mamba2NormArgs n;
    n.rows = rows; n.E = E; n.r_in = r_in; n.r_in_dir = r_in_dir; n.w = L.norm_w; n.y = xn_; n.y_bf16 = bf;
    n.nh = heads_; n.w_dt = L.w_dt; n.dt_raw = dt_;
    if (i > 0) {   // r_{i+1} = h_i + r_i
      n.t = t_; n.ssq = ssq_; n.d_inner = d_inner_; n.r_out = res_;
      r_in = res_;
      r_in_dir = rows * E;
    }
    mamba2_norm(n, st);
    for (int dir = 0; dir < 2; ++dir)
      conv_gemm(lin(dir_at(xn_, dir, E), (int)rows, E, L.in_proj[dir], nullptr, dir_at(zx_, dir, ldz_), ldz_), bf, st);
    Mamba2ScanArgs s;
    s.zx = zx_; s.ldz = ldz_; s.bf16 = bf; s.rows = rows; s.B = B; s.G = G; s.I = I;
    s.d_inner = d_inner_; s.d_state = N_;
    s.conv_w = L.conv_w; s.conv_b = L.conv_b; s.dt_bias = L.dt_bias; s.A = L.A; s.D = L.D;
    s.g = g_; s.ssq = ssq_; s.dt_raw = dt_;
    mamba2_scan(s, st);
    for (int dir = 0; dir < 2; ++dir)
      conv_gemm(lin(dir_at(g_, dir, d_inner_), (int)rows, d_inner_, L.out_proj[dir], nullptr,
                    Tens{t_ + (size_t)dir * rows * E, false}, E), bf, st);
  }
  Mamba2FinishArgs f;
  f.rows = rows; f.E = E; f.r_in = r_in; f.r_in_dir = r_in_dir; f.t = t_; f.ssq = ssq_; f.nh = heads_;
  f.d_inner = d_inner_; f.NS = NS; f.T = T; f.out = out; f.out_bf16 = out_bf16;
  mamba2_finish(f, st);
}

}  // namespace sd
