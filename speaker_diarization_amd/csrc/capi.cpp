// extern "C" boundary (include/sdiar.h).  Exceptions never cross it: every
// entry point maps sd::Error to a status code + thread-local message.
#include "../../include/sdiar.h"

#include <cmath>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include <algorithm>

#include "encoder.h"
#include "kernels.h"
#include "prof.h"
#include "eda.h"
#include "fseend.h"
#include "fseend_stream.h"
#include "tsvad.h"
#include "campp.h"
#include "resemb.h"
#include "simam_emb.h"
#include "eres2net.h"
#include "ecapa.h"
#include "redimnet.h"
#include "wavlm.h"
#include "w2vbert.h"
#include "whisper.h"
#include "tsvad_stream.h"
#include "ssnd.h"

namespace sd {
static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
const char* last_error() { return g_err.c_str(); }
}  // namespace sd

// Every opaque handle type of sdiar.h is this, over its kind's runner.
template <class M>
struct Handle {
  bool x3 = false;   // precision 2: conv_gemm's exact path in bf16x3 (GemmX3Scope around compute)
  std::unique_ptr<M> model;
};

struct sd_tsvad : Handle<sd::TsvadModel> {};
struct sd_tsvad_stream : Handle<sd::TsvadStreamModel> {};
struct sd_eda : Handle<sd::EdaModel> {};
struct sd_fseend : Handle<sd::FsEendModel> {};
struct sd_fseend_stream : Handle<sd::FsEendStream> {};
struct sd_campp : Handle<sd::CamppModel> {};
struct sd_resnet34 : Handle<sd::ResEmbModel> {};
struct sd_simam_resnet34 : Handle<sd::SimamEmbModel> {};
struct sd_eres2netv2 : Handle<sd::ERes2NetV2Model> {};
struct sd_ecapa : Handle<sd::EcapaModel> {};
struct sd_redimnet : Handle<sd::RedimNetModel> {};
struct sd_wavlm : Handle<sd::WavlmModel> {};
struct sd_w2vbert : Handle<sd::W2vBertModel> {};
struct sd_whisper : Handle<sd::WhisperModel> {};
struct sd_ssnd : Handle<sd::SsndModel> {};

namespace {

template <typename F>
int guard(F&& f) {
  try {
    f();
    return SD_OK;
  } catch (const sd::Error& e) {
    sd::set_error(e.msg);
    return e.code;
  } catch (const std::exception& e) {
    sd::set_error(e.what());
    return SD_ERR_HIP;
  } catch (...) {
    sd::set_error("unknown error");
    return SD_ERR_HIP;
  }
}

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Scratch for test-only ops (packed weights); freed after the stream drains.
struct Scratch {
  void* p = nullptr;
  hipStream_t st;
  Scratch(size_t bytes, hipStream_t s) : st(s) { SD_HIP(hipMalloc(&p, bytes ? bytes : 4)); }
  ~Scratch() {
    (void)hipStreamSynchronize(st);
    (void)hipFree(p);
  }
};

// `w` (N, Cin, taps) packed into scratch as conv_gemm's Wt[N][tap * Cin + c], bf16 bits when bf; a null w (an
// optional weight the caller does not have) leaves the scratch unpacked.
struct PackedScratch : Scratch {
  PackedScratch(const float* w, int N, int Cin, int taps, bool bf, hipStream_t s)
      : Scratch((size_t)N * Cin * taps * (bf ? 2 : 4), s) {
    if (w) sd::pack_weight(w, N, Cin, taps, p, bf, s);
  }
};

// The A operand a test op hands conv_gemm: the caller's fp32 activations, or their bf16 copy at precision 2.
struct Activations : Scratch {
  const void* a;
  bool bf16;
  Activations(const float* x, int64_t n, int precision, hipStream_t s)
      : Scratch(precision == 2 ? (size_t)n * 2 : 4, s), a(x), bf16(precision == 2) {
    if (!bf16) return;
    sd::f32_to_bf16(x, n, p, s);
    a = p;
  }
};

// ---- the handle lifecycle, the same for every kind: create -> set_param* -> finalize -> (forward)* -> destroy
// The tail of every sd_<kind>_create, after its argument checks: *out receives the handle only once its runner is
// constructed, so a throwing constructor leaks nothing.
template <class H, class... Args>
void create(H** out, bool x3, Args&&... args) {
  auto h = std::make_unique<H>();
  h->x3 = x3;
  h->model.reset(new typename decltype(h->model)::element_type(std::forward<Args>(args)...));
  *out = h.release();
}

template <class H>
int set_param(H* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return guard([&] {
    SD_CHECK(h && name && (data || ndim == 0), sd::kErrInvalid, "null argument");
    SD_CHECK(!h->model->finalized(), sd::kErrState, "set_param after finalize");
    h->model->params().set(name, data, shape, ndim);
  });
}

template <class H>
int finalize(H* h) {
  return guard([&] {
    SD_CHECK(h, sd::kErrInvalid, "null handle");
    h->model->finalize();
  });
}

template <class H>
int64_t device_bytes(const H* h) {
  return h ? (int64_t)h->model->device_bytes() : 0;
}

template <class H>
int destroy(H* h) {
  return guard([&] { delete h; });
}

}  // namespace

extern "C" {

const char* sd_last_error(void) { return sd::last_error(); }
int sd_version(void) { return 1; }

void sd_prof_enable(int on) { sd::prof_enable(on != 0); }
void sd_prof_reset(void) { sd::prof_reset(); }
int sd_prof_query(int i, char* name, int name_len, int64_t* launches, double* flops, double* bytes,
                  double* ms) {
  std::string n;
  long long l;
  if (!sd::prof_query(i, n, l, *flops, *bytes, *ms)) return 0;
  *launches = l;
  if (name && name_len > 0) {
    size_t k = std::min<size_t>(n.size(), (size_t)name_len - 1);
    n.copy(name, k);
    name[k] = '\0';
  }
  return 1;
}

double sd_prof_query_steps(int i) { return sd::prof_query_steps(i); }

static int probe_lstm_granule(const char* what, int steps, float* us_per_step, void* stream, int nwg) {
  return guard([&] {
    SD_CHECK(steps >= 1 && us_per_step, sd::kErrInvalid, std::string(what) + ": bad argument");
    *us_per_step = sd::lstm_granule_probe(steps, S(stream), nwg);
  });
}

int sd_probe_lstm_granule(int steps, float* us_per_step, void* stream) {
  return probe_lstm_granule("probe_lstm_granule", steps, us_per_step, stream, 4);
}

int sd_probe_lstm_granule2(int steps, float* us_per_step, void* stream) {
  return probe_lstm_granule("probe_lstm_granule2", steps, us_per_step, stream, 2);
}

int sd_probe_lstm_handoff(int steps, float* us_per_step, void* stream) {
  return guard([&] {
    SD_CHECK(steps >= 1 && us_per_step, sd::kErrInvalid, "probe_lstm_handoff: bad argument");
    *us_per_step = sd::lstm_handoff_probe(steps, S(stream));
  });
}

// sd_whisper_config's geometry rules, shared by sd_whisper_create and sd_tsvad_create_whisper
static void check_whisper_geometry(const sd_whisper_config* c) {
  SD_CHECK(c->n_mels == 80 || c->n_mels == 128, sd::kErrInvalid, "n_mels must be 80 or 128");
  SD_CHECK(c->n_audio_ctx >= 1, sd::kErrInvalid, "n_audio_ctx must be positive");
  SD_CHECK(c->n_audio_head >= 1 && c->n_audio_state == 64 * c->n_audio_head, sd::kErrInvalid,
           "n_audio_state must be 64 * n_audio_head (head size 64 only)");
  SD_CHECK(c->n_audio_state % 32 == 0, sd::kErrInvalid, "n_audio_state must be a multiple of 32");
  SD_CHECK(c->n_audio_layer >= 1 && c->n_audio_layer <= 32, sd::kErrInvalid, "n_audio_layer must be 1..32");
  SD_CHECK(c->layer_st >= 0 && c->layer_st <= c->layer_ed, sd::kErrInvalid, "layer_st must be 0..layer_ed");
  SD_CHECK(c->layer_ed < c->n_audio_layer, sd::kErrInvalid, "layer_ed must be below n_audio_layer");
  SD_CHECK((int64_t)c->n_audio_state * (c->layer_ed - c->layer_st + 1) <= sd::kWhisperMaxWide, sd::kErrInvalid,
           "n_audio_state * (layer_ed - layer_st + 1) must be at most 16384 (ln_post2's row)");
}

// rows times the widest row are counted in int: the DFT's (B F, 402) and the MLP's (B T', 4 D)
static void check_whisper_workspace(const sd_whisper_config* c, int max_batch, int max_samples) {
  SD_CHECK(max_batch > 0 && max_batch <= 65535, sd::kErrInvalid, "max_batch must be 1..65535");
  SD_CHECK(max_samples >= sd::WhisperTrunk::kMinSamples, sd::kErrInvalid, "max_samples must be at least 400");
  const int64_t rf = (int64_t)max_batch * sd::WhisperTrunk::mel_frames(max_samples);
  SD_CHECK(rf * std::max(2 * sd::kWhisperBins, 2 * c->n_audio_state) < (1ll << 31), sd::kErrInvalid,
           "max_batch * frames * row width must be below 2^31");
}

static sd::WhisperConfig whisper_geometry(const sd_whisper_config* c) {
  sd::WhisperConfig t;
  t.n_mels = c->n_mels; t.n_ctx = c->n_audio_ctx; t.state = c->n_audio_state; t.heads = c->n_audio_head;
  t.layers = c->n_audio_layer; t.layer_st = c->layer_st; t.layer_ed = c->layer_ed;
  return t;
}

static int tsvad_create(const sd_tsvad_config* c, const sd_whisper_config* wc, sd_tsvad** out,
                        int frame_level_gsp = 0) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(frame_level_gsp == 0 || frame_level_gsp == 1, sd::kErrInvalid, "frame_level_gsp must be 0 or 1");
    SD_CHECK(c->variant >= 0 && c->variant <= 8, sd::kErrInvalid, "unknown TS-VAD variant");
    SD_CHECK(c->variant != 8 || wc, sd::kErrInvalid,
             "variant 8 (whisper) takes the trunk's own geometry: create it with sd_tsvad_create_whisper");
    SD_CHECK(c->variant == 8 || !wc, sd::kErrInvalid, "sd_tsvad_create_whisper builds variant 8 only");
    const bool wave = c->variant == 5 || c->variant == 6 || c->variant == 8;
    SD_CHECK(c->variant != 8 || c->precision != 2, sd::kErrInvalid,
             "the whisper speech encoder (variant 8) does not build bf16x3: the Whisper trunk runs in fp32 or bf16");
    SD_CHECK(c->variant != 7 || c->precision != 2, sd::kErrInvalid,
             "the w2v-bert2 speech encoder (variant 7) does not build bf16x3: the w2v-BERT trunk runs in fp32 or bf16");
    SD_CHECK(!wave || c->precision != 2, sd::kErrInvalid,
             "the WavLM speech encoders (variants 5 / 6) do not build bf16x3: the WavLM trunk runs in fp32 or bf16");
    SD_CHECK(c->precision >= 0 && c->precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
    SD_CHECK(c->max_batch > 0 && (wave || c->max_fbank_frames > 0), sd::kErrInvalid, "bad workspace sizes");
    SD_CHECK(c->max_num_speaker > 0 && c->num_transformer_layer >= 1 && c->transformer_ffn_embed_dim > 0 &&
                 c->speaker_embed_dim > 0, sd::kErrInvalid, "bad model dimensions");
    SD_CHECK(c->num_attention_head > 0 && c->transformer_embed_dim % c->num_attention_head == 0, sd::kErrInvalid,
             "transformer_embed_dim must be divisible by num_attention_head");
    sd::TsvadConfig t;
    t.variant = c->variant;
    t.max_num_speaker = c->max_num_speaker;
    t.rs_len = c->rs_len;
    t.max_batch = c->max_batch;
    t.max_fbank_frames = c->max_fbank_frames;
    t.bf16 = c->precision == 1;
    t.num_transformer_layer = c->num_transformer_layer;
    t.num_attention_head = c->num_attention_head;
    t.embed_dim = c->transformer_embed_dim;
    t.ffn_dim = c->transformer_ffn_embed_dim;
    t.speaker_embed_dim = c->speaker_embed_dim;
    t.backend = c->backend;
    t.d_state = c->d_state;
    t.expand = c->expand;
    t.wavlm_embed_dim = c->wavlm_embed_dim;
    t.wavlm_layers = c->wavlm_layers;
    t.wavlm_layer_norm_mode = c->wavlm_layer_norm_mode != 0;
    t.wavlm_pre_ln = c->wavlm_pre_ln != 0;
    t.max_samples = c->max_samples;
    t.w2vbert_layers = c->w2vbert_layers;
    t.frame_level_gsp = frame_level_gsp != 0;
    if (wc) {
      check_whisper_geometry(wc);
      check_whisper_workspace(wc, c->max_batch, c->max_samples);
      t.whisper = whisper_geometry(wc);
    }
    // proj_layer configurations (speaker_embed_dim * 2 != transformer_embed_dim); backend / d_state / expand
    sd::TsvadModel::validate(t);
    create(out, c->precision == 2, t);
  });
}

int sd_tsvad_create(const sd_tsvad_config* c, sd_tsvad** out) { return tsvad_create(c, nullptr, out); }

int sd_tsvad_create_ex(const sd_tsvad_config_ex* c, sd_tsvad** out) {
  if (!c) return guard([] { SD_CHECK(false, sd::kErrInvalid, "null argument"); });
  return tsvad_create(&c->base, nullptr, out, c->frame_level_gsp);
}

int sd_tsvad_create_whisper(const sd_tsvad_config* c, const sd_whisper_config* wc, sd_tsvad** out) {
  if (!wc) return guard([] { SD_CHECK(false, sd::kErrInvalid, "null argument"); });
  return tsvad_create(c, wc, out);
}

int sd_tsvad_set_param(sd_tsvad* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_tsvad_finalize(sd_tsvad* h) { return finalize(h); }

int sd_tsvad_forward(sd_tsvad* h, const float* ref, const float* ts, int B, int Tf, int Tl,
                     float* logits, void* stream) {
  return guard([&] {
    const sd::GemmX3Scope x3(h && h->x3);
    SD_CHECK(h && ref && ts && logits, sd::kErrInvalid, "null argument");
    h->model->forward(ref, ts, B, Tf, Tl, logits, S(stream));
  });
}

int sd_tsvad_forward_graph(sd_tsvad* h, const float* ref, const float* ts, int B, int Tf, int Tl, float* logits,
                           int replays, const char* dot_path, void* stream) {
  return guard([&] {
    const sd::GemmX3Scope x3(h && h->x3);
    SD_CHECK(h && ref && ts && logits, sd::kErrInvalid, "null argument");
    h->model->forward_graph(ref, ts, B, Tf, Tl, logits, replays, dot_path, S(stream));
  });
}

int sd_tsvad_debug_buffer(const sd_tsvad* h, int which, void** ptr, int64_t* bytes) {
  return guard([&] {
    SD_CHECK(h && ptr && bytes, sd::kErrInvalid, "null argument");
    h->model->debug_buffer(which, ptr, bytes);
  });
}

int sd_tsvad_status(sd_tsvad* h, void* stream) {
  return guard([&] {
    SD_CHECK(h, sd::kErrInvalid, "null argument");
    h->model->status(S(stream));
  });
}

int sd_tsvad_forward_batched(sd_tsvad* h, const float* ref, const float* ts, int B, int Tf, int Tl,
                             int forward_batch, int force, float* logits, void* stream) {
  return guard([&] {
    const sd::GemmX3Scope x3(h && h->x3);
    SD_CHECK(h && ref && ts && logits, sd::kErrInvalid, "null argument");
    h->model->forward(ref, ts, B, Tf, Tl, logits, S(stream), forward_batch, force);
  });
}

int64_t sd_tsvad_device_bytes(const sd_tsvad* h) { return device_bytes(h); }

int sd_tsvad_destroy(sd_tsvad* h) { return destroy(h); }

int sd_eda_create(const sd_eda_config* c, sd_eda** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->variant >= 0 && c->variant <= 3, sd::kErrInvalid, "Unknown model type.");
    SD_CHECK(c->variant != 3 || c->n_speakers > 0, sd::kErrInvalid, "n_speakers must be positive");
    SD_CHECK(c->precision >= 0 && c->precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
    SD_CHECK(c->max_seqs > 0 && c->max_frames > 0 && c->max_n_speakers >= 2, sd::kErrInvalid,
             "bad workspace sizes");
    SD_CHECK(c->n_units > 0 && c->n_heads > 0 && c->n_units % c->n_heads == 0, sd::kErrInvalid,
             "n_units must be divisible by n_heads");
    sd::EdaConfig t;
    t.variant = c->variant;
    t.in_size = c->in_size;
    t.n_units = c->n_units;
    t.n_heads = c->n_heads;
    t.n_layers = c->n_layers;
    t.dim_feedforward = c->dim_feedforward;
    t.max_seqs = c->max_seqs;
    t.max_frames = c->max_frames;
    t.max_n_speakers = c->max_n_speakers;
    t.n_speakers = c->n_speakers;
    t.bf16 = c->precision == 1;
    create(out, c->precision == 2, t);
  });
}

int sd_eda_set_param(sd_eda* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_eda_finalize(sd_eda* h) { return finalize(h); }

int sd_eda_input_stride(const sd_eda* h) { return h && h->model->finalized() ? h->model->in_ld() : 0; }

int sd_eda_forward(sd_eda* h, const float* feats, int ld_feats, int S_, int T, const int* lengths,
                   const int* key_len, const int* perm, float* probs, float* act, void* stream) {
  return guard([&] {
    const sd::GemmX3Scope x3(h && h->x3);
    SD_CHECK(h && feats && act, sd::kErrInvalid, "null argument");
    h->model->forward(feats, ld_feats, S_, T, lengths, key_len, perm, probs, act, S(stream));
  });
}

int sd_eda_status(sd_eda* h, void* stream) {
  return guard([&] {
    SD_CHECK(h, sd::kErrInvalid, "null argument");
    h->model->status(S(stream));
  });
}

int64_t sd_eda_device_bytes(const sd_eda* h) { return device_bytes(h); }

int sd_eda_destroy(sd_eda* h) { return destroy(h); }

int sd_fseend_create(const sd_fseend_config* c, sd_fseend** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision >= 0 && c->precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
    SD_CHECK(c->max_seqs > 0 && c->max_frames > 0 && c->max_nspks > 0, sd::kErrInvalid, "bad workspace sizes");
    SD_CHECK(c->n_units > 0 && c->n_heads > 0 && c->n_units % c->n_heads == 0, sd::kErrInvalid,
             "n_units must be divisible by n_heads");
    SD_CHECK(c->dec_n_layers >= 1 && c->enc_n_layers >= 0 && c->mask_delay >= 0, sd::kErrInvalid,
             "bad layer counts");
    sd::FsEendConfig t;
    t.in_size = c->in_size;
    t.n_units = c->n_units;
    t.n_heads = c->n_heads;
    t.enc_n_layers = c->enc_n_layers;
    t.enc_ffn = c->enc_dim_feedforward;
    t.dec_n_layers = c->dec_n_layers;
    t.dec_ffn = c->dec_dim_feedforward;
    t.conv_delay = c->conv_delay;
    t.mask_delay = c->mask_delay;
    t.has_mask = c->has_mask;
    t.max_seqs = c->max_seqs;
    t.max_frames = c->max_frames;
    t.max_nspks = c->max_nspks;
    t.bf16 = c->precision == 1;
    create(out, c->precision == 2, t);
  });
}

int sd_fseend_set_param(sd_fseend* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_fseend_finalize(sd_fseend* h) { return finalize(h); }

int sd_fseend_input_stride(const sd_fseend* h) { return h && h->model->finalized() ? h->model->in_ld() : 0; }

int sd_fseend_test(sd_fseend* h, const float* feats, int ld_feats, int S_, int T, const int* ilens_host,
                   int max_nspks, float* preds, float* emb, float* attractors, void* stream) {
  return guard([&] {
    const sd::GemmX3Scope x3(h && h->x3);
    SD_CHECK(h && feats && preds, sd::kErrInvalid, "null argument");
    h->model->forward(feats, ld_feats, S_, T, ilens_host, max_nspks, preds, emb, attractors, S(stream));
  });
}

int64_t sd_fseend_device_bytes(const sd_fseend* h) { return device_bytes(h); }

int sd_fseend_destroy(sd_fseend* h) { return destroy(h); }

int sd_fseend_stream_create(sd_fseend* h, int chunk, int max_frames, int max_nspks, int use_graph,
                            sd_fseend_stream** out) {
  return guard([&] {
    SD_CHECK(h && out, sd::kErrInvalid, "null argument");
    create(out, false, *h->model, chunk, max_frames, max_nspks, use_graph != 0);
  });
}

int sd_fseend_stream_push(sd_fseend_stream* s, const float* feats, int ld_feats, int n, float* preds, int cap,
                          int* n_out, void* stream) {
  return guard([&] {
    SD_CHECK(s && n_out, sd::kErrInvalid, "null argument");
    *n_out = s->model->push(feats, ld_feats, n, preds, cap, S(stream));
  });
}

int sd_fseend_stream_set_audio(sd_fseend_stream* s, const float* mel_fb, int n_mels, int frame_size, int frame_shift,
                               int context_size, int subsampling) {
  return guard([&] {
    SD_CHECK(s, sd::kErrInvalid, "null handle");
    s->model->set_audio(mel_fb, n_mels, frame_size, frame_shift, context_size, subsampling);
  });
}

int sd_fseend_stream_push_audio(sd_fseend_stream* s, const float* samples, int64_t n, float* preds, int cap,
                                int* n_out, void* stream) {
  return guard([&] {
    SD_CHECK(s && n_out, sd::kErrInvalid, "null argument");
    *n_out = s->model->push_audio(samples, n, preds, cap, S(stream));
  });
}

int sd_fseend_stream_flush(sd_fseend_stream* s, float* preds, int cap, int* n_out, void* stream) {
  return guard([&] {
    SD_CHECK(s && n_out, sd::kErrInvalid, "null argument");
    *n_out = s->model->flush(preds, cap, S(stream));
  });
}

int sd_fseend_stream_reset(sd_fseend_stream* s, void* stream) {
  return guard([&] {
    SD_CHECK(s, sd::kErrInvalid, "null handle");
    s->model->reset(S(stream));
  });
}

int sd_fseend_stream_stats(const sd_fseend_stream* s, int64_t* enc_runs, int64_t* dec_runs, int* enc_nodes,
                           int* dec_nodes) {
  return guard([&] {
    SD_CHECK(s && enc_runs && dec_runs && enc_nodes && dec_nodes, sd::kErrInvalid, "null argument");
    *enc_runs = s->model->runs(0);
    *dec_runs = s->model->runs(1);
    *enc_nodes = s->model->graph_nodes(0);
    *dec_nodes = s->model->graph_nodes(1);
  });
}

int sd_fseend_stream_debug_counters(const sd_fseend_stream* s, unsigned* host_out, int cap, int* n, void* stream) {
  return guard([&] {
    SD_CHECK(s && n && (host_out || cap == 0), sd::kErrInvalid, "null argument");
    *n = s->model->debug_counters(host_out, cap, S(stream));
  });
}

int64_t sd_fseend_stream_device_bytes(const sd_fseend_stream* h) { return device_bytes(h); }

int sd_fseend_stream_destroy(sd_fseend_stream* h) { return destroy(h); }

// Test-only single ops of the streaming kernels (stream_ops.hip): raw device pointers, the caller's own
// workspaces, counters and cursors, data already in the io dtype.
int sd_attn_decode_blocks(int max_keys) { return max_keys < 1 ? 0 : sd::attn_decode_blocks(max_keys); }

int sd_op_attn_decode(const void* q, int64_t q_tok, int64_t q_seq, const void* k, const void* v, int64_t kv_tok,
                      int64_t kv_seq, void* out, int64_t o_tok, int64_t o_seq, int nseq, int nq, int nh, float scale,
                      const int* pos, int delay, int max_keys, int io_bf16, float* ws, int n_blocks, unsigned* cnt,
                      const void* wo, const float* bo, void* o2, float* ws2, unsigned* cnt2, int* ran_out_proj,
                      void* stream) {
  return guard([&] {
    SD_CHECK(q && k && v && out && pos && ws && ran_out_proj, sd::kErrInvalid, "attn_decode: null argument");
    SD_CHECK(nseq >= 1 && nh >= 1 && max_keys >= 1 && delay >= 0, sd::kErrInvalid, "attn_decode: bad argument");
    SD_CHECK(io_bf16 == 0 || io_bf16 == 1, sd::kErrInvalid, "attn_decode: io_bf16 must be 0 or 1");
    // K rows are read as 16-byte vectors
    const int64_t v16 = io_bf16 ? 8 : 4;
    SD_CHECK(((uintptr_t)k | (uintptr_t)v) % 16 == 0 && kv_tok % v16 == 0 && kv_seq % v16 == 0, sd::kErrInvalid,
             "attn_decode: k / v must be 16-byte aligned, their strides 16-byte multiples");
    SD_CHECK(!(wo || bo || o2 || ws2 || cnt2) || (cnt && wo && bo && o2 && ws2 && cnt2), sd::kErrInvalid,
             "attn_decode: the out-projection needs cnt, wo, bo, o2, ws2 and cnt2 together");
    sd::DecodeAttnArgs a;
    a.q = q; a.q_tok = q_tok; a.q_seq = q_seq;
    a.k = k; a.v = v; a.kv_tok = kv_tok; a.kv_seq = kv_seq;
    a.out = out; a.o_tok = o_tok; a.o_seq = o_seq;
    a.nseq = nseq; a.nq = nq; a.nh = nh; a.hd = 64; a.scale = scale;
    a.pos = pos; a.delay = delay; a.max_keys = max_keys; a.n_blocks = n_blocks; a.ws = ws; a.io_bf16 = io_bf16 != 0;
    a.cnt = cnt; a.wo = wo; a.bo = bo; a.o2 = o2; a.ws2 = ws2; a.cnt2 = cnt2;
    *ran_out_proj = 0;
    *ran_out_proj = sd::attn_decode(a, S(stream)) ? 1 : 0;
  });
}

int sd_op_stream_slot_block(const float* ln_x, const void* ln_t, int t_bf16, const float* ln_g, const float* ln_b,
                            float eps, float* ln_out, const void* w_in, const float* b_in, const void* w_out,
                            const float* b_out, int w_bf16, void* out, int out_bf16, float* ws, unsigned* cnt, int c,
                            int C, int D, int nh, float scale, int* ran, void* stream) {
  return guard([&] {
    SD_CHECK(ln_x && ln_g && ln_b && ln_out && w_in && b_in && w_out && b_out && out && ran, sd::kErrInvalid,
             "stream_slot_block: null argument");
    sd::SlotBlockArgs a;
    a.ln_x = ln_x; a.ln_t = ln_t; a.t_bf16 = t_bf16 != 0; a.ln_g = ln_g; a.ln_b = ln_b; a.eps = eps; a.ln_out = ln_out;
    a.w_in = w_in; a.b_in = b_in; a.w_out = w_out; a.b_out = b_out; a.w_bf16 = w_bf16 != 0;
    a.out = out; a.out_bf16 = out_bf16 != 0; a.ws = ws; a.cnt = cnt;
    a.c = c; a.C = C; a.D = D; a.nh = nh; a.scale = scale;
    *ran = 0;
    *ran = sd::stream_slot_block(a, S(stream)) ? 1 : 0;
  });
}

int sd_op_stream_ffn_pair(const float* ln_x, const void* ln_t, int t_bf16, const float* ln_g, const float* ln_b,
                          float eps, float* ln_out, const void* w1, const float* b1, const void* w2, const float* b2,
                          int w_bf16, void* out, int out_bf16, float* ws, unsigned* cnt, int n, int D, int F, int* ran,
                          void* stream) {
  return guard([&] {
    SD_CHECK(ln_x && w1 && b1 && w2 && b2 && out && ran, sd::kErrInvalid, "stream_ffn_pair: null argument");
    sd::FfnPairArgs a;
    a.ln_x = ln_x; a.ln_t = ln_t; a.t_bf16 = t_bf16 != 0; a.ln_g = ln_g; a.ln_b = ln_b; a.eps = eps; a.ln_out = ln_out;
    a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.w_bf16 = w_bf16 != 0;
    a.out = out; a.out_bf16 = out_bf16 != 0; a.ws = ws; a.cnt = cnt; a.n = n; a.D = D; a.F = F;
    *ran = 0;
    *ran = sd::stream_ffn_pair(a, S(stream)) ? 1 : 0;
  });
}

int sd_op_kv_append(const void* src, int64_t ld_src_bytes, int rows, int width_bytes, void* dst, int64_t ld_dst_bytes,
                    const int* cursor, int mult, void* stream) {
  return guard([&] {
    SD_CHECK(src && dst && cursor, sd::kErrInvalid, "kv_append: null argument");
    SD_CHECK(rows >= 0 && width_bytes >= 16 && mult >= 1 && ld_src_bytes >= width_bytes && ld_dst_bytes >= width_bytes,
             sd::kErrInvalid, "kv_append: bad argument");
    sd::kv_append(src, ld_src_bytes, rows, width_bytes, dst, ld_dst_bytes, cursor, mult, S(stream));
  });
}

int sd_op_gather_window(const float* hist, int D, const int* cursor, const int* n_valid, int pad, int rows, float* dst,
                        void* stream) {
  return guard([&] {
    SD_CHECK(hist && cursor && n_valid && dst, sd::kErrInvalid, "gather_window: null argument");
    SD_CHECK(D >= 1 && rows >= 1 && pad >= 0, sd::kErrInvalid, "gather_window: bad argument");
    sd::gather_window(hist, D, cursor, n_valid, pad, rows, dst, S(stream));
  });
}

int sd_op_cursor_advance(int* cursor, int by, int* mirror, void* stream) {
  return guard([&] {
    SD_CHECK(cursor, sd::kErrInvalid, "cursor_advance: null argument");
    sd::cursor_advance(cursor, by, mirror, S(stream));
  });
}

int sd_op_stream_enc_finish(const float* x, const void* t, int t_bf16, const float* g, const float* b, float eps, int c,
                            int D, float* hist, int* cursor, int* mirror, void* stream) {
  return guard([&] {
    SD_CHECK(x && g && b && hist && cursor, sd::kErrInvalid, "stream_enc_finish: null argument");
    SD_CHECK(c >= 1 && D >= 256, sd::kErrInvalid, "stream_enc_finish: D must be 256/512/768/1024, c >= 1");
    sd::stream_enc_finish(x, t, t_bf16 != 0, g, b, eps, c, D, hist, cursor, mirror, S(stream));
  });
}

int sd_op_stream_dec_finish(const float* x, const void* t, int t_bf16, const float* g, const float* b, float eps, int c,
                            int C, int D, const float* emb, float* scores, int* cursor, void* stream) {
  return guard([&] {
    SD_CHECK(x && g && b && emb && scores && cursor, sd::kErrInvalid, "stream_dec_finish: null argument");
    SD_CHECK(c >= 1 && C >= 1 && D >= 256, sd::kErrInvalid, "stream_dec_finish: D must be 256/512/768/1024, c and C >= 1");
    sd::stream_dec_finish(x, t, t_bf16 != 0, g, b, eps, c, C, D, emb, scores, cursor, S(stream));
  });
}

int sd_eend_features(const float* wav, int64_t n_samples, int frame_size, int frame_shift, int n_frames,
                     const float* mel_fb, int n_mels, int mean_norm, int context_size, int subsampling,
                     double* work, float* out, int ld_out, void* stream) {
  return guard([&] {
    SD_CHECK(wav && mel_fb && work && out, sd::kErrInvalid, "null argument");
    SD_CHECK(frame_size > 0 && frame_shift > 0 && subsampling > 0 && context_size >= 0, sd::kErrInvalid,
             "bad frame geometry");
    const int n_fft = 1 << (32 - __builtin_clz((unsigned)(frame_size - 1)));
    const int64_t nf_max = 1 + n_samples / frame_shift;
    SD_CHECK(n_frames >= 1 && n_frames <= nf_max, sd::kErrInvalid, "n_frames exceeds the STFT frames");
    hipStream_t st = S(stream);
    double* lm = work;
    double* mean = work + (int64_t)n_frames * n_mels;
    sd::stft_logmel(wav, n_samples, n_frames, n_fft, frame_shift, frame_size, mel_fb, n_mels, lm, st);
    if (mean_norm) sd::col_mean(lm, n_frames, n_mels, mean, st);
    const int n_out = (n_frames + subsampling - 1) / subsampling;
    sd::splice_subsample(lm, n_frames, n_mels, mean_norm ? mean : nullptr, context_size, subsampling, n_out,
                         out, ld_out, st);
  });
}

int sd_fbank_kaldi_ex(const float* wav, int64_t n_samples, float in_scale, int n_frames, const float* mel_fb,
                      int n_mels, int window_type, float* out, void* stream) {
  return guard([&] {
    SD_CHECK(n_frames >= 0 && (n_frames == 0 || n_samples >= 400 + (int64_t)(n_frames - 1) * 160),
             sd::kErrInvalid, "fbank: n_frames exceeds the samples");
    sd::fbank_kaldi(wav, n_samples, in_scale, n_frames, mel_fb, n_mels, out, S(stream), window_type);
  });
}

int sd_fbank_kaldi(const float* wav, int64_t n_samples, float in_scale, int n_frames,
                   const float* mel_fb, int n_mels, float* out, void* stream) {
  return sd_fbank_kaldi_ex(wav, n_samples, in_scale, n_frames, mel_fb, n_mels, /*hamming*/ 0, out, stream);
}

int sd_tsvad_stream_create(const sd_tsvad_stream_config* c, sd_tsvad_stream** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision == 0 || c->precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    SD_CHECK(c->max_labels > 0 && c->max_num_speaker > 0 && c->max_windows > 0, sd::kErrInvalid,
             "bad workspace sizes");
    SD_CHECK(c->num_attention_head > 0 && c->transformer_embed_dim % c->num_attention_head == 0, sd::kErrInvalid,
             "transformer_embed_dim must be divisible by num_attention_head");
    SD_CHECK(c->num_transformer_layer >= 1, sd::kErrInvalid, "num_transformer_layer must be >= 1");
    SD_CHECK(c->transformer_ffn_embed_dim > 0 && c->speaker_embed_dim > 0, sd::kErrInvalid,
             "transformer_ffn_embed_dim and speaker_embed_dim must be > 0");
    sd::TsvadStreamConfig t;
    t.max_num_speaker = c->max_num_speaker;
    t.max_labels = c->max_labels;
    t.max_windows = c->max_windows;
    t.bf16 = c->precision == 1;
    t.num_transformer_layer = c->num_transformer_layer;
    t.num_attention_head = c->num_attention_head;
    t.embed_dim = c->transformer_embed_dim;
    t.ffn_dim = c->transformer_ffn_embed_dim;
    t.speaker_embed_dim = c->speaker_embed_dim;
    create(out, false, t);
  });
}

int sd_tsvad_stream_set_param(sd_tsvad_stream* h, const char* name, const float* data, const int64_t* shape,
                              int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_tsvad_stream_finalize(sd_tsvad_stream* h) { return finalize(h); }

int sd_tsvad_stream_forward(sd_tsvad_stream* h, const float* feats, const float* ts, int B, int T_label, int chunk,
                            int left_chunks, float* logits, void* stream) {
  return guard([&] {
    SD_CHECK(h && feats && ts && logits, sd::kErrInvalid, "null argument");
    SD_CHECK(chunk > 0, sd::kErrShape, "decoding_chunk_size must be > 0");
    h->model->forward(feats, ts, B, T_label, chunk, left_chunks, logits, S(stream));
  });
}

int64_t sd_tsvad_stream_device_bytes(const sd_tsvad_stream* h) { return device_bytes(h); }

int sd_tsvad_stream_destroy(sd_tsvad_stream* h) { return destroy(h); }

int sd_campp_create(const sd_campp_config* c, sd_campp** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision == 0 || c->precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    SD_CHECK(c->feat_dim == 80, sd::kErrInvalid, "CAM++ FCM head supports feat_dim 80 only");
    SD_CHECK(c->embedding_size > 0, sd::kErrInvalid, "embedding_size must be positive");
    SD_CHECK(c->max_batch > 0 && c->max_frames >= 8, sd::kErrInvalid, "bad workspace sizes");
    sd::CamppConfig t;
    t.feat_dim = c->feat_dim;
    t.embedding_size = c->embedding_size;
    t.max_batch = c->max_batch;
    t.max_frames = c->max_frames;
    t.bf16 = c->precision == 1;
    create(out, false, t);
  });
}

int sd_campp_set_param(sd_campp* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_campp_finalize(sd_campp* h) { return finalize(h); }

int sd_campp_forward(sd_campp* h, const float* feats, int B, int T, float* emb, float* time_out, void* stream) {
  return guard([&] {
    SD_CHECK(h && feats && (emb || time_out), sd::kErrInvalid, "null argument");
    h->model->forward(feats, B, T, emb, time_out, S(stream));
  });
}

int64_t sd_campp_device_bytes(const sd_campp* h) { return device_bytes(h); }

int sd_campp_destroy(sd_campp* h) { return destroy(h); }

int sd_resnet34_create(const sd_resnet34_config* c, sd_resnet34** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision == 0 || c->precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    SD_CHECK(c->feat_dim == 80, sd::kErrInvalid, "ResNet34 (MI355X backend) supports feat_dim 80 only");
    SD_CHECK(c->embed_dim >= 8 && c->embed_dim % 8 == 0, sd::kErrInvalid, "embed_dim must be a positive multiple of 8");
    SD_CHECK(c->max_batch > 0 && c->max_frames >= 8, sd::kErrInvalid, "bad workspace sizes");
    sd::ResEmbConfig t;
    t.feat_dim = c->feat_dim;
    t.embed_dim = c->embed_dim;
    t.two_emb_layer = c->two_emb_layer != 0;
    t.max_batch = c->max_batch;
    t.max_frames = c->max_frames;
    t.bf16 = c->precision == 1;
    create(out, false, t);
  });
}

int sd_resnet34_set_param(sd_resnet34* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_resnet34_finalize(sd_resnet34* h) { return finalize(h); }

int sd_resnet34_forward(sd_resnet34* h, const float* feats, int B, int T, float* emb, float* emb_a, float* time_out,
                        void* stream) {
  return guard([&] {
    SD_CHECK(h && feats && (emb || emb_a || time_out), sd::kErrInvalid, "null argument");
    h->model->forward(feats, B, T, emb, emb_a, time_out, S(stream));
  });
}

int64_t sd_resnet34_device_bytes(const sd_resnet34* h) { return device_bytes(h); }

int sd_resnet34_destroy(sd_resnet34* h) { return destroy(h); }

int sd_simam_resnet34_create(const sd_simam_resnet34_config* c, sd_simam_resnet34** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision == 0 || c->precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    SD_CHECK(c->in_planes == 64 && c->acoustic_dim == 80, sd::kErrInvalid,
             "SimAM_ResNet34_ASP (MI355X backend) supports in_planes 64 and acoustic_dim 80 only");
    SD_CHECK(c->embed_dim >= 8 && c->embed_dim % 8 == 0, sd::kErrInvalid, "embed_dim must be a positive multiple of 8");
    SD_CHECK(c->max_batch > 0 && c->max_frames >= 8, sd::kErrInvalid, "bad workspace sizes");
    sd::SimamEmbConfig t;
    t.in_planes = c->in_planes;
    t.embed_dim = c->embed_dim;
    t.acoustic_dim = c->acoustic_dim;
    t.max_batch = c->max_batch;
    t.max_frames = c->max_frames;
    t.bf16 = c->precision == 1;
    create(out, false, t);
  });
}

int sd_simam_resnet34_set_param(sd_simam_resnet34* h, const char* name, const float* data, const int64_t* shape,
                                int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_simam_resnet34_finalize(sd_simam_resnet34* h) { return finalize(h); }

int sd_simam_resnet34_forward(sd_simam_resnet34* h, const float* feats, int B, int T, float* emb, float* front_out,
                              void* stream) {
  return guard([&] {
    SD_CHECK(h && feats && (emb || front_out), sd::kErrInvalid, "null argument");
    h->model->forward(feats, B, T, emb, front_out, S(stream));
  });
}

int sd_debug_simam_variant(int variant) {
  return guard([&] {
    SD_CHECK(variant == 0 || variant == 1, sd::kErrInvalid, "simam variant must be 0 or 1");
    sd::simam_debug_variant(variant);
  });
}

int64_t sd_simam_resnet34_device_bytes(const sd_simam_resnet34* h) { return device_bytes(h); }

int sd_simam_resnet34_destroy(sd_simam_resnet34* h) { return destroy(h); }

int sd_eres2netv2_create(const sd_eres2netv2_config* c, sd_eres2netv2** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision == 0 || c->precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    SD_CHECK(c->feat_dim == 80 && c->m_channels == 64, sd::kErrInvalid,
             "ERes2NetV2 (MI355X backend) supports feat_dim 80 and m_channels 64 only");
    SD_CHECK((c->base_width == 26 && c->scale == 2 && c->expansion == 2) ||
                 (c->base_width == 24 && c->scale == 4 && c->expansion == 4),
             sd::kErrInvalid,
             "ERes2NetV2 (MI355X backend) builds (baseWidth, scale, expansion) = (26, 2, 2) or (24, 4, 4) only");
    SD_CHECK(c->embedding_size >= 8 && c->embedding_size % 8 == 0, sd::kErrInvalid,
             "embedding_size must be a positive multiple of 8");
    SD_CHECK(c->max_batch > 0 && c->max_frames >= 8, sd::kErrInvalid, "bad workspace sizes");
    sd::ERes2NetV2Config t;
    t.feat_dim = c->feat_dim;
    t.embedding_size = c->embedding_size;
    t.m_channels = c->m_channels;
    t.base_width = c->base_width;
    t.scale = c->scale;
    t.expansion = c->expansion;
    t.max_batch = c->max_batch;
    t.max_frames = c->max_frames;
    t.bf16 = c->precision == 1;
    create(out, false, t);
  });
}

int sd_eres2netv2_set_param(sd_eres2netv2* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_eres2netv2_finalize(sd_eres2netv2* h) { return finalize(h); }

int sd_eres2netv2_forward(sd_eres2netv2* h, const float* feats, int B, int T, float* emb, float* frame_out,
                          float* frame25_out, void* stream) {
  return guard([&] {
    SD_CHECK(h && feats && (emb || frame_out || frame25_out), sd::kErrInvalid, "null argument");
    h->model->forward(feats, B, T, emb, frame_out, frame25_out, S(stream));
  });
}

int sd_debug_clamp_route(int route) {
  return guard([&] {
    SD_CHECK(route == 0 || route == 1, sd::kErrInvalid, "clamp route must be 0 or 1");
    sd::clamp_route_debug(route);
  });
}

int64_t sd_eres2netv2_device_bytes(const sd_eres2netv2* h) { return device_bytes(h); }

int sd_eres2netv2_destroy(sd_eres2netv2* h) { return destroy(h); }

int sd_ecapa_create(const sd_ecapa_config* c, sd_ecapa** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision == 0 || c->precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    SD_CHECK(c->channels == 1024, sd::kErrInvalid, "ECAPA-TDNN (MI355X backend) builds channels 1024 only");
    SD_CHECK(c->embed_dim >= 4 && c->embed_dim % 4 == 0, sd::kErrInvalid, "embed_dim must be a positive multiple of 4");
    SD_CHECK(c->max_batch > 0 && c->max_frames >= 2, sd::kErrInvalid, "bad workspace sizes");
    sd::EcapaConfig t;
    t.embed_dim = c->embed_dim;
    t.max_batch = c->max_batch;
    t.max_frames = c->max_frames;
    t.bf16 = c->precision == 1;
    create(out, false, t);
  });
}

int sd_ecapa_set_param(sd_ecapa* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_ecapa_finalize(sd_ecapa* h) { return finalize(h); }

int sd_ecapa_forward(sd_ecapa* h, const float* feats, int B, int T, float* emb, float* time_out, void* stream) {
  return guard([&] {
    SD_CHECK(h && feats && (emb || time_out), sd::kErrInvalid, "null argument");
    h->model->forward(feats, B, T, emb, time_out, S(stream));
  });
}

int sd_ecapa_debug_stats(const sd_ecapa* h, void** ptr) {
  return guard([&] {
    SD_CHECK(h && ptr, sd::kErrInvalid, "null argument");
    SD_CHECK(h->model->finalized(), sd::kErrState, "model not finalized");
    *ptr = const_cast<float*>(h->model->stats());
  });
}

int64_t sd_ecapa_device_bytes(const sd_ecapa* h) { return device_bytes(h); }

int sd_ecapa_destroy(sd_ecapa* h) { return destroy(h); }

int sd_redimnet_create(const sd_redimnet_config* c, sd_redimnet** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision >= 0 && c->precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
    SD_CHECK(c->feat_dim == 72, sd::kErrInvalid, "ReDimNetB2 (MI355X backend) supports feat_dim 72 only");
    SD_CHECK(c->embed_dim >= 4 && c->embed_dim % 4 == 0, sd::kErrInvalid, "embed_dim must be a positive multiple of 4");
    SD_CHECK(c->max_batch > 0 && c->max_frames >= 2, sd::kErrInvalid, "bad workspace sizes");
    // the trunk counts pixel rows (B T 72) and map values per launch in int
    SD_CHECK((int64_t)c->max_batch * c->max_frames * sd::kRedimCF < (1ll << 31), sd::kErrInvalid,
             "max_batch * max_frames * 1152 must be below 2^31");
    sd::RedimNetConfig t;
    t.feat_dim = c->feat_dim;
    t.embed_dim = c->embed_dim;
    t.max_batch = c->max_batch;
    t.max_frames = c->max_frames;
    t.bf16 = c->precision == 1;
    create(out, c->precision == 2, t);
  });
}

int sd_redimnet_set_param(sd_redimnet* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_redimnet_finalize(sd_redimnet* h) { return finalize(h); }

int sd_redimnet_forward(sd_redimnet* h, const float* feats, int B, int T, float* emb, float* frames, void* stream) {
  return guard([&] {
    const sd::GemmX3Scope x3(h && h->x3);
    SD_CHECK(h && feats && (emb || frames), sd::kErrInvalid, "null argument");
    h->model->forward(feats, B, T, emb, frames, S(stream));
  });
}

int sd_redimnet_debug_generic(sd_redimnet* h, int on) {
  return guard([&] {
    SD_CHECK(h, sd::kErrInvalid, "null handle");
    SD_CHECK(on == 0 || on == 1, sd::kErrInvalid, "on must be 0 or 1");
    h->model->set_generic(on != 0);
  });
}

int64_t sd_redimnet_device_bytes(const sd_redimnet* h) { return device_bytes(h); }

int sd_redimnet_destroy(sd_redimnet* h) { return destroy(h); }

int sd_wavlm_create(const sd_wavlm_config* c, sd_wavlm** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision == 0 || c->precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    SD_CHECK((c->embed_dim == 768 && c->ffn_dim == 3072 && c->heads == 12) ||
                 (c->embed_dim == 1024 && c->ffn_dim == 4096 && c->heads == 16),
             sd::kErrInvalid,
             "WavLM (MI355X backend) builds (embed_dim, ffn_dim, heads) = (768, 3072, 12) or (1024, 4096, 16) only");
    SD_CHECK(c->encoder_layers >= 1 && c->encoder_layers <= 24, sd::kErrInvalid, "encoder_layers must be 1..24");
    SD_CHECK((c->extractor_mode == 0 && c->layer_norm_first == 0) || (c->extractor_mode == 1 && c->layer_norm_first == 1),
             sd::kErrInvalid,
             "WavLM (MI355X backend) builds (extractor_mode, layer_norm_first) = (0 default, 0) or (1 layer_norm, 1) only");
    SD_CHECK(c->max_batch > 0, sd::kErrInvalid, "max_batch must be positive");
    SD_CHECK(c->max_samples >= sd::WavlmModel::kMinSamples, sd::kErrInvalid, "max_samples must be at least 400");
    // rows (B T) and map values per launch are counted in int
    SD_CHECK((int64_t)c->max_batch * sd::WavlmModel::frames(c->max_samples) * c->ffn_dim < (1ll << 31) &&
                 (int64_t)std::min(c->max_batch, sd::WavlmModel::kSlice) * (c->max_samples / 5) * 512 < (1ll << 31),
             sd::kErrInvalid, "max_batch * frames(max_samples) * ffn_dim must be below 2^31");
    sd::WavlmConfig t;
    t.embed_dim = c->embed_dim; t.ffn_dim = c->ffn_dim; t.heads = c->heads; t.layers = c->encoder_layers;
    t.layer_norm_mode = c->extractor_mode == 1;
    t.pre_ln = c->layer_norm_first == 1;
    t.max_batch = c->max_batch; t.max_samples = c->max_samples;
    t.bf16 = c->precision == 1;
    create(out, false, t);
  });
}

int sd_wavlm_set_param(sd_wavlm* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_wavlm_finalize(sd_wavlm* h) { return finalize(h); }

int sd_wavlm_forward(sd_wavlm* h, const float* source, int B, int n_samples, int output_layer, float* x_out,
                     float* features_out, float* layers_out, void* stream) {
  return guard([&] {
    SD_CHECK(h && source && (x_out || features_out || layers_out), sd::kErrInvalid, "null argument");
    h->model->forward(source, B, n_samples, output_layer, x_out, features_out, layers_out, S(stream));
  });
}

int64_t sd_wavlm_device_bytes(const sd_wavlm* h) { return device_bytes(h); }

int sd_wavlm_destroy(sd_wavlm* h) { return destroy(h); }

int sd_wavlm_frames(int n_samples) { return sd::WavlmModel::frames(n_samples); }

int sd_probe_wavlm_buckets(int n, int32_t* out) {
  return guard([&] {
    SD_CHECK(out, sd::kErrInvalid, "null argument");
    SD_CHECK(n >= 1, sd::kErrInvalid, "probe_wavlm_buckets: n must be at least 1");
    for (int r = -(n - 1); r <= n - 1; ++r) out[r + n - 1] = sd::wavlm_bucket(r);
  });
}

int sd_probe_wavlm_pos_weight(const float* g, const float* v, int D, float* out) {
  return guard([&] {
    SD_CHECK(g && v && out, sd::kErrInvalid, "null argument");
    SD_CHECK(D == 768 || D == 1024, sd::kErrInvalid, "probe_wavlm_pos_weight: D must be 768 or 1024");
    sd::wavlm_fold_pos_weight(g, v, D, out);
  });
}

int sd_op_wavlm_layer0(const float* wav, int B, int n, const float* w, const float* g, const float* b, int layer_norm,
                       void* out, int out_bf16, void* stream) {
  return guard([&] {
    SD_CHECK(wav && w && g && b && out, sd::kErrInvalid, "wavlm_layer0: null argument");
    SD_CHECK(B >= 1 && n >= 10, sd::kErrInvalid, "wavlm_layer0: B >= 1 and n >= 10");
    hipStream_t st = S(stream);
    const int T0 = (n - 10) / 5 + 1;
    Scratch partial((size_t)B * sd::wavlm_l0_parts(T0) * 3 * 512 * 4, st), ss((size_t)B * 2 * 512 * 4, st);
    sd::wavlm_layer0(wav, B, n, w, g, b, layer_norm != 0, static_cast<float*>(partial.p), static_cast<float*>(ss.p),
                     out, out_bf16 != 0, st);
  });
}

int sd_op_wavlm_conv(const float* x, int B, int T, const float* w, int k, const float* ln_g, const float* ln_b,
                     void* out, int precision, void* stream) {
  return guard([&] {
    SD_CHECK(x && w && out && (ln_g == nullptr) == (ln_b == nullptr), sd::kErrInvalid, "wavlm_conv: bad argument");
    SD_CHECK(B >= 1 && (k == 2 || k == 3) && T >= k, sd::kErrInvalid, "wavlm_conv: k must be 2 or 3 and T >= k");
    SD_CHECK(precision >= 0 && precision <= 2, sd::kErrInvalid, "wavlm_conv: precision must be 0, 1 or 2");
    hipStream_t st = S(stream);
    const bool bf = precision >= 1, obf = precision == 2;
    PackedScratch wt(w, 512, 512, k, bf, st);
    Activations xa(x, (int64_t)B * T * 512, bf ? 2 : 0, st);
    sd::ConvGemmArgs p;
    p.A = xa.a; p.a_bf16 = bf; p.B = B; p.H = 1; p.W = T; p.Cin = 512; p.lda = 512;
    p.kh = 1; p.kw = k; p.sw = 2; p.Ho = 1; p.Wo = (T - k) / 2 + 1;
    p.Wt = wt.p; p.N = 512; p.K = 512 * k;
    p.act = ln_g ? sd::kActNone : sd::kActGelu;
    p.out = out; p.out_bf16 = obf; p.o_sb = (int64_t)p.Wo * 512; p.o_sw = 512; p.o_sn = 1;
    sd::conv_gemm(p, bf, st);
    if (ln_g) sd::wavlm_ln_gelu(out, obf, (int64_t)B * p.Wo, ln_g, ln_b, st);
  });
}

int sd_op_wavlm_pos_conv(const float* x, int B, int T, int D, const float* w, const float* bias, float* out,
                         int precision, void* stream) {
  return guard([&] {
    SD_CHECK(x && w && bias && out, sd::kErrInvalid, "wavlm_pos_conv: null argument");
    SD_CHECK(D == 768 || D == 1024, sd::kErrInvalid, "wavlm_pos_conv: D must be 768 or 1024");
    SD_CHECK(precision == 0 || precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    hipStream_t st = S(stream);
    const bool bf = precision == 1;
    PackedScratch wt(w, D, D / 16, 128, bf, st);   // (D, D / 16, 128) -> [D][tap * D / 16 + c]
    sd::wavlm_pos_conv(x, B, T, D, wt.p, bf, bias, out, st);
  });
}

int sd_op_wavlm_attention(const float* qkv, const float* xin, int B, int T, int H, const float* grep_w,
                          const float* grep_b, const float* grep_a, const float* table, float* out, int precision,
                          void* stream) {
  return guard([&] {
    SD_CHECK(qkv && xin && grep_w && grep_b && grep_a && table && out, sd::kErrInvalid, "wavlm_attention: null argument");
    SD_CHECK(B >= 1 && T >= 1 && H >= 1, sd::kErrInvalid, "wavlm_attention: empty problem");
    SD_CHECK(precision == 0 || precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    hipStream_t st = S(stream);
    const bool bf = precision == 1;
    Activations qa(qkv, (int64_t)B * T * 3 * H * 64, bf ? 2 : 0, st);
    sd::WavlmAttnArgs a;
    a.qkv = qa.a; a.bf16 = bf; a.xin = xin; a.B = B; a.T = T; a.D = H * 64; a.H = H;
    a.grep_w = grep_w; a.grep_b = grep_b; a.grep_a = grep_a; a.table = table;
    a.out = out; a.out_bf16 = false;
    sd::wavlm_attention(a, st);
  });
}

int sd_op_wavlm_bias_table(const float* emb, int T, int H, float* table, void* stream) {
  return guard([&] {
    SD_CHECK(emb && table && T >= 1 && H >= 1, sd::kErrInvalid, "wavlm_bias_table: bad argument");
    hipStream_t st = S(stream);
    std::vector<int> bm(2 * T - 1);
    for (int r = -(T - 1); r <= T - 1; ++r) bm[r + T - 1] = sd::wavlm_bucket(r);
    Scratch d(bm.size() * sizeof(int), st);
    SD_HIP(hipMemcpy(d.p, bm.data(), bm.size() * sizeof(int), hipMemcpyHostToDevice));
    sd::wavlm_bias_table(emb, static_cast<const int*>(d.p), T - 1, T, H, table, st);
  });
}

int sd_op_wavlm_layer_mix(const float* x, int L, int64_t n, const float* w_host, float* acc, void* stream) {
  return guard([&] {
    SD_CHECK(x && w_host && acc && L >= 1 && n >= 4, sd::kErrInvalid, "wavlm_layer_mix: bad argument");
    for (int l = 0; l < L; ++l) sd::wavlm_layer_mix(acc, x + (int64_t)l * n, w_host[l], l == 0, n, S(stream));
  });
}

int sd_op_wavlm_mix_proj_ln(const float* acc, int rows, int D, const float* w, const float* bias, const float* g,
                            const float* beta, int SE, float* out, int precision, void* stream) {
  return guard([&] {
    SD_CHECK(acc && w && bias && g && beta && out && rows >= 1, sd::kErrInvalid, "wavlm_mix_proj_ln: bad argument");
    SD_CHECK(SE == 192 || SE == 256, sd::kErrInvalid, "wavlm_mix_proj_ln: SE must be 192 or 256");
    SD_CHECK(D >= 32 && D % 32 == 0, sd::kErrInvalid, "wavlm_mix_proj_ln: D must be a multiple of 32");
    SD_CHECK(precision == 0 || precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    hipStream_t st = S(stream);
    const bool bf = precision == 1;
    PackedScratch wt(w, SE, D, 1, bf, st);
    if (!bf) {
      sd::wavlm_mix_proj_ln(acc, rows, D, wt.p, false, bias, g, beta, SE, out, st);
      return;
    }
    Scratch ob((size_t)rows * SE * 2, st);
    sd::wavlm_mix_proj_ln(acc, rows, D, wt.p, true, bias, g, beta, SE, ob.p, st);
    sd::bf16_to_f32(ob.p, (int64_t)rows * SE, out, st);
  });
}

int sd_w2vbert_create(const sd_w2vbert_config* c, sd_w2vbert** out) {
  return guard([&] {
    using T = sd::W2vBertTrunk;
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision == 0 || c->precision == 1, sd::kErrInvalid,
             "precision must be 0 or 1 (w2v-BERT 2.0 does not build bf16x3)");
    SD_CHECK(c->hidden == T::kHidden, sd::kErrInvalid, "w2v-BERT 2.0 (MI355X backend) builds hidden 1024 only");
    SD_CHECK(c->heads == T::kHeads, sd::kErrInvalid, "w2v-BERT 2.0 (MI355X backend) builds heads 16 only");
    SD_CHECK(c->ffn == T::kFfn, sd::kErrInvalid, "w2v-BERT 2.0 (MI355X backend) builds ffn 4096 only");
    SD_CHECK(c->layers >= 1 && c->layers <= 24, sd::kErrInvalid, "layers must be 1..24");
    SD_CHECK(c->conv_kernel == T::kConvK, sd::kErrInvalid, "w2v-BERT 2.0 (MI355X backend) builds conv_kernel 31 only");
    SD_CHECK(c->left == T::kLeft, sd::kErrInvalid, "w2v-BERT 2.0 (MI355X backend) builds left 64 only");
    SD_CHECK(c->right == T::kRight, sd::kErrInvalid, "w2v-BERT 2.0 (MI355X backend) builds right 8 only");
    SD_CHECK(c->in_dim == T::kInDim, sd::kErrInvalid, "w2v-BERT 2.0 (MI355X backend) builds in_dim 160 only");
    SD_CHECK(c->position_embeddings == 0, sd::kErrInvalid,
             "w2v-BERT 2.0 (MI355X backend) builds position_embeddings 0 (relative_key) only");
    SD_CHECK(c->add_adapter == 0, sd::kErrInvalid, "w2v-BERT 2.0 (MI355X backend) builds add_adapter 0 only");
    SD_CHECK(c->max_batch > 0, sd::kErrInvalid, "max_batch must be positive");
    SD_CHECK(c->max_frames > 0, sd::kErrInvalid, "max_frames must be positive");
    // rows (B T2) times the widest row are counted in int
    SD_CHECK((int64_t)c->max_batch * c->max_frames * T::kFfn < (1ll << 31), sd::kErrInvalid,
             "max_batch * max_frames * ffn must be below 2^31");
    sd::W2vBertConfig t;
    t.layers = c->layers; t.max_batch = c->max_batch; t.max_frames = c->max_frames; t.bf16 = c->precision == 1;
    create(out, false, t);
  });
}

int sd_w2vbert_set_param(sd_w2vbert* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_w2vbert_finalize(sd_w2vbert* h) { return finalize(h); }

int sd_w2vbert_forward(sd_w2vbert* h, const float* in, int B, int T2, float* x_out, float* layers_out, void* stream) {
  return guard([&] {
    SD_CHECK(h && in && (x_out || layers_out), sd::kErrInvalid, "null argument");
    h->model->forward(in, B, T2, x_out, layers_out, S(stream));
  });
}

int64_t sd_w2vbert_device_bytes(const sd_w2vbert* h) { return device_bytes(h); }

int sd_w2vbert_destroy(sd_w2vbert* h) { return destroy(h); }

int sd_op_w2vbert_attention(const float* qkv, int B, int T, int H, const float* dist, float* out, int precision,
                            void* stream) {
  return guard([&] {
    SD_CHECK(qkv && dist && out, sd::kErrInvalid, "w2vbert_attention: null argument");
    SD_CHECK(B >= 1 && T >= 1 && H >= 1, sd::kErrInvalid, "w2vbert_attention: empty problem");
    SD_CHECK(precision == 0 || precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    hipStream_t st = S(stream);
    const bool bf = precision == 1;
    Activations qa(qkv, (int64_t)B * T * 3 * H * 64, bf ? 2 : 0, st);
    // distance_embedding.weight (73, 64) zero-padded to the kernel's 80 rows, in the operands' type
    Scratch e32((size_t)sd::kW2vDistRows * 64 * 4, st), e16((size_t)sd::kW2vDistRows * 64 * 2, st);
    sd::zero_fill(e32.p, (size_t)sd::kW2vDistRows * 64 * 4, st);
    SD_HIP(hipMemcpyAsync(e32.p, dist, (size_t)73 * 64 * 4, hipMemcpyDeviceToDevice, st));
    if (bf) sd::f32_to_bf16(static_cast<const float*>(e32.p), (int64_t)sd::kW2vDistRows * 64, e16.p, st);
    sd::W2vAttnArgs a;
    a.qkv = qa.a; a.bf16 = bf; a.dist = bf ? e16.p : e32.p; a.B = B; a.T = T; a.D = H * 64; a.H = H;
    a.out = out; a.out_bf16 = false;
    sd::w2vbert_attention(a, st);
  });
}

int sd_op_w2vbert_conv_mix(const float* x, int B, int T, const float* w, const float* g, const float* beta, float* out,
                           int precision, void* stream) {
  return guard([&] {
    SD_CHECK(x && w && g && beta && out, sd::kErrInvalid, "w2vbert_conv_mix: null argument");
    SD_CHECK(B >= 1 && T >= 1, sd::kErrInvalid, "w2vbert_conv_mix: empty problem");
    SD_CHECK(precision == 0 || precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    hipStream_t st = S(stream);
    if (precision == 0) {
      sd::w2vbert_conv_mix(x, B, T, w, g, beta, out, false, st);
      return;
    }
    const int64_t rows = (int64_t)B * T;
    Activations xa(x, rows * 2 * sd::kW2vConvC, 2, st);
    Scratch ob((size_t)rows * sd::kW2vConvC * 2, st);
    sd::w2vbert_conv_mix(xa.a, B, T, w, g, beta, ob.p, true, st);
    sd::bf16_to_f32(ob.p, rows * sd::kW2vConvC, out, st);
  });
}

int sd_whisper_create(const sd_whisper_config* c, sd_whisper** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision == 0 || c->precision == 1, sd::kErrInvalid,
             "precision must be 0 or 1 (the Whisper encoder does not build bf16x3)");
    check_whisper_geometry(c);
    check_whisper_workspace(c, c->max_batch, c->max_samples);
    sd::WhisperConfig t = whisper_geometry(c);
    t.max_batch = c->max_batch; t.max_samples = c->max_samples; t.bf16 = c->precision == 1;
    create(out, false, t);
  });
}

int sd_whisper_set_param(sd_whisper* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_whisper_finalize(sd_whisper* h) { return finalize(h); }

int sd_whisper_frames(int n_samples) { return n_samples < 400 ? 0 : sd::WhisperTrunk::frames(n_samples); }

int sd_whisper_forward(sd_whisper* h, const float* wavs, int B, int n_samples, float* out, void* stream) {
  return guard([&] {
    SD_CHECK(h && wavs && out, sd::kErrInvalid, "null argument");
    h->model->forward(wavs, B, n_samples, out, S(stream));
  });
}

int64_t sd_whisper_device_bytes(const sd_whisper* h) { return device_bytes(h); }

int sd_whisper_destroy(sd_whisper* h) { return destroy(h); }

int sd_op_whisper_logmel(const float* wav, int B, int n, int n_mels, const float* mel, float* out, void* stream) {
  return guard([&] {
    SD_CHECK(wav && mel && out, sd::kErrInvalid, "whisper_logmel: null argument");
    SD_CHECK(B >= 1 && n >= 400 && (n_mels == 80 || n_mels == 128), sd::kErrInvalid, "whisper_logmel: bad argument");
    hipStream_t st = S(stream);
    const int64_t rows = (int64_t)B * (n / sd::kWhisperHop);
    std::vector<float> basis, hann, m((size_t)n_mels * sd::kWhisperBins), mt(m.size());
    sd::whisper_dft_basis(basis, hann);
    SD_HIP(hipStreamSynchronize(st));
    SD_HIP(hipMemcpy(m.data(), mel, m.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n_mels; ++i)
      for (int k = 0; k < sd::kWhisperBins; ++k) mt[(size_t)k * n_mels + i] = m[(size_t)i * sd::kWhisperBins + k];
    Scratch db(basis.size() * 4, st), dh(hann.size() * 4, st), dm(mt.size() * 4, st);
    SD_HIP(hipMemcpy(db.p, basis.data(), basis.size() * 4, hipMemcpyHostToDevice));
    SD_HIP(hipMemcpy(dh.p, hann.data(), hann.size() * 4, hipMemcpyHostToDevice));
    SD_HIP(hipMemcpy(dm.p, mt.data(), mt.size() * 4, hipMemcpyHostToDevice));
    Scratch fr((size_t)rows * sd::kWhisperNfft * 4, st), sp((size_t)rows * 2 * sd::kWhisperBins * 4, st),
        raw((size_t)rows * n_mels * 4, st), mx((size_t)B * 4, st);
    sd::WhisperLogmelArgs a;
    a.wav = wav; a.B = B; a.n = n; a.n_mels = n_mels;
    a.hann = static_cast<const float*>(dh.p); a.basis = static_cast<const float*>(db.p);
    a.melT = static_cast<const float*>(dm.p);
    a.frames = static_cast<float*>(fr.p); a.spec = static_cast<float*>(sp.p); a.raw = static_cast<float*>(raw.p);
    a.wmax = static_cast<uint32_t*>(mx.p);
    a.out = out; a.ldo = n_mels; a.out_bf16 = false;
    sd::whisper_logmel(a, st);
  });
}

int sd_op_whisper_stem(const float* feat, int B, int F, int n_mels, int D, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* pe, float* out, int precision, void* stream) {
  return guard([&] {
    SD_CHECK(feat && w1 && b1 && w2 && b2 && pe && out, sd::kErrInvalid, "whisper_stem: null argument");
    SD_CHECK(B >= 1 && F >= 1 && n_mels >= 4 && n_mels % 4 == 0 && D >= 32 && D % 32 == 0, sd::kErrInvalid,
             "whisper_stem: bad argument");
    SD_CHECK(precision == 0 || precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    hipStream_t st = S(stream);
    const bool bf = precision == 1;
    const int ld = (n_mels + 31) / 32 * 32;
    const int64_t rows = (int64_t)B * F;
    // the rows padded to ld channels, and conv1's weight (D, n_mels, 3) padded alike
    Scratch f32((size_t)rows * ld * 4, st), wp((size_t)D * ld * 3 * 4, st);
    sd::zero_fill(f32.p, (size_t)rows * ld * 4, st);
    SD_HIP(hipMemcpy2DAsync(f32.p, (size_t)ld * 4, feat, (size_t)n_mels * 4, (size_t)n_mels * 4, rows,
                            hipMemcpyDeviceToDevice, st));
    sd::zero_fill(wp.p, (size_t)D * ld * 3 * 4, st);
    // (n, c, tap): the n_mels * 3 values of output channel n start at n * ld * 3 of the padded weight
    SD_HIP(hipMemcpy2DAsync(wp.p, (size_t)ld * 12, w1, (size_t)n_mels * 12, (size_t)n_mels * 12, D,
                            hipMemcpyDeviceToDevice, st));
    Activations fa(static_cast<const float*>(f32.p), rows * ld, bf ? 2 : 0, st);
    PackedScratch p1(static_cast<const float*>(wp.p), D, ld, 3, bf, st), p2(w2, D, D, 3, bf, st);
    Scratch c1((size_t)rows * D * (bf ? 2 : 4), st);
    sd::WhisperStemW w;
    w.conv1 = p1.p; w.conv2 = p2.p; w.b1 = b1; w.b2 = b2; w.pe = pe; w.mel_ld = ld; w.D = D;
    sd::whisper_stem(w, fa.a, B, F, bf, c1.p, out, st);
  });
}

int sd_op_whisper_add(const float* x, int ldx, const float* t, float* out, int ldo, int64_t rows, int D, void* stream) {
  return guard([&] { sd::whisper_add(x, ldx, t, out, ldo, rows, D, S(stream)); });
}

int sd_op_whisper_ln_wide(const float* x, int ldx, int64_t rows, int W, const float* g, const float* b, float* out,
                          int precision, void* stream) {
  return guard([&] {
    SD_CHECK(precision == 0 || precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    SD_CHECK(rows >= 1 && W >= 4, sd::kErrInvalid, "whisper_ln_wide: empty problem");
    hipStream_t st = S(stream);
    if (precision == 0) {
      sd::whisper_ln_wide(x, ldx, rows, W, g, b, 1e-5f, out, W, false, st);
      return;
    }
    Scratch ob((size_t)rows * W * 2, st);
    sd::whisper_ln_wide(x, ldx, rows, W, g, b, 1e-5f, ob.p, W, true, st);
    sd::bf16_to_f32(ob.p, rows * W, out, st);
  });
}

int sd_ssnd_create(const sd_ssnd_config* c, sd_ssnd** out) {
  return guard([&] {
    SD_CHECK(c && out, sd::kErrInvalid, "null argument");
    SD_CHECK(c->precision == 0 || c->precision == 1, sd::kErrInvalid, "precision must be 0 or 1");
    SD_CHECK(c->max_batch > 0 && c->max_fbank_frames >= 8 && c->max_speakers > 0, sd::kErrInvalid,
             "bad workspace sizes");
    SD_CHECK(c->num_layers >= 1 && c->nhead > 0 && c->d_model > 0 && c->d_ff > 0 && c->emb_dim > 0 &&
                 c->q_det_aux_dim > 0 && c->q_rep_aux_dim > 0 && c->pos_emb_dim > 0 && c->vad_out_len > 0 &&
                 c->max_seq_len >= c->vad_out_len && c->n_all_speakers > 0,
             sd::kErrInvalid, "bad model dimensions");
    SD_CHECK(c->conformer_kernel >= 1 && c->conformer_kernel % 2 == 1 && c->conformer_kernel <= 31, sd::kErrInvalid,
             "conformer_kernel must be odd and <= 31");
    SD_CHECK(c->q_det_aux_dim == c->emb_dim, sd::kErrInvalid,
             "q_det_aux_dim must equal emb_dim (the speaker embeddings are the detection queries)");
    sd::SsndConfig t;
    t.max_batch = c->max_batch; t.max_fbank_frames = c->max_fbank_frames; t.max_speakers = c->max_speakers;
    t.feat_dim = c->feat_dim; t.emb_dim = c->emb_dim; t.q_det_aux_dim = c->q_det_aux_dim;
    t.q_rep_aux_dim = c->q_rep_aux_dim; t.d_model = c->d_model; t.nhead = c->nhead; t.d_ff = c->d_ff;
    t.num_layers = c->num_layers; t.vad_out_len = c->vad_out_len; t.pos_emb_dim = c->pos_emb_dim;
    t.max_seq_len = c->max_seq_len; t.n_all_speakers = c->n_all_speakers; t.conformer_kernel = c->conformer_kernel;
    t.bf16 = c->precision == 1;
    create(out, false, t);
  });
}

int sd_ssnd_set_param(sd_ssnd* h, const char* name, const float* data, const int64_t* shape, int ndim) {
  return set_param(h, name, data, shape, ndim);
}

int sd_ssnd_finalize(sd_ssnd* h) { return finalize(h); }

int sd_ssnd_infer(sd_ssnd* h, const float* feats, const float* spk, int B, int T_fbank, float* vad, float* emb,
                  void* stream) {
  return guard([&] {
    SD_CHECK(h && feats && spk && vad && emb, sd::kErrInvalid, "null argument");
    h->model->infer(feats, spk, B, T_fbank, vad, emb, S(stream));
  });
}

int sd_ssnd_decode(sd_ssnd* h, const float* enc, const float* x, const float* spk, int B, int T, float* vad,
                   float* emb, void* stream) {
  return guard([&] {
    SD_CHECK(h && enc && x && spk && vad && emb, sd::kErrInvalid, "null argument");
    h->model->decode(enc, x, spk, B, T, vad, emb, S(stream));
  });
}

int64_t sd_ssnd_device_bytes(const sd_ssnd* h) { return device_bytes(h); }

int sd_ssnd_destroy(sd_ssnd* h) { return destroy(h); }

int sd_window_wave(const float* wav, int64_t n_total, const int* win_start, const int* win_n, int n_win, int n_out,
                   float* out, void* stream) {
  return guard([&] {
    if (n_win == 0) return;
    sd::window_wave(wav, n_total, win_start, win_n, n_win, n_out, out, S(stream));
  });
}

int sd_window_cmn(const float* feats, int n_mels, const int* win_start, const int* win_n, int n_win,
                  int T_out, float* out, void* stream) {
  return guard([&] {
    if (n_win == 0) return;
    sd::window_cmn(feats, n_mels, win_start, win_n, n_win, T_out, out, S(stream));
  });
}

// sd_overlap_average (sigmoid of logits, then the mean) and sd_overlap_mean (the mean of probabilities)
static int overlap(const std::string& what, bool sigmoid, const float* x, int n_win, int NS, int Tw, const int* start,
                   const int* len, int dis, int chunk, int n_frames, float* out, void* stream) {
  return guard([&] {
    SD_CHECK(dis > 0 && chunk > 0, sd::kErrInvalid, what + ": bad window geometry");
    SD_CHECK((chunk + dis - 1) / dis <= sd::kOverlapMaxWindows, sd::kErrInvalid,
             what + ": more covering windows per frame than the pairwise mean supports");
    sd::overlap_average(x, n_win, NS, Tw, start, len, dis, chunk, n_frames, out, S(stream), sigmoid);
  });
}

int sd_overlap_average(const float* logits, int n_win, int NS, int Tw, const int* start,
                       const int* len, int dis, int chunk, int n_frames, float* out, void* stream) {
  return overlap("overlap_average", true, logits, n_win, NS, Tw, start, len, dis, chunk, n_frames, out, stream);
}

int sd_overlap_mean(const float* probs, int n_win, int NS, int Tw, const int* start, const int* len, int dis,
                    int chunk, int n_frames, float* out, void* stream) {
  return overlap("overlap_mean", false, probs, n_win, NS, Tw, start, len, dis, chunk, n_frames, out, stream);
}

int sd_postprocess_segments(const float* post, int rows, int T, int med_filter, const float* thresholds,
                            int n_thresholds, int min_silence_frames, int min_speech_frames, int cap,
                            int* seg_begin, int* seg_end, int* n_seg, int flags, void* stream) {
  return guard([&] {
    SD_CHECK(rows >= 0 && T >= 0, sd::kErrInvalid, "postprocess: negative shape");
    SD_CHECK(n_thresholds >= 1 && n_thresholds <= sd::ThresholdSet::kMax, sd::kErrInvalid,
             "postprocess: 1..16 thresholds");
    SD_CHECK(T <= sd::segments_max_frames(), sd::kErrInvalid, "postprocess: track too long");
    SD_CHECK(cap >= (T + 1) / 2, sd::kErrInvalid, "postprocess: cap < (T+1)/2");
    if (rows == 0 || T == 0) {
      if (rows > 0) SD_HIP(hipMemsetAsync(n_seg, 0, sizeof(int) * rows * n_thresholds, S(stream)));
      return;
    }
    hipStream_t st = S(stream);
    sd::ThresholdSet thr;
    thr.n = n_thresholds;
    thr.strict = flags & 1;
    for (int i = 0; i < n_thresholds; ++i) thr.v[i] = thresholds[i];
    Scratch med((size_t)rows * T * sizeof(float), st);
    sd::medfilt(post, rows, T, med_filter, static_cast<float*>(med.p), st);
    sd::run_segments(static_cast<const float*>(med.p), rows, T, thr, min_silence_frames, min_speech_frames, cap,
                     seg_begin, seg_end, n_seg, st);
  });
}

int sd_op_linear(const float* x, int M, int K, const float* w, const float* b, int N, int act,
                 float* out, int precision, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    const bool bf = precision >= 1;
    PackedScratch wt(w, N, K, 1, bf, st);
    Activations xa(x, (int64_t)M * K, precision, st);
    sd::ConvGemmArgs p = sd::linear_args(xa.a, M, K, K, wt.p, N, out, N);
    p.a_bf16 = xa.bf16;
    p.beta = b;
    p.act = act;
    sd::conv_gemm(p, bf, st);
  });
}

int sd_op_gemm_bf16(const void* x, int M, int K, int lda, int a_coff, const float* w, int N,
                    const float* pre_scale, const float* pre_shift, const float* alpha, const float* beta,
                    int act, void* out, int ldo, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(M > 0 && K > 0 && N > 0 && lda >= a_coff + K && ldo >= N, sd::kErrInvalid, "gemm_bf16: bad shape");
    SD_CHECK((pre_scale == nullptr) == (pre_shift == nullptr), sd::kErrInvalid, "gemm_bf16: pre_scale/pre_shift");
    PackedScratch wt(w, N, K, 1, true, st);
    sd::ConvGemmArgs p = sd::linear_args(x, M, K, lda, wt.p, N, out, ldo);
    p.a_bf16 = true;
    p.a_coff = a_coff;
    p.out_bf16 = true;
    p.pre_scale = pre_scale;
    p.pre_shift = pre_shift;
    p.alpha = alpha;
    p.beta = beta;
    p.act = act;
    sd::conv_gemm(p, true, st);
  });
}

int sd_op_conv_gemm(const sd_gemm_op* op, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(op, sd::kErrInvalid, "conv_gemm op: null argument");
    SD_CHECK(op->precision >= 0 && op->precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
    SD_CHECK(op->w && op->N > 0 && op->B > 0 && op->H > 0 && op->W > 0 && op->Cin > 0, sd::kErrInvalid,
             "conv_gemm op: bad shape");
    SD_CHECK(op->kh > 0 && op->kw > 0 && op->sh > 0 && op->sw > 0 && op->dh > 0 && op->dw > 0 && op->ph >= 0 &&
                 op->pw >= 0,
             sd::kErrInvalid, "conv_gemm op: bad conv geometry");
    const int Ho = (op->H + 2 * op->ph - op->dh * (op->kh - 1) - 1) / op->sh + 1;
    const int Wo = (op->W + 2 * op->pw - op->dw * (op->kw - 1) - 1) / op->sw + 1;
    SD_CHECK(Ho > 0 && Wo > 0, sd::kErrInvalid, "conv_gemm op: empty output");
    const bool prologue_rows = op->ln_g || op->pro_mode != 0;   // the A rows come from ln_x
    SD_CHECK(op->A || prologue_rows, sd::kErrInvalid, "conv_gemm op: no A");
    SD_CHECK(op->a_coff >= 0 && op->lda >= op->a_coff + op->Cin, sd::kErrInvalid, "conv_gemm op: lda < a_coff + Cin");
    SD_CHECK((op->pre_scale == nullptr) == (op->pre_shift == nullptr), sd::kErrInvalid,
             "conv_gemm op: pre_scale and pre_shift come together");
    SD_CHECK(!op->res || op->res_ld >= op->N, sd::kErrInvalid, "conv_gemm op: res_ld < N");
    SD_CHECK(!op->gate || (op->gate_seg > 0 && op->gate_nseg > 0 && (Wo - 1) / op->gate_seg < op->gate_nseg),
             sd::kErrInvalid, "conv_gemm op: gate segments do not cover the output");
    SD_CHECK(!op->glu || op->N % 32 == 0, sd::kErrInvalid, "conv_gemm op: GLU needs N % 32 == 0");
    SD_CHECK(op->ksplit_out ? op->slabs != nullptr : op->out != nullptr, sd::kErrInvalid, "conv_gemm op: no output");
    const bool bf = op->precision == 1;
    const int taps = op->kh * op->kw, K = taps * op->Cin;
    // GLU: rows [0, N/2) are the values and [N/2, N) their gates in torch order; the kernels read 32-row groups
    // (glu_interleave_row), alpha and beta with them, as the encoder packs its pointwise_conv1
    Scratch perm(op->glu ? (size_t)op->N * K * sizeof(float) : 0, st);
    Scratch ab(op->glu ? (size_t)2 * op->N * sizeof(float) : 0, st);
    const float *w = op->w, *alpha = op->alpha, *beta = op->beta;
    if (op->glu) {
      for (int r = 0; r < op->N; ++r)
        SD_HIP(hipMemcpyAsync(static_cast<float*>(perm.p) + (size_t)sd::glu_interleave_row(r, op->N / 2) * K,
                              op->w + (size_t)r * K, (size_t)K * sizeof(float), hipMemcpyDeviceToDevice, st));
      w = static_cast<const float*>(perm.p);
      SD_HIP(hipStreamSynchronize(st));
      std::vector<float> src(op->N), dst(op->N);
      int slot = 0;
      for (const float** v : {&alpha, &beta}) {
        if (!*v) continue;
        SD_HIP(hipMemcpy(src.data(), *v, op->N * sizeof(float), hipMemcpyDeviceToHost));
        for (int r = 0; r < op->N; ++r) dst[sd::glu_interleave_row(r, op->N / 2)] = src[r];
        float* d = static_cast<float*>(ab.p) + (size_t)slot++ * op->N;
        SD_HIP(hipMemcpy(d, dst.data(), op->N * sizeof(float), hipMemcpyHostToDevice));
        *v = d;
      }
    }
    PackedScratch wt(w, op->N, op->Cin, taps, bf, st);
    sd::ConvGemmArgs p;
    p.A = op->A; p.a_bf16 = op->a_bf16 != 0; p.a_tiled = op->a_tiled;
    p.B = op->B; p.H = op->H; p.W = op->W; p.Cin = op->Cin; p.lda = op->lda; p.a_coff = op->a_coff;
    p.Ho = Ho; p.Wo = Wo;
    p.kh = op->kh; p.kw = op->kw; p.sh = op->sh; p.sw = op->sw; p.ph = op->ph; p.pw = op->pw; p.dh = op->dh;
    p.dw = op->dw;
    p.Wt = wt.p; p.N = op->N; p.K = K;
    p.pre_scale = op->pre_scale; p.pre_shift = op->pre_shift; p.alpha = alpha; p.beta = beta;
    p.res = op->res; p.res_bf16 = op->res_bf16 != 0; p.res_ld = op->res_ld;
    p.act = op->act;
    p.post_scale = op->post_scale; p.post_shift = op->post_shift;
    p.gate = op->gate; p.gate_seg = op->gate ? op->gate_seg : 1; p.gate_nseg = op->gate ? op->gate_nseg : 1;
    p.out = op->out; p.out_bf16 = op->out_bf16 != 0;
    p.o_sb = op->o_sb; p.o_sh = op->o_sh; p.o_sw = op->o_sw; p.o_sn = op->o_sn;
    p.glu = op->glu;
    p.ln_x = op->ln_x; p.ln_t = op->ln_t; p.ln_t_bf16 = op->ln_t_bf16 != 0; p.ln_g = op->ln_g; p.ln_b = op->ln_b;
    p.ln_eps = op->ln_eps; p.ln_out = op->ln_out;
    p.pro_mode = op->pro_mode; p.pro_p = op->pro_p; p.pro_C = op->pro_C; p.pro_pad = op->pro_pad;
    p.pro_cursor = op->pro_cursor; p.pro_nvalid = op->pro_nvalid;
    p.kv_out = op->kv_out; p.kv_cursor = op->kv_cursor; p.kv_mult = op->kv_mult; p.kv_col0 = op->kv_col0;
    p.kv_ld = op->kv_ld;
    if (op->ksplit_out) {
      SD_CHECK(bf, sd::kErrInvalid, "conv_gemm op: split-K is a bf16 path");
      const int ks = sd::gemm_splitk_count(p);
      SD_HIP(hipMemcpyAsync(op->ksplit_out, &ks, sizeof(int), hipMemcpyHostToDevice, st));
      SD_HIP(hipStreamSynchronize(st));
      if (ks > 1) {
        SD_CHECK(ks <= op->slab_cap, sd::kErrInvalid, "conv_gemm op: fewer slabs than the split count");
        sd::conv_gemm_splitk(p, ks, op->slabs, st);
        return;
      }
      SD_CHECK(op->out, sd::kErrInvalid, "conv_gemm op: no split and no output");
    }
    // the production dispatch: which kernel runs follows from the arguments alone, as in the models
    const sd::GemmX3Scope x3(op->precision == 2);
    sd::conv_gemm(p, bf, st);
  });
}

int sd_op_tstp_pool(const void* x, int x_bf16, int B, int T, int C, float* stats, void* stream) {
  return guard([&] {
    SD_CHECK(x && stats, sd::kErrInvalid, "tstp_pool: null argument");
    sd::tstp_pool(x, x_bf16 != 0, B, T, C, stats, nullptr, S(stream));
  });
}

int sd_op_res2_chain(const void* x, int B, int T, int dilation, const float* w, const float* bias, const float* s,
                     const float* h, void* out, int use_generic, int precision, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && w && bias && s && h && out && B >= 1 && T >= 1 && dilation >= 1, sd::kErrInvalid,
             "res2_chain: bad argument");
    SD_CHECK(precision >= 0 && precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
    SD_CHECK(use_generic || precision == 1, sd::kErrInvalid,
             "res2_chain: the fused kernel is bf16 (precision 1); fp32 and bf16x3 take use_generic 1");
    const bool bf = precision == 1;
    const sd::GemmX3Scope x3(precision == 2);
    constexpr int G = 128, NS = sd::Res2ChainW::kStages;
    Scratch wt((size_t)NS * G * 3 * G * (bf ? 2 : 4), st), tmp((size_t)B * T * G * (bf ? 2 : 4), st);
    sd::Res2ChainW W;
    for (int i = 0; i < NS; ++i) {
      void* wi = static_cast<char*>(wt.p) + (size_t)i * G * 3 * G * (bf ? 2 : 4);
      sd::pack_weight(w + (size_t)i * G * G * 3, G, G, 3, wi, bf, st);
      W.w[i] = wi; W.bias[i] = bias + i * G; W.s[i] = s + i * G; W.h[i] = h + i * G;
    }
    sd::res2_chain(x, B, T, dilation, W, tmp.p, out, bf, use_generic != 0, st);
  });
}

int sd_op_astp_pool_c(const void* x, int x_bf16, int B, int T, int C, const float* w1, const float* b1, const float* w2,
                      const float* b2, float* stats, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && w1 && b1 && w2 && b2 && stats && B >= 1, sd::kErrInvalid, "astp_pool: bad argument");
    SD_CHECK(C >= 64 && C % 64 == 0, sd::kErrInvalid, "astp_pool: C must be a multiple of 64");
    SD_CHECK(T >= 2, sd::kErrShape, "ASTP needs at least 2 frames (the unbiased variance of one frame is NaN)");
    constexpr int H = 128;
    const size_t rows = (size_t)B * T;
    // linear1.weight (128, 3 C) split on its input axis: the per-frame half (packed for conv_gemm) and the context half
    Scratch halves((size_t)3 * H * C * 4, st), w1x((size_t)H * C * 4, st), w2p((size_t)C * H * 4, st);
    float* hx = static_cast<float*>(halves.p);
    float* hc = hx + (size_t)H * C;
    SD_HIP(hipMemcpy2DAsync(hx, (size_t)C * 4, w1, (size_t)3 * C * 4, (size_t)C * 4, H, hipMemcpyDeviceToDevice, st));
    SD_HIP(hipMemcpy2DAsync(hc, (size_t)2 * C * 4, w1 + C, (size_t)3 * C * 4, (size_t)2 * C * 4, H,
                            hipMemcpyDeviceToDevice, st));
    sd::pack_weight(hx, H, C, 1, w1x.p, false, st);
    sd::pack_weight(w2, C, H, 1, w2p.p, false, st);
    Scratch ctx((size_t)B * 2 * C * 4, st), cv((size_t)B * H * 4, st), x32(x_bf16 ? rows * C * 4 : 4, st),
        hh(rows * H * 4, st), e(rows * C * 4, st);
    sd::AstpArgs a;
    a.x = x; a.x_bf16 = x_bf16 != 0; a.B = B; a.T = T;
    a.w1x = w1x.p; a.w1c = hc; a.b1 = b1; a.w2 = w2p.p; a.b2 = b2; a.stats = stats;
    a.ctx = static_cast<float*>(ctx.p); a.cv = static_cast<float*>(cv.p); a.x32 = static_cast<float*>(x32.p);
    a.h = static_cast<float*>(hh.p); a.e = static_cast<float*>(e.p);
    a.C = C;
    sd::astp_pool(a, st);
  });
}

int sd_op_astp_pool(const void* x, int x_bf16, int B, int T, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* stats, void* stream) {
  return sd_op_astp_pool_c(x, x_bf16, B, T, 1536, w1, b1, w2, b2, stats, stream);
}

int sd_op_redim_block2d(const void* x, int B, int T, int c, const float* dw_w, const float* dw_b, const float* bn_s,
                        const float* bn_h, const float* pw_w, const float* pw_b, void* out, int use_generic,
                        int precision, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && dw_w && dw_b && bn_s && bn_h && pw_w && pw_b && out && B >= 1 && T >= 1, sd::kErrInvalid,
             "redim_block2d: bad argument");
    SD_CHECK(c == 16 || c == 32 || c == 64 || c == 128, sd::kErrInvalid, "redim_block2d: c must be 16, 32, 64 or 128");
    SD_CHECK(precision >= 0 && precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
    SD_CHECK(use_generic || precision == 1, sd::kErrInvalid,
             "redim_block2d: the fused kernel is bf16 (precision 1); fp32 and bf16x3 take use_generic 1");
    const bool bf = precision == 1;
    const sd::GemmX3Scope x3(precision == 2);
    // fold on the host, as the model's load does
    std::vector<float> w((size_t)c * 36), b(c), s(c), h(c), dw, dwb;
    SD_HIP(hipStreamSynchronize(st));
    SD_HIP(hipMemcpy(w.data(), dw_w, w.size() * 4, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(b.data(), dw_b, (size_t)c * 4, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(s.data(), bn_s, (size_t)c * 4, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(h.data(), bn_h, (size_t)c * 4, hipMemcpyDeviceToHost));
    sd::redim_pack_dw(w.data(), b.data(), s.data(), h.data(), c, dw, dwb);
    Scratch d_dw(dw.size() * 4, st), d_b(dwb.size() * 4, st), tmp((size_t)B * T * sd::kRedimCF * (bf ? 2 : 4), st);
    SD_HIP(hipMemcpy(d_dw.p, dw.data(), dw.size() * 4, hipMemcpyHostToDevice));
    SD_HIP(hipMemcpy(d_b.p, dwb.data(), dwb.size() * 4, hipMemcpyHostToDevice));
    PackedScratch pw(pw_w, c, c, 1, bf, st);
    sd::RedimBlock2dW W;
    W.dw = static_cast<const float*>(d_dw.p); W.dw_b = static_cast<const float*>(d_b.p);
    W.pw = pw.p; W.pw_b = pw_b;
    sd::redim_block2d(x, B, T, c, W, tmp.p, out, bf, use_generic != 0, st);
  });
}

int sd_op_redim_dwconv1d(const float* x, int B, int T, int hC, int k, const float* w, const float* bias,
                         const float* bn_s, const float* bn_h, void* out, int out_bf16, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && w && bias && bn_s && bn_h && out && B >= 1 && T >= 1 && hC >= 1 && k >= 1 && k <= 59 && k % 2 == 1,
             sd::kErrInvalid, "redim_dwconv1d: bad argument");
    std::vector<float> hw((size_t)hC * k), hb(hC), s(hC), h(hC), wt((size_t)hC * k), fb(hC);
    SD_HIP(hipStreamSynchronize(st));
    SD_HIP(hipMemcpy(hw.data(), w, hw.size() * 4, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(hb.data(), bias, (size_t)hC * 4, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(s.data(), bn_s, (size_t)hC * 4, hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(h.data(), bn_h, (size_t)hC * 4, hipMemcpyDeviceToHost));
    for (int ch = 0; ch < hC; ++ch) {
      for (int j = 0; j < k; ++j) wt[(size_t)j * hC + ch] = (float)((double)hw[(size_t)ch * k + j] * s[ch]);
      fb[ch] = (float)((double)hb[ch] * s[ch] + h[ch]);
    }
    Scratch d_w(wt.size() * 4, st), d_b(fb.size() * 4, st);
    SD_HIP(hipMemcpy(d_w.p, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
    SD_HIP(hipMemcpy(d_b.p, fb.data(), fb.size() * 4, hipMemcpyHostToDevice));
    sd::redim_dwconv1d(x, B, T, hC, k, static_cast<const float*>(d_w.p), static_cast<const float*>(d_b.p), out,
                       out_bf16 != 0, st);
  });
}

int sd_op_redim_stage_mix(const void* x, int n, int64_t rows, const float* w, void* out, int bf16, void* stream) {
  return guard([&] {
    SD_CHECK(x && w && out && n >= 2 && n <= sd::RedimMixArgs::kMax && rows >= 1, sd::kErrInvalid,
             "redim_stage_mix: 2 to 7 inputs, rows >= 1");
    sd::RedimMixArgs a;
    a.n = n;
    a.w = w;
    for (int k = 0; k < n; ++k) a.x[k] = static_cast<const char*>(x) + (size_t)k * rows * sd::kRedimCF * (bf16 ? 2 : 4);
    sd::redim_stage_mix(a, rows, out, bf16 != 0, S(stream));
  });
}

int sd_op_redim_stem(const float* fbank, int B, int T, const float* w, const float* bias, const float* g,
                     const float* beta, void* out, int out_bf16, void* stream) {
  return guard([&] { sd::redim_stem(fbank, B, T, w, bias, g, beta, out, out_bf16 != 0, S(stream)); });
}


int sd_op_asp_pool(const void* x, int x_bf16, int B, int T, int C, const float* w1, const float* b1, const float* bn_s,
                   const float* bn_h, const float* w2, const float* b2, float* stats, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && w1 && b1 && bn_s && bn_h && w2 && b2 && stats && B >= 1 && T >= 1 && C >= 64 && C % 64 == 0,
             sd::kErrInvalid, "asp_pool: bad argument");
    constexpr int H = 128;
    const size_t rows = (size_t)B * T;
    Scratch w1p((size_t)H * C * 4, st), w2p((size_t)C * H * 4, st);
    sd::pack_weight(w1, H, C, 1, w1p.p, false, st);
    sd::pack_weight(w2, C, H, 1, w2p.p, false, st);
    const size_t gemm_rows = std::max<size_t>(rows, sd::kAspMinRows);
    Scratch x32(x_bf16 ? rows * C * 4 : 4, st), hh(gemm_rows * H * 4, st), e(gemm_rows * C * 4, st);
    sd::AspArgs a;
    a.x = x; a.x_bf16 = x_bf16 != 0; a.B = B; a.T = T; a.C = C;
    a.w1 = w1p.p; a.b1 = b1; a.bn_s = bn_s; a.bn_h = bn_h; a.w2 = w2p.p; a.b2 = b2; a.stats = stats;
    a.x32 = static_cast<float*>(x32.p); a.h = static_cast<float*>(hh.p); a.e = static_cast<float*>(e.p);
    sd::asp_pool(a, st);
  });
}

int sd_op_simam(const void* y, const void* residual, int dtype, int B, int H, int W, int C, void* out, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(y && out && (dtype == 0 || dtype == 1) && B >= 1 && H >= 1 && W >= 1 && C >= 64 && C % 64 == 0,
             sd::kErrInvalid, "simam: bad argument");
    Scratch partial((size_t)B * sd::simam_tiles(H * W) * C * 24, st), stat((size_t)B * C * 16, st);
    sd::SimamArgs a;
    a.y = y; a.res = residual; a.bf16 = dtype == 1; a.B = B; a.H = H; a.W = W; a.C = C;
    a.out = out; a.o_sb = (int64_t)H * W * C; a.o_sh = (int64_t)W * C; a.o_sw = C; a.o_sn = 1;
    a.partial = partial.p; a.stat = stat.p;
    sd::simam_gate(a, st);
  });
}

namespace {
// a device fp32 array of n floats on the host (test ops only: synchronises the stream)
std::vector<float> to_host(const float* d, size_t n, hipStream_t st) {
  std::vector<float> h(n);
  SD_HIP(hipStreamSynchronize(st));
  SD_HIP(hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost));
  return h;
}
}  // namespace

int sd_op_res2_conv3x3(const void* x, int B, int H, int W, int ldx, int x_coff, int width, const void* add, int ld_add,
                       int add_coff, const float* w, const float* alpha, const float* beta, void* out, int ldo,
                       int o_coff, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && w && alpha && beta && out && width >= 2 && width <= 512, sd::kErrInvalid, "res2_conv3x3: bad argument");
    const int Cp = sd::res2_padded(width);
    const std::vector<float> hw = to_host(w, (size_t)width * width * 9, st), ha = to_host(alpha, width, st),
                             hb = to_host(beta, width, st);
    std::vector<float> pw((size_t)Cp * 9 * Cp, 0.f), pa(Cp, 0.f), pb(Cp, 0.f);
    for (int n = 0; n < width; ++n) {
      pa[n] = ha[n];
      pb[n] = hb[n];
      for (int c = 0; c < width; ++c)
        for (int t = 0; t < 9; ++t) pw[((size_t)n * 9 + t) * Cp + c] = hw[((size_t)n * width + c) * 9 + t];
    }
    sd::DeviceArena arena;   // freed once the stream has drained, below
    const sd::PackedW k = sd::upload_packed(arena, pw, Cp, Cp, 3, 3, true);
    sd::Res2ConvArgs a;
    a.x = x; a.ldx = ldx; a.x_coff = x_coff;
    a.add = add; a.ld_add = ld_add; a.add_coff = add_coff;
    a.B = B; a.H = H; a.W = W; a.width = width;
    a.w = k.w; a.alpha = arena.upload(pa); a.beta = arena.upload(pb);
    a.out = out; a.ldo = ldo; a.o_coff = o_coff;
    sd::res2_conv3x3(a, st);
    SD_HIP(hipStreamSynchronize(st));
  });
}

int sd_op_aff_gate(const void* x, const void* y, int dtype, int64_t P, int C, int I, const float* w1, const float* a1,
                   const float* c1, const float* w2, const float* a2, const float* c2, void* out, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && y && out && w1 && a1 && c1 && w2 && a2 && c2 && (dtype == 0 || dtype == 1) && P >= 1 && C >= 2 &&
                 C % 2 == 0 && C <= 224 && I >= 1 && I <= 52,
             sd::kErrInvalid, "aff_gate: bad argument");
    const sd::AffPacked k =
        sd::aff_pack(to_host(w1, (size_t)I * 2 * C, st).data(), to_host(a1, I, st).data(), to_host(c1, I, st).data(),
                     to_host(w2, (size_t)C * I, st).data(), to_host(a2, C, st).data(), to_host(c2, C, st).data(), C, I, C);
    sd::DeviceArena arena;
    sd::AffGateArgs a;
    a.x = x; a.ldx = C; a.y = y; a.ldy = C; a.out = out; a.ldo = C;
    a.bf16 = dtype == 1; a.P = P; a.C = C; a.I = I;
    a.w1 = arena.upload(k.w1); a.a1 = arena.upload(k.a1); a.c1 = arena.upload(k.c1);
    a.w2 = arena.upload(k.w2); a.a2 = arena.upload(k.a2); a.c2 = arena.upload(k.c2);
    sd::aff_gate(a, st);
    SD_HIP(hipStreamSynchronize(st));
  });
}

int sd_op_stem_conv(const float* fbank, int B, int T, int F, const float* w, const float* alpha, const float* beta,
                    int C, void* out, int out_bf16, void* stream) {
  return guard([&] {
    SD_CHECK(fbank && w && alpha && beta && out && B >= 1 && T >= 1 && F >= 1, sd::kErrInvalid, "stem_conv: bad argument");
    sd::fcm_conv1(fbank, B, T, F, w, alpha, beta, out, out_bf16 != 0, S(stream), C);
  });
}

int sd_op_speaker_input_proj(const float* ts, const float* mix, int B, int NS, int T, int Tmix, int SE, int E,
                             const float* w, const float* bias, const float* pe, const float* bn_a, const float* bn_b,
                             const int* grp, int group, float* out, void* out_bf16, int precision, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(ts && mix && w && bias && out, sd::kErrInvalid, "speaker_input_proj: null argument");
    SD_CHECK(precision >= 0 && precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
    SD_CHECK(B >= 1 && NS >= 1 && T >= 1 && Tmix >= 1 && sd::speaker_input_proj_supported(SE, E), sd::kErrInvalid,
             "speaker_input_proj: bad shape");
    SD_CHECK((bn_a == nullptr) == (bn_b == nullptr) && group >= 1, sd::kErrInvalid, "speaker_input_proj: bn_a / bn_b");
    const bool bf = precision == 1;
    const sd::GemmX3Scope x3(precision == 2);
    // proj_layer.weight (E, 2 SE) as a 2-tap weight (E, SE, 2) would interleave the halves; pack them one by one
    Scratch wt((size_t)E * SE * (bf ? 2 : 4), st), wm((size_t)E * SE * (bf ? 2 : 4), st);
    Scratch halves((size_t)2 * E * SE * 4, st);
    float* h0 = static_cast<float*>(halves.p);
    float* h1 = h0 + (size_t)E * SE;
    SD_HIP(hipMemcpy2DAsync(h0, (size_t)SE * 4, w, (size_t)2 * SE * 4, (size_t)SE * 4, E, hipMemcpyDeviceToDevice, st));
    SD_HIP(hipMemcpy2DAsync(h1, (size_t)SE * 4, w + SE, (size_t)2 * SE * 4, (size_t)SE * 4, E,
                            hipMemcpyDeviceToDevice, st));
    sd::pack_weight(h0, E, SE, 1, wt.p, bf, st);
    sd::pack_weight(h1, E, SE, 1, wm.p, bf, st);
    Scratch mixa((size_t)B * Tmix * SE * 4, st), pts((size_t)B * NS * E * 4, st), pmix((size_t)B * Tmix * E * 4, st);
    sd::SpeakerProjArgs a;
    a.ts = ts; a.mix = mix; a.ldmix = SE; a.Tmix = Tmix; a.B = B; a.NS = NS; a.T = T; a.SE = SE; a.E = E;
    a.w_ts = wt.p; a.w_mix = wm.p; a.bias = bias; a.pe = pe;
    a.bn.a = bn_a; a.bn.b = bn_b; a.bn.grp = grp; a.bn.group = group;
    a.mix_a = mixa.p; a.p_ts = static_cast<float*>(pts.p); a.p_mix = static_cast<float*>(pmix.p);
    a.out = out; a.xb = static_cast<uint16_t*>(out_bf16);
    sd::speaker_input_proj(a, bf, st);
  });
}

int sd_op_gsp_down(const void* x, int x_bf16, const float* s, const float* h, const float* gw, const float* gb,
                   const float* w, const float* cb, int B, int T2, int SE, float* y, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && s && h && gw && gb && w && cb && y, sd::kErrInvalid, "gsp_down: null argument");
    SD_CHECK(SE >= 32 && SE % 32 == 0, sd::kErrInvalid, "gsp_down: SE must be a multiple of 32");
    SD_CHECK(B >= 1 && T2 >= 1, sd::kErrInvalid, "gsp_down: B and T2 must be at least 1");
    // the runtime's fold (TsvadModel::build): gsp_fc and the conv weight come back to the host, the 15 coefficients
    // per channel go up again
    constexpr int F = sd::kGspFcDim;
    std::vector<float> hgw((size_t)F * 2), hgb(F), hw((size_t)SE * F * 5), coef;
    SD_HIP(hipStreamSynchronize(st));
    SD_HIP(hipMemcpy(hgw.data(), gw, hgw.size() * sizeof(float), hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(hgb.data(), gb, hgb.size() * sizeof(float), hipMemcpyDeviceToHost));
    SD_HIP(hipMemcpy(hw.data(), w, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    sd::gsp_down_fold(hgw.data(), hgb.data(), hw.data(), SE, coef);
    Scratch dc(coef.size() * sizeof(float), st);
    SD_HIP(hipMemcpyAsync(dc.p, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice, st));
    sd::gsp_down(x, x_bf16 != 0, B, T2, s, h, static_cast<const float*>(dc.p), cb, SE, y, st);
    SD_HIP(hipStreamSynchronize(st));   // coef (host) and dc live until the kernel is done
  });
}

int sd_gsp_down_frame_tile(void) { return sd::gsp_down_frame_tile(); }

int sd_op_mamba2_stack(const float* x, int R, int L, int E, const float* weights, int64_t n_weights, int n_layer,
                       int d_state, int expand, int precision, float* out, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && weights && out && R >= 1 && L >= 1 && E >= 8 && n_layer >= 1, sd::kErrInvalid,
             "mamba2_stack: bad argument");
    SD_CHECK(precision >= 0 && precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
    sd::Mamba2Stack::validate(E, d_state, expand);
    const sd::GemmX3Scope x3(precision == 2);
    const int64_t DI = (int64_t)expand * E, H = DI / sd::kMamba2HeadDim, CD = DI + 2 * d_state, dip = 2 * DI + 2 * d_state + H;
    struct Key { const char* name; std::vector<int64_t> shape; };
    const std::vector<Key> keys = {{"norm.weight", {E}}, {"mixer.in_proj.weight", {dip, E}},
                                   {"mixer.conv1d.weight", {CD, 1, 4}}, {"mixer.conv1d.bias", {CD}},
                                   {"mixer.dt_bias", {H}}, {"mixer.A_log", {H}}, {"mixer.D", {H}},
                                   {"mixer.norm.weight", {DI}}, {"mixer.out_proj.weight", {E, DI}}};
    int64_t per_block = 0;
    for (const Key& k : keys) {
      int64_t n = 1;
      for (int64_t d : k.shape) n *= d;
      per_block += n;
    }
    SD_CHECK(n_weights == 2 * n_layer * per_block, sd::kErrInvalid,
             "mamba2_stack: weights must hold " + std::to_string(2 * n_layer * per_block) + " floats");
    std::vector<float> host((size_t)n_weights);
    SD_HIP(hipStreamSynchronize(st));
    SD_HIP(hipMemcpy(host.data(), weights, host.size() * sizeof(float), hipMemcpyDeviceToHost));
    sd::ParamStore ps;
    const float* w = host.data();
    for (int dir = 0; dir < 2; ++dir)
      for (int i = 0; i < n_layer; ++i)
        for (const Key& k : keys) {
          int64_t n = 1;
          for (int64_t d : k.shape) n *= d;
          ps.set(std::string(dir ? "backward_blocks." : "forward_blocks.") + std::to_string(i) + "." + k.name, w,
                 k.shape.data(), (int)k.shape.size());
          w += n;
        }
    sd::DeviceArena arena;   // freed on return, after the stream has drained
    sd::Mamba2Stack stack;
    stack.load(ps, arena, "", E, n_layer, d_state, expand, precision == 1);
    stack.alloc(arena, (int64_t)R * L);
    // R sequences of L contiguous rows: groups of G = L "windows" with one inner row each
    Scratch o16(precision == 1 ? (size_t)R * L * 2 * E * 2 : 4, st);
    stack.forward(x, R * L, L, 1, precision == 1 ? o16.p : out, precision == 1, 1, R * L, st);
    if (precision == 1) sd::bf16_to_f32(o16.p, (int64_t)R * L * 2 * E, out, st);
    SD_HIP(hipStreamSynchronize(st));
  });
}

int sd_probe_graph_memset(int n, int replays, int fork, int* bad_per_replay, void* stream) {
  return guard([&] {
    SD_CHECK(n > 0 && replays > 0 && bad_per_replay, sd::kErrInvalid, "probe_graph_memset: bad argument");
    sd::graph_memset_probe(n, replays, fork != 0, bad_per_replay, S(stream));
  });
}

int sd_debug_cam_dense_probe(void* stamps) {
  return guard([&] { sd::cam_dense_set_probe(stamps); });
}

int sd_debug_rowprog_probe(void* stamps) {
  return guard([&] { sd::rowprog_set_probe(stamps); });
}

int sd_op_cam_dense(const void* x, int B, int T, int ld, int cin, int dil, const float* s1, const float* h1,
                    const float* wb, const float* a2, const float* b2, const float* wl, const float* bl,
                    const float* w1, const float* c1, const float* w2, const float* c2, void* out, int repeats,
                    void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(B >= 1 && repeats >= 1 && ld >= cin + 32 &&
                 sd::cam_dense_supported(T, cin, ld, 128, 64, 32, 32, 3, dil, 100, true),
             sd::kErrInvalid, "cam_dense: unsupported shape");
    PackedScratch wbt(wb, 128, cin, 1, true, st), wlt(wl, 32, 128, 3, true, st);   // wlt: Wt[o][tap * 128 + c]
    Scratch rec(sd::cam_dense_record_bytes(B), st), cnt(sd::cam_dense_counter_bytes(B), st);
    SD_HIP(hipMemsetAsync(cnt.p, 0, sd::cam_dense_counter_bytes(B), st));
    for (int r = 0; r < repeats; ++r)
      sd::cam_dense(x, B, T, ld, cin, dil, s1, h1, wbt.p, a2, b2, wlt.p, bl, w1, c1, w2, c2, out, rec.p,
                    static_cast<unsigned*>(cnt.p), st);
  });
}

namespace {
// an FCM BasicResBlock over packed 32-channel weights for the trunk's unfused launches (a shortcut where wsc is set)
sd::ResBlockL fcm_res_block(int stride, const void* w1, const float* a1, const float* b1, const void* w2,
                            const float* a2, const float* b2, const void* wsc, const float* asc, const float* bsc) {
  auto conv = [](const void* w, int taps, const float* al, const float* be) {
    sd::ConvL L;
    L.w.w = w; L.w.N = 32; L.w.Cin = 32; L.w.K = 32 * taps * taps; L.w.kh = taps; L.w.kw = taps;
    L.alpha = al; L.beta = be;
    return L;
  };
  sd::ResBlockL rb;
  rb.stride = stride;
  rb.has_sc = wsc != nullptr;
  rb.c1 = conv(w1, 3, a1, b1);
  rb.c2 = conv(w2, 3, a2, b2);
  if (wsc) rb.sc = conv(wsc, 1, asc, bsc);
  return rb;
}
}  // namespace

int sd_op_fcm_block(const void* x, int B, int H, int W, int stride, const float* w1, const float* a1, const float* b1,
                    const float* w2, const float* a2, const float* b2, const float* wsc, const float* asc,
                    const float* bsc, void* out, int fused, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && out && w1 && a1 && b1 && w2 && a2 && b2 && B > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2),
             sd::kErrInvalid, "fcm_block: bad argument");
    SD_CHECK(stride == 2 ? (wsc && asc && bsc) : !wsc, sd::kErrInvalid, "fcm_block: the shortcut goes with stride 2");
    PackedScratch p1(w1, 32, 32, 9, true, st), p2(w2, 32, 32, 9, true, st), ps(wsc, 32, 32, 1, true, st);
    const int Ho = (H - 1) / stride + 1;
    if (fused) {
      sd::FcmBlockArgs a;
      a.x = x; a.B = B; a.H = H; a.W = W; a.stride = stride;
      a.w1 = p1.p; a.a1 = a1; a.b1 = b1; a.w2 = p2.p; a.a2 = a2; a.b2 = b2;
      if (wsc) { a.wsc = ps.p; a.asc = asc; a.bsc = bsc; }
      a.out = out;
      sd::conv_fcm_block(a, st);   // raises on arguments the kernel cannot compute
      return;
    }
    // the trunk's two launches on three maps of its own (the pair overwrites its input map when it has a shortcut)
    const size_t in_bytes = (size_t)B * H * W * 64;
    Scratch m0(in_bytes, st), m1(in_bytes, st), m2(in_bytes, st);
    SD_HIP(hipMemcpyAsync(m0.p, x, in_bytes, hipMemcpyDeviceToDevice, st));
    const sd::ResBlockL rb = fcm_res_block(stride, p1.p, a1, b1, p2.p, a2, b2, wsc ? ps.p : nullptr, asc, bsc);
    float* const bufs[3] = {static_cast<float*>(m0.p), static_cast<float*>(m1.p), static_cast<float*>(m2.p)};
    int h = H, w = W;
    const float* r = sd::fcm_block_pair(rb, bufs, bufs[0], true, B, h, w, sd::FcmFuse{}, st);
    SD_HIP(hipMemcpyAsync(out, r, (size_t)B * Ho * W * 64, hipMemcpyDeviceToDevice, st));
  });
}

int sd_op_fcm_stem_block(const float* fbank, int B, int W, int F, const float* stem_w, const float* stem_alpha,
                         const float* stem_beta, const float* w1, const float* a1, const float* b1, const float* w2,
                         const float* a2, const float* b2, const float* wsc, const float* asc, const float* bsc,
                         void* out, int fused, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(fbank && out && stem_w && stem_alpha && stem_beta && w1 && a1 && b1 && w2 && a2 && b2 && B > 0 && W > 0 &&
                 F > 0,
             sd::kErrInvalid, "fcm_stem_block: bad argument");
    SD_CHECK(wsc && asc && bsc, sd::kErrInvalid, "fcm_stem_block: layer1.0 has a shortcut");
    PackedScratch p1(w1, 32, 32, 9, true, st), p2(w2, 32, 32, 9, true, st), ps(wsc, 32, 32, 1, true, st);
    const int Ho = (F - 1) / 2 + 1;
    if (fused) {
      sd::FcmStemBlockArgs a;
      a.fbank = fbank; a.B = B; a.W = W; a.F = F;
      a.stem_w = stem_w; a.stem_alpha = stem_alpha; a.stem_beta = stem_beta;
      a.w1 = p1.p; a.a1 = a1; a.b1 = b1; a.w2 = p2.p; a.a2 = a2; a.b2 = b2;
      a.wsc = ps.p; a.asc = asc; a.bsc = bsc;
      a.out = out;
      sd::conv_fcm_stem_block(a, st);   // raises on arguments the kernel cannot compute
      return;
    }
    // the trunk's two launches (below W 113: its fp32 stem and three) on three scratch maps
    const size_t map_bytes = (size_t)B * F * W * 64;
    Scratch m0(map_bytes, st), m1(map_bytes, st), m2(map_bytes, st);
    const sd::ResBlockL rb = fcm_res_block(2, p1.p, a1, b1, p2.p, a2, b2, ps.p, asc, bsc);
    sd::FcmFuse stem;
    stem.fbank = fbank; stem.fb_F = F;
    stem.stem_w = stem_w; stem.stem_alpha = stem_alpha; stem.stem_beta = stem_beta;
    float* const bufs[3] = {static_cast<float*>(m0.p), static_cast<float*>(m1.p), static_cast<float*>(m2.p)};
    int h = F, w = W;
    const float* r = sd::fcm_block_pair(rb, bufs, bufs[0], true, B, h, w, stem, st);
    SD_HIP(hipMemcpyAsync(out, r, (size_t)B * Ho * W * 64, hipMemcpyDeviceToDevice, st));
  });
}

int sd_op_mha_block(const void* y, const float* w, const float* bias, int nseq, int T, const int* key_len, void* out,
                    int variant, int flags, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(nseq >= 1 && sd::mha_block_supported(384, 8, T, true), sd::kErrInvalid, "mha_block: unsupported shape");
    SD_CHECK(flags >= 0 && flags <= 3, sd::kErrInvalid, "mha_block: flags");
    PackedScratch wt(w, 3 * 384, 384, 1, true, st);
    sd::MhaBlockArgs m;
    m.y = y; m.W = wt.p; m.bias = bias; m.out = out; m.ldo = 384;
    m.S = nseq; m.T = T; m.D = 384; m.nh = 8; m.scale = 1.f / std::sqrt(48.f); m.key_len = key_len;
    m.y_tiled = flags & 1;     // y in RowProgArgs::a_tiled's fragment layout (what the FFN programs hand over)
    m.out_tiled = (flags >> 1) & 1;   // the output in that layout (what the out-projection program reads)
    sd::mha_block(m, st, variant);
  });
}

int sd_op_glu_dwconv(const void* x, int nseq, int T, int C, const float* w, const float* bias, int k, int glu_in,
                     int io_bf16, int mode, const float* gn_g, const float* gn_b, void* y, float* partial,
                     void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && w && y && nseq >= 1 && T >= 1 && C >= 16, sd::kErrInvalid, "glu_dwconv: bad argument");
    SD_CHECK(mode >= 0 && mode <= 2, sd::kErrInvalid, "glu_dwconv: mode must be 0, 1 or 2");
    SD_CHECK(mode == 0 || partial, sd::kErrInvalid, "glu_dwconv: modes 1 and 2 need the partial sums buffer");
    SD_CHECK(mode != 2 || (gn_g && gn_b), sd::kErrInvalid, "glu_dwconv: mode 2 needs gn_g / gn_b");
    // which kernel runs is glu_dwconv's own decision from the shape, as in the product
    sd::glu_dwconv(x, nseq, T, C, w, bias, k, y, mode == 0 ? nullptr : partial, mode == 0, glu_in != 0, io_bf16 != 0,
                   st);
    if (mode == 2) sd::groupnorm_silu(y, nseq, T, C, partial, gn_g, gn_b, 1e-5f, io_bf16 != 0, st);
  });
}

int sd_op_rowprog(const sd_rowprog_op* op, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    constexpr int D = 384;
    SD_CHECK(op && op->M >= 1 && op->flags >= 0 && op->flags <= 15, sd::kErrInvalid, "rowprog: bad argument");
    SD_CHECK(op->Xo || op->yt, sd::kErrInvalid, "rowprog: no output");
    SD_CHECK((op->X != nullptr) != (op->ts != nullptr), sd::kErrInvalid, "rowprog: exactly one of X and ts");
    SD_CHECK(!op->ts || (op->mix && op->NS > 0 && op->T_seq > 0 && op->Tmix > 0 && op->ldmix >= D / 2 &&
                         op->M % (op->NS * op->T_seq) == 0),
             sd::kErrInvalid, "rowprog: speaker source arguments");
    SD_CHECK(!op->yt || (op->yt_NS > 0 && op->T_seq > 0 && op->M % (op->yt_NS * op->T_seq) == 0), sd::kErrInvalid,
             "rowprog: speaker sink arguments");
    SD_CHECK((op->w0 != nullptr) == (op->A != nullptr) && (op->w0 != nullptr) == (op->b0 != nullptr), sd::kErrInvalid,
             "rowprog: A, w0 and b0 go together");
    SD_CHECK(!op->gn_partial || (op->w0 && op->gn_g && op->gn_b && op->gn_T > 0 && op->gn_nblk >= 1 &&
                                 op->M % op->gn_T == 0),
             sd::kErrInvalid, "rowprog: GroupNorm-on-load arguments");
    SD_CHECK(op->n_ffn >= 0 && op->n_ffn <= 2, sd::kErrInvalid, "rowprog: n_ffn");
    SD_CHECK((op->y != nullptr) == (op->y_g != nullptr) && (op->y != nullptr) == (op->y_b != nullptr), sd::kErrInvalid,
             "rowprog: y, y_g and y_b go together");
    for (int i = 0; i < op->n_ffn; ++i) {
      const sd_rowprog_ffn& f = op->ffn[i];
      SD_CHECK(f.ln_g && f.ln_b && f.w1 && f.b1 && f.w2 && f.b2 && sd::rowprog_supported(D, f.hidden, true) &&
                   (f.post_g != nullptr) == (f.post_b != nullptr),
               sd::kErrInvalid, "rowprog: ffn arguments");
    }
    SD_HIP(hipStreamSynchronize(st));
    auto host = [](const float* d, size_t n) {
      std::vector<float> h(n);
      SD_HIP(hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost));
      return h;
    };
    std::vector<std::unique_ptr<Scratch>> keep;   // the packed pieces, freed once the stream has drained
    auto put = [&](const void* h, size_t bytes) -> const void* {
      keep.emplace_back(new Scratch(bytes, st));
      SD_HIP(hipMemcpy(keep.back()->p, h, bytes, hipMemcpyHostToDevice));
      return keep.back()->p;
    };
    sd::RowProgArgs r;
    r.M = op->M;
    r.X = op->X; r.Xo = op->Xo;
    r.x_ts = op->ts; r.x_mix = op->mix; r.x_ldmix = op->ldmix; r.x_Tmix = op->Tmix; r.x_NS = op->NS;
    r.T_seq = op->T_seq;
    r.yt = op->yt; r.yt_NS = op->yt_NS;
    if (op->w0) {
      const std::vector<uint16_t> p = sd::rowprog_pack_pre(host(op->w0, (size_t)D * D), D, D);
      r.w0 = put(p.data(), p.size() * 2);
      r.A = op->A; r.b0 = op->b0;
    }
    if (op->gn_partial) {
      r.gn_partial = op->gn_partial; r.gn_nblk = op->gn_nblk; r.gn_T = op->gn_T; r.gn_g = op->gn_g; r.gn_b = op->gn_b;
    }
    r.n_ffn = op->n_ffn;
    for (int i = 0; i < op->n_ffn; ++i) {
      const sd_rowprog_ffn& f = op->ffn[i];
      const size_t hd = (size_t)f.hidden;
      std::vector<float> b1;
      // W2 / b2 as the kernel consumes them: the caller has folded the module's 1/2, nothing is scaled here
      const std::vector<uint16_t> p = sd::rowprog_pack_ffn(host(f.w1, hd * D), host(f.w2, D * hd), f.hidden,
                                                           host(f.ln_g, D), host(f.ln_b, D), host(f.b1, hd), b1);
      r.ffn[i].w = put(p.data(), p.size() * 2);
      r.ffn[i].hidden = f.hidden;
      r.ffn[i].b1 = static_cast<const float*>(put(b1.data(), b1.size() * sizeof(float)));
      r.ffn[i].b2 = f.b2;
      r.ffn[i].post_g = f.post_g; r.ffn[i].post_b = f.post_b;
    }
    r.y = op->y; r.y_g = op->y_g; r.y_b = op->y_b;
    r.x_tiled = op->flags & 1; r.xo_tiled = (op->flags >> 1) & 1;
    r.a_tiled = (op->flags >> 2) & 1; r.y_tiled = (op->flags >> 3) & 1;
    // the profiler name the conformer stack gives a program of this structure (encoder.cpp run_conformer_stack)
    const char* name = op->w0 ? (op->n_ffn ? "rowprog_pw2_ffn" : "rowprog_out")
                              : (op->n_ffn == 1 ? "rowprog_ffn" : "rowprog");
    sd::rowprog(r, name, st);
  });
}

int sd_debug_conformer_wide_route(int route) {
  return guard([&] {
    SD_CHECK(route == 0 || route == 1, sd::kErrInvalid, "conformer wide route must be 0 or 1");
    sd::conformer_wide_route_debug(route);
  });
}

int sd_op_conformer_stack(const float* x, int nseq, int T, const float* weights, int64_t n_weights, int n_layers,
                          int ffn_dim, int nh, int kernel, int group_norm, const int* key_len, int precision,
                          int use_generic, const float* ts, const float* mix, int ldmix, int Tmix, int NS, void* out,
                          void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    constexpr int E = 384;
    SD_CHECK(weights && out && nseq >= 1 && T >= 1 && n_layers >= 1 && ffn_dim >= 8 && ffn_dim % 8 == 0 && nh >= 1 &&
                 E % nh == 0 && kernel >= 1 && kernel % 2 == 1,
             sd::kErrInvalid, "conformer_stack: bad argument");
    SD_CHECK(precision >= 0 && precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
    const bool spk = ts != nullptr;
    SD_CHECK(spk ? (mix && !x && NS >= 1 && nseq % NS == 0 && Tmix >= 1 && ldmix >= E / 2 && ldmix % 4 == 0) : x != nullptr,
             sd::kErrInvalid, "conformer_stack: x, or the speaker streams ts / mix / NS / Tmix / ldmix");
    const sd::GemmX3Scope x3(precision == 2);
    const bool bf = precision == 1;
    const int64_t F = ffn_dim;
    // the flat blob's key order, per layer (torchaudio ConformerLayer's state_dict order)
    std::vector<std::pair<std::string, std::vector<int64_t>>> order;
    auto add_ffn = [&](const std::string& f) {
      order.push_back({f + ".sequential.0.weight", {E}});
      order.push_back({f + ".sequential.0.bias", {E}});
      order.push_back({f + ".sequential.1.weight", {F, E}});
      order.push_back({f + ".sequential.1.bias", {F}});
      order.push_back({f + ".sequential.4.weight", {E, F}});
      order.push_back({f + ".sequential.4.bias", {E}});
    };
    add_ffn("ffn1");
    order.push_back({"self_attn_layer_norm.weight", {E}});
    order.push_back({"self_attn_layer_norm.bias", {E}});
    order.push_back({"self_attn.in_proj_weight", {3 * E, E}});
    order.push_back({"self_attn.in_proj_bias", {3 * E}});
    order.push_back({"self_attn.out_proj.weight", {E, E}});
    order.push_back({"self_attn.out_proj.bias", {E}});
    order.push_back({"conv_module.layer_norm.weight", {E}});
    order.push_back({"conv_module.layer_norm.bias", {E}});
    order.push_back({"conv_module.sequential.0.weight", {2 * E, E, 1}});
    order.push_back({"conv_module.sequential.0.bias", {2 * E}});
    order.push_back({"conv_module.sequential.2.weight", {E, 1, kernel}});
    order.push_back({"conv_module.sequential.2.bias", {E}});
    order.push_back({"conv_module.sequential.3.weight", {E}});
    order.push_back({"conv_module.sequential.3.bias", {E}});
    if (!group_norm) {
      order.push_back({"conv_module.sequential.3.running_mean", {E}});
      order.push_back({"conv_module.sequential.3.running_var", {E}});
    }
    order.push_back({"conv_module.sequential.5.weight", {E, E, 1}});
    order.push_back({"conv_module.sequential.5.bias", {E}});
    add_ffn("ffn2");
    order.push_back({"final_layer_norm.weight", {E}});
    order.push_back({"final_layer_norm.bias", {E}});
    auto numel = [](const std::vector<int64_t>& s) {
      int64_t n = 1;
      for (int64_t d : s) n *= d;
      return n;
    };
    int64_t per_layer = 0;
    for (const auto& k : order) per_layer += numel(k.second);
    SD_CHECK(n_weights == n_layers * per_layer, sd::kErrInvalid,
             "conformer_stack: weights must hold " + std::to_string(n_layers * per_layer) + " floats");
    std::vector<float> host((size_t)n_weights);
    SD_HIP(hipStreamSynchronize(st));
    SD_HIP(hipMemcpy(host.data(), weights, host.size() * sizeof(float), hipMemcpyDeviceToHost));
    sd::ParamStore ps;
    const float* wp = host.data();
    for (int i = 0; i < n_layers; ++i)
      for (const auto& k : order) {
        ps.set("conformer_layers." + std::to_string(i) + "." + k.first, wp, k.second.data(), (int)k.second.size());
        wp += numel(k.second);
      }
    sd::DeviceArena arena;   // freed on return, after the stream has drained
    sd::LayerLoader loader{ps, arena, bf};
    std::vector<sd::ConformerL> Ls;
    for (int i = 0; i < n_layers; ++i) Ls.push_back(loader.conformer("conformer_layers." + std::to_string(i), group_norm != 0));
    ps.require_all_used();
    const int64_t rows = (int64_t)nseq * T;
    SD_CHECK(rows * std::max<int64_t>(ffn_dim, 3 * E) < (int64_t)1 << 31, sd::kErrInvalid, "conformer_stack: too many rows");
    auto ws = [&](int64_t n) { return static_cast<float*>(arena.alloc((size_t)n * sizeof(float))); };
    sd::EncoderWork w;
    w.Y = ws(rows * E);
    w.QKV = ws(rows * 3 * E);
    w.AO = ws(rows * E);
    w.H = ws(rows * std::max(ffn_dim, 2 * E));
    w.partial = ws((int64_t)nseq * ((E + 63) / 64) * 2);
    w.bf16 = bf;
    w.split_k = false;
    if (spk) {
      SD_CHECK(!use_generic && sd::conformer_stack_fused(Ls, E, bf), sd::kErrInvalid,
               "conformer_stack: the speaker streams need the fused stack (precision 1, use_generic 0)");
      sd::SpeakerStreams io;
      io.ts = ts; io.mix = mix; io.ldmix = ldmix; io.Tmix = Tmix; io.NS = NS; io.out = out;
      sd::run_conformer_stack(Ls, ws(rows * E), nseq, T, E, nh, kernel, key_len, w, st, &io);
    } else {
      float* X = static_cast<float*>(out);
      SD_HIP(hipMemcpyAsync(X, x, (size_t)rows * E * sizeof(float), hipMemcpyDeviceToDevice, st));
      if (use_generic) {
        for (const sd::ConformerL& L : Ls) sd::run_conformer(L, X, nseq, T, E, nh, kernel, key_len, w, st);
      } else {
        SD_CHECK(sd::conformer_stack_fused(Ls, E, bf), sd::kErrInvalid,
                 "conformer_stack: use_generic 0 needs the row programs (precision 1, ffn_dim % 32 == 0, <= 1536)");
        sd::run_conformer_stack(Ls, X, nseq, T, E, nh, kernel, key_len, w, st);
      }
    }
    SD_HIP(hipStreamSynchronize(st));
  });
}

int sd_op_conv1d(const float* x, int B, int T, int Cin, const float* w, const float* b, int Cout,
                 int k, int stride, int pad, int dil, int act, float* out, int precision,
                 void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    const bool bf = precision >= 1;
    PackedScratch wt(w, Cout, Cin, k, bf, st);
    Activations xa(x, (int64_t)B * T * Cin, precision, st);
    sd::ConvGemmArgs p;
    p.A = xa.a; p.a_bf16 = xa.bf16; p.B = B; p.H = 1; p.W = T; p.Cin = Cin; p.lda = Cin;
    p.kh = 1; p.kw = k; p.sw = stride; p.pw = pad; p.dw = dil;
    p.Ho = 1; p.Wo = (T + 2 * pad - dil * (k - 1) - 1) / stride + 1;
    SD_CHECK(p.Wo > 0, sd::kErrInvalid, "conv1d: empty output");
    p.Wt = wt.p; p.N = Cout; p.K = Cin * k;
    p.beta = b; p.act = act;
    p.out = out; p.o_sb = (int64_t)p.Wo * Cout; p.o_sw = Cout; p.o_sn = 1;
    sd::conv_gemm(p, bf, st);
  });
}

int sd_op_conv2d(const float* x, int B, int H, int W, int Cin, const float* w, int Cout, int kh,
                 int kw, int sh, int sw, int ph, int pw, float* out, int precision, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    const bool bf = precision >= 1;
    PackedScratch wt(w, Cout, Cin, kh * kw, bf, st);
    Activations xa(x, (int64_t)B * H * W * Cin, precision, st);
    sd::ConvGemmArgs p;
    p.A = xa.a; p.a_bf16 = xa.bf16; p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.lda = Cin;
    p.kh = kh; p.kw = kw; p.sh = sh; p.sw = sw; p.ph = ph; p.pw = pw;
    p.Ho = (H + 2 * ph - kh) / sh + 1;
    p.Wo = (W + 2 * pw - kw) / sw + 1;
    p.Wt = wt.p; p.N = Cout; p.K = Cin * kh * kw;
    p.out = out; p.o_sb = (int64_t)p.Ho * p.Wo * Cout; p.o_sh = (int64_t)p.Wo * Cout; p.o_sw = Cout;
    p.o_sn = 1;
    sd::conv_gemm(p, bf, st);
  });
}

int sd_op_res_conv(const void* x, int B, int H, int W, int Cin, const float* w, int Cout, int stride,
                   const float* alpha, const float* beta, const void* res, const float* sc_w, const float* sc_alpha,
                   const float* sc_beta, void* out, void* sc_out, int use_generic, void* stream) {
  return guard([&] {
    hipStream_t st = S(stream);
    SD_CHECK(x && w && out && B > 0 && H > 0 && W > 0 && (stride == 1 || stride == 2), sd::kErrInvalid,
             "res_conv: bad argument");
    SD_CHECK(!sc_w || (sc_alpha && sc_beta && sc_out), sd::kErrInvalid, "res_conv: incomplete shortcut");
    PackedScratch wt(w, Cout, Cin, 9, true, st), swt(sc_w, Cout, Cin, 1, true, st);   // sc_w: nullable
    sd::ConvGemmArgs p;
    p.A = x; p.a_bf16 = true; p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.lda = Cin;
    p.kh = 3; p.kw = 3; p.sh = stride; p.sw = stride; p.ph = 1; p.pw = 1;
    p.Ho = (H - 1) / stride + 1;
    p.Wo = (W - 1) / stride + 1;
    p.Wt = wt.p; p.N = Cout; p.K = 9 * Cin;
    p.alpha = alpha; p.beta = beta; p.act = sd::kActRelu;
    p.res = res; p.res_bf16 = true; p.res_ld = Cout;
    p.out = out; p.out_bf16 = true;
    p.o_sb = (int64_t)p.Ho * p.Wo * Cout; p.o_sh = (int64_t)p.Wo * Cout; p.o_sw = Cout; p.o_sn = 1;
    if (!use_generic) {
      sd::ResFuse f;
      if (sc_w) { f.sc_w = swt.p; f.sc_alpha = sc_alpha; f.sc_beta = sc_beta; f.sc_out = sc_out; }
      sd::res_conv3x3(p, f, st);   // raises on arguments the kernel cannot compute
      return;
    }
    sd::conv_gemm(p, true, st);
    if (sc_w) {
      sd::ConvGemmArgs q = p;
      q.kh = 1; q.kw = 1; q.ph = 0; q.pw = 0; q.Wt = swt.p; q.K = Cin;
      q.alpha = sc_alpha; q.beta = sc_beta; q.act = sd::kActNone; q.res = nullptr; q.out = sc_out;
      sd::conv_gemm(q, true, st);
    }
  });
}

namespace {
void op_attention(const float* qkv, int S_, int T, int D, int nh, int causal, int causal_delay, const int* key_len,
                  int chunk, int left, float* out, int precision, hipStream_t st, int* mask_dump = nullptr,
                  int grid_c = 0, float scale = 0.f) {
  SD_CHECK(precision >= 0 && precision <= 2, sd::kErrInvalid, "precision must be 0, 1 or 2");
  sd::AttnArgs a;
  a.qkv = qkv; a.S = S_; a.T = T; a.D = D; a.nh = nh; a.ld_qkv = 3 * D;
  a.out = out; a.ldo = D; a.scale = scale > 0.f ? scale : 1.f / std::sqrt((float)(D / nh));
  a.causal = causal; a.causal_delay = causal_delay; a.key_len = key_len;
  a.chunk = chunk; a.left = left;
  a.mask_dump = mask_dump;
  if (grid_c > 0) {   // time attention over a (S/C, T, C) token grid: sequence (s, c) walks tokens with stride C
    a.seq_inner = grid_c; a.seq_outer = (int64_t)T * grid_c; a.seq_inner_stride = 1; a.tok_stride = grid_c;
  }
  if (precision == 2) {   // bf16 storage: qkv and out in bf16 (the encoders' layout)
    Scratch qb((size_t)S_ * T * 3 * D * 2, st), ob((size_t)S_ * T * D * 2, st);
    sd::f32_to_bf16(qkv, (int64_t)S_ * T * 3 * D, qb.p, st);
    a.qkv = qb.p; a.out = ob.p; a.io_bf16 = true;
    sd::attention(a, true, st);
    sd::bf16_to_f32(ob.p, (int64_t)S_ * T * D, out, st);
    return;
  }
  sd::attention(a, precision == 1, st);
}
}  // namespace

int sd_op_attention(const float* qkv, int S_, int T, int D, int nh, int causal, int causal_delay,
                    const int* key_len, float* out, int precision, void* stream) {
  return guard([&] { op_attention(qkv, S_, T, D, nh, causal, causal_delay, key_len, 0, -1, out, precision, S(stream)); });
}

int sd_op_attention_scaled(const float* qkv, int S_, int T, int D, int nh, float scale, float* out, int precision,
                           void* stream) {
  return guard([&] {
    SD_CHECK(qkv && out && scale > 0.f, sd::kErrInvalid, "attention_scaled: bad argument");
    op_attention(qkv, S_, T, D, nh, 0, 0, nullptr, 0, -1, out, precision, S(stream), nullptr, 0, scale);
  });
}

int sd_op_attention_grid(const float* qkv, int S_, int T, int C, int D, int nh, int causal, int causal_delay,
                         float* out, int precision, void* stream) {
  return guard([&] {
    SD_CHECK(S_ >= 1 && C >= 1 && T >= 1, sd::kErrInvalid, "attention_grid: empty grid");
    op_attention(qkv, S_ * C, T, D, nh, causal, causal_delay, nullptr, 0, -1, out, precision, S(stream), nullptr, C);
  });
}

int sd_op_attention_chunk(const float* qkv, int S_, int T, int D, int nh, int chunk, int left, float* out,
                          int precision, void* stream) {
  return guard([&] {
    SD_CHECK(chunk > 0, sd::kErrInvalid, "decoding chunk must be > 0");
    op_attention(qkv, S_, T, D, nh, 0, 0, nullptr, chunk, left, out, precision, S(stream));
  });
}

int sd_probe_attention_mask(const float* qkv, int S_, int T, int D, int nh, int causal, int causal_delay,
                            const int* key_len, int chunk, int left, int* mask_dump, float* out,
                            int precision, void* stream) {
  return guard([&] {
    SD_CHECK(mask_dump != nullptr, sd::kErrInvalid, "mask_dump is required");
    op_attention(qkv, S_, T, D, nh, causal, causal_delay, key_len, chunk, left, out, precision, S(stream),
                 mask_dump);
  });
}

int sd_op_layernorm(const float* x, int rows, int D, const float* g, const float* b, float eps,
                    float* y, void* stream) {
  return guard([&] { sd::layernorm(x, rows, D, D, g, b, eps, y, D, false, S(stream)); });
}

int sd_op_add_layernorm(float* x, const void* t, int t_bf16, int rows, int D, const float* g, const float* b,
                        float eps, int write_x, void* y, int y_bf16, void* stream) {
  return guard([&] {
    sd::add_layernorm(x, t, t_bf16 != 0, rows, D, g, b, eps, write_x != 0, y, y_bf16 != 0, S(stream));
  });
}

int sd_op_lstm(const float* gx, int B, int T, int H, int ndir, const float* whh, const int* lengths,
               float* out, float* hT, float* cT, float* work, void* stream) {
  return guard([&] {
    sd::lstm_recurrence(gx, B, T, H, ndir, whh, lengths, nullptr, nullptr, out, ndir * H, hT, cT,
                        work, S(stream));
  });
}

}  // extern "C"
