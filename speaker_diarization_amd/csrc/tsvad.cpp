// Native TS-VAD forward (egs/alimeeting/ts_vad2/model.py) on gfx950.
//
// TsvadModel::forward is one path for every variant:
//   ref_speech fbank (B, T_fb, 80)
//     -> speech encoder trunk (trunk_forward), over the batch or as two window slices on two streams (run_sliced)
//          variants 0, 1: CAM++ FCM head + xvector[:-2]       cam_pplus_wespeaker.py:271-399
//          variant 2 (speech_encoder_type resnet34_wespeaker, model.py:584-606): ResNet34 trunk (resnet.h)
//          variant 3 (ecapa_channel_1024_wespeaker, model.py:631-654): ECAPA-TDNN trunk (ecapa.h)
//          variant 4 (ReDimNetB2, egs/magicdata-ramc/ts_vad2/model.py:694-715): ReDimNetB2 trunk on 72-bin fbank
//                    (redimnet.h), get_frame_level_feat (:1246-1262)
//          variants 5, 6 (WavLM / WavLM_weight_sum, magicdata model.py:867-927, 1171-1204): ref_speech is the raw
//                    waveform (B, n_samples); the WavLM trunk (wavlm.h) on the caller's stream; 6 accumulates the
//                    layer-weighted sum as the layers run, then wavlmproj + wavlmlnorm in one kernel
//          variant 8 (whisper, magicdata model.py:928-955, 1216-1223): ref_speech is the raw waveform; the Whisper-PMFA
//                    trunk (whisper.h) on the caller's stream, its ln_post2 output the conv's A operand
//          variant 7 (w2v-bert2, magicdata model.py:805-840, 1225-1237): ref_speech (B, T, 80) read as (B, T / 2, 160)
//                    (a plain reshape: the same memory); the w2v-BERT 2.0 trunk (w2vbert.h) on the caller's stream
//     -> speech_down_or_up (down_gemm) -> mix (B, T3, SE)
//          frame_level_gsp ("CAM++_frame_level_gsp_fc", magicdata model.py:543-563, 1275-1287; variant 0's trunk): frame
//          mean / std over the channels + gsp_fc + the conv as one folded gsp_down launch instead
//          variants 0, 1: conv + BN + ReLU                    model.py:385-395 / 406-416
//          variant 2: SpeechFeatUpsample2 transposed conv + BN + ReLU (model.py:114-134)
//          variants 3, 4: conv k5 stride 4 pad 2 + BN + ReLU (model.py:641-654; magicdata :703-715)
//          variants 5, 6: conv k5 stride 2 pad 2 + BN + ReLU (magicdata :879-889, 913-927)
//          variant 7: the same conv on 1024 channels (magicdata :830-840)
//          variant 8: the same conv on n_audio_state * n_cat channels (10240 published; magicdata :945-955)
//     -> transformer_backend, variants 0, 2, 3 and 4 (forward_common, model.py:758-897):
//          [ts_embed | mix] + PE, 2-layer transformer per speaker (batched over speakers)
//          -> backend_down conv(1536->384, k5)+BN+ReLU -> PE -> 2-layer transformer -> fc
//          backend 1 / 2 (variant 0; egs/magicdata-ramc/ts_vad2/model.py:377-403, 488-504, 1337-1399): the per-speaker
//          encoder, and with 2 the multi-speaker one (+ multi_backend_proj), is a bidirectional Mamba2BlockV2 (mamba2.h)
//          that scans along the WINDOWS of a reference forward call; backend_down reads 2 E NS channels
//          backend 4 / 5 (variant 0; magicdata model.py:290-313, 451-463, 1340-1351, 1382-1390): the per-speaker encoder,
//          and with 5 the multi-speaker one, is a torchaudio Conformer (BatchNorm conv module, kernel 31) along time
//        ots_vad_backend, variant 1 (forward_common_ots_vad, model.py:669-756):
//          GSP + gsp_fc -> [ts_embed | mix] -> 6-layer Conformer per speaker (conformer_slice: the fused stack,
//          which runs inside each window slice) -> BiLSTM(1536 -> 2x256) -> fc
//   -> logits (B, NS, T_lab)
// All activations are fp32 channel-last; every contraction is conv_gemm (bf16 or
// exact-f32 MFMA), eval BatchNorms are folded into GEMM prologues/epilogues.
#include "tsvad.h"
#include "prof.h"

#include <algorithm>
#include <cmath>

namespace sd {

ConvL TsvadModel::conv_bn(const std::string& wname, const std::string& bn, const std::string& bias) {
  return load_conv_bn(ps_, arena_, cfg_.bf16, wname, bn, bias);
}

void TsvadModel::validate(const TsvadConfig& c) {
  SD_CHECK(c.backend >= 0 && c.backend <= 5 && c.backend != 3, kErrInvalid, "backend must be 0, 1, 2, 4 or 5");
  if (c.backend == 1 || c.backend == 2) {
    SD_CHECK(c.variant == 0, kErrInvalid,
             "backend 1 / 2 (Mamba2 back ends) is built for variant 0 (speech_encoder_type CAM++) only");
    Mamba2Stack::validate(c.embed_dim, c.d_state, c.expand);
  }
  if (c.backend == 4 || c.backend == 5)   // d_state / expand are not read
    SD_CHECK(c.variant == 0, kErrInvalid,
             "backend 4 / 5 (conformer back ends) is built for variant 0 (speech_encoder_type CAM++) only");
  if (c.frame_level_gsp) {   // any of variant 0's back ends
    SD_CHECK(c.variant == 0, kErrInvalid,
             "frame_level_gsp (speech_encoder_type CAM++_frame_level_gsp_fc) is built on variant 0 (the CAM++ trunk with "
             "the transformer, Mamba2 or conformer back ends) only");
    SD_CHECK(c.speaker_embed_dim % 32 == 0, kErrInvalid,
             "frame_level_gsp: speaker_embed_dim must be a multiple of 32");
  }
  if (c.variant == 5 || c.variant == 6) {
    SD_CHECK(c.backend == 0, kErrInvalid,
             "the WavLM speech encoders (variants 5 / 6) are built with the transformer back end only (backend 0)");
    SD_CHECK(c.wavlm_embed_dim == 768 || c.wavlm_embed_dim == 1024, kErrInvalid,
             "variants 5 / 6 need the WavLM geometry: wavlm_embed_dim must be 768 or 1024");
    SD_CHECK(c.wavlm_layers >= 1 && c.wavlm_layers <= 24, kErrInvalid, "wavlm_layers must be 1..24");
    SD_CHECK(c.wavlm_layer_norm_mode == c.wavlm_pre_ln, kErrInvalid,
             "WavLM (MI355X backend) builds (extractor_mode, layer_norm_first) = (0 default, 0) or (1 layer_norm, 1) only");
    SD_CHECK(c.max_samples >= WavlmTrunk::kMinSamples, kErrInvalid, "max_samples must be at least 400");
    SD_CHECK((int64_t)c.max_batch * WavlmTrunk::frames(c.max_samples) * (c.wavlm_embed_dim * 4) < (1ll << 31) &&
                 (int64_t)std::min(c.max_batch, WavlmTrunk::kSlice) * (c.max_samples / 5) * 512 < (1ll << 31),
             kErrInvalid, "max_batch * frames(max_samples) * ffn_dim must be below 2^31");
    SD_CHECK(c.variant != 6 || c.speaker_embed_dim == 192 || c.speaker_embed_dim == 256, kErrInvalid,
             "WavLM_weight_sum (variant 6) is built for speaker_embed_dim 192 or 256");
    SD_CHECK(c.speaker_embed_dim % 32 == 0, kErrInvalid, "variants 5 / 6: speaker_embed_dim must be a multiple of 32");
  }
  if (c.variant == 8) {
    SD_CHECK(c.backend == 0, kErrInvalid,
             "the whisper speech encoder (variant 8) is built with the transformer back end only (backend 0)");
    SD_CHECK(c.max_samples >= WhisperTrunk::kMinSamples, kErrInvalid, "max_samples must be at least 400");
    SD_CHECK(c.speaker_embed_dim % 32 == 0, kErrInvalid, "variant 8: speaker_embed_dim must be a multiple of 32");
  }
  if (c.variant == 7) {
    SD_CHECK(c.backend == 0, kErrInvalid,
             "the w2v-bert2 speech encoder (variant 7) is built with the transformer back end only (backend 0)");
    SD_CHECK(c.w2vbert_layers >= 1 && c.w2vbert_layers <= 24, kErrInvalid,
             "variant 7 (w2v-bert2): w2vbert_layers must be 1..24");
    SD_CHECK(c.max_fbank_frames >= 2, kErrInvalid, "variant 7: max_fbank_frames must be at least 2");
    SD_CHECK((int64_t)c.max_batch * (c.max_fbank_frames / 2) * W2vBertTrunk::kFfn < (1ll << 31), kErrInvalid,
             "max_batch * (max_fbank_frames / 2) * 4096 must be below 2^31");
    SD_CHECK(c.speaker_embed_dim % 32 == 0, kErrInvalid, "variant 7: speaker_embed_dim must be a multiple of 32");
  }
  if (c.speaker_embed_dim * 2 == c.embed_dim) return;
  // proj_layer = nn.Linear(2 SE, E) on cat(ts_embed, mix_embeds) (model.py:212-217, 873-874)
  SD_CHECK(c.variant != 1, kErrInvalid,
           "speaker_embed_dim*2 != transformer_embed_dim needs proj_layer, which the reference's ots_vad forward "
           "never applies (model.py:730-731 is commented out; its conformer then fails on the 2*speaker_embed_dim "
           "wide input): not supported for ots_vad_style v1");
  SD_CHECK(speaker_input_proj_supported(c.speaker_embed_dim, c.embed_dim), kErrInvalid,
           "proj_layer: speaker_embed_dim and transformer_embed_dim must be multiples of 8");
}

// One layer of a backend 4 / 5 Conformer, its shapes held to the configuration the workspace was sized for.
ConformerL TsvadModel::conformer_layer(const std::string& p) {
  const int E = cfg_.embed_dim, F = cfg_.ffn_dim;
  const ConformerL L = loader().conformer(p, false);
  const HostTensor& dw = ps_.get(p + ".conv_module.sequential.2.weight");
  SD_CHECK(dw.shape[0] == E && dw.shape[2] == kConformerKernel, kErrParam,
           p + ".conv_module.sequential.2.weight must be (transformer_embed_dim, 1, 31)");
  SD_CHECK(L.f1_w1.N == F && L.f1_w1.K == E && L.f2_w1.N == F && L.f2_w1.K == E && L.f1_w2.N == E && L.f1_w2.K == F &&
               L.f2_w2.N == E && L.f2_w2.K == F,
           kErrParam, p + ".ffn1 / ffn2 must be Linear(transformer_embed_dim, transformer_ffn_embed_dim) and back");
  SD_CHECK(L.in_proj.N == 3 * E && L.in_proj.K == E && L.out_proj.N == E && L.out_proj.K == E && L.pw1.N == 2 * E &&
               L.pw1.K == E && L.pw2.N == E && L.pw2.K == E,
           kErrParam, p + ": self_attn / conv_module weights must be transformer_embed_dim wide");
  return L;
}

void TsvadModel::build() {
  validate(cfg_);
  const std::string se = "speech_encoder.";
  if (cfg_.variant == 2) {
    res_ = std::make_unique<ResTrunk>();
    res_->load(ps_, arena_, se, cfg_.bf16);   // resnet_wespeaker.py:108-171
  } else if (cfg_.variant == 3) {
    ecapa_ = std::make_unique<EcapaTrunk>();
    ecapa_->load(ps_, arena_, se, cfg_.bf16);   // ecapa_tdnn_wespeaker.py:161-209 (no pool / bn / linear keys)
  } else if (cfg_.variant == 8) {
    // WhisperEncoder(ModelDimensions) under speech_encoder.* (magicdata model.py:936-943)
    WhisperConfig w = cfg_.whisper;
    w.max_batch = cfg_.max_batch;
    w.max_samples = cfg_.max_samples;
    w.bf16 = cfg_.bf16;
    whisper_ = std::make_unique<WhisperTrunk>(w);
    whisper_->load(ps_, arena_, se);
  } else if (waveform()) {
    // WavLM(wavlm_cfg) with encoder_layers = select_encoder_layer_nums (5) or the checkpoint's (6)
    // (magicdata model.py:867-877, 890-899)
    WavlmConfig w;
    w.embed_dim = cfg_.wavlm_embed_dim;
    w.ffn_dim = 4 * w.embed_dim;
    w.heads = w.embed_dim / 64;
    w.layers = cfg_.wavlm_layers;
    w.layer_norm_mode = cfg_.wavlm_layer_norm_mode;
    w.pre_ln = cfg_.wavlm_pre_ln;
    w.max_batch = cfg_.max_batch;
    w.max_samples = cfg_.max_samples;
    w.bf16 = cfg_.bf16;
    w.split_k = false;   // windows are sharded over ranks: no row-count-dependent summation order
    wavlm_ = std::make_unique<WavlmTrunk>(w);
    wavlm_->load(ps_, arena_, se);
    if (cfg_.variant == 6) {
      // weights = Linear(L, 1, bias=False), wavlmproj = Linear(D, SE), wavlmlnorm = LayerNorm(SE) (:904-909)
      const HostTensor& mw = ps_.get("weights.weight");
      SD_CHECK(mw.shape.size() == 2 && mw.shape[0] == 1 && mw.shape[1] == cfg_.wavlm_layers, kErrParam,
               "weights.weight must be (1, wavlm encoder layers)");
      mix_w_ = mw.data;
      wproj_ = loader().linear("wavlmproj");
      SD_CHECK(wproj_.w.N == cfg_.speaker_embed_dim && wproj_.w.K == cfg_.wavlm_embed_dim, kErrParam,
               "wavlmproj.weight must be (speaker_embed_dim, wavlm embed dim)");
      SD_CHECK(ps_.get("wavlmproj.bias").numel() == cfg_.speaker_embed_dim, kErrParam, "wavlmproj.bias size");
      SD_CHECK(ps_.get("wavlmlnorm.weight").numel() == cfg_.speaker_embed_dim &&
                   ps_.get("wavlmlnorm.bias").numel() == cfg_.speaker_embed_dim, kErrParam, "wavlmlnorm size");
      wln_g_ = arena_.upload(ps_.get("wavlmlnorm.weight").data);
      wln_b_ = arena_.upload(ps_.get("wavlmlnorm.bias").data);
    }
  } else if (cfg_.variant == 7) {
    // Wav2Vec2BertModel with num_hidden_layers = select_encoder_layer_nums (magicdata model.py:811-824)
    W2vBertConfig w;
    w.layers = cfg_.w2vbert_layers;
    w.max_batch = cfg_.max_batch;
    w.max_frames = cfg_.max_fbank_frames / 2;
    w.bf16 = cfg_.bf16;
    w2v_ = std::make_unique<W2vBertTrunk>(w);
    w2v_->load(ps_, arena_, se);
  } else if (cfg_.variant == 4) {
    redim_ = std::make_unique<RedimTrunk>();
    redim_->load(ps_, arena_, se, cfg_.bf16);   // redimnet_wespeaker.py:623-790
    // ReDimNetB2(feat_dim=72, embed_dim=192, pooling_func="ASTP") is built whole (model.py:694-697); its pooling head
    // is not on the get_frame_level_feat path
    for (const char* k : {"pool.linear1.weight", "pool.linear1.bias", "pool.linear2.weight", "pool.linear2.bias",
                          "seg_1.weight", "seg_1.bias"})
      ps_.mark(se + k);
  } else {
    cam_ = std::make_unique<CamTrunk>();
    cam_->load(ps_, arena_, se, cfg_.bf16);   // cam_pplus_wespeaker.py:271-372
    // The pooled embedding head (stats + dense) is not on the get_time_out path.
    for (const char* k : {"xvector.dense.linear.weight", "xvector.dense.nonlinear.batchnorm.running_mean",
                          "xvector.dense.nonlinear.batchnorm.running_var"})
      ps_.mark(se + k);
  }
  // ---- speech_down_or_up (model.py:385-395)
  // BatchNorm1D (model.py:161-171) is not folded into the conv: a batch holding a NaN skips it, so the conv
  // stores conv + bias and its consumer applies BN + ReLU, or ReLU alone for such a batch (BnRelu)
  auto bn_only = [&](const std::string& bn) {
    std::vector<float> sc, sh;
    ps_.bn_fold(bn, sc, sh);
    BnRelu r;
    r.a = arena_.upload(sc);
    r.b = arena_.upload(sh);
    return r;
  };
  if (cfg_.variant == 2) {
    // SpeechFeatUpsample2.up (model.py:118-125), weight (2560, D, 5): output o = 2 i - 2 + k, so
    //   even y[2j]   = w[..4] x[j-1] + w[..2] x[j] + w[..0] x[j+1]
    //   odd  y[2j+1] =                 w[..3] x[j] + w[..1] x[j+1]
    // i.e. taps (x[j-1], x[j], x[j+1]) of a k-3 pad-1 conv with the phases stacked on the output channels
    const HostTensor& w = ps_.get("speech_down_or_up.up.weight");
    const HostTensor& ub = ps_.get("speech_down_or_up.up.bias");
    const int C = ResTrunk::kChannels, D = cfg_.speaker_embed_dim;
    SD_CHECK(w.shape.size() == 3 && w.shape[0] == C && w.shape[1] == D && w.shape[2] == 5, kErrParam,
             "speech_down_or_up.up.weight must be (2560, speaker_embed_dim, 5)");
    SD_CHECK(ub.numel() == D, kErrParam, "speech_down_or_up.up.bias size");
    std::vector<float> wt((size_t)2 * D * 3 * C, 0.f), bias((size_t)2 * D);
    const int even_k[3] = {4, 2, 0}, odd_k[3] = {-1, 3, 1};
    for (int n = 0; n < D; ++n) {
      for (int t = 0; t < 3; ++t)
        for (int c = 0; c < C; ++c) {
          const float* wc = w.data.data() + ((size_t)c * D + n) * 5;
          wt[((size_t)n * 3 + t) * C + c] = wc[even_k[t]];
          if (odd_k[t] >= 0) wt[((size_t)(D + n) * 3 + t) * C + c] = wc[odd_k[t]];
        }
      bias[n] = bias[D + n] = ub.data[n];
    }
    down_.w = upload_packed(arena_, wt, 2 * D, C, 1, 3, cfg_.bf16);
    down_.beta = arena_.upload(bias);
    down_bn_ = bn_only("speech_down_or_up.batchnorm.bn");
  } else if (cfg_.variant == 3) {
    // Conv1d(1536 -> D, k5, stride 4, pad 2) (model.py:643-650) on the trunk's ReLU output: no prologue
    down_ = conv_bn("speech_down_or_up.0.weight", "", "speech_down_or_up.0.bias");
    SD_CHECK(down_.w.N == cfg_.speaker_embed_dim && down_.w.Cin == EcapaTrunk::kChannels && down_.w.kw == 5, kErrParam,
             "speech_down_or_up.0.weight must be (speaker_embed_dim, 1536, 5)");
    SD_CHECK(ps_.get("speech_down_or_up.0.bias").numel() == cfg_.speaker_embed_dim, kErrParam,
             "speech_down_or_up.0.bias size");
    down_bn_ = bn_only("speech_down_or_up.1.bn");
  } else if (cfg_.variant == 4) {
    // Conv1d(1152 -> D, k5, stride 4, pad 2) (magicdata model.py:703-715) on the frame-level map: no prologue
    down_ = conv_bn("speech_down_or_up.0.weight", "", "speech_down_or_up.0.bias");
    SD_CHECK(down_.w.N == cfg_.speaker_embed_dim && down_.w.Cin == RedimTrunk::kChannels && down_.w.kw == 5, kErrParam,
             "speech_down_or_up.0.weight must be (speaker_embed_dim, 1152, 5)");
    SD_CHECK(ps_.get("speech_down_or_up.0.bias").numel() == cfg_.speaker_embed_dim, kErrParam,
             "speech_down_or_up.0.bias size");
    down_bn_ = bn_only("speech_down_or_up.1.bn");
  } else if (waveform() || cfg_.variant == 7) {
    // Conv1d(D -> SE, k5, stride 2, pad 2), D the WavLM width (5), speaker_embed_dim behind wavlmproj (6), w2v-BERT's
    // 1024 (7) or Whisper's n_audio_state * n_cat (8): no prologue
    const int cin = cfg_.variant == 8 ? whisper_->wide() : cfg_.variant == 7 ? W2vBertTrunk::kHidden
                    : cfg_.variant == 6 ? cfg_.speaker_embed_dim : cfg_.wavlm_embed_dim;
    down_ = conv_bn("speech_down_or_up.0.weight", "", "speech_down_or_up.0.bias");
    SD_CHECK(down_.w.N == cfg_.speaker_embed_dim && down_.w.Cin == cin && down_.w.kw == 5, kErrParam,
             "speech_down_or_up.0.weight must be (speaker_embed_dim, " + std::to_string(cin) + ", 5)");
    SD_CHECK(ps_.get("speech_down_or_up.0.bias").numel() == cfg_.speaker_embed_dim, kErrParam,
             "speech_down_or_up.0.bias size");
    down_bn_ = bn_only("speech_down_or_up.1.bn");
  } else if (cfg_.frame_level_gsp) {
    // gsp_fc = Linear(2, 256) on the per-frame (mean, std), then Conv1d(256 -> SE, k5, stride 2, pad 2) (magicdata
    // model.py:550-563): rank 2 in (mean, std), so the pair folds to 15 coefficients per output channel (gsp_down)
    const int SE = cfg_.speaker_embed_dim;
    const HostTensor& gw = ps_.get("gsp_fc.weight");
    const HostTensor& gb = ps_.get("gsp_fc.bias");
    const HostTensor& w = ps_.get("speech_down_or_up.0.weight");
    const HostTensor& cb = ps_.get("speech_down_or_up.0.bias");
    SD_CHECK(gw.shape.size() == 2 && gw.shape[0] == kGspFcDim && gw.shape[1] == 2, kErrParam,
             "gsp_fc.weight must be (256, 2)");
    SD_CHECK(gb.numel() == kGspFcDim, kErrParam, "gsp_fc.bias size");
    SD_CHECK(w.shape.size() == 3 && w.shape[0] == SE && w.shape[1] == kGspFcDim && w.shape[2] == 5, kErrParam,
             "speech_down_or_up.0.weight must be (speaker_embed_dim, 256, 5)");
    SD_CHECK(cb.numel() == SE, kErrParam, "speech_down_or_up.0.bias size");
    std::vector<float> coef;
    gsp_down_fold(gw.data.data(), gb.data.data(), w.data.data(), SE, coef);
    gsp_coef_ = arena_.upload(coef);
    gsp_cb_ = arena_.upload(cb.data);
    down_bn_ = bn_only("speech_down_or_up.1.bn");
  } else {
    down_ = conv_bn("speech_down_or_up.0.weight", "", "speech_down_or_up.0.bias");
    down_bn_ = bn_only("speech_down_or_up.1.bn");
    down_.pre_s = cam_->out_s();
    down_.pre_h = cam_->out_h();
  }

  if (transformer_variant()) {
    const HostTensor& pe = ps_.get("pos_encoder.pe");
    SD_CHECK(pe.shape.size() == 3 && pe.shape[2] == cfg_.embed_dim, kErrParam, "pos_encoder.pe shape");
    pe_len_ = (int)pe.shape[0];
    pe_ = arena_.upload(pe.data);
    if (cfg_.speaker_embed_dim * 2 != cfg_.embed_dim) {
      // proj_layer.weight (E, 2 SE) split on its input axis into [W_ts | W_mix] (speaker_input_proj)
      const int E = cfg_.embed_dim, SE = cfg_.speaker_embed_dim;
      const HostTensor& w = ps_.get("proj_layer.weight");
      const HostTensor& b = ps_.get("proj_layer.bias");
      SD_CHECK(w.shape.size() == 2 && w.shape[0] == E && w.shape[1] == 2 * SE, kErrParam,
               "proj_layer.weight must be (transformer_embed_dim, 2 * speaker_embed_dim)");
      SD_CHECK(b.numel() == E, kErrParam, "proj_layer.bias size");
      std::vector<float> wt((size_t)E * SE), wm((size_t)E * SE);
      for (int n = 0; n < E; ++n)
        for (int k = 0; k < SE; ++k) {
          wt[(size_t)n * SE + k] = w.data[(size_t)n * 2 * SE + k];
          wm[(size_t)n * SE + k] = w.data[(size_t)n * 2 * SE + SE + k];
        }
      proj_ts_ = upload_packed(arena_, wt, E, SE, 1, 1, cfg_.bf16);
      proj_mix_ = upload_packed(arena_, wm, E, SE, 1, 1, cfg_.bf16);
      proj_b_ = arena_.upload(b.data);
    }
    if (mamba2_backend()) {
      // Mamba2BlockV2(E, n_layer=num_transformer_layer, d_state, d_conv=4, expand, bidirectional=True)
      // (magicdata model.py:377-403)
      single_m_ = std::make_unique<Mamba2Stack>();
      single_m_->load(ps_, arena_, "single_backend.", cfg_.embed_dim, cfg_.num_transformer_layer, cfg_.d_state,
                      cfg_.expand, cfg_.bf16);
    }
    if (cfg_.backend == 2) {
      // the same stack over the speaker-merged rows, then multi_backend_proj = Linear(2 E, E) (:488-504, 1396-1397)
      multi_m_ = std::make_unique<Mamba2Stack>();
      multi_m_->load(ps_, arena_, "multi_backend.", cfg_.embed_dim, cfg_.num_transformer_layer, cfg_.d_state,
                     cfg_.expand, cfg_.bf16);
      multi_proj_ = loader().linear("multi_backend_proj");
      SD_CHECK(multi_proj_.w.N == cfg_.embed_dim && multi_proj_.w.K == 2 * cfg_.embed_dim, kErrParam,
               "multi_backend_proj.weight must be (transformer_embed_dim, 2 * transformer_embed_dim)");
      SD_CHECK(ps_.get("multi_backend_proj.bias").numel() == cfg_.embed_dim, kErrParam, "multi_backend_proj.bias size");
    }
    // backend 4 / 5: torchaudio.models.Conformer(E, num_attention_head, transformer_ffn_embed_dim, num_transformer_layer,
    // depthwise_conv_kernel_size=31), use_group_norm False: eval BatchNorm1d folded into the depthwise conv
    // (egs/magicdata-ramc/ts_vad2/model.py:290-313, 451-463)
    for (int i = 0; i < cfg_.num_transformer_layer; ++i) {
      const std::string n = std::to_string(i);
      if (cfg_.backend == 0) single_.push_back(loader().transformer("single_backend.layers." + n));
      // (num_batches_tracked is accepted and ignored: require_all_used skips it)
      if (conformer_backend()) single_c_.push_back(conformer_layer("single_backend.conformer_layers." + n));
      if (cfg_.backend == 5) multi_c_.push_back(conformer_layer("multi_backend.conformer_layers." + n));
      else if (cfg_.backend != 2) multi_.push_back(loader().transformer("multi_backend.layers." + n));
    }
    backend_down_ = conv_bn("backend_down.0.weight", "", "backend_down.0.bias");
    if (mamba2_backend())   // the two directions are concatenated: Conv1d(2 E NS -> E, k5, pad 2)
      SD_CHECK(backend_down_.w.N == cfg_.embed_dim && backend_down_.w.kw == 5 &&
                   backend_down_.w.Cin == 2 * cfg_.embed_dim * cfg_.max_num_speaker,
               kErrParam, "backend_down.0.weight must be (transformer_embed_dim, 2 * transformer_embed_dim * "
                          "max_num_speaker, 5) behind a Mamba2 single back end");
    backend_bn_ = bn_only("backend_down.1.bn");
    fc_ = loader().linear("fc");
  } else {
    gsp_w_ = arena_.upload(ps_.get("gsp_fc.weight").data);
    gsp_b_ = arena_.upload(ps_.get("gsp_fc.bias").data);
    for (int i = 0; i < cfg_.conformer_layers; ++i)
      conf_.push_back(loader().conformer("single_backend.conformer_layers." + std::to_string(i), true));
    // BiLSTM: stack both directions' W_ih, fold b_ih + b_hh.
    const int H = cfg_.lstm_hidden;
    std::vector<float> wih, bias, whh;
    for (const char* sfx : {"", "_reverse"}) {
      const HostTensor& wi = ps_.get(std::string("multi_backend.weight_ih_l0") + sfx);
      const HostTensor& wh = ps_.get(std::string("multi_backend.weight_hh_l0") + sfx);
      const HostTensor& bi = ps_.get(std::string("multi_backend.bias_ih_l0") + sfx);
      const HostTensor& bh = ps_.get(std::string("multi_backend.bias_hh_l0") + sfx);
      SD_CHECK(wh.shape[0] == 4 * H && wh.shape[1] == H, kErrParam, "weight_hh shape");
      wih.insert(wih.end(), wi.data.begin(), wi.data.end());
      whh.insert(whh.end(), wh.data.begin(), wh.data.end());
      for (int64_t i = 0; i < bi.numel(); ++i) bias.push_back(bi.data[i] + bh.data[i]);
    }
    const HostTensor& wi0 = ps_.get("multi_backend.weight_ih_l0");
    lstm_ih_ = upload_packed(arena_, wih, 8 * H, (int)wi0.shape[1], 1, 1, cfg_.bf16);
    lstm_b_ = arena_.upload(bias);
    lstm_hh_ = arena_.upload(whh);
    // bf16 copy for the bf16 recurrence; fp32 handles keep hi / lo for the bf16x3 mode's split recurrence
    lstm_hh_bf_ = upload_packed(arena_, whh, 2 * 4 * H, H, 1, 1, true).w;
    if (!cfg_.bf16) lstm_hh_lo_ = upload_bf16_lo(arena_, whh);
    fc_ = loader().linear("fc");
  }
  ps_.require_all_used();
  alloc_workspace();
}

TsvadModel::Geometry TsvadModel::geometry() const {
  Geometry g;
  g.T3 = mix_frames(max_input());
  g.Tl = std::max<int64_t>(g.T3 + 3, (int64_t)cfg_.rs_len * 25);   // the longest label a forward accepts
  g.rows = (int64_t)cfg_.max_batch * cfg_.max_num_speaker * g.Tl;
  g.mix_elems = (int64_t)cfg_.max_batch * g.T3 * cfg_.speaker_embed_dim;
  g.token_elems = g.rows * cfg_.embed_dim;
  return g;
}

void TsvadModel::alloc_workspace() {
  const Geometry g = geometry();
  const int64_t Bm = cfg_.max_batch, NS = cfg_.max_num_speaker, E = cfg_.embed_dim;
  if (res_) res_->alloc(arena_, cfg_.max_batch, cfg_.max_fbank_frames);
  else if (ecapa_) ecapa_->alloc(arena_, cfg_.max_batch, cfg_.max_fbank_frames);
  else if (redim_) redim_->alloc(arena_, cfg_.max_batch, cfg_.max_fbank_frames);
  else if (wavlm_) {
    wavlm_->alloc(arena_);
    if (cfg_.variant == 6) {   // one (B T, D) accumulator and one (B T, SE) map: nothing grows with the layer count
      const int64_t rows = Bm * WavlmTrunk::frames(cfg_.max_samples);
      acc_ = ws(rows * cfg_.wavlm_embed_dim);
      z_ = arena_.alloc(rows * cfg_.speaker_embed_dim * (cfg_.bf16 ? 2 : 4));
    }
  }
  else if (w2v_) w2v_->alloc(arena_);
  else if (whisper_) whisper_->alloc(arena_, true);
  else cam_->alloc(arena_, cfg_.max_batch, cfg_.max_fbank_frames);
  mix_ = ws(g.mix_elems);
  mixg_ = ws(g.mix_elems);
  X_ = ws(g.token_elems);
  Y_ = ws(g.token_elems);
  QKV_ = ws(g.token_elems * 3);
  AO_ = ws(g.token_elems);
  H_ = ws(g.rows * std::max<int64_t>({(int64_t)cfg_.ffn_dim, 2 * E, (int64_t)cfg_.conformer_ffn}));
  // behind a Mamba2 single back end X2_ holds both directions: (B, Tl, NS * 2 E)
  X2_ = ws(g.token_elems * (single_m_ ? 2 : 1));
  // the Mamba2 stages' own buffers (in_proj's zxbcdt is the large one), sized for max_batch windows
  if (single_m_) single_m_->alloc(arena_, g.rows);
  if (multi_m_) multi_m_->alloc(arena_, Bm * g.Tl);
  partial_ = ws(Bm * NS * ((E + 63) / 64) * 2);
  lstm_work_ = ws(lstm_work_floats((int)Bm, cfg_.lstm_hidden, 2));
  nonfinite_ = static_cast<int*>(arena_.alloc(4 * (size_t)Bm * sizeof(int)));
  if (proj_b_) {
    pts_ = ws(Bm * NS * E);
    pmix_ = ws(Bm * g.T3 * E);
  }
}

TsvadModel::~TsvadModel() {
  if (ev_fork_) (void)hipEventDestroy(ev_fork_);
  if (ev_join_) (void)hipEventDestroy(ev_join_);
  if (side_) (void)hipStreamDestroy(side_);
}

void TsvadModel::forward_graph(const float* ref, const float* ts, int B, int Tf, int Tl, float* logits, int replays,
                               const char* dot, hipStream_t st) {
  SD_CHECK(replays >= 0, kErrInvalid, "forward_graph: replays < 0");
  hipStream_t cap = nullptr;
  SD_HIP(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
  hipGraph_t g = nullptr;
  hipGraphExec_t ex = nullptr;
  try {
    SD_HIP(hipStreamSynchronize(st));
    SD_HIP(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
    try {
      forward(ref, ts, B, Tf, Tl, logits, cap);
    } catch (...) {
      hipGraph_t bad = nullptr;
      (void)hipStreamEndCapture(cap, &bad);
      if (bad) (void)hipGraphDestroy(bad);
      throw;
    }
    SD_HIP(hipStreamEndCapture(cap, &g));
    if (dot) SD_HIP(hipGraphDebugDotPrint(g, dot, 0));
    SD_HIP(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    for (int r = 0; r < replays; ++r) SD_HIP(hipGraphLaunch(ex, st));
    SD_HIP(hipStreamSynchronize(st));
  } catch (...) {
    if (ex) (void)hipGraphExecDestroy(ex);
    if (g) (void)hipGraphDestroy(g);
    (void)hipStreamDestroy(cap);
    throw;
  }
  (void)hipGraphExecDestroy(ex);
  (void)hipGraphDestroy(g);
  (void)hipStreamDestroy(cap);
}

void TsvadModel::debug_buffer(int which, void** ptr, int64_t* bytes) const {
  const Geometry g = geometry();
  switch (which) {
    case 0: *ptr = mix_; *bytes = g.mix_elems * 4; break;
    case 1: *ptr = mixg_; *bytes = g.mix_elems * 4; break;
    case 2: *ptr = X2_; *bytes = g.token_elems * 4; break;
    case 3: *ptr = H_; *bytes = g.token_elems * 4; break;
    case 4: *ptr = Y_; *bytes = g.token_elems * 4; break;
    default: throw Error{kErrInvalid, "debug_buffer: unknown buffer"};
  }
}

// forward_common's back end from the mix embeddings on (model.py:856-897), shared by variants 0, 2, 3 and 4: mix_ holds
// speech_down_or_up's conv + bias (B, T3, SE); its BatchNorm1D + ReLU are applied on load (sd_bn).
void TsvadModel::transformer_backend(const float* ts, int T3, int B, int Tl, float* logits, hipStream_t st,
                                     const BnRelu& sd_bn, const BnRelu& bd_bn) {
  const bool bf = cfg_.bf16;
  const int E = cfg_.embed_dim, SE = cfg_.speaker_embed_dim, NS = cfg_.max_num_speaker, S = B * NS;
  // Per-speaker encoder over S = B*NS sequences (model.py:869-879).
  if (proj_b_) {
    // 2 SE != E: proj_layer on cat(ts_embed, mix_embeds) (model.py:873-874) as two small GEMMs + a combine pass that
    // also writes bf16(X) (mixg_ holds the mix GEMM's BN-ReLU'd A operand)
    SpeakerProjArgs a;
    a.ts = ts; a.mix = mix_; a.ldmix = SE; a.Tmix = T3; a.B = B; a.NS = NS; a.T = Tl; a.SE = SE; a.E = E;
    a.w_ts = proj_ts_.w; a.w_mix = proj_mix_.w; a.bias = proj_b_; a.pe = pe_; a.bn = sd_bn;
    a.mix_a = mixg_; a.p_ts = pts_; a.p_mix = pmix_; a.out = X_;
    a.xb = bf ? reinterpret_cast<uint16_t*>(enc_work().AO) : nullptr;
    speaker_input_proj(a, bf, st);
  } else {
    build_speaker_input(ts, mix_, SE, T3, B, NS, Tl, SE, pe_, X_, st, sd_bn);
    // bf16(X) for the first layer's in-projection too (every later layer gets it from the LayerNorms): an
    // fp32 A operand would send that GEMM to the register-staged kernel (C4: 1.5 ms per 640 windows vs 0.3)
    if (bf && !single_m_ && single_c_.empty()) f32_to_bf16(X_, (int64_t)S * Tl * E, enc_work().AO, st);
  }
  // Mamba2 back ends: the reference hands the seq-first (T, B, E) tensor to a batch-first module (magicdata
  // model.py:1366-1367, 1393), so each (speaker, frame) is a sequence over the windows of one reference forward call:
  // the groups of `group` windows the BatchNorm1D bypass already names
  const int G = bd_bn.group;
  int ch = NS * E;   // backend_down's input channels per frame
  if (single_m_) {
    // both directions of every speaker straight into the speakers-to-channels layout (B, Tl, NS * 2 E)
    single_m_->forward(X_, B, G, NS * Tl, X2_, bf, NS, Tl, st);
    ch = NS * 2 * E;
  } else if (!single_c_.empty()) {
    // the sequence axis is time: every (window, speaker) is one sequence of Tl frames, all of full length (:1340-1351)
    if (conformer_stack_default_fused(single_c_, E, bf)) {
      // (not the shipped route at hidden 1536: encoder.h) the row programs, the last one writing bf16 rows straight
      // into the speakers-to-channels layout
      SpeakerStreams io;
      io.NS = NS; io.out = X2_;
      run_conformer_stack(single_c_, X_, S, Tl, E, cfg_.num_attention_head, kConformerKernel, nullptr, enc_work(), st, &io);
    } else {
      for (const ConformerL& L : single_c_)
        run_conformer(L, X_, S, Tl, E, cfg_.num_attention_head, kConformerKernel, nullptr, enc_work(), st);
      speakers_to_channels(X_, B, NS, Tl, E, X2_, bf, st);
    }
  } else {
    for (size_t i = 0; i < single_.size(); ++i)
      run_transformer(single_[i], X_, S, Tl, E, cfg_.num_attention_head, nullptr, enc_work(), st, 0, 0, bf || i > 0);
    speakers_to_channels(X_, B, NS, Tl, E, X2_, bf, st);
  }
  ConvGemmArgs p = cam_conv1d(Tens{X2_, bf}, B, Tl, ch, backend_down_, 1, 2, 1, Tens{X_, false}, E);
  conv_gemm(p, bf, st);
  add_pe(X_, B * Tl, Tl, E, E, pe_, st, bd_bn);   // backend_down's BatchNorm1D + ReLU, then the PE
  if (multi_m_) {
    multi_m_->forward(X_, B, G, Tl, X2_, bf, 1, Tl, st);
    conv_gemm(lin(Tens{X2_, bf}, B * Tl, 2 * E, multi_proj_.w, multi_proj_.beta, Tens{X_, false}, E), bf, st);
  } else if (!multi_c_.empty()) {
    if (conformer_stack_default_fused(multi_c_, E, bf))   // :1382-1390
      run_conformer_stack(multi_c_, X_, B, Tl, E, cfg_.num_attention_head, kConformerKernel, nullptr, enc_work(), st);
    else
      for (const ConformerL& L : multi_c_)
        run_conformer(L, X_, B, Tl, E, cfg_.num_attention_head, kConformerKernel, nullptr, enc_work(), st);
  } else {
    if (bf) f32_to_bf16(X_, (int64_t)B * Tl * E, enc_work().AO, st);
    for (size_t i = 0; i < multi_.size(); ++i)
      run_transformer(multi_[i], X_, B, Tl, E, cfg_.num_attention_head, nullptr, enc_work(), st, 0, 0, bf || i > 0);
  }
  conv_gemm(logits_fc(X_, B, Tl, E, fc_, NS, logits), bf, st);
}

// forward_common_ots_vad's back end (model.py:669-756) over windows [b0, b0 + Bh) up to the BiLSTM, with the fused
// conformer stack: gsp_fc on the slice's mix rows, then the stack with every buffer addressed from the slice's
// first row (bf16 y / qkv / ao / h, fp32 X, per-sequence GroupNorm partials, the speaker streams).
void TsvadModel::conformer_slice(const float* ts, int T3, int b0, int Bh, int Tl, hipStream_t s, const BnRelu& sd_bn) {
  const int E = cfg_.embed_dim, SE = cfg_.speaker_embed_dim, NS = cfg_.max_num_speaker;
  const int64_t m0 = (int64_t)b0 * T3 * SE, s0 = (int64_t)b0 * NS, r0 = s0 * Tl;
  BnRelu sb = sd_bn;
  sb.win0 = b0;
  gsp_fc(mix_ + m0, Bh * T3, SE, SE, gsp_w_, gsp_b_, SE, mixg_ + m0, SE, s, sb, T3);
  auto at = [](float* p, int64_t bytes) { return reinterpret_cast<float*>(reinterpret_cast<char*>(p) + bytes); };
  EncoderWork w = enc_work();
  w.Y = at(Y_, r0 * E * 2);
  w.QKV = at(QKV_, r0 * 3 * E * 2);
  w.AO = at(AO_, r0 * E * 2);
  w.H = at(H_, r0 * 2 * E * 2);
  w.partial = partial_ + s0 * ((E + 63) / 64) * 2;
  SpeakerStreams io;
  io.ts = ts + s0 * SE; io.mix = mixg_ + m0; io.ldmix = SE; io.Tmix = T3; io.NS = NS;
  io.out = at(X2_, (int64_t)b0 * Tl * NS * E * 2);
  run_conformer_stack(conf_, X_ + r0 * E, Bh * NS, Tl, E, cfg_.conformer_heads, cfg_.conformer_kernel, nullptr, w, s,
                      &io);
}

// The rest of that back end from the mix embeddings on.  conformer_done: conformer_slice has run over every window
// (X2_ holds the stack's output); else gsp_fc and the conformer stack run here, layer by layer over the batch.
void TsvadModel::ots_vad_backend(const float* ts, int T3, int B, int Tl, float* logits, hipStream_t st,
                                 const BnRelu& sd_bn, bool conformer_done) {
  const bool bf = cfg_.bf16;
  const int E = cfg_.embed_dim, SE = cfg_.speaker_embed_dim, NS = cfg_.max_num_speaker, Hh = cfg_.lstm_hidden;
  if (!conformer_done) {
    gsp_fc(mix_, B * T3, SE, SE, gsp_w_, gsp_b_, SE, mixg_, SE, st, sd_bn, T3);
    build_speaker_input(ts, mixg_, SE, T3, B, NS, Tl, SE, nullptr, X_, st);
    run_conformer_stack(conf_, X_, B * NS, Tl, E, cfg_.conformer_heads, cfg_.conformer_kernel, nullptr, enc_work(), st);
    speakers_to_channels(X_, B, NS, Tl, E, X2_, bf, st);
  }
  conv_gemm(lin(Tens{X2_, bf}, B * Tl, NS * E, lstm_ih_, lstm_b_, Tens{H_, false}, 8 * Hh), bf, st);
  // SDIAR_LSTM_FP32 (diagnostic, tools/parity_stages.py): the exact-fp32 recurrence in bf16 mode too
  static const bool lstm_fp32 = getenv("SDIAR_LSTM_FP32") != nullptr;
  const bool x3 = !bf && gemm_x3();   // bf16x3 (precision 2): the split recurrence; fp32: exact step kernel
  lstm_recurrence(H_, B, Tl, Hh, 2, lstm_hh_, nullptr, nullptr, nullptr, Y_, 2 * Hh, nullptr,
                  nullptr, lstm_work_, st, (bf && !lstm_fp32) || x3 ? lstm_hh_bf_ : nullptr, lstm_err_.get(0),
                  x3 ? lstm_hh_lo_ : nullptr);
  conv_gemm(logits_fc(Y_, B, Tl, 2 * Hh, fc_, NS, logits), bf, st);
}

void TsvadModel::check_label_frames(int T3, int Tl) const {
  const std::string diff = "label and ref_speech(mix speech) diff: " + std::to_string(T3 - Tl);
  if (cfg_.variant == 1) {
    SD_CHECK(std::abs(T3 - Tl) <= 3, kErrShape, diff);
    return;
  }
  if (cfg_.variant >= 4) {
    // egs/magicdata-ramc/ts_vad2/model.py:1296-1309: |gap| <= 3; a short encoder output is zero-padded by 1 to 3
    // frames after the ReLU (the consumers read mix rows >= T3 as zeros), a long one is cut at the label length
    SD_CHECK(std::abs(T3 - Tl) <= 3, kErrShape,
             diff + ", label len: " + std::to_string(Tl) + ", ref_speech len: " + std::to_string(T3));
    SD_CHECK(Tl <= pe_len_, kErrShape, "label length exceeds positional-encoding max_len");
    return;
  }
  // model.py:849-854; with the ResNet34 encoder the reference's own -1 branch raises too (its pad call is
  // misspelt: AttributeError)
  SD_CHECK(T3 - Tl <= 2 && T3 - Tl >= -1, kErrShape, diff);
  SD_CHECK(cfg_.variant != 2 || T3 - Tl != -1, kErrShape,
           "label and ref_speech(mix speech) diff: -1 (the reference raises here: module 'torch.nn' has no "
           "attribute 'functinal')");
  SD_CHECK(Tl <= pe_len_, kErrShape, "label length exceeds positional-encoding max_len");
}

void TsvadModel::run_sliced(int B, bool two, hipStream_t st,
                            const std::function<void(int b0, int Bh, hipStream_t s)>& body) {
  if (!two) {
    body(0, B, st);
    return;
  }
  if (!side_) {
    SD_HIP(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking));
    SD_HIP(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
    SD_HIP(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming));
  }
  const int B1 = B / 2;
  SD_HIP(hipEventRecord(ev_fork_, st));
  SD_HIP(hipStreamWaitEvent(side_, ev_fork_, 0));
  body(0, B1, st);
  body(B1, B - B1, side_);
  SD_HIP(hipEventRecord(ev_join_, side_));
  SD_HIP(hipStreamWaitEvent(st, ev_join_, 0));
}

Tens TsvadModel::trunk_forward(const float* ref, int Bh, int Tf, hipStream_t s, int b0) const {
  if (wavlm_) {
    SD_CHECK(b0 == 0, kErrInvalid, "the WavLM trunk runs over the whole batch");
    if (cfg_.variant == 5) return wavlm_->encode(ref, Bh, Tf, s);   // extract_features(ref_speech)[0] (:1174)
    // hss[1:] weighted by `weights` as the layers run (:1193-1200), then wavlmproj + wavlmlnorm (:1201-1202)
    const int D = cfg_.wavlm_embed_dim, rows = Bh * WavlmTrunk::frames(Tf);
    wavlm_->encode_layers(ref, Bh, Tf, [&](int layer, const float* x, hipStream_t q) {
      wavlm_layer_mix(acc_, x, mix_w_[layer], layer == 0, (int64_t)rows * D, q);
    }, s);
    wavlm_mix_proj_ln(acc_, rows, D, wproj_.w.w, cfg_.bf16, wproj_.beta, wln_g_, wln_b_, cfg_.speaker_embed_dim, z_, s);
    return Tens{z_, cfg_.bf16};
  }
  if (whisper_) {
    SD_CHECK(b0 == 0, kErrInvalid, "the Whisper trunk runs over the whole batch");
    return whisper_->encode(ref, Bh, Tf, s);   // self.speech_encoder(ref_speech) (:1221)
  }
  if (w2v_) {
    SD_CHECK(b0 == 0, kErrInvalid, "the w2v-BERT trunk runs over the whole batch");
    // torch.reshape(ref_speech, (B, T // 2, 160)) is the same memory (:1228-1231); hidden_states[-1] (:1232-1235)
    return w2v_->encode(ref, Bh, Tf / 2, s);
  }
  if (ecapa_) return ecapa_->forward(ref, Bh, Tf, s, b0);
  if (redim_) {
    SD_CHECK(b0 == 0, kErrInvalid, "the ReDimNetB2 trunk runs over the whole batch");
    return redim_->forward(ref, Bh, Tf, s);
  }
  return res_ ? res_->forward(ref, Bh, Tf, s, b0) : cam_->forward(ref, Bh, Tf, s, b0);
}

// conv + bias, fp32 out; its BatchNorm1D + ReLU are applied by the consumer (gsp_fc / build_speaker_input)
ConvGemmArgs TsvadModel::down_gemm(Tens x, int Bh, int Tf, float* out) const {
  const int SE = cfg_.speaker_embed_dim;
  // ResNet34: (Bh, T4, 2560) -> (Bh, T4, [y[2j] | y[2j+1]]) = (Bh, 2 T4, SE), the upsampler as a k3 pad-1 conv
  if (res_) return cam_conv1d(x, Bh, ResTrunk::out_frames(Tf), ResTrunk::kChannels, down_, 1, 1, 1, Tens{out, false}, 2 * SE);
  // ECAPA: k5 stride-4 pad-2 conv over the unsubsampled (Bh, Tf, 1536) map
  if (ecapa_) return cam_conv1d(x, Bh, Tf, EcapaTrunk::kChannels, down_, 4, 2, 1, Tens{out, false}, SE);
  // ReDimNetB2: the same conv over the unsubsampled (Bh, Tf, 1152) frame-level map
  if (redim_) return cam_conv1d(x, Bh, Tf, RedimTrunk::kChannels, down_, 4, 2, 1, Tens{out, false}, SE);
  // WavLM: k5 stride-2 pad-2 conv over the (Bh, T, D) encoder output (5) or the (Bh, T, SE) projected map (6)
  if (wavlm_)
    return cam_conv1d(x, Bh, WavlmTrunk::frames(Tf), cfg_.variant == 6 ? SE : cfg_.wavlm_embed_dim, down_, 2, 2, 1,
                      Tens{out, false}, SE);
  // Whisper: the same conv over the (Bh, T', n_audio_state * n_cat) normalised concatenation
  if (whisper_) return cam_conv1d(x, Bh, WhisperTrunk::frames(Tf), whisper_->wide(), down_, 2, 2, 1, Tens{out, false}, SE);
  // w2v-BERT: the same conv over the (Bh, T / 2, 1024) encoder output
  if (w2v_) return cam_conv1d(x, Bh, Tf / 2, W2vBertTrunk::kHidden, down_, 2, 2, 1, Tens{out, false}, SE);
  // CAM++: k5 stride-2 pad-2 conv, out_nonlinear's BN-ReLU fused as its prologue
  return cam_conv1d(x, Bh, CamTrunk::out_frames(Tf), CamTrunk::kChannels, down_, 2, 2, 1, Tens{out, false}, SE);
}

// Direct launches.  A hipGraph replay of this forward (forward_graph above) measured no faster on C2 (34.3 vs
// 34.4 ms per 10-min step in round 3: ~150 launches against a 34-ms GPU span).  Its round-3 replay divergence
// was root-caused in round 4: the captured hipMemsetAsync nodes that reset the BiLSTM's h/c state and exchange
// counters stopped taking effect from the second replay on, so the recurrence started from the previous
// replay's state.  Every forward now zeroes device state with zero_fill kernels, and replays are
// bit-identical to direct launches (tests/test_gpu_tsvad_graph.py).
void TsvadModel::forward(const float* ref, const float* ts, int B, int Tf, int Tl, float* logits,
                         hipStream_t st, int forward_batch, int force) {
  SD_CHECK(forward_batch >= 0 && force >= 0 && force <= 3, kErrInvalid, "forward: bad forward_batch / force");
  require_finalized();
  SD_CHECK(B >= 1 && B <= cfg_.max_batch, kErrInvalid, "batch exceeds max_batch");
  // a Mamba2 back end scans over the windows of a reference forward call: the call must hold each of them whole
  SD_CHECK(!single_m_ || force == 0, kErrInvalid,
           "force: a Mamba2 back end cannot run a slice of a reference batch (raise max_batch to forward_batch)");
  // ECAPA and ReDimNetB2 never subsample inside the trunk: any window of at least one frame runs
  if (waveform()) {
    SD_CHECK(Tf >= WavlmTrunk::kMinSamples, kErrInvalid, "n_samples must be at least 400");
    SD_CHECK(Tf <= cfg_.max_samples, kErrInvalid, "n_samples exceeds max_samples");
    SD_CHECK(Tf % 4 == 0, kErrInvalid, "n_samples must be a multiple of 4 (16-byte window rows)");
    SD_CHECK(!gemm_x3(), kErrInvalid,
             "the waveform speech encoders (WavLM, variants 5 / 6; whisper, variant 8) do not build bf16x3");
  } else {
    SD_CHECK(Tf >= (cfg_.variant >= 3 ? 1 : 8) && Tf <= cfg_.max_fbank_frames, kErrInvalid,
             "fbank frames exceed max_fbank_frames");
    // the reference's torch.reshape(ref_speech, (B, T // 2, 160)) raises on an odd T (magicdata model.py:1228-1231)
    SD_CHECK(!w2v_ || Tf % 2 == 0, kErrInvalid,
             "w2v-bert2 needs an even number of fbank frames: the reference reshapes (B, T, 80) to (B, T / 2, 160) "
             "and raises on an odd T (shape is invalid for input of size)");
    SD_CHECK(!w2v_ || !gemm_x3(), kErrInvalid, "the w2v-bert2 speech encoder (variant 7) does not build bf16x3");
  }
  raise_if_set();
  const int T3 = mix_frames(Tf);
  check_label_frames(T3, Tl);
  const bool bf = cfg_.bf16;
  const int E = cfg_.embed_dim, SE = cfg_.speaker_embed_dim, NS = cfg_.max_num_speaker;
  // Batches of more than one round of CUs run the speech encoder as two window slices on two streams
  // (bit-identical per window: every kernel up to the BiLSTM computes a window independently of the rest of the
  // batch).  SDIAR_CAM_ONE_STREAM: one launch sequence over the whole batch.
  // Under the libsdiar kernel timer (bench.py's extra profiled step) the forward stays on one stream, so
  // each kernel's HIP-event time is its own and not shared with the other slice's kernels.
  static const bool one_stream_env = getenv("SDIAR_CAM_ONE_STREAM") != nullptr;
  const bool two = !(one_stream_env || prof_enabled()) && B >= 384 && !redim_ && !wavlm_ && !w2v_ && !whisper_;   // these trunks take no window slice
  // ---------------- BatchNorm1D's NaN bypass: which windows hold a non-finite input, which reference forwards
  // (groups of forward_batch windows) therefore skip the BatchNorm (from the inputs alone, so first: the window
  // slices below then need nothing from each other until the LSTM)
  const int G = forward_batch > 0 ? forward_batch : B;
  int* win_fb = nonfinite_;
  int* win_ts = nonfinite_ + cfg_.max_batch;
  int* grp_sd = nonfinite_ + 2 * cfg_.max_batch;
  int* grp_bd = nonfinite_ + 3 * cfg_.max_batch;
  zero_fill(nonfinite_, 4 * (size_t)cfg_.max_batch * sizeof(int), st);
  nonfinite_windows(ref, B, (int64_t)Tf * feat_dim(), G, win_fb, grp_sd, grp_bd, st);
  nonfinite_windows(ts, B, (int64_t)NS * SE, G, win_ts, nullptr, cfg_.variant != 1 ? grp_bd : nullptr, st);
  if (force & 1) fill_u32(grp_sd, (size_t)cfg_.max_batch * sizeof(int), 1u, st);
  if (force & 3) fill_u32(grp_bd, (size_t)cfg_.max_batch * sizeof(int), 1u, st);
  BnRelu sd_bn = down_bn_, bd_bn = backend_bn_;
  sd_bn.grp = grp_sd; sd_bn.group = G;
  bd_bn.grp = grp_bd; bd_bn.group = G;
  // ---------------- speech encoder + speech_down_or_up -> mix_ (B, T3, SE)
  const bool fused_v1 = cfg_.variant == 1 && SE == 192 && E == 2 * SE && conformer_stack_fused(conf_, E, bf);
  if (fused_v1) {
    // Each slice runs the whole per-window part of the model on its own stream: trunk, speech_down conv, gsp_fc,
    // conformer stack.  Nothing joins between the trunk and the conformer, so one slice's HBM-bound CAM++ kernels
    // overlap the other's MFMA-bound conformer programs.
    run_sliced(B, two, st, [&](int b0, int Bh, hipStream_t s) {
      const Tens x4 = trunk_forward(ref, Bh, Tf, s, b0);
      conv_gemm(down_gemm(x4, Bh, Tf, mix_ + (int64_t)b0 * T3 * SE), bf, s);
      conformer_slice(ts, T3, b0, Bh, Tl, s, sd_bn);
    });
  } else if (cfg_.frame_level_gsp) {
    // per window, so inside the trunk's slice: out_nonlinear + frame stats + the folded gsp_fc / conv in one launch
    const int T2 = CamTrunk::out_frames(Tf);
    run_sliced(B, two, st, [&](int b0, int Bh, hipStream_t s) {
      const Tens x = trunk_forward(ref, Bh, Tf, s, b0);   // the slice's own map: windows [b0, b0 + Bh)
      gsp_down(x.p, x.bf, Bh, T2, cam_->out_s(), cam_->out_h(), gsp_coef_, gsp_cb_, SE, mix_ + (int64_t)b0 * T3 * SE, s);
    });
  } else {
    // the trunk alone runs sliced; the speech_down_or_up GEMM covers the whole batch after the join
    Tens x4{};
    run_sliced(B, two, st, [&](int b0, int Bh, hipStream_t s) {
      const Tens x = trunk_forward(ref, Bh, Tf, s, b0);
      if (b0 == 0) x4 = x;   // the batch's output map
    });
    conv_gemm(down_gemm(x4, B, Tf, mix_), bf, st);
  }
  // ---------------- back end -> logits (B, NS, Tl)
  if (cfg_.variant == 1) ots_vad_backend(ts, T3, B, Tl, logits, st, sd_bn, fused_v1);
  else transformer_backend(ts, T3, B, Tl, logits, st, sd_bn, bd_bn);
  // a window whose fbank or target-speaker embeddings hold a NaN / Inf has NaN logits in the reference
  poison_windows(logits, B, (int64_t)NS * Tl, win_fb, win_ts, st);
  // behind a Mamba2 back end the forward and backward scans carry that NaN to every window of its reference forward
  // call, and backend_down mixes the two directions: the whole group is NaN there (the flags are taken at the source
  // for the same reason as poison_windows': the trunk's ReLUs drop NaN)
  if (single_m_) poison_groups(logits, B, (int64_t)NS * Tl, grp_bd, G, st);
}

}  // namespace sd
