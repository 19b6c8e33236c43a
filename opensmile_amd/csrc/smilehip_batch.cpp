// libsmilehip, C ABI part 3: batches (packed utterances), the fused chain runs, functionals, timing.
#include "smilehip_internal.hpp"
#include "batch_layout.hpp"

// ------------------------------------------------------------------ batch
// A batch is (1) its layout -- host index arithmetic, batch_layout.hpp --, (2) that layout's index vectors on the device and
// (3) the scratch matrices of its plan's chain kind, one alloc_*_scratch below per kind. The order and the sizes of the device
// allocations are part of the behaviour: the block cache behind DevBuf hands blocks out by exact size.
smilehip_batch::~smilehip_batch() { delete f0_batch; }

static inline bool mfcc_like(const smilehip_plan *p) {
  return p->cfg.chain_kind == SMILEHIP_CHAIN_MFCC || p->cfg.chain_kind == SMILEHIP_CHAIN_PLP;
}

static BatchLayoutSpec layout_spec(const smilehip_plan *plan) {
  const smilehip_lld_config &c = plan->cfg;
  BatchLayoutSpec s;
  s.chain_kind = c.chain_kind;
  s.N = plan->geo.N; s.H = plan->geo.H; s.period = plan->geo.period;
  s.row_extra = plan_row_extra(plan);
  s.fused_delta_eligible = plan->use_fast && mfcc_like(plan) && c.n_delta == 2 && c.delta_win == 2 && !c.append_log_energy && !c.cms &&
                           !getenv("SMILEHIP_NO_FUSED_DELTA");
  s.fast_slots = std::max<int64_t>(1, plan->fast.max_blocks) * 8;
  s.tile_frames = plan->use_fast ? fast512_tile_frames() : (f0_front_chain(c.chain_kind) ? f0_tile_frames() : (int64_t(1) << 40));
  s.dtile_rows = chain_tile_rows(); s.short_T = chain_short_max(); s.jitter_chunk = jitter_chunk_frames();
  if (const char *rf = getenv("SMILEHIP_RUN_FRAMES")) { const int v = atoi(rf); if (v >= 1 && v <= 4096) s.run_frames_override = v; }   // A/B switch
  return s;
}

static inline size_t at_least_one(int64_t n) { return size_t(n ? n : 1); }

// MFCC / PLP: the delta-fused fast kernel's tiles, or -- with deltas to follow and no fused run -- the compact static block
static int alloc_mfcc_scratch(const smilehip_plan *plan, smilehip_batch *b, const BatchLayout &L) {
  b->n_ftiles = (int32_t)L.ftiles.size();
  if (b->n_ftiles) return b->d_ftile_rec.upload(L.ftiles);
  if (plan->cfg.n_delta > 0 && b->total_frames > 0 && b->d_static.alloc(size_t(b->total_frames) * size_t(plan_n_static(plan))))
    return fail(SMILEHIP_ERR_HIP, "hipMalloc of the static-block scratch failed");
  return SMILEHIP_OK;
}

static int alloc_is09_scratch(smilehip_batch *b, const BatchLayout &L) {
  int rc;
  if (b->total_frames > 0 && (rc = b->d_frame_utt.upload(L.frame_utt))) return rc;
  if (b->d_raw16.alloc(size_t(b->total_frames) * 16)) return fail(SMILEHIP_ERR_HIP, "hipMalloc of the IS09 scratch matrix failed");
  return SMILEHIP_OK;
}

// prosodyAcf: the utterance of every frame, and three floats per frame (voiceProb | pitch candidate, then contour | loudness)
static int alloc_prosody_acf_scratch(smilehip_batch *b, const BatchLayout &L) {
  int rc;
  if (b->total_frames > 0 && (rc = b->d_frame_utt.upload(L.frame_utt))) return rc;
  if (b->d_raw3.alloc(at_least_one(b->total_frames) * 3)) return fail(SMILEHIP_ERR_HIP, "hipMalloc of the prosodyAcf scratch matrix failed");
  return SMILEHIP_OK;
}

// emobase: the utterance of every 25 ms frame; 15 + p floats per frame for the 25 ms levels and three for the level pitch (a row per
// 25 ms frame: an utterance's first T40 are written; the rest stays zero)
static int alloc_emobase_scratch(const smilehip_plan *plan, smilehip_batch *b, const BatchLayout &L) {
  int rc;
  if (b->total_frames > 0 && (rc = b->d_frame_utt.upload(L.frame_utt))) return rc;
  b->emo_p = plan->emo_lpc_order;
  const size_t nf = at_least_one(b->total_frames);
  if (b->d_raw25.alloc(nf * (size_t)emobase::n25_cols(b->emo_p)) || b->d_raw3.alloc(nf * 3))
    return fail(SMILEHIP_ERR_HIP, "hipMalloc of the emobase scratch matrices failed");
  HIP_TRY(hipMemset(b->d_raw3.p, 0, nf * 3 * sizeof(float)));
  return SMILEHIP_OK;
}

// chroma_fft: the utterance of every frame, and the level tonespec
static int alloc_chroma_scratch(smilehip_plan *plan, smilehip_batch *b, const BatchLayout &L) {
  int rc;
  if (b->total_frames > 0 && (rc = b->d_frame_utt.upload(L.frame_utt))) return rc;
  if (b->d_tonespec.alloc(at_least_one(b->total_frames) * (size_t)plan->tonespec.n_notes))
    return fail(SMILEHIP_ERR_HIP, "hipMalloc of the chroma_fft scratch matrix failed");
  return SMILEHIP_OK;
}

// audspec: the utterance of every frame, and -- with deltas to follow -- the compact static block (smilehip_mfcc_run's arrangement)
static int alloc_audspec_scratch(const smilehip_plan *plan, smilehip_batch *b, const BatchLayout &L) {
  int rc;
  if (b->total_frames > 0 && (rc = b->d_frame_utt.upload(L.frame_utt))) return rc;
  if (plan->cfg.n_delta > 0 && b->total_frames > 0 && b->d_static.alloc(size_t(b->total_frames) * size_t(plan_n_static(plan))))
    return fail(SMILEHIP_ERR_HIP, "hipMalloc of the static-block scratch failed");
  return SMILEHIP_OK;
}

// spectrogram: the utterance of every frame; the rows go straight to the caller's matrix
static int alloc_spectrogram_scratch(smilehip_batch *b, const BatchLayout &L) {
  return b->total_frames > 0 ? b->d_frame_utt.upload(L.frame_utt) : SMILEHIP_OK;
}

// chroma_filt: the level tonespec; inputs that would carry the recursion's argument out of sincos_d's domain are refused here
static int alloc_chroma_filt_scratch(smilehip_plan *plan, smilehip_batch *b) {
  int64_t longest = 0;
  for (int32_t u = 0; u < b->n_utt; ++u) longest = std::max(longest, b->h_samp_off[u + 1] - b->h_samp_off[u]);
  longest = tonefilt::rows_of(longest, plan->tonefilt.P) * plan->tonefilt.P;   // (the last block runs to its end)
  if (tonefilt_check_domain(plan->tonefilt, longest))
    return fail(SMILEHIP_ERR_INVALID, "chroma_filt chain: an utterance of %lld samples carries 2 pi freq[nNotes - 1] t past the domain of sincos_d (2^30)",
                (long long)longest);
  if (b->d_tonespec.alloc(at_least_one(b->total_frames) * (size_t)plan->tonefilt.n_notes))
    return fail(SMILEHIP_ERR_HIP, "hipMalloc of the chroma_filt scratch matrix failed");
  return SMILEHIP_OK;
}

static int alloc_compare_ab_scratch(smilehip_batch *b, const BatchLayout &L) {
  int rc;
  b->n_runs = (int32_t)L.run_utt.size();
  if ((rc = b->d_run_utt.upload(L.run_utt)) || (rc = b->d_run_t0.upload(L.run_t0))) return rc;
  const size_t nf = at_least_one(b->total_frames);
  if (b->d_rawA.alloc(nf * 4) || b->d_rawB.alloc(nf * 55) || b->d_mel1.alloc(nf * 26) || b->d_b_extra.alloc(at_least_one(b->n_utt) * 110))
    return fail(SMILEHIP_ERR_HIP, "hipMalloc of the ComParE scratch matrices failed");
  (void)hipMemset(b->d_rawA.p, 0, nf * 4 * sizeof(float));
  return SMILEHIP_OK;
}

// what the F0 front end's frame kernels write and hand to one another: the cPitchShs rows, the frame energies, a chunk of rows
static int alloc_f0_frame_scratch(const smilehip_plan *plan, smilehip_batch *b) {
  const size_t nf = at_least_one(b->total_frames);
  if (b->d_shs.alloc(nf * 21) || b->d_e60.alloc(nf)) return fail(SMILEHIP_ERR_HIP, "hipMalloc of the F0 scratch matrices failed");
  const size_t nab = (size_t)std::max<int64_t>(f0_scratch_doubles(b->n_tiles, (int)plan->geo.K), 1);
  if (b->d_f0_ab.alloc(nab)) return fail(SMILEHIP_ERR_HIP, "hipMalloc of the F0 row scratch (%zu MB) failed", nab * sizeof(double) >> 20);
  // SMILEHIP_F0_PIPE=1 (round 6, measured and NOT the default): a second set of rows for the chunk pipeline (F0Pipe). Bit-identical
  // (tests/test_gpu_f0_pipe.py) and no faster: config 4 243.4 ms piped against 241.0 ms chunk after chunk, config 5 1087 against
  // 1081 -- side by side the three kernels stretch (spec 39 -> 102 ms, cand 36 -> 45, sweep 26 -> 38 summed) by what they gain;
  // the idle issue slots their counters show are not slots another kernel's waves can use.
  static const bool pipe_on = [] { const char *e = getenv("SMILEHIP_F0_PIPE"); return e && e[0] == '1'; }();
  if (pipe_on && b->n_tiles > f0_chunk_tiles()) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b / 4 <= nab * sizeof(double) || b->d_f0_ab2.alloc(nab))
      (void)hipGetLastError();                            // (optional: the run goes chunk after chunk without it)
  }
  return SMILEHIP_OK;
}

static int alloc_f0_scratch(const smilehip_plan *plan, smilehip_batch *b, const BatchLayout &L) {
  int rc;
  if ((rc = alloc_f0_frame_scratch(plan, b))) return rc;
  const std::vector<int32_t> zp(at_least_one(b->n_utt), 0);
  if ((rc = b->d_pending.upload(zp)) || (rc = b->d_jit_redo.upload(zp)) || (rc = b->d_jit_utt.upload(L.jit_utt)) ||
      (rc = b->d_jit_t0.upload(L.jit_t0)) || (rc = b->d_jit_ctl.upload(std::vector<int32_t>(2, 0))))
    return rc;
  return SMILEHIP_OK;
}

// The whole ComParE level: groups A+B here, the F0 group in a 60 ms sub-batch of plan->f0_plan
static int alloc_compare_scratch(smilehip_plan *plan, smilehip_batch *b, const BatchLayout &L) {
  int rc;
  if ((rc = alloc_compare_ab_scratch(b, L)) || (rc = smilehip_batch_create(plan->f0_plan, b->h_samp_off.data(), b->n_utt, &b->f0_batch)))
    return rc;
  const size_t nf = at_least_one(b->f0_batch->total_frames);
  if (b->d_pitch2.alloc(nf * 2) || b->d_jit4.alloc(nf * 4)) return fail(SMILEHIP_ERR_HIP, "hipMalloc of the F0 group's scratch matrices failed");
  return SMILEHIP_OK;
}

// cHarmonics reads gemapsv01b_fftmagG60, the level cSpecScale reads: lld_f0_spec keeps its magnitudes (2 KB per 60 ms frame) and
// lld_gemaps_harm starts from them instead of windowing and transforming every voiced frame a second time. Kept only while it
// is a modest part of what is free (the caller's output matrices come after this); SMILEHIP_HARM_KEEP_MAG=0 / =1 forces it.
static void try_keep_magnitudes(const smilehip_plan *f0_plan, smilehip_batch *fb) {
  if (fb->total_frames <= 0) return;
  const int64_t ld = (f0_plan->geo.K + 3) & ~int64_t(3);
  const size_t n = size_t(fb->total_frames) * size_t(ld);
  size_t free_b = 0, total_b = 0;
  const char *env = getenv("SMILEHIP_HARM_KEEP_MAG");
  bool keep = hipMemGetInfo(&free_b, &total_b) == hipSuccess && n * sizeof(float) <= free_b / 2;
  if (env && env[0] == '0') keep = false;
  if (env && env[0] == '1') keep = true;
  if (keep && fb->d_mag_keep.alloc(n) == SMILEHIP_OK)
    fb->mag_ld = ld;
  else
    (void)hipGetLastError();                              // (optional: cHarmonics transforms again without it)
}

static int alloc_egemaps_scratch(smilehip_plan *plan, smilehip_batch *b, const BatchLayout &L) {
  int rc;
  b->n_runs = (int32_t)L.run_utt.size();
  if ((rc = b->d_run_utt.upload(L.run_utt)) || (rc = b->d_run_t0.upload(L.run_t0)) || (rc = b->d_fin_off.upload(b->h_fin_off)) ||
      (rc = smilehip_batch_create(plan->f0_plan, b->h_samp_off.data(), b->n_utt, &b->f0_batch)))
    return rc;
  const size_t nf = at_least_one(b->total_frames), nf60 = at_least_one(b->f0_batch->total_frames), nfin = at_least_one(b->h_fin_off[b->n_utt]);
  if (b->d_raw20.alloc(nf * 12) || b->d_spec220.alloc(nf * 220) || b->d_lpc.alloc(nf * 12) || b->d_formants.alloc(nf * 10) ||
      b->d_pitch3.alloc(nf60 * 3) || b->d_jit4.alloc(nf60 * 4) || b->d_shim.alloc(nf60) || b->d_harm6.alloc(nf60 * 6) ||
      b->d_func_in.alloc(nfin * 36))
    return fail(SMILEHIP_ERR_HIP, "hipMalloc of the eGeMAPS scratch matrices failed (%.1f GB needed)",
                double(nf * 254 + nf60 * 14 + nfin * 36) * 4e-9);
  if ((rc = b->d_pending_j.upload(std::vector<int32_t>(at_least_one(b->n_utt), 0))) || (rc = b->d_harm_ctl.upload(std::vector<int32_t>(2, 0))) ||
      (rc = b->d_fm_flags.upload(std::vector<uint64_t>(2 * ((nf + 63) / 64), 0))))
    return rc;
  try_keep_magnitudes(plan->f0_plan, b->f0_batch);
  return SMILEHIP_OK;
}

extern "C" int smilehip_batch_create(smilehip_plan *plan, const int64_t *h_off, int32_t n_utt, smilehip_batch **out) {
  if (!plan || !out || n_utt < 0 || (n_utt > 0 && !h_off)) return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_create: bad argument");
  *out = nullptr;
  if (!plan->ctx) return fail(SMILEHIP_ERR_NO_DEVICE, "host-only plan: no device attached (tables only)");
  if (plan->stage_mask != SMILEHIP_STAGE_ALL) return fail(SMILEHIP_ERR_INVALID, "single-component plan cannot run the fused chain");
  if (plan->cfg.chain_kind != SMILEHIP_CHAIN_CHROMA_FILT)   // (the one chain without a transform: its blocks may be shorter than 64 samples)
    if (int rt = require_transform(plan, "smilehip_batch_create")) return rt;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  std::unique_ptr<smilehip_batch> b(new (std::nothrow) smilehip_batch());
  if (!b) return fail(SMILEHIP_ERR_NOMEM, "out of host memory");
  BatchLayout L;
  if (const int bad = batch_layout(layout_spec(plan), h_off, n_utt, L))
    return fail(SMILEHIP_ERR_INVALID, "sample offsets must be non-decreasing (utterance %d)", bad - 1);
  b->plan = plan;
  b->n_utt = n_utt;
  b->total_frames = L.total_frames; b->total_rows = L.total_rows;
  b->n_tiles = (int32_t)L.tile_utt.size(); b->n_dtiles = (int32_t)L.dtile_utt.size();
  b->run_frames = L.run_frames; b->all_even = L.all_even;
  int rc;
  if ((rc = b->d_samp_off.upload(L.samp_off)) || (rc = b->d_frame_off.upload(L.frame_off)) || (rc = b->d_row_off.upload(L.row_off)) ||
      (rc = b->d_tile_utt.upload(L.tile_utt)) || (rc = b->d_tile_t0.upload(L.tile_t0)) || (rc = b->d_tile_rec.upload(L.tile_rec)) ||
      (rc = b->d_dtile_utt.upload(L.dtile_utt)) || (rc = b->d_dtile_t0.upload(L.dtile_t0)) || (rc = b->d_short.upload(L.short_utts)))
    return rc;
  b->h_samp_off = std::move(L.samp_off);                  // what the runs and the functionals read on the host
  b->h_frame_off = std::move(L.frame_off); b->h_row_off = std::move(L.row_off);
  b->h_fin_off = std::move(L.fin_off); b->h_short = std::move(L.short_utts);
  switch (plan->cfg.chain_kind) {
    case SMILEHIP_CHAIN_IS09: rc = alloc_is09_scratch(b.get(), L); break;
    case SMILEHIP_CHAIN_COMPARE_AB: rc = alloc_compare_ab_scratch(b.get(), L); break;
    case SMILEHIP_CHAIN_COMPARE_F0: rc = alloc_f0_scratch(plan, b.get(), L); break;
    case SMILEHIP_CHAIN_PROSODY_SHS: rc = alloc_f0_frame_scratch(plan, b.get()); break;   // (no Viterbi, no jitter pass: their vectors stay empty)
    case SMILEHIP_CHAIN_PROSODY_ACF: rc = alloc_prosody_acf_scratch(b.get(), L); break;
    case SMILEHIP_CHAIN_CHROMA_FFT: rc = alloc_chroma_scratch(plan, b.get(), L); break;
    case SMILEHIP_CHAIN_CHROMA_FILT: rc = alloc_chroma_filt_scratch(plan, b.get()); break;
    case SMILEHIP_CHAIN_AUDSPEC: rc = alloc_audspec_scratch(plan, b.get(), L); break;
    case SMILEHIP_CHAIN_SPECTROGRAM: rc = alloc_spectrogram_scratch(b.get(), L); break;
    case SMILEHIP_CHAIN_EMOBASE: rc = alloc_emobase_scratch(plan, b.get(), L); break;
    case SMILEHIP_CHAIN_COMPARE: rc = alloc_compare_scratch(plan, b.get(), L); break;
    case SMILEHIP_CHAIN_EGEMAPS: rc = alloc_egemaps_scratch(plan, b.get(), L); break;
    case SMILEHIP_CHAIN_MFCC:
    case SMILEHIP_CHAIN_PLP: rc = alloc_mfcc_scratch(plan, b.get(), L); break;
  }
  if (rc) return rc;
  *out = b.release();
  return SMILEHIP_OK;
}

extern "C" void smilehip_batch_destroy(smilehip_batch *b) { delete b; }
extern "C" int64_t smilehip_batch_total_frames(const smilehip_batch *b) { return b ? b->total_frames : 0; }
extern "C" int64_t smilehip_batch_total_rows(const smilehip_batch *b) { return b ? b->total_rows : 0; }
extern "C" int smilehip_batch_delta_fused(const smilehip_batch *b) { return b && b->n_ftiles > 0 ? 1 : 0; }
extern "C" int smilehip_batch_frame_offsets(const smilehip_batch *b, int64_t *o) {
  if (!b || !o) return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_frame_offsets: null argument");
  std::memcpy(o, b->h_row_off.data(), b->h_row_off.size() * sizeof(int64_t));
  return SMILEHIP_OK;
}

// -------------------------------------------------------------------- run
static bool serial_forced() {                              // SMILEHIP_SERIAL=1: every kernel alone on the device (kernel tables)
  static const bool v = [] { const char *e = getenv("SMILEHIP_SERIAL"); return e && e[0] != '0'; }();
  return v;
}
static bool serial_streams(int64_t total_frames) {
  static const int forced = [] { const char *e = getenv("SMILEHIP_SERIAL"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
  return forced >= 0 ? forced != 0 : total_frames >= (int64_t)4000000;
}
static void fill_params(const smilehip_plan *p, const smilehip_batch *b, const int16_t *d_pcm, float *d_out,
                        int64_t ld, LldParams &P) {
  std::memset(&P, 0, sizeof(P));
  P.pcm = d_pcm;
  P.pcm_f32 = b->run_pcm_f32;
  P.pcm_total = b->h_samp_off.back();
  P.samp_off = b->d_samp_off.p;
  P.frame_off = b->d_frame_off.p;
  P.frame_utt = b->d_frame_utt.p;
  P.tile_utt = b->d_tile_utt.p;
  P.tile_t0 = b->d_tile_t0.p;
  P.tile_rec = b->d_tile_rec.p;
  P.ftile_rec = b->d_ftile_rec.p;
  P.n_ftiles = b->n_ftiles;
  P.n_utt = b->n_utt;
  P.n_tiles = b->n_tiles;
  P.total_frames = b->total_frames;
  P.out = d_out;
  P.ld_out = ld;
  P.N = (int32_t)p->geo.N;
  P.H = (int32_t)p->geo.H;
  P.Nfft = (int32_t)p->geo.Nfft;
  P.K = (int32_t)p->geo.K;
  P.pad_left = p->cfg.zero_pad_symmetric ? (int32_t)((p->geo.Nfft - p->geo.N) / 2) : 0;
  P.preemph = p->cfg.preemph;
  P.de = p->cfg.preemph_de;
  P.k = p->cfg.preemph_k;
  P.one_minus_k = 1 - p->cfg.preemph_k;     // (1-k) in float, vectorPreemphasis.cpp:94
  P.win_offset = (float)p->cfg.win_offset;
  P.window = p->d_window.p;
  P.oo = p->oo.tab();
  P.mel_coef = p->d_mel_coef.p;
  P.mel_rng = p->d_mel_rng.p;
  P.mel_scale = p->mel.scale;
  P.use_power = p->cfg.use_power;
  P.n_bands = p->mel.n_bands;
  P.dct_rows = p->d_dct_rows.p;
  P.dct_gain = p->d_dct_gain.p;
  P.n_mfcc = p->dct.n_mfcc;
  P.melfloor = p->dct.melfloor;
  P.log_floor = p->dct.log_floor;
  P.plp = p->cfg.chain_kind == SMILEHIP_CHAIN_PLP;
  P.plp_order = p->cfg.plp_lp_order;
  P.plp_compression = p->cfg.plp_compression;
  P.plp_eql = p->d_plp_eql.p;
  P.plp_cos = p->d_plp_cos.p;
  P.plp_sin = p->d_plp_sin.p;
}

// The window chain (lld_kernels.hip) over a batch's rows: level 0 = x, the batch's window-chain tiles and its short utterances.
// The caller sets the stages (copy_col, n_stages, kind[], W[], out_col[]).
static ChainParams chain_params(const smilehip_batch *b, const float *x, int64_t ld_x, int32_t D, float *out, int64_t ld_out) {
  ChainParams Q;
  std::memset(&Q, 0, sizeof(Q));
  Q.frame_off = b->d_frame_off.p;
  Q.row_off = b->d_row_off.p;
  Q.tile_utt = b->d_dtile_utt.p;
  Q.tile_t0 = b->d_dtile_t0.p;
  Q.n_tiles = b->n_dtiles;
  Q.n_utt = b->n_utt;
  Q.x = x;
  Q.ld_x = ld_x;
  Q.out = out;
  Q.ld_out = ld_out;
  Q.D = D;
  Q.short_T = chain_short_max();
  Q.short_utts = b->d_short.p;
  Q.n_short = (int32_t)b->h_short.size();
  return Q;
}

// R13 for a batch whose rows == frames: level 0 = x (leading dimension ld_x); writes [copy of x at copy_col (if >= 0) |
// order 1 at D | order 2 at 2D] into out
static int delta_chain_from(smilehip_plan *plan, smilehip_batch *b, const float *d_x, int64_t ld_x, int copy_col, float *d_io,
                            int64_t ld, int32_t D, int32_t W, int32_t n_orders, void *stream) {
  if (!plan || !b || !d_io) return fail(SMILEHIP_ERR_INVALID, "smilehip_delta_chain: null argument");
  if (n_orders < 1 || n_orders > 2 || W < 1 || W > 4 || D < 1 || D > 64 || ld < (int64_t)D * (1 + n_orders))   // D: column blocks of 16 on blockIdx.y
    return fail(SMILEHIP_ERR_INVALID, "smilehip_delta_chain: unsupported D=%d W=%d orders=%d ld=%lld", D, W, n_orders, (long long)ld);
  if (b->total_frames == 0) return SMILEHIP_OK;
  // rows == frames is what this entry point assumes (d_io holds the static block)
  if (b->total_rows != b->total_frames) return fail(SMILEHIP_ERR_INVALID, "smilehip_delta_chain: batch belongs to a chain with extra rows");
  ChainParams Q = chain_params(b, d_x, ld_x, D, d_io, ld);
  Q.copy_col = copy_col;
  Q.n_stages = n_orders;
  Q.kind[0] = Q.kind[1] = 0;
  Q.W[0] = Q.W[1] = W;
  Q.out_col[0] = D;
  Q.out_col[1] = 2 * D;
  hipError_t e = launch_chain(Q, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "window-chain kernel launch failed: %s", hipGetErrorString(e));
  return SMILEHIP_OK;
}

extern "C" int smilehip_delta_chain(smilehip_plan *plan, smilehip_batch *b, float *d_io, int64_t ld, int32_t D,
                                    int32_t W, int32_t n_orders, void *stream) {
  return delta_chain_from(plan, b, d_io, ld, -1, d_io, ld, D, W, n_orders, stream);
}

extern "C" int smilehip_mfcc_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out,
                                 int64_t ld_out, void *stream) {
  if (!plan || !b || b->plan != plan) return fail(SMILEHIP_ERR_INVALID, "smilehip_mfcc_run: plan/batch mismatch");
  if (plan->cfg.chain_kind != SMILEHIP_CHAIN_MFCC && plan->cfg.chain_kind != SMILEHIP_CHAIN_PLP)
    return fail(SMILEHIP_ERR_INVALID, "smilehip_mfcc_run: plan is not an MFCC / PLP chain (use smilehip_lld_run)");
  const int n_static = plan_n_static(plan), n_cep = plan->dct.n_mfcc;      // cepstra [+ log energy]
  const int n_out = n_static * (1 + plan->cfg.n_delta);
  if (ld_out < n_out) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < n_out %d", (long long)ld_out, n_out);
  if (b->total_frames == 0) return SMILEHIP_OK;
  if (!d_pcm || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_mfcc_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  // With deltas to follow, the static block goes to a compact [frames x n_mfcc] scratch: the frame kernel
  // then writes whole lines, the window-chain kernel reads 1/3 of what it would read from 39-float rows,
  // and writes every output row in one piece (static | delta | accel).
  const bool aligned_in = b->all_even && ((reinterpret_cast<uintptr_t>(d_pcm) & 3) == 0);
  const bool fused_delta = plan->use_fast && !b->run_pcm_f32 && b->n_ftiles > 0 && aligned_in;   // the regression stages inside the frame kernel
  const bool compact = !fused_delta && plan->cfg.n_delta > 0 && b->d_static.p != nullptr;
  if (compact) {
    P.out = b->d_static.p;
    P.ld_out = n_static;
  }
  hipEvent_t *ev = plan->ev[plan->n_timed % smilehip_plan::kRing];
  if (plan->timing) {
    for (int i = 0; i < 3; ++i)
      if (!ev[i]) HIP_TRY(hipEventCreate(&ev[i]));
    HIP_TRY(hipEventRecord(ev[0], s));
  }
  hipError_t e;
  if (plan->use_fast && !b->run_pcm_f32) {               // (float input: the reference-order kernel; the fast one converts int16 itself)
    Fast512Tables F;
    F.tw256 = plan->d_tw256.p;
    F.tw512 = plan->d_tw512.p;
    F.win = plan->d_fwin.p;
    F.melw = plan->d_melw.p;
    F.melo = plan->d_melo.p;
    F.dct28 = plan->d_dct28.p;
    F.lane_bands = plan->d_lane_bands.p;
    F.mel_units = plan->fast.mel_units;
    F.mel_scale = plan->fast.mel_scale;
    F.plp_eql = plan->d_plp_eql.p;
    F.plp_sin = plan->d_plp_sin.p;
    const bool aligned = aligned_in;
    e = launch_mfcc512(P, F, plan->fast, aligned, fused_delta, s);
  } else {
    e = launch_mfcc_generic(P, s);
  }
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "mfcc kernel launch failed: %s", hipGetErrorString(e));
  if (plan->cfg.append_log_energy) {                   // E variants: [energy:cEnergy] into the static block's last column
    e = launch_log_energy(P, b->d_dtile_utt.p, b->d_dtile_t0.p, b->n_dtiles, P.out, P.ld_out, n_cep, s);
    if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "log-energy kernel launch failed: %s", hipGetErrorString(e));
  }
  if (plan->timing) HIP_TRY(hipEventRecord(ev[1], s));
  if (fused_delta) {                                   // what is left: the tick-accurate path of the very short utterances, in place
    if (!b->h_short.empty()) {
      ChainParams Q = chain_params(b, d_out, ld_out, n_static, d_out, ld_out);
      Q.tile_utt = Q.tile_t0 = nullptr; Q.n_tiles = 0;   // (no tiles: the long utterances' rows are written already)
      Q.copy_col = -1;
      Q.n_stages = 2;
      Q.kind[0] = Q.kind[1] = 0;
      Q.W[0] = Q.W[1] = plan->cfg.delta_win;
      Q.out_col[0] = n_static;
      Q.out_col[1] = 2 * n_static;
      e = launch_chain(Q, s);
      if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "window-chain kernel launch failed: %s", hipGetErrorString(e));
    }
  } else if (plan->cfg.n_delta > 0) {
    int rc = compact ? delta_chain_from(plan, b, b->d_static.p, n_static, 0, d_out, ld_out, n_static,
                                        plan->cfg.delta_win, plan->cfg.n_delta, stream)
                     : smilehip_delta_chain(plan, b, d_out, ld_out, n_static, plan->cfg.delta_win, plan->cfg.n_delta, stream);
    if (rc) return rc;
  }
  if (plan->cfg.cms) {                                 // Z variants: [cms:cFullinputMean] on the cepstra of the output rows
    e = launch_cms(b->d_frame_off.p, b->n_utt, P.out, P.ld_out, d_out, ld_out, n_cep, s);   // P.out: the un-normalised block
    if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "mean-subtraction kernel launch failed: %s", hipGetErrorString(e));
  }
  if (plan->timing) {
    HIP_TRY(hipEventRecord(ev[2], s));
    plan->n_timed++;
  }
  return SMILEHIP_OK;
}

// HIP-event marks of the timing ring for the chains run through smilehip_lld_run: 0 / 1 bracket the chain's dominant frame
// kernel(s) ON THE STREAM THEY ARE LAUNCHED ON, 2 closes the run on the caller's stream (smilehip_plan_last_timing)
static int timing_mark(smilehip_plan *plan, int which, hipStream_t s) {
  if (!plan->timing) return SMILEHIP_OK;
  hipEvent_t *ev = plan->ev[plan->n_timed % smilehip_plan::kRing];
  if (!ev[which]) HIP_TRY(hipEventCreate(&ev[which]));
  HIP_TRY(hipEventRecord(ev[which], s));
  if (which == 2) plan->n_timed++;
  return SMILEHIP_OK;
}

// IS09 LLD set: frame kernel -> pitch smoother -> SMA + delta chain
static int is09_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream) {
  const int n_out = plan_n_out(plan);
  if (ld_out < n_out) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < n_out %d", (long long)ld_out, n_out);
  if (b->total_frames == 0) return SMILEHIP_OK;
  if (!d_pcm || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  Is09Params I;
  I.raw16 = b->d_raw16.p;
  I.fsSec = (float)plan->geo.fft_frame_size_sec;
  I.maxPitch = plan->cfg.pitch_max;
  I.voicingCutoff = plan->cfg.voicing_cutoff;
  if (I.voicingCutoff > 1.0) I.voicingCutoff = 1.0;       // pitchACF.cpp:96-98
  if (I.voicingCutoff < 0.0) I.voicingCutoff = 0.0;
  if (I.maxPitch < 0.0) I.maxPitch = 0.0;
  int trc;
  if ((trc = timing_mark(plan, 0, s))) return trc;
  hipError_t e = launch_is09(P, I, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "IS09 kernel launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, s))) return trc;
  ChainParams Q = chain_params(b, b->d_raw16.p, 16, 16, d_out, ld_out);
  Q.copy_col = -1;
  Q.n_stages = 2;
  Q.kind[0] = 1; Q.W[0] = plan->cfg.sma_win / 2;          // cContourSmoother
  Q.kind[1] = 0; Q.W[1] = plan->cfg.delta_win;            // cDeltaRegression
  Q.out_col[0] = 0;
  Q.out_col[1] = 16;
  e = launch_chain(Q, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "window-chain kernel launch failed: %s", hipGetErrorString(e));
  return timing_mark(plan, 2, s);
}

// SMILEHIP_CHAIN_PROSODY_ACF: lld_acf_pitch_frame (voicing, pitch candidate, loudness per frame) -> cPitchACF's contour per
// utterance -> cContourSmoother as one SMA stage of the window chain over the scratch's three columns
static int prosody_acf_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream) {
  if (ld_out < 3) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < n_out 3", (long long)ld_out);
  if (b->total_frames == 0) return SMILEHIP_OK;
  if (!d_pcm || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  ProsodyAcfParams A;
  std::memset(&A, 0, sizeof(A));
  A.raw3 = b->d_raw3.p;
  A.fsSec = (float)plan->geo.fft_frame_size_sec;          // the level's frameSizeSec: Tsamp = fsSec / Nfft (pitchACF.cpp:113-116, :151-153)
  A.cep_use_power = plan->cfg.acf_cep_use_power;
  A.maxPitch = plan->cfg.pitch_max;
  A.voicingCutoff = plan->cfg.voicing_cutoff;
  if (A.voicingCutoff > 1.0) A.voicingCutoff = 1.0;       // pitchACF.cpp:96-98
  if (A.voicingCutoff < 0.0) A.voicingCutoff = 0.0;
  if (A.maxPitch < 0.0) A.maxPitch = 0.0;
  // cIntensity::setupNamesForField (intensity.cpp:91-112): the Hamming window as doubles (smileUtil.c:1291-1303), summed in index order
  {
    const double NN = (double)plan->geo.N;
    double sum = 0.0;
    for (double i = 0.0; i < NN; i += 1.0) sum += 0.54 - 0.46 * std::cos((2.0 * M_PI * i) / (NN - 1.0));
    if (sum <= 0.0) sum = 1.0;
    A.win0 = 0.54 - 0.46 * std::cos((2.0 * M_PI * 0.0) / (NN - 1.0));
    A.win_sum = sum;
  }
  int trc;
  if ((trc = timing_mark(plan, 0, s))) return trc;
  hipError_t e = launch_prosody_acf(P, A, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "prosodyAcf kernel launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, s))) return trc;
  ChainParams Q = chain_params(b, b->d_raw3.p, 3, 3, d_out, ld_out);
  Q.copy_col = -1;
  Q.n_stages = 1;
  Q.kind[0] = 1; Q.W[0] = plan->cfg.sma_win / 2;          // cContourSmoother
  Q.out_col[0] = 0;
  e = launch_chain(Q, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "window-chain kernel launch failed: %s", hipGetErrorString(e));
  return timing_mark(plan, 2, s);
}

// SMILEHIP_CHAIN_CHROMA_FFT: one launch of lld_chroma_frame writes the tonespec level into the scratch and the chroma rows into d_out
static int chroma_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream) {
  const int n_out = plan->cfg.chroma_octave_size;
  if (ld_out < n_out) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < n_out %d", (long long)ld_out, n_out);
  if (b->total_frames == 0) return SMILEHIP_OK;
  if (!d_pcm || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  ChromaParams Q;
  std::memset(&Q, 0, sizeof(Q));
  Q.tonespec = b->d_tonespec.p;
  Q.fmap = plan->d_ts_fmap.p;
  Q.rec = plan->d_ts_rec.p;
  Q.n_notes = plan->tonespec.n_notes;
  Q.use_power = plan->cfg.tonespec_use_power != 0;
  Q.octave_size = n_out;
  Q.sil_thresh = plan->cfg.chroma_sil_thresh;
  int trc;
  if ((trc = timing_mark(plan, 0, s))) return trc;
  hipError_t e = launch_chroma(P, Q, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "chroma_fft kernel launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, s))) return trc;
  return timing_mark(plan, 2, s);
}

// SMILEHIP_CHAIN_CHROMA_FILT: lld_tonefilt_scan writes the tonespec level into the scratch, lld_chroma_rows the chroma rows into d_out
static int chroma_filt_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream) {
  const int n_out = plan->cfg.chroma_octave_size;
  if (ld_out < n_out) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < n_out %d", (long long)ld_out, n_out);
  if (b->total_frames == 0) return SMILEHIP_OK;
  if (!(d_pcm || b->run_pcm_f32) || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  TonefiltParams Q;
  std::memset(&Q, 0, sizeof(Q));
  Q.tab = plan->d_tf_tab.p;
  Q.n_notes = plan->tonefilt.n_notes;
  Q.P = (int32_t)plan->tonefilt.P;
  Q.period = plan->tonefilt.period;
  Q.samp_off = b->d_samp_off.p;
  Q.frame_off = b->d_frame_off.p;
  Q.n_utt = b->n_utt;
  Q.total_frames = b->total_frames;
  Q.tonespec = b->d_tonespec.p;
  int trc;
  if ((trc = timing_mark(plan, 0, s))) return trc;
  hipError_t e = launch_tonefilt(Q, d_pcm, b->run_pcm_f32, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "chroma_filt scan kernel launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, s))) return trc;
  e = stage_chroma(Q.n_notes, n_out, plan->cfg.chroma_sil_thresh, Q.tonespec, Q.n_notes, d_out, ld_out, b->total_frames, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "chroma_filt chroma kernel launch failed: %s", hipGetErrorString(e));
  return timing_mark(plan, 2, s);
}

// SMILEHIP_CHAIN_AUDSPEC: lld_audspec_frame writes the band rows -- into the compact static scratch when deltas follow, into d_out
// otherwise --, then the window chain writes static | de | de_de
static int audspec_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream) {
  const int n_static = plan_n_static(plan), n_out = plan_n_out(plan);
  if (ld_out < n_out) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < n_out %d", (long long)ld_out, n_out);
  if (b->total_frames == 0) return SMILEHIP_OK;
  if (!d_pcm || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  const bool compact = plan->cfg.n_delta > 0;              // (P.plp_eql: the chain's 64 HTK weights, P.melfloor: 1.0)
  if (compact) {
    if (!b->d_static.p) return fail(SMILEHIP_ERR_INVALID, "audspec chain: the batch has no static-block scratch");
    P.out = b->d_static.p;
    P.ld_out = n_static;
  }
  int trc;
  if ((trc = timing_mark(plan, 0, s))) return trc;
  hipError_t e = launch_audspec(P, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "audspec kernel launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, s))) return trc;
  if (compact) {
    const int rc = delta_chain_from(plan, b, b->d_static.p, n_static, 0, d_out, ld_out, n_static, plan->cfg.delta_win, plan->cfg.n_delta, stream);
    if (rc) return rc;
  }
  return timing_mark(plan, 2, s);
}

// SMILEHIP_CHAIN_SPECTROGRAM: one launch of lld_spectrogram_frame writes the K-wide rows into d_out in the plan's form as it is now
static int spectrogram_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream) {
  const int n_out = plan_n_out(plan);
  if (ld_out < n_out) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < n_out %d", (long long)ld_out, n_out);
  if (b->total_frames == 0) return SMILEHIP_OK;
  if (!d_pcm || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  int trc;
  if ((trc = timing_mark(plan, 0, s))) return trc;
  hipError_t e = launch_spectrogram(P, plan->spg_form, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "spectrogram kernel launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, s))) return trc;
  return timing_mark(plan, 2, s);
}

// SMILEHIP_CHAIN_EMOBASE: lld_emobase_frame (both framers' per-frame values) -> lld_emobase_lsp (cLpc, cLsp per 25 ms frame) ->
// cPitchACF's contour and F0env per utterance -> lld_emobase_tail (cContourSmoother and cDeltaRegression by the measured row rules)
static int emobase_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream) {
  const int n_out = plan_n_out(plan);
  if (ld_out < n_out) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < n_out %d", (long long)ld_out, n_out);
  if (b->emo_p != plan->emo_lpc_order)
    return fail(SMILEHIP_ERR_INVALID, "emobase chain: the batch was laid out for cLpc p = %d, the plan now has %d (smilehip_plan_set_lpc_order before smilehip_batch_create)",
                b->emo_p, plan->emo_lpc_order);
  if (b->total_frames == 0) return SMILEHIP_OK;
  if (!d_pcm || (!d_out && b->total_rows > 0)) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  EmobaseParams E;
  std::memset(&E, 0, sizeof(E));
  E.N40 = (int32_t)plan->geo40.N;
  E.Nfft40 = (int32_t)plan->geo40.Nfft;
  E.window40 = plan->d_window40.p;
  E.oo40 = plan->oo40.tab();
  E.fsSec40 = (float)plan->geo40.fft_frame_size_sec;      // the level's frameSizeSec: Tsamp = fsSec / Nfft (pitchACF.cpp:113-116, :151-153)
  E.maxPitch = plan->cfg.pitch_max;
  E.voicingCutoff = plan->cfg.voicing_cutoff;
  if (E.voicingCutoff > 1.0) E.voicingCutoff = 1.0;       // pitchACF.cpp:96-98
  if (E.voicingCutoff < 0.0) E.voicingCutoff = 0.0;
  if (E.maxPitch < 0.0) E.maxPitch = 0.0;
  // cIntensity::setupNamesForField (intensity.cpp:91-112): the Hamming window as doubles (smileUtil.c:1291-1303), summed in index order
  {
    const double NN = (double)plan->geo.N;
    double sum = 0.0;
    for (double i = 0.0; i < NN; i += 1.0) sum += 0.54 - 0.46 * std::cos((2.0 * M_PI * i) / (NN - 1.0));
    if (sum <= 0.0) sum = 1.0;
    E.w0 = 0.54 - 0.46 * std::cos((2.0 * M_PI * 0.0) / (NN - 1.0));
    E.w1 = 0.54 - 0.46 * std::cos((2.0 * M_PI * 1.0) / (NN - 1.0));
    E.win_sum = sum;
  }
  E.p = b->emo_p;
  E.n25 = emobase::n25_cols(E.p);
  E.W = plan->cfg.sma_win / 2;
  E.raw25 = b->d_raw25.p;
  E.raw3 = b->d_raw3.p;
  E.row_off = b->d_row_off.p;
  E.total_rows = b->total_rows;
  int trc;
  if ((trc = timing_mark(plan, 0, s))) return trc;
  hipError_t e = launch_emobase(P, E, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "emobase kernel launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, s))) return trc;
  return timing_mark(plan, 2, s);
}

// ComParE groups A+B: frame kernel -> RASTA scan -> group A (multi-length SMA+delta) + group B chain
static int compare_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream,
                       int de_col = 59) {
  const int n_out = plan_n_out(plan);
  if (ld_out < n_out) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < n_out %d", (long long)ld_out, n_out);
  if (b->total_frames == 0 || b->total_rows == 0) return SMILEHIP_OK;
  if (!d_pcm || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  CompareParams Q;
  std::memset(&Q, 0, sizeof(Q));
  Q.run_utt = b->d_run_utt.p;
  Q.run_t0 = b->d_run_t0.p;
  Q.run_frames = b->run_frames;
  Q.rawA = b->d_rawA.p;
  Q.rawB = b->d_rawB.p;
  Q.mel1 = b->d_mel1.p;
  Q.eql = plan->d_eql.p;
  Q.eql_log = plan->d_eql_log.p;
  Q.sharp_w = plan->d_sharp.p;
  Q.plp_melfloor = 0.00000000093f;     // cPlp melfloor default (plp.cpp:66), htkcompatible = 0
  Q.compression = 0.33f;
  Q.rasta_iir = plan->rasta_iir;
  for (int i = 0; i < 5; ++i) Q.rasta_fir[i] = plan->rasta_fir[i];
  Q.fsSec = plan->geo.fft_frame_size_sec;
  Q.N60 = (int32_t)samples_60ms(plan->geo.period);
  Q.max_utt_samples = 0;
  for (size_t u2 = 0; u2 + 1 < b->h_samp_off.size(); ++u2) Q.max_utt_samples = std::max<int64_t>(Q.max_utt_samples, b->h_samp_off[u2 + 1] - b->h_samp_off[u2]);
  for (int i = 0; i < 2; ++i) {
    Q.band_iL[i] = plan->band_iL[i]; Q.band_iR[i] = plan->band_iR[i];
    Q.band_wL[i] = plan->band_wL[i]; Q.band_wR[i] = plan->band_wR[i];
  }
  Q.slope_Sf = plan->slope_Sf;
  Q.slope_S2f = plan->slope_S2f;
  int trc;
  if ((trc = timing_mark(plan, 0, s))) return trc;
  hipError_t e = launch_compare(P, Q, b->n_runs, b->d_row_off.p, b->total_rows, d_out, ld_out, de_col, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "ComParE kernel launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, s))) return trc;
  ChainParams C = chain_params(b, b->d_rawB.p, 55, 55, d_out, ld_out);
  C.copy_col = -1;
  C.n_stages = 2;
  C.kind[0] = 1; C.W[0] = 1;
  C.kind[1] = 0; C.W[1] = 2;
  C.out_col[0] = 4;
  C.out_col[1] = de_col + 4;
  e = launch_chain(C, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "window-chain kernel launch failed: %s", hipGetErrorString(e));
  e = launch_compare_b_extra(b->d_frame_off.p, b->d_row_off.p, b->n_utt, b->d_rawB.p, b->d_b_extra.p, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "group-B extra-row kernel launch failed: %s", hipGetErrorString(e));
  return de_col == 59 ? timing_mark(plan, 2, s) : SMILEHIP_OK;     // (inside the whole-level chain the caller closes the run)
}

void fill_f0_params(const smilehip_plan *plan, F0Params &Q) {
  std::memset(&Q, 0, sizeof(Q));
  Q.N = (int32_t)plan->geo.N; Q.H = (int32_t)plan->geo.H; Q.Nfft = (int32_t)plan->geo.Nfft; Q.K = (int32_t)plan->geo.K;
  Q.pad_left = plan->cfg.zero_pad_symmetric ? (int32_t)((plan->geo.Nfft - plan->geo.N) / 2) : 0;
  Q.window = plan->d_window.p;
  Q.oo = plan->oo.tab();
  Q.sp_rec = plan->d_f0_rec.p; Q.sp_d1 = plan->d_f0_d1.p; Q.sp_d2 = plan->d_f0_d2.p;
  Q.ip_k = plan->d_f0_k.p; Q.ip_co = plan->d_f0_co.p; Q.audw = plan->d_f0_audw.p;
  Q.ip_rec = plan->d_f0_iprec.p; Q.ip_cnt = plan->d_f0_ipcnt.p; Q.sw_rec = plan->d_f0_swrec.p;
  Q.n_harm = plan->f0.n_harm;
  for (int i = 0; i < 16; ++i) { Q.shift[i] = plan->f0.shift[i]; Q.scale[i] = plan->f0.scale[i]; }
  Q.Fmint = plan->f0.Fmint; Q.Fstept = plan->f0.Fstept;
  Q.log_base = plan->f0.log_base;
  Q.min_pitch = plan->cfg.pitch_min; Q.max_pitch = plan->cfg.pitch_max;
  Q.voicing_cutoff = (float)plan->cfg.voicing_cutoff;
  Q.min_energy = plan->cfg.f0_min_energy;
  Q.jit_Tw = plan->geo.period;                 // 1.0 / (double)sampleRate, waveSource.cpp:190
  Q.jit_broken_thresh = plan->cfg.jitter_broken_thresh;
  Q.jit_step_sec = plan->cfg.frame_step_sec;
  Q.ld_tap = plan->geo.K;
  Q.ld_shs = 21;
  // [is13_pitchSmoothViterbi]: wLocal 2, wTvv 10, wTvvd 5, wTvuv 10, wThr 4, wRange 1 -- but
  // cSmileViterbiPitchSmooth::setWeights stores tvv into wTvvd (pitchSmootherViterbi.hpp:291-299): 10
  Q.vit_w[0] = 2.0; Q.vit_w[1] = 10.0; Q.vit_w[2] = 10.0; Q.vit_w[3] = 10.0; Q.vit_w[4] = 4.0; Q.vit_w[5] = 1.0;
  Q.vit_buf = plan->cfg.vit_buffer_len > 0 ? plan->cfg.vit_buffer_len : 30;
  Q.jit_search_range = plan->cfg.jitter_search_range > 0.0 ? plan->cfg.jitter_search_range : 0.25;
  Q.n_cand = plan->cfg.shs_n_candidates > 0 ? plan->cfg.shs_n_candidates : 6;
  Q.old_peaks = plan->cfg.shs_old_peak_algo ? 1 : 0;
  Q.scale_off = plan->cfg.specscale_off & 7;
}

// cPitchJitter's work items and redo marks of an F0-group batch (lld_jitter.hip)
static void set_jitter_items(const smilehip_batch *fb, F0Params &Q) {
  Q.jit_item_utt = fb->d_jit_utt.p;
  Q.jit_item_t0 = fb->d_jit_t0.p;
  Q.n_jit_items = (int32_t)fb->d_jit_utt.n;
  Q.jit_redo = fb->d_jit_redo.p;
  Q.jit_ctl = fb->d_jit_ctl.p;
  // (the chain's F0 values are cPitchShs candidates: inside [minPitch, maxPitch], pitchBase.cpp:211-222)
  Q.jit_cap = jitter_wave_capacity(Q.jit_Tw, Q.N, Q.min_pitch, Q.jit_search_range);
}

// The chunk pipeline of the frame kernels, where the batch holds a second set of rows (SMILEHIP_F0_PIPE=1)
static int f0_pipe_of(smilehip_plan *plan, smilehip_batch *b, const F0Pipe **pipe) {
  *pipe = nullptr;
  if (!b->d_f0_ab2.p || serial_forced()) return SMILEHIP_OK;
  F0Pipe &fp = plan->f0_pipe;
  if (!fp.spec) {
    HIP_TRY(hipStreamCreateWithFlags(&fp.spec, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&fp.sweep, hipStreamNonBlocking));
    for (hipEvent_t *ev_ : {&fp.start, &fp.spec_done[0], &fp.spec_done[1], &fp.sweep_done[0], &fp.sweep_done[1], &fp.cand_done[0], &fp.cand_done[1]})
      HIP_TRY(hipEventCreateWithFlags(ev_, hipEventDisableTiming));
  }
  fp.ab2 = b->d_f0_ab2.p;
  *pipe = &fp;
  return SMILEHIP_OK;
}

// log_out: rows [F0final, F0finalLog, voicingFinalUnclipped] (the eGeMAPS sub-chain, ld_out >= 3) instead of [F0final, voicing]
static int f0_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream,
                  bool log_out = false, hipEvent_t frames_done = nullptr) {
  if (ld_out < (log_out ? 3 : 2)) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld too small", (long long)ld_out);
  if (b->total_frames == 0) return SMILEHIP_OK;
  if (!d_pcm || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  if (plan->cfg.specscale_off & 7)
    return fail(SMILEHIP_ERR_INVALID, "the fused F0 chain runs cSpecScale with enhancement, smoothing and weighting on (specscale_off is for smilehip_specscale_frames)");
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  F0Params Q;
  fill_f0_params(plan, Q);
  Q.shs = b->d_shs.p;
  Q.e60 = b->d_e60.p;
  Q.ab = b->d_f0_ab.p;
  Q.ab_rows = f0_scratch_rows(b->n_tiles);
  Q.hps_tap = b->d_hps_tap;
  Q.mag_keep = b->d_mag_keep.p;
  Q.mag_ld = b->mag_ld;
  Q.pending = b->d_pending.p;
  Q.vit_log_out = log_out ? 1 : 0;
  int trc;
  if ((trc = timing_mark(plan, 0, (hipStream_t)stream))) return trc;       // (a sub-chain's plan never has timing switched on)
  const F0Pipe *pipe = nullptr;
  if ((trc = f0_pipe_of(plan, b, &pipe))) return trc;
  hipError_t e = launch_f0(P, Q, plan->ctx->prop.multiProcessorCount, d_out, ld_out, (hipStream_t)stream, frames_done, pipe);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "F0 kernel launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, (hipStream_t)stream))) return trc;
  return timing_mark(plan, 2, (hipStream_t)stream);
}

// SMILEHIP_CHAIN_PROSODY_SHS: the F0 front end's frame kernels (cPitchShs rows into the batch's scratch), then ONE kernel over the
// output rows: cPitchSmoother, cIntensity and cContourSmoother (lld_prosody.hip)
static int prosody_shs_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream) {
  if (ld_out < 3) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < n_out 3", (long long)ld_out);
  if (plan->cfg.specscale_off & 7)
    return fail(SMILEHIP_ERR_INVALID, "the fused prosodyShs chain runs cSpecScale with enhancement, smoothing and weighting on (specscale_off is for smilehip_specscale_frames)");
  if (b->total_frames == 0) return SMILEHIP_OK;
  if (!d_pcm || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  F0Params Q;
  fill_f0_params(plan, Q);
  Q.shs = b->d_shs.p;
  Q.e60 = b->d_e60.p;
  Q.ab = b->d_f0_ab.p;
  Q.ab_rows = f0_scratch_rows(b->n_tiles);
  Q.hps_tap = b->d_hps_tap;
  int trc;
  if ((trc = timing_mark(plan, 0, s))) return trc;
  const F0Pipe *pipe = nullptr;
  if ((trc = f0_pipe_of(plan, b, &pipe))) return trc;
  hipError_t e = launch_f0_frames(P, Q, s, pipe);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "F0 kernel launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, s))) return trc;
  ProsodyParams R;
  std::memset(&R, 0, sizeof(R));
  R.pcm = d_pcm;
  R.pcm_f32 = b->run_pcm_f32;
  R.samp_off = b->d_samp_off.p; R.frame_off = b->d_frame_off.p; R.row_off = b->d_row_off.p;
  R.tile_utt = b->d_dtile_utt.p; R.tile_t0 = b->d_dtile_t0.p; R.n_tiles = b->n_dtiles;
  R.H = (int32_t)plan->geo.H;
  R.shs = b->d_shs.p;
  R.voicing_cutoff = (float)plan->cfg.voicing_cutoff;
  R.W = plan->cfg.sma_win / 2;
  // cIntensity::setupNamesForField (intensity.cpp:91-112): the Hamming window as doubles (smileUtil.c:1291-1303), summed in index order
  {
    const double NN = (double)plan->geo.N;
    double sum = 0.0;
    for (double i = 0.0; i < NN; i += 1.0) sum += 0.54 - 0.46 * std::cos((2.0 * M_PI * i) / (NN - 1.0));
    if (sum <= 0.0) sum = 1.0;
    R.win0 = 0.54 - 0.46 * std::cos((2.0 * M_PI * 0.0) / (NN - 1.0));
    R.win_sum = sum;
  }
  R.out = d_out;
  R.ld_out = ld_out;
  e = launch_prosody_tail(R, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "prosodyShs tail kernel launch failed: %s", hipGetErrorString(e));
  return timing_mark(plan, 2, s);
}

// SMILEHIP_CHAIN_COMPARE: groups A+B into columns 6..64 / 71..129, the 60 ms sub-chain (F0 contour into scratch), then
// cPitchJitter and the F0 group's 12 LLD columns into 0..5 / 65..70
static int compare_full_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream) {
  if (ld_out < 130) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < 130", (long long)ld_out);
  if (b->total_rows == 0) return SMILEHIP_OK;
  if (!d_pcm || !d_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  // The two groups share nothing but the PCM. The F0 group's frame kernels fill the device; its Viterbi and jitter passes
  // are one wave per utterance: groups A+B start on the plan's side stream when the frame kernels are done and run beside
  // those (both groups filling the device at once only took turns).
  hipStream_t s = (hipStream_t)stream;
  smilehip_batch *fb = b->f0_batch;
  int rc = f0_run(plan->f0_plan, fb, d_pcm, b->d_pitch2.p, 2, stream, false, plan->ev_fork);
  if (rc) return rc;
  if (fb->total_frames == 0) HIP_TRY(hipEventRecord(plan->ev_fork, s));
  // Small batches: the one-wave-per-utterance passes leave most of the device idle (500 x 10 s: 32.8 -> 28.5 ms with the side stream).
  // Batches that fill the device on their own: rounds 3-5 measured one stream a hair faster (config 4 315 -> 313 ms); with round 6's
  // kernels the side stream is (217.5 / 218.1 / 218.9 ms on one stream, 216.6 / 217.7 / 217.5 beside: groups A+B fill the tails of the
  // Viterbi and jitter passes), so this chain always forks. The eGeMAPS chain keeps the threshold (config 5: 1012.5 on one stream, 1028.9
  // forked, 1029 with the 20 ms chain alone forked beside the Viterbi pass: profiles/r06_streams_ab.txt). SMILEHIP_SERIAL=1 forces one stream (a kernel trace then shows each kernel alone).
  const bool serial = serial_forced();
  hipStream_t side = serial ? s : plan->side_stream;
  HIP_TRY(hipStreamWaitEvent(side, plan->ev_fork, 0));
  if ((rc = compare_run(plan, b, d_pcm, d_out + 6, ld_out, side, 65))) return rc;
  HIP_TRY(hipEventRecord(plan->ev_join, side));
  LldParams P;
  fill_params(plan->f0_plan, fb, d_pcm, d_out, ld_out, P);
  F0Params Q;
  fill_f0_params(plan->f0_plan, Q);
  Q.pending = fb->d_pending.p;
  set_jitter_items(fb, Q);
  hipError_t e = launch_f0_lld(P, Q, b->d_row_off.p, b->d_pitch2.p, b->d_jit4.p, d_out, ld_out, 0, 65, (hipStream_t)stream);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "F0 LLD kernel launch failed: %s", hipGetErrorString(e));
  HIP_TRY(hipStreamWaitEvent(s, plan->ev_join, 0));
  return timing_mark(plan, 2, s);
}

// SMILEHIP_CHAIN_EGEMAPS: the 20 ms kernels on the plan's side stream, the F0 group on the caller's; then cPitchJitter and
// cHarmonics (which need the decided F0 contour, cHarmonics also the formants), then the selectors / smoothers
void gemaps_plan_consts(const smilehip_plan *plan, GemapsParams &G) {
  std::memset(&G, 0, sizeof(G));
  G.eql = plan->d_eql.p;
  G.plp_melfloor = 0.00000000093f;     // cPlp melfloor default (plp.cpp:66), htkcompatible = 0
  G.compression = 0.33f;
  G.fsSec = plan->geo.fft_frame_size_sec;
  for (int i = 0; i < 2; ++i) {
    G.sl_iL[i] = plan->gm_sl_iL[i]; G.sl_iR[i] = plan->gm_sl_iR[i];
    G.sl_wL[i] = plan->gm_sl_wL[i]; G.sl_wR[i] = plan->gm_sl_wR[i]; G.sl_Nind[i] = plan->gm_sl_Nind[i];
  }
  G.rng_lo = plan->gm_rng_lo; G.rng_hi = plan->gm_rng_hi;
  G.ar_n1 = plan->gm_ar_n1; G.ar_n2 = plan->gm_ar_n2;
  G.spec_floor = plan->gm_spec_floor; G.log_spec_floor = plan->gm_log_spec_floor; G.log_spec_factor = plan->gm_log_spec_factor;
  G.rs_cos = plan->d_rs_cos.p; G.rs_sin = plan->d_rs_sin.p;
  G.rs_norm = (float)(plan->geo.Nfft / 2);
  G.fm_T = 1.0 / plan->gm_target_fs;   // cSpecResample::configureWriter: basePeriod = 1 / targetFs
  G.fm_min = 50.0;                     // [gemapsv01b_formantLpc] minF; maxF 5450 (v01b / v02) or 5500 (v01a)
  G.fm_max = plan->cfg.formant_max_freq > 0.0 ? plan->cfg.formant_max_freq : 5450.0;
  G.fsSec60 = plan->f0_plan->geo.fft_frame_size_sec;
  G.lpc_ld = 12; G.fm_ld = 10;
}

static void fill_gemaps_params(const smilehip_plan *plan, const smilehip_batch *b, GemapsParams &G) {
  gemaps_plan_consts(plan, G);
  const smilehip_batch *fb = b->f0_batch;
  G.run_utt = b->d_run_utt.p; G.run_t0 = b->d_run_t0.p; G.run_frames = b->run_frames;
  G.raw20 = b->d_raw20.p; G.spec220 = b->d_spec220.p;
  G.lpc = b->d_lpc.p; G.formants = b->d_formants.p;
  G.total_frames20 = b->total_frames;
  G.fm_flags = b->d_fm_flags.p; G.frame_off20 = b->d_frame_off.p; G.n_utt20 = b->n_utt;
  G.pitch3 = b->d_pitch3.p; G.jit4 = b->d_jit4.p; G.shim_db = b->d_shim.p; G.harm6 = b->d_harm6.p;
  G.frame_off60 = fb->d_frame_off.p;
  G.tile60 = fb->d_tile_rec.p;
  G.n_tiles60 = fb->n_tiles;
  G.pending = fb->d_pending.p;
  G.harm_ctl = b->d_harm_ctl.p;
  G.mag60 = fb->d_mag_keep.p;
  G.mag60_ld = fb->mag_ld;
  G.func_in = b->d_func_in.p;
  G.fin_off = b->d_fin_off.p;
  G.pending_j = b->d_pending_j.p;
}

static int egemaps_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out, void *stream) {
  if (ld_out < 25) return fail(SMILEHIP_ERR_INVALID, "ld_out %lld < 25", (long long)ld_out);
  b->gm_ran = false;
  if (b->total_frames == 0) { b->gm_ran = true; return SMILEHIP_OK; }
  if (!d_pcm || (!d_out && b->total_rows > 0)) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: null device pointer");
  hipStream_t s = (hipStream_t)stream;
  smilehip_batch *fb = b->f0_batch;
  LldParams P;
  fill_params(plan, b, d_pcm, d_out, ld_out, P);
  GemapsParams G;
  fill_gemaps_params(plan, b, G);
  // The F0 group's frame kernels fill the device, its Viterbi and jitter passes are one wave per utterance: the 20 ms chain
  // (frame kernel, resampling + LPC, formant roots) starts on the side stream when the frame kernels are done
  hipError_t e = hipSuccess;
  const bool serial = serial_streams(b->total_frames);  // (see compare_full_run)
  hipStream_t side = serial ? s : plan->side_stream, bg = serial ? s : plan->bg_stream;
  if (fb->total_frames > 0) {
    int rc = f0_run(plan->f0_plan, fb, d_pcm, b->d_pitch3.p, 3, stream, true, plan->ev_fork);   // SHS candidates -> Viterbi -> energy gate
    if (rc) return rc;
  } else {
    HIP_TRY(hipEventRecord(plan->ev_fork, s));
  }
  HIP_TRY(hipStreamWaitEvent(side, plan->ev_fork, 0));
  int trc;
  if ((trc = timing_mark(plan, 0, side))) return trc;
  e = launch_gemaps_frames(P, G, b->n_runs, side);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "eGeMAPS 20 ms kernels: launch failed: %s", hipGetErrorString(e));
  if ((trc = timing_mark(plan, 1, side))) return trc;
  HIP_TRY(hipEventRecord(plan->ev_join, side));
  if (fb->total_frames > 0) {
    LldParams P60;
    fill_params(plan->f0_plan, fb, d_pcm, nullptr, 0, P60);
    F0Params Q;
    fill_f0_params(plan->f0_plan, Q);
    Q.jit_shim_db = b->d_shim.p;
    set_jitter_items(fb, Q);
    // cPitchJitter is one wave per utterance and latency-bound (a fifth of the VALU issue slots): it runs on the plan's
    // lowest-priority stream beside the 20 ms chain and cHarmonics instead of holding the wave slots they need
    HIP_TRY(hipEventRecord(plan->ev_bg_fork, s));
    HIP_TRY(hipStreamWaitEvent(bg, plan->ev_bg_fork, 0));
    e = launch_f0_jitter(P60, Q, b->d_pitch3.p, 3, b->d_jit4.p, bg);
    if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "jitter kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(plan->ev_bg_join, bg));
    HIP_TRY(hipStreamWaitEvent(s, plan->ev_join, 0));                          // cHarmonics reads the formants
    e = launch_gemaps_harm(P, Q, G, plan->ctx->prop.multiProcessorCount, s);
    if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "harmonics kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamWaitEvent(s, plan->ev_bg_join, 0));
  } else {
    HIP_TRY(hipStreamWaitEvent(s, plan->ev_join, 0));
  }
  e = launch_gemaps_tail(b->d_frame_off.p, b->d_row_off.p, b->n_utt, G, d_out, ld_out, s);
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "eGeMAPS tail kernel launch failed: %s", hipGetErrorString(e));
  b->gm_ran = true;
  return timing_mark(plan, 2, s);
}

extern "C" int smilehip_batch_f0_pending(smilehip_batch *b, const int32_t **d_pending) {
  if (!b || !d_pending) return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_f0_pending: null argument");
  const smilehip_batch *fb = b->f0_batch ? b->f0_batch : b;
  if (!fb->d_pending.p) return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_f0_pending: not an F0 / ComParE / eGeMAPS chain batch");
  *d_pending = fb->d_pending.p;
  return SMILEHIP_OK;
}

extern "C" int smilehip_batch_egemaps_taps(smilehip_batch *b, const float **d_raw20, const float **d_lpc, const float **d_formants,
                                           const float **d_pitch3, const float **d_jit4, const float **d_shim_db, const float **d_harm6,
                                           const float **d_func_in, const int32_t **d_pending, int64_t *h_frame_off60) {
  if (!b || b->plan->cfg.chain_kind != SMILEHIP_CHAIN_EGEMAPS) return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_egemaps_taps: not an eGeMAPS chain batch");
  if (d_raw20) *d_raw20 = b->d_raw20.p;
  if (d_lpc) *d_lpc = b->d_lpc.p;
  if (d_formants) *d_formants = b->d_formants.p;
  if (d_pitch3) *d_pitch3 = b->d_pitch3.p;
  if (d_jit4) *d_jit4 = b->d_jit4.p;
  if (d_shim_db) *d_shim_db = b->d_shim.p;
  if (d_harm6) *d_harm6 = b->d_harm6.p;
  if (d_func_in) *d_func_in = b->d_func_in.p;
  if (d_pending) *d_pending = b->f0_batch->d_pending.p;
  if (h_frame_off60) std::memcpy(h_frame_off60, b->f0_batch->h_frame_off.data(), b->f0_batch->h_frame_off.size() * sizeof(int64_t));
  return SMILEHIP_OK;
}

// prosodyAcf chain tap: the per-frame scratch of the last run, [total_frames x 3] = voiceProb | F0 (contour) | pcm_loudness
extern "C" int smilehip_batch_prosody_acf_taps(smilehip_batch *b, float **d_raw3, int64_t *n_frames) {
  if (!b || b->plan->cfg.chain_kind != SMILEHIP_CHAIN_PROSODY_ACF)
    return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_prosody_acf_taps: not a prosodyAcf chain batch");
  if (d_raw3) *d_raw3 = b->d_raw3.p;
  if (n_frames) *n_frames = b->total_frames;
  return SMILEHIP_OK;
}

// chroma_fft / chroma_filt chain tap: the level tonespec of the last run, [total_frames x n_notes]
extern "C" int smilehip_batch_chroma_taps(smilehip_batch *b, float **d_tonespec, int64_t *n_frames) {
  if (!b || (b->plan->cfg.chain_kind != SMILEHIP_CHAIN_CHROMA_FFT && b->plan->cfg.chain_kind != SMILEHIP_CHAIN_CHROMA_FILT))
    return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_chroma_taps: not a chroma_fft chain batch (nor a chroma_filt one)");
  if (d_tonespec) *d_tonespec = b->d_tonespec.p;
  if (n_frames) *n_frames = b->total_frames;
  return SMILEHIP_OK;
}

// emobase chain tap: the per-frame scratch of the last run (a row per 25 ms frame in both)
extern "C" int smilehip_batch_emobase_taps(smilehip_batch *b, float **d_raw25, float **d_raw3, int64_t *n_frames, int32_t *n25) {
  if (!b || b->plan->cfg.chain_kind != SMILEHIP_CHAIN_EMOBASE)
    return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_emobase_taps: not an emobase chain batch");
  if (d_raw25) *d_raw25 = b->d_raw25.p;
  if (d_raw3) *d_raw3 = b->d_raw3.p;
  if (n_frames) *n_frames = b->total_frames;
  if (n25) *n25 = emobase::n25_cols(b->emo_p);
  return SMILEHIP_OK;
}

// Test/diagnostic taps of the F0 chain: device pointers to the per-frame scratch of the LAST run
// (candidates: total_frames x 21, level is13_pitchShsG60; energy: total_frames, level is13_e60) and an optional
// destination for the octave-scaled spectra (total_frames x K, level is13_hpsG60; pass NULL to switch it off).
extern "C" int smilehip_batch_f0_taps(smilehip_batch *b, float *d_hps_dst, const float **d_shs, const float **d_e60) {
  if (!b || !f0_front_chain(b->plan->cfg.chain_kind))
    return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_f0_taps: not an F0 / prosodyShs chain batch");
  b->d_hps_tap = d_hps_dst;
  if (d_shs) *d_shs = b->d_shs.p;
  if (d_e60) *d_e60 = b->d_e60.p;
  return SMILEHIP_OK;
}

// ------------------------------------------------------------- functionals
extern "C" uint32_t smilehip_functionals_is09_mask(void) {
  return SMILEHIP_FUNC_MAX | SMILEHIP_FUNC_MIN | SMILEHIP_FUNC_RANGE | SMILEHIP_FUNC_MAXPOS | SMILEHIP_FUNC_MINPOS |
         SMILEHIP_FUNC_AMEAN | SMILEHIP_FUNC_LINREGC1 | SMILEHIP_FUNC_LINREGC2 | SMILEHIP_FUNC_LINREGERRQ |
         SMILEHIP_FUNC_STDDEV | SMILEHIP_FUNC_SKEWNESS | SMILEHIP_FUNC_KURTOSIS;
}

extern "C" int smilehip_functionals_count(uint32_t mask) {
  if (mask & ~SMILEHIP_FUNC_ALL) return -1;
  return __builtin_popcount(mask);
}

static const int kIs09FuncRowsCut = 3;      // rows = T+1; functionals see max(1, T-2)

extern "C" int smilehip_batch_func_rows(const smilehip_batch *b, int64_t *rows) {
  if (!b || !rows) return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_func_rows: null argument");
  if (b->plan->cfg.chain_kind != SMILEHIP_CHAIN_IS09)
    return fail(SMILEHIP_ERR_INVALID, "functionals are defined for IS09 chain plans only");
  for (int32_t u = 0; u < b->n_utt; ++u) {
    const int64_t r = b->h_row_off[u + 1] - b->h_row_off[u];
    rows[u] = r > 0 ? std::max<int64_t>(1, r - kIs09FuncRowsCut) : 0;
  }
  return SMILEHIP_OK;
}

extern "C" int smilehip_batch_functionals(smilehip_plan *plan, smilehip_batch *b, const float *d_lld, int64_t ld_lld,
                                          uint32_t mask, float *d_func, int64_t ld_func, void *stream) {
  if (!plan || !b || b->plan != plan) return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_functionals: plan/batch mismatch");
  if (plan->cfg.chain_kind != SMILEHIP_CHAIN_IS09)
    return fail(SMILEHIP_ERR_INVALID, "functionals are defined for IS09 chain plans only");
  const int per = smilehip_functionals_count(mask);
  if (per <= 0) return fail(SMILEHIP_ERR_INVALID, "invalid functionals mask 0x%x", mask);
  const int n_cols = plan_n_out(plan);
  if (ld_lld < n_cols || ld_func < (int64_t)n_cols * per)
    return fail(SMILEHIP_ERR_INVALID, "leading dimensions too small (ld_lld %lld, ld_func %lld)", (long long)ld_lld,
                (long long)ld_func);
  if (b->n_utt == 0) return SMILEHIP_OK;
  if (!d_func || (!d_lld && b->total_rows > 0)) return fail(SMILEHIP_ERR_INVALID, "smilehip_batch_functionals: null device pointer");
  // the mask is a cFunctionals instance with functionalsEnabled = Extremes;Regression;Moments, frame-normalised
  // positions and the linear regression only: one spec of the general engine (lld_funcspec.hip), which walks every
  // contour in the reference's order
  smilehip_func_spec spec;
  int rc = smilehip_funcspec_from_mask(mask, plan->geo.frame_period > 0.0 ? plan->geo.frame_period : 0.01, &spec);
  if (rc) return rc;
  return smilehip_batch_funcspec(plan, b, &spec, d_lld, ld_lld, 0, n_cols, kIs09FuncRowsCut, nullptr, 0, d_func, ld_func, stream);
}

extern "C" int smilehip_functionals_matrix(smilehip_context *ctx, const float *d_x, int64_t ld_x, int64_t rows, int32_t cols,
                                           uint32_t mask, float *d_out, void *stream) {
  const int per = smilehip_functionals_count(mask);
  if (!ctx || per <= 0 || rows < 1 || cols < 1 || ld_x < cols || !d_x || !d_out)
    return fail(SMILEHIP_ERR_INVALID, "smilehip_functionals_matrix: bad argument");
  smilehip_func_spec spec;
  int rc = smilehip_funcspec_from_mask(mask, 0.01, &spec);
  if (rc) return rc;
  return smilehip_funcspec_matrix(ctx, &spec, d_x, ld_x, rows, cols, d_out, stream);
}

extern "C" int smilehip_lld_run(smilehip_plan *plan, smilehip_batch *b, const int16_t *d_pcm, float *d_out, int64_t ld_out,
                                void *stream) {
  if (!plan || !b || b->plan != plan) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run: plan/batch mismatch");
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_MFCC || plan->cfg.chain_kind == SMILEHIP_CHAIN_PLP)
    return smilehip_mfcc_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_COMPARE_AB) return compare_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_COMPARE_F0) return f0_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_PROSODY_SHS) return prosody_shs_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_PROSODY_ACF) return prosody_acf_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_EMOBASE) return emobase_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FFT) return chroma_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FILT) return chroma_filt_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_AUDSPEC) return audspec_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_SPECTROGRAM) return spectrogram_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_COMPARE) return compare_full_run(plan, b, d_pcm, d_out, ld_out, stream);
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_EGEMAPS) return egemaps_run(plan, b, d_pcm, d_out, ld_out, stream);
  return is09_run(plan, b, d_pcm, d_out, ld_out, stream);
}

extern "C" int smilehip_lld_run_f32(smilehip_plan *plan, smilehip_batch *b, const float *d_pcm_f32, float *d_out, int64_t ld_out,
                                    void *stream) {
  if (!plan || !b || b->plan != plan) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run_f32: plan/batch mismatch");
  if (!d_pcm_f32 && b->total_frames > 0) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run_f32: null device pointer");
  b->run_pcm_f32 = d_pcm_f32;
  if (b->f0_batch) b->f0_batch->run_pcm_f32 = d_pcm_f32;
  // the int16 pointer is never dereferenced while run_pcm_f32 is set (PcmIn, lld_device.hpp); it only has to be non-null
  const int rc = smilehip_lld_run(plan, b, reinterpret_cast<const int16_t *>(d_pcm_f32), d_out, ld_out, stream);
  b->run_pcm_f32 = nullptr;
  if (b->f0_batch) b->f0_batch->run_pcm_f32 = nullptr;
  return rc;
}

extern "C" int smilehip_lld_run_host(smilehip_plan *plan, smilehip_batch *b, const int16_t *h_pcm, int64_t n_samples,
                                     float *h_out) {
  if (!plan || !b || b->plan != plan) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run_host: plan/batch mismatch");
  if (n_samples < b->h_samp_off.back()) return fail(SMILEHIP_ERR_INVALID, "PCM buffer shorter than the batch layout");
  if (b->total_rows == 0) return SMILEHIP_OK;
  if (!h_pcm || !h_out) return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_run_host: null pointer");
  HIP_TRY(hipSetDevice(plan->ctx->device));
  const int n_out = plan_n_out(plan);
  int16_t *d_pcm = nullptr;
  float *d_out = nullptr;
  HIP_TRY(hipMalloc((void **)&d_pcm, size_t(n_samples) * sizeof(int16_t)));
  hipError_t e = hipMalloc((void **)&d_out, size_t(b->total_rows) * n_out * sizeof(float));
  if (e != hipSuccess) {
    (void)hipFree(d_pcm);
    return fail(SMILEHIP_ERR_HIP, "hipMalloc(out) failed: %s", hipGetErrorString(e));
  }
  int rc = SMILEHIP_OK;
  e = hipMemcpy(d_pcm, h_pcm, size_t(n_samples) * sizeof(int16_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    rc = smilehip_lld_run(plan, b, d_pcm, d_out, n_out, nullptr);
    if (rc == SMILEHIP_OK) e = hipMemcpy(h_out, d_out, size_t(b->total_rows) * n_out * sizeof(float), hipMemcpyDeviceToHost);
  }
  (void)hipFree(d_pcm);
  (void)hipFree(d_out);
  if (rc) return rc;
  if (e != hipSuccess) return fail(SMILEHIP_ERR_HIP, "HIP copy failed: %s", hipGetErrorString(e));
  return SMILEHIP_OK;
}

extern "C" int smilehip_mfcc_run_host(smilehip_plan *plan, smilehip_batch *b, const int16_t *h_pcm, int64_t n_samples,
                                      float *h_out) {
  if (!plan || plan->cfg.chain_kind != SMILEHIP_CHAIN_MFCC) return fail(SMILEHIP_ERR_INVALID, "smilehip_mfcc_run_host: plan is not an MFCC chain");
  return smilehip_lld_run_host(plan, b, h_pcm, n_samples, h_out);
}

extern "C" int smilehip_plan_set_timing(smilehip_plan *plan, int enable) {
  if (!plan) return fail(SMILEHIP_ERR_INVALID, "null plan");
  plan->timing = enable != 0;
  plan->n_timed = 0;
  return SMILEHIP_OK;
}

// Average over the runs recorded since set_timing (at most the last kRing).
// The caller must have synchronised the stream.
extern "C" int smilehip_plan_last_timing(smilehip_plan *plan, float *ms_main, float *ms_delta) {
  if (!plan || plan->n_timed <= 0) return fail(SMILEHIP_ERR_INVALID, "no timing recorded");
  const int64_t n = plan->n_timed < smilehip_plan::kRing ? plan->n_timed : smilehip_plan::kRing;
  double sa = 0.0, sd = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    float a = 0.f, d = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, plan->ev[i][0], plan->ev[i][1]));
    HIP_TRY(hipEventElapsedTime(&d, plan->ev[i][1], plan->ev[i][2]));
    sa += a;
    sd += d;
  }
  if (ms_main) *ms_main = float(sa / double(n));
  if (ms_delta) *ms_delta = float(sd / double(n));
  return SMILEHIP_OK;
}
