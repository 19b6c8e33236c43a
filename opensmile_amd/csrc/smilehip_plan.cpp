// libsmilehip, C ABI part 2: configuration presets, plan creation (host tables -> device), plan getters.
#include "smilehip_internal.hpp"

static_assert(offsetof(smilehip_lld_config, acf_cep_use_power) + sizeof(int32_t) == SMILEHIP_LLD_CONFIG_SIZE_V1,
              "SMILEHIP_LLD_CONFIG_SIZE_V1 is the struct's size up to and including acf_cep_use_power");
static_assert(offsetof(smilehip_lld_config, tonespec_n_octaves) == SMILEHIP_LLD_CONFIG_SIZE_V1, "the chroma fields start where the older struct ends");
static_assert(offsetof(smilehip_lld_config, reserved_chroma) + sizeof(int32_t) == SMILEHIP_LLD_CONFIG_SIZE_V2 &&
                  offsetof(smilehip_lld_config, tonefilt_n_notes) == SMILEHIP_LLD_CONFIG_SIZE_V2,
              "SMILEHIP_LLD_CONFIG_SIZE_V2 is the struct's size up to and including reserved_chroma; the tonefilt fields start there");

// the base of every preset that existed before the struct grew: it fills SMILEHIP_LLD_CONFIG_SIZE_V1 bytes and says so in struct_size (the
// header's struct_size rules: a caller whose struct ends there is not written past its end)
extern "C" void smilehip_config_mfcc12_0_d_a(smilehip_lld_config *c) {
  std::memset(c, 0, SMILEHIP_LLD_CONFIG_SIZE_V1);
  c->struct_size = SMILEHIP_LLD_CONFIG_SIZE_V1;
  c->sample_rate = 16000.0;
  c->frame_size_sec = 0.0250;
  c->frame_step_sec = 0.010;
  c->preemph = 1;
  c->preemph_k = 0.97f;
  c->preemph_de = 0;
  c->win_func = SMILEHIP_WIN_HAMM;
  c->win_sigma = 0.4;
  c->win_gain = 1.0;
  c->win_offset = 0.0;
  c->zero_pad_symmetric = 0;
  c->n_bands = 26;
  c->lofreq = 0.0f;
  c->hifreq = 8000.0f;
  c->use_power = 1;
  c->mel_htk_compatible = 1;
  c->first_mfcc = 0;
  c->last_mfcc = 12;
  c->cep_lifter = 22.0f;
  c->mfcc_htk_compatible = 1;
  c->melfloor = 1e-8f;
  c->n_delta = 2;
  c->delta_win = 2;
}

extern "C" void smilehip_config_is09_lld(smilehip_lld_config *c) {
  smilehip_config_mfcc12_0_d_a(c);
  c->chain_kind = SMILEHIP_CHAIN_IS09;
  c->use_power = 0;            // [is09_mspec] usePower = 0
  c->first_mfcc = 1;
  c->last_mfcc = 12;
  c->n_delta = 1;
  c->delta_win = 2;
  c->pitch_max = 500.0;
  c->voicing_cutoff = 0.55;
  c->sma_win = 3;
}

extern "C" void smilehip_config_plp_0_d_a(smilehip_lld_config *c) {
  smilehip_config_mfcc12_0_d_a(c);        // same front end: 25 ms / 10 ms, k = 0.97, ham, 26 HTK mel bands
  c->chain_kind = SMILEHIP_CHAIN_PLP;
  c->plp_lp_order = 5;                    // [plp:cPlp] lpOrder = 5, compression = 0.33, cepLifter = 22
  c->plp_compression = 0.33f;
  c->cep_lifter = 22.0f;
  c->first_mfcc = 0;
  c->last_mfcc = 5;
}

extern "C" int smilehip_config_htk_variant(smilehip_lld_config *c, const char *name) {
  if (!c || !name) return fail(SMILEHIP_ERR_INVALID, "smilehip_config_htk_variant: null argument");
  std::string n(name);
  const bool plp = n.rfind("PLP_", 0) == 0, mfcc = n.rfind("MFCC12_", 0) == 0;
  if (!plp && !mfcc) return fail(SMILEHIP_ERR_INVALID, "unknown config name '%s'", name);
  std::string rest = n.substr(plp ? 4 : 7);
  bool z = false;
  if (rest.size() > 2 && rest.compare(rest.size() - 2, 2, "_Z") == 0) { z = true; rest.resize(rest.size() - 2); }
  if (rest != "0_D_A" && rest != "E_D_A") return fail(SMILEHIP_ERR_INVALID, "unknown config name '%s'", name);
  const bool e = rest[0] == 'E';
  if (plp) smilehip_config_plp_0_d_a(c); else smilehip_config_mfcc12_0_d_a(c);
  if (e) { c->first_mfcc = 1; c->append_log_energy = 1; }     // [mfcc] firstMfcc = 1 / [plp] firstCC = 1, [energy:cEnergy]
  if (z) { c->cms = 1; c->zero_pad_symmetric = 1; }           // the _Z files do not set [fft] zeroPadSymmetric = 0
  return SMILEHIP_OK;
}

extern "C" void smilehip_config_compare16_ab(smilehip_lld_config *c) {
  smilehip_config_mfcc12_0_d_a(c);
  c->chain_kind = SMILEHIP_CHAIN_COMPARE_AB;
  c->frame_size_sec = 0.020;       // [is13_frame25]
  c->preemph = 0;
  c->win_func = SMILEHIP_WIN_HAMM; // [is13_win25]
  c->zero_pad_symmetric = 1;       // [is13_fft25]
  c->lofreq = 20.0f;               // [is13_melspec1], [is13_melspecMfcc]
  c->use_power = 1;
  c->first_mfcc = 1;               // [is13_mfcc]
  c->last_mfcc = 14;
  c->n_delta = 1;
  c->delta_win = 2;
  c->sma_win = 3;
}

extern "C" void smilehip_config_compare16_f0(smilehip_lld_config *c) {
  smilehip_config_mfcc12_0_d_a(c);
  c->chain_kind = SMILEHIP_CHAIN_COMPARE_F0;
  c->frame_size_sec = 0.060;        // [is13_frame60]
  c->preemph = 0;
  c->win_func = SMILEHIP_WIN_GAUSS; // [is13_win60] sigma 0.4
  c->win_sigma = 0.4;
  c->zero_pad_symmetric = 1;        // [is13_fft60]
  c->n_delta = 0;
  c->pitch_min = 52.0;              // [is13_shs]
  c->pitch_max = 620.0;
  c->voicing_cutoff = 0.7;
  c->shs_n_harmonics = 15;
  c->shs_compression = 0.85f;
  c->f0_min_energy = 0.001f;        // [is13_volmerge] threshold
}

extern "C" void smilehip_config_compare16(smilehip_lld_config *c) {
  smilehip_config_compare16_ab(c);
  c->chain_kind = SMILEHIP_CHAIN_COMPARE;
  // the F0 group's parameters (forwarded to the 60 ms sub-chain by smilehip_plan_create): [is13_shs], [is13_volmerge],
  // [is13_pitchSmoothViterbi] bufferLength, [is13_pitchJitter] searchRangeRel
  c->pitch_min = 52.0;
  c->pitch_max = 620.0;
  c->voicing_cutoff = 0.7;
  c->shs_n_harmonics = 15;
  c->shs_compression = 0.85f;
  c->f0_min_energy = 0.001f;
  c->vit_buffer_len = 30;
  c->jitter_search_range = 0.25;
}

// config/is09-13/IS13_ComParE_core.lld.conf.inc = ComParE_2016_core.lld.conf.inc except [is13_fft25] / [is13_fft60]
// zeroPadSymmetric = 0 and [is13_pitchJitter] useBrokenJitterThresh = 1
extern "C" void smilehip_config_is13_compare(smilehip_lld_config *c) {
  smilehip_config_compare16(c);
  c->zero_pad_symmetric = 0;
  c->jitter_broken_thresh = 1;
}

// config/egemaps/v02/eGeMAPSv02.conf: the 20 ms chain of GeMAPSv01b_core.lld.conf.inc ([gemapsv01b_frame25] 20 ms / 10 ms,
// Hamming, symmetric zero padding, 26 mel bands from 20 Hz; [egemapsv02_mfcc] 1..4, lifter 22); the 60 ms sub-chain is
// created by smilehip_plan_create
extern "C" void smilehip_config_egemapsv02(smilehip_lld_config *c) {
  smilehip_config_compare16_ab(c);
  c->chain_kind = SMILEHIP_CHAIN_EGEMAPS;
  c->first_mfcc = 1;
  c->last_mfcc = 4;
  c->n_delta = 0;
  c->sma_win = 3;
  c->pitch_min = 55.0;               // [gemapsv01b_shs]
  c->pitch_max = 1000.0;
  c->voicing_cutoff = 0.7;
  c->shs_n_harmonics = 15;
  c->shs_compression = 0.85f;
  c->f0_min_energy = 0.001f;         // [gemapsv01b_volmerge]
  c->vit_buffer_len = 40;            // [gemapsv01b_pitchSmoothViterbi] bufferLength
  c->jitter_search_range = 0.1;      // [gemapsv01b_pitchJitter] searchRangeRel
}

extern "C" void smilehip_config_egemapsv01a(smilehip_lld_config *c) {
  smilehip_config_egemapsv02(c);
  c->zero_pad_symmetric = 0;         // [gemapsv01a_fft60] / [gemapsv01a_fft25]: "for compatibility with 2.2.0 and older versions"
  c->jitter_broken_thresh = 1;       // [gemapsv01a_pitchJitter]
  c->formant_max_freq = 5500.0;      // [gemapsv01a_formantLpc]
}

// config/prosody/prosodyShs.conf: the F0 front end on 50 ms frames, cPitchSmoother without state, cIntensity loudness, SMA(3)
extern "C" void smilehip_config_prosody_shs(smilehip_lld_config *c) {
  smilehip_config_compare16_f0(c);   // [win] gauss 0.4, [scale] minF 25 (specscale_min_f 0), [shs] 52 .. 620 Hz, 15 harmonics, 0.85, cutoff 0.7
  c->chain_kind = SMILEHIP_CHAIN_PROSODY_SHS;
  c->frame_size_sec = 0.050;         // [frame:cFramer] frameSize = 0.050, frameStep = 0.010
  c->zero_pad_symmetric = 0;         // [fft:cTransformFFT]
  c->shs_n_candidates = 4;           // [shs:cPitchShs] nCandidates = 4
  c->shs_old_peak_algo = 1;          // ... greedyPeakAlgo not set: 0 (pitchShs.cpp:286-302)
  c->f0_min_energy = 0.0f;           // (no cValbasedSelector in this file)
  c->sma_win = 3;                    // [smo:cContourSmoother] smaWin = 3
}

// config/prosody/prosodyAcf.conf: ACF / cepstrum pitch on 50 ms gauss-windowed frames, cIntensity loudness, SMA(3)
extern "C" void smilehip_config_prosody_acf(smilehip_lld_config *c) {
  smilehip_config_mfcc12_0_d_a(c);   // (the mel / DCT fields are not read by this chain)
  c->chain_kind = SMILEHIP_CHAIN_PROSODY_ACF;
  c->frame_size_sec = 0.050;         // [frame:cFramer] frameSize = 0.050, frameStep = 0.010
  c->preemph = 0;
  c->win_func = SMILEHIP_WIN_GAUSS;  // [win:cWindower] winFunc = gauss, sigma = 0.4, gain = 1
  c->win_sigma = 0.4;
  c->zero_pad_symmetric = 0;         // [fft:cTransformFFT]
  c->n_delta = 0;
  c->pitch_max = 500.0;              // [pitch:cPitchACF] maxPitch = 500, voicingCutoff = 0.55
  c->voicing_cutoff = 0.55;
  c->acf_cep_use_power = 0;          // [cep:cAcf] sets cepstrum = 1 only: usePower stays 0 (acf.cpp:91-102)
  c->sma_win = 3;                    // [smo:cContourSmoother] smaWin = 3
}

// config/chroma/chroma_fft.conf: the struct as far as its own fields reach (SMILEHIP_LLD_CONFIG_SIZE_V2)
extern "C" void smilehip_config_chroma_fft(smilehip_lld_config *c, double sample_rate) {
  std::memset(c, 0, SMILEHIP_LLD_CONFIG_SIZE_V2);
  smilehip_config_mfcc12_0_d_a(c);   // (the mel / DCT fields are not read by this chain)
  c->struct_size = SMILEHIP_LLD_CONFIG_SIZE_V2;
  c->chain_kind = SMILEHIP_CHAIN_CHROMA_FFT;
  c->sample_rate = sample_rate;
  c->frame_size_sec = 0.064;         // [framer:cFramer] frameSize = 0.064, frameStep = 0.010
  c->frame_step_sec = 0.010;
  c->preemph = 0;
  c->win_func = SMILEHIP_WIN_GAUSS;  // [windower:cWindower] winFunc = Gau, sigma = 0.4, gain = 1, offset = 0
  c->win_sigma = 0.4;
  c->zero_pad_symmetric = 1;         // [transformFFT:cTransformFFT] sets nothing: the component's default
  c->n_delta = 0;
  c->tonespec_n_octaves = 6;         // [tonespec:cTonespec]
  c->tonespec_first_note = 55.0f;
  c->tonespec_filter_type = SMILEHIP_TONESPEC_GAUSS;
  c->tonespec_use_power = 1;
  c->tonespec_dba = 1;
  c->chroma_octave_size = 12;        // [chroma:cChroma]
  c->chroma_sil_thresh = (float)0.001;   // the default (chroma.cpp:49), kept as FLOAT_DMEM (:71)
}

// config/chroma/chroma_filt.conf: the full struct
extern "C" void smilehip_config_chroma_filt(smilehip_lld_config *c, double sample_rate) {
  std::memset(c, 0, sizeof(*c));
  smilehip_config_mfcc12_0_d_a(c);   // (nothing of the window / transform / mel / DCT part is read by this chain)
  c->struct_size = sizeof(*c);
  c->chain_kind = SMILEHIP_CHAIN_CHROMA_FILT;
  c->sample_rate = sample_rate;
  c->tonefilt_n_notes = 72;          // [tonefilt:cTonefilt]
  c->tonefilt_first_note = 55.0;
  c->tonefilt_decay_f0 = 0.9999;
  c->tonefilt_decay_fn = 0.999;
  c->tonefilt_output_period = 0.01;
  c->frame_size_sec = c->frame_step_sec = c->tonefilt_output_period;   // the block length as the plan's frame geometry
  c->preemph = 0;
  c->win_func = SMILEHIP_WIN_RECT;
  c->n_delta = 0;
  c->chroma_octave_size = 12;        // [chroma:cChroma]
  c->chroma_sil_thresh = (float)0.001;
}

// config/audspec/audspec.conf: the MFCC12 front end, cPlp as auditory spectrum in cMfcc's place; every field lies in V1
extern "C" void smilehip_config_audspec(smilehip_lld_config *c) {
  smilehip_config_mfcc12_0_d_a(c);   // 25 ms / 10 ms, k = 0.97, ham, 26 HTK power mel bands 0 .. 8000 Hz, two delta stages of deltawin 2
  c->chain_kind = SMILEHIP_CHAIN_AUDSPEC;
  c->zero_pad_symmetric = 1;         // [audspec_fft:cTransformFFT] sets nothing: the component's default
  c->plp_compression = 0.33f;        // [audspec_plp:cPlp] compression = 0.33
  c->plp_lp_order = 5;               // (lpOrder = 5, firstCC = 0, cepLifter = 22: as the file has them; not read by this chain)
  c->first_mfcc = 0;
  c->last_mfcc = 5;
}
extern "C" void smilehip_config_audspec_compat(smilehip_lld_config *c) {
  smilehip_config_audspec(c);
  c->zero_pad_symmetric = 0;         // [fft:cTransformFFT] zeroPadSymmetric = 0: "for compatibility with 2.2.0 and older versions"
}

// config/spectrum/spectrogram.conf: framer, Hamming window, transform, cFFTmagphase; every field lies in V1
extern "C" void smilehip_config_spectrogram(smilehip_lld_config *c) {
  smilehip_config_mfcc12_0_d_a(c);   // 25 ms / 10 ms, ham, gain 1, offset 0 (the mel / DCT fields are not read by this chain)
  c->chain_kind = SMILEHIP_CHAIN_SPECTROGRAM;
  c->preemph = 0;                    // the file has no cVectorPreemphasis
  c->zero_pad_symmetric = 1;         // [fft:cTransformFFT] sets nothing: the component's default
  c->n_delta = 0;
}

// config/emobase/emobase.conf, levels lld and lld_de; every field lies in V1 (cLpc's order is the plan's: smilehip_plan_set_lpc_order)
extern "C" void smilehip_config_emobase(smilehip_lld_config *c) {
  smilehip_config_mfcc12_0_d_a(c);   // [fr25] 25 ms / 10 ms, [pe] k = 0.97, [win] ham, [fft] zeroPadSymmetric = 0, [mspec] 26 HTK power bands 0 .. 8000 Hz
  c->chain_kind = SMILEHIP_CHAIN_EMOBASE;
  c->first_mfcc = 1;                 // [mfcc:cMfcc] firstMfcc = 1, lastMfcc = 12, cepLifter = 22, htkcompatible
  c->last_mfcc = 12;
  c->n_delta = 1;                    // [delta1:cDeltaRegression] deltawin = 2
  c->delta_win = 2;
  c->pitch_max = 500.0;              // [pitchACF:cPitchACF] maxPitch = 500, voicingCutoff = 0.55
  c->voicing_cutoff = 0.55;
  c->sma_win = 3;                    // [lld:cContourSmoother] smaWin = 3
}

static inline bool is_compare_ab_like(const smilehip_lld_config &c) {
  return c.chain_kind == SMILEHIP_CHAIN_COMPARE_AB || c.chain_kind == SMILEHIP_CHAIN_COMPARE;
}

// ------------------------------------------------------------------- plan
// the caller's struct as far as its struct_size reaches (the header's struct_size rules), zeros behind it
static bool config_size_known(uint32_t n) {
  return n == sizeof(smilehip_lld_config) || n == SMILEHIP_LLD_CONFIG_SIZE_V2 || n == SMILEHIP_LLD_CONFIG_SIZE_V1;
}
static void copy_config(smilehip_lld_config &dst, const smilehip_lld_config *src) {
  std::memset(&dst, 0, sizeof(dst));
  std::memcpy(&dst, src, std::min<size_t>(src->struct_size, sizeof(dst)));
}

static int build_tables(smilehip_plan *p, bool upload = true) {
  int rc;
  if ((rc = make_geometry(p->cfg, p->geo)) != SMILEHIP_OK) return fail(rc, "invalid framing parameters");
  if (p->geo.Nfft > 8192) return fail(SMILEHIP_ERR_INVALID, "FFT length %lld > 8192 unsupported", (long long)p->geo.Nfft);
  const uint32_t mask = p->cfg.stage_mask ? p->cfg.stage_mask : SMILEHIP_STAGE_ALL;
  // the tables built: the prosodyAcf chain has no mel bank and no DCT (its frames may be shorter than a bank has bands)
  const bool no_mel = p->cfg.chain_kind == SMILEHIP_CHAIN_PROSODY_ACF || p->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FFT ||
                      p->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FILT ||   // (chroma_fft and chroma_filt likewise,
                      p->cfg.chain_kind == SMILEHIP_CHAIN_SPECTROGRAM;     //  and the spectrogram chain)
  const bool is_aud = p->cfg.chain_kind == SMILEHIP_CHAIN_AUDSPEC;   // (a mel bank and no DCT: first_mfcc / last_mfcc are not read)
  const uint32_t tmask = no_mel ? (mask & ~(SMILEHIP_STAGE_MEL | SMILEHIP_STAGE_MFCC)) : (is_aud ? (mask & ~SMILEHIP_STAGE_MFCC) : mask);
  p->h_window.assign(size_t(p->geo.N), 1.0f);
  if ((mask & SMILEHIP_STAGE_WINDOW) && (rc = make_window(p->cfg, p->geo.N, p->h_window)) != SMILEHIP_OK)
    return fail(rc, "unknown window function %d", p->cfg.win_func);
  if (is_aud && (p->cfg.n_bands < 1 || p->cfg.n_bands > audspec::kMaxBands))
    return fail(SMILEHIP_ERR_INVALID, "audspec chain: n_bands (cMelspec nBands) must be 1 .. %d (a lane per band, the window chain's widest level); got %d",
                audspec::kMaxBands, p->cfg.n_bands);
  if (tmask & SMILEHIP_STAGE_MEL) {
    if ((rc = make_mel(p->cfg, p->geo, p->mel)) != SMILEHIP_OK)
      return is_aud ? fail(rc, "audspec chain: n_bands = %d, lofreq = %g, hifreq = %g build no mel bank on %lld bins", p->cfg.n_bands, (double)p->cfg.lofreq,
                           (double)p->cfg.hifreq, (long long)p->geo.K)
                    : fail(rc, "invalid mel bank parameters");
  } else {
    p->mel = MelBank();
    p->mel.n_bands = p->cfg.n_bands;
  }
  if (tmask & SMILEHIP_STAGE_MFCC) {
    if ((rc = make_dct(p->cfg, p->dct)) != SMILEHIP_OK) return fail(rc, "invalid MFCC range");
  } else {
    p->dct = DctTables();
  }
  p->stage_mask = mask;
  if (p->cfg.n_delta < 0 || p->cfg.n_delta > 2) return fail(SMILEHIP_ERR_INVALID, "n_delta must be 0..2");
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_IS09) {
    if (mask != SMILEHIP_STAGE_ALL || p->dct.n_mfcc != 12 || p->cfg.n_delta != 1 || p->cfg.sma_win < 3 || !(p->cfg.sma_win & 1) ||
        p->cfg.sma_win > 9)
      return fail(SMILEHIP_ERR_INVALID, "IS09 chain needs 12 MFCC, one delta stage and an odd smaWin in 3..9");
  } else if (is_compare_ab_like(p->cfg)) {
    if (mask != SMILEHIP_STAGE_ALL || p->dct.n_mfcc != 14 || p->mel.n_bands != 26 || p->cfg.n_delta != 1 ||
        p->cfg.delta_win != 2 || p->cfg.sma_win != 3 || !p->cfg.use_power || p->cfg.preemph ||
        (p->geo.Nfft != 256 && p->geo.Nfft != 512 && p->geo.Nfft != 1024))
      return fail(SMILEHIP_ERR_INVALID, "ComParE A+B chain: unsupported parameter set (20 ms frames at 8 .. 48 kHz)");
  } else if (p->cfg.chain_kind == SMILEHIP_CHAIN_EGEMAPS) {
    if (mask != SMILEHIP_STAGE_ALL || p->dct.n_mfcc != 4 || p->mel.n_bands != 26 || p->cfg.n_delta != 0 || p->cfg.sma_win != 3 ||
        !p->cfg.use_power || p->cfg.preemph || (p->geo.Nfft != 256 && p->geo.Nfft != 512 && p->geo.Nfft != 1024))
      return fail(SMILEHIP_ERR_INVALID, "eGeMAPS chain: unsupported parameter set (20 ms frames at 8 .. 48 kHz, 26 bands, MFCC 1..4)");
  } else if (p->cfg.chain_kind == SMILEHIP_CHAIN_PLP) {
    if (mask != SMILEHIP_STAGE_ALL || p->cfg.plp_lp_order < 1 || p->cfg.plp_lp_order > 15 || !p->cfg.mel_htk_compatible ||
        !p->cfg.use_power || p->mel.n_bands > 30 || p->cfg.plp_compression < 0.0f)
      return fail(SMILEHIP_ERR_INVALID, "PLP chain: lpOrder 1..15, HTK-scaled power mel bands (<= 30) required");
    if (p->cfg.first_mfcc != 0 && p->cfg.first_mfcc != 1) return fail(SMILEHIP_ERR_INVALID, "PLP chain: firstCC must be 0 or 1");
    p->dct.n_mfcc = p->cfg.plp_lp_order + (p->cfg.first_mfcc == 0 ? 1 : 0);   // c1..c_lpOrder [, c0]: outputs of cPlp
    p->dct.melfloor = 1.0f;                              // htkcompatible forces melfloor = 1.0 (plp.cpp:150-160)
  } else if (f0_front_chain(p->cfg.chain_kind)) {
    if (p->cfg.chain_kind == SMILEHIP_CHAIN_PROSODY_SHS && (p->cfg.sma_win < 3 || !(p->cfg.sma_win & 1) || p->cfg.sma_win > 9))
      return fail(SMILEHIP_ERR_INVALID, "prosodyShs chain: cContourSmoother smaWin must be odd, 3 .. 9");
    if (mask != SMILEHIP_STAGE_ALL || p->cfg.preemph || p->cfg.n_delta != 0 || p->cfg.win_offset != 0.0)
      return fail(SMILEHIP_ERR_INVALID, "F0 chain: no pre-emphasis / deltas / window offset");
    if (p->geo.Nfft != 512 && p->geo.Nfft != 1024 && p->geo.Nfft != 2048 && p->geo.Nfft != 4096)
      return fail(SMILEHIP_ERR_INVALID, "F0 chain: the kernels are instantiated for spectra of 512 .. 4096 points (60 ms frames at 8 .. 48 kHz); "
                  "this configuration gives %lld points", (long long)p->geo.Nfft);
    if (p->cfg.shs_n_harmonics < 1 || p->cfg.shs_n_harmonics > 17 || !(p->cfg.pitch_max > p->cfg.pitch_min) || p->cfg.pitch_min < 40.0)
      return fail(SMILEHIP_ERR_INVALID, "F0 chain: nHarmonics 1..17, minPitch >= 40 Hz (period search window of the jitter kernel), "
                  "maxPitch > minPitch");
    if (p->cfg.shs_n_candidates < 0 || p->cfg.shs_n_candidates > 6)
      return fail(SMILEHIP_ERR_INVALID, "F0 chain: cPitchShs nCandidates 1 .. 6 (0 = 6)");
    if ((rc = make_f0_tables(p->geo.K, p->geo.fft_frame_size_sec, p->cfg.shs_n_harmonics, p->cfg.shs_compression,
                             p->cfg.specscale_min_f > 0.0 ? p->cfg.specscale_min_f : 25.0, p->f0)))
      return fail(rc, "F0 chain: spectrum geometry / nHarmonics not usable by cSpecScale / cPitchShs");
  } else if (p->cfg.chain_kind == SMILEHIP_CHAIN_PROSODY_ACF) {
    // everything the chain cannot express is refused with the option named
    if (mask != SMILEHIP_STAGE_ALL) return fail(SMILEHIP_ERR_INVALID, "prosodyAcf chain: stage_mask must be all stages");
    if (p->cfg.sma_win < 3 || !(p->cfg.sma_win & 1) || p->cfg.sma_win > 9)
      return fail(SMILEHIP_ERR_INVALID, "prosodyAcf chain: sma_win (cContourSmoother smaWin) must be odd, 3 .. 9; got %d", p->cfg.sma_win);
    if (p->cfg.n_delta != 0) return fail(SMILEHIP_ERR_INVALID, "prosodyAcf chain: n_delta must be 0 (the file has no cDeltaRegression); got %d", p->cfg.n_delta);
    if (p->cfg.preemph) return fail(SMILEHIP_ERR_INVALID, "prosodyAcf chain: preemph must be 0 (the file has no cVectorPreemphasis)");
    if (p->cfg.win_offset != 0.0) return fail(SMILEHIP_ERR_INVALID, "prosodyAcf chain: win_offset must be 0");
    if (p->cfg.zero_pad_symmetric) return fail(SMILEHIP_ERR_INVALID, "prosodyAcf chain: zero_pad_symmetric must be 0 ([fft:cTransformFFT] zeroPadSymmetric = 0)");
    if (p->cfg.acf_cep_use_power != 0 && p->cfg.acf_cep_use_power != 1)
      return fail(SMILEHIP_ERR_INVALID, "prosodyAcf chain: acf_cep_use_power must be 0 or 1; got %d", p->cfg.acf_cep_use_power);
    if (p->geo.Nfft < 64 || p->geo.Nfft > 8192)
      return fail(SMILEHIP_ERR_INVALID, "prosodyAcf chain: the transform length must be 64 .. 8192 points; frame_size_sec at this sample_rate gives %lld",
                  (long long)p->geo.Nfft);
  } else if (p->cfg.chain_kind == SMILEHIP_CHAIN_EMOBASE) {
    // everything the chain cannot express is refused with the parameter named
    const smilehip_lld_config &c = p->cfg;
    if (mask != SMILEHIP_STAGE_ALL) return fail(SMILEHIP_ERR_INVALID, "emobase chain: stage_mask must be all stages");
    if (c.sma_win < 3 || !(c.sma_win & 1) || c.sma_win > 9)
      return fail(SMILEHIP_ERR_INVALID, "emobase chain: sma_win (cContourSmoother smaWin) must be odd, 3 .. 9; got %d", c.sma_win);
    if (c.n_delta != 1 || c.delta_win != emobase::kDeltaWin)
      return fail(SMILEHIP_ERR_INVALID, "emobase chain: n_delta must be 1 and delta_win %d ([delta1:cDeltaRegression]); got %d / %d", emobase::kDeltaWin, c.n_delta, c.delta_win);
    if (!c.preemph || c.preemph_de) return fail(SMILEHIP_ERR_INVALID, "emobase chain: preemph must be 1 and preemph_de 0 ([pe:cVectorPreemphasis])");
    if (c.win_offset != 0.0) return fail(SMILEHIP_ERR_INVALID, "emobase chain: win_offset must be 0");
    if (c.zero_pad_symmetric) return fail(SMILEHIP_ERR_INVALID, "emobase chain: zero_pad_symmetric must be 0 ([fft:cTransformFFT] zeroPadSymmetric = 0)");
    if (c.append_log_energy) return fail(SMILEHIP_ERR_INVALID, "emobase chain: append_log_energy must be 0 (the file has no cEnergy)");
    if (c.cms) return fail(SMILEHIP_ERR_INVALID, "emobase chain: cms must be 0 (the file has no cFullinputMean)");
    if (p->dct.n_mfcc != 12) return fail(SMILEHIP_ERR_INVALID, "emobase chain: first_mfcc .. last_mfcc must give 12 coefficients; got %d", p->dct.n_mfcc);
    if (p->mel.n_bands < 1 || p->mel.n_bands > 32) return fail(SMILEHIP_ERR_INVALID, "emobase chain: n_bands must be 1 .. 32; got %d", p->mel.n_bands);
    if (c.frame_size_sec >= 0.040) return fail(SMILEHIP_ERR_INVALID, "emobase chain: frame_size_sec must lie below the second framer's 0.040 s; got %g", c.frame_size_sec);
    if (p->geo.Nfft < 64 || p->geo.Nfft > 8192)
      return fail(SMILEHIP_ERR_INVALID, "emobase chain: the transform length must be 64 .. 8192 points; frame_size_sec at this sample_rate gives %lld",
                  (long long)p->geo.Nfft);
    smilehip_lld_config c40 = c;                          // [fr40:cFramer] .. [fft40:cTransformFFT]: the same step, window and padding
    c40.frame_size_sec = 0.040;
    if ((rc = make_geometry(c40, p->geo40)) != SMILEHIP_OK) return fail(rc, "emobase chain: invalid framing parameters of the 40 ms framer");
    if (p->geo40.Nfft < 64 || p->geo40.Nfft > 8192 || p->geo40.H != p->geo.H || p->geo40.N < p->geo.N)
      return fail(SMILEHIP_ERR_INVALID, "emobase chain: the 40 ms framer gives a transform of %lld points (64 .. 8192 are built)", (long long)p->geo40.Nfft);
    p->h_window40.assign(size_t(p->geo40.N), 1.0f);
    if ((rc = make_window(c40, p->geo40.N, p->h_window40)) != SMILEHIP_OK) return fail(rc, "unknown window function %d", c.win_func);
  } else if (p->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FFT) {
    // everything the chain cannot express is refused with the option named
    const smilehip_lld_config &c = p->cfg;
    if (c.struct_size < SMILEHIP_LLD_CONFIG_SIZE_V2)
      return fail(SMILEHIP_ERR_INVALID, "chroma_fft chain: struct_size %u does not cover the tonespec / chroma fields (%u)", c.struct_size, SMILEHIP_LLD_CONFIG_SIZE_V2);
    if (mask != SMILEHIP_STAGE_ALL) return fail(SMILEHIP_ERR_INVALID, "chroma_fft chain: stage_mask must be all stages");
    if (c.n_delta != 0) return fail(SMILEHIP_ERR_INVALID, "chroma_fft chain: n_delta must be 0 (the file has no cDeltaRegression); got %d", c.n_delta);
    if (c.preemph) return fail(SMILEHIP_ERR_INVALID, "chroma_fft chain: preemph must be 0 (the file has no cVectorPreemphasis)");
    if (c.win_offset != 0.0) return fail(SMILEHIP_ERR_INVALID, "chroma_fft chain: win_offset must be 0");
    if (p->geo.Nfft < 64 || p->geo.Nfft > 8192)
      return fail(SMILEHIP_ERR_INVALID, "chroma_fft chain: the transform length must be 64 .. 8192 points; frame_size_sec at this sample_rate gives %lld",
                  (long long)p->geo.Nfft);
    if (c.chroma_octave_size < 1 || c.chroma_octave_size > chroma::kMaxOctaveSize)
      return fail(SMILEHIP_ERR_INVALID, "chroma_fft chain: chroma_octave_size (cChroma octaveSize) must be 1 .. %d; got %d", chroma::kMaxOctaveSize, c.chroma_octave_size);
    if (c.tonespec_n_octaves < 1 || c.tonespec_n_octaves * 12 > chroma::kMaxNotes)
      return fail(SMILEHIP_ERR_INVALID, "chroma_fft chain: tonespec_n_octaves (cTonespec nOctaves) must be 1 .. %d; got %d", chroma::kMaxNotes / 12, c.tonespec_n_octaves);
    if ((c.tonespec_n_octaves * 12) % c.chroma_octave_size)
      return fail(SMILEHIP_ERR_INVALID, "chroma_fft chain: 12 tonespec_n_octaves = %d notes are no multiple of chroma_octave_size %d (cChroma writes no values then)",
                  c.tonespec_n_octaves * 12, c.chroma_octave_size);
    if (!(c.chroma_sil_thresh == c.chroma_sil_thresh)) return fail(SMILEHIP_ERR_INVALID, "chroma_fft chain: chroma_sil_thresh is not a number");
    const smilehip_tonespec_opts to = {c.tonespec_n_octaves, c.tonespec_first_note, c.tonespec_filter_type, c.tonespec_use_power, c.tonespec_dba};
    const char *why = "";
    if ((rc = make_tonespec_tables(to, p->geo.K, p->geo.fft_frame_size_sec, p->tonespec, &why)))
      return fail(rc, "chroma_fft chain: cTonespec (tonespec_*): %s", why);
  } else if (p->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FILT) {
    const smilehip_lld_config &c = p->cfg;
    if (c.struct_size < sizeof(smilehip_lld_config))
      return fail(SMILEHIP_ERR_INVALID, "chroma_filt chain: struct_size %u does not cover the tonefilt fields (%zu)", c.struct_size, sizeof(smilehip_lld_config));
    if (mask != SMILEHIP_STAGE_ALL) return fail(SMILEHIP_ERR_INVALID, "chroma_filt chain: stage_mask must be all stages");
    if (c.n_delta != 0) return fail(SMILEHIP_ERR_INVALID, "chroma_filt chain: n_delta must be 0 (the file has no cDeltaRegression); got %d", c.n_delta);
    if (c.preemph) return fail(SMILEHIP_ERR_INVALID, "chroma_filt chain: preemph must be 0 (the file has no cVectorPreemphasis)");
    const smilehip_tonefilt_opts to = {c.tonefilt_n_notes, 0, c.tonefilt_first_note, c.tonefilt_decay_f0, c.tonefilt_decay_fn, c.tonefilt_output_period};
    const char *why = "";
    if ((rc = make_tonefilt_tables(to, c.sample_rate, p->tonefilt, &why))) return fail(rc, "chroma_filt chain: cTonefilt (tonefilt_*): %s", why);
    // the batch layout's frames are the blocks: frame_size_sec = frame_step_sec = outputPeriod must have given N = H = P
    if (p->geo.N != p->tonefilt.P || p->geo.H != p->tonefilt.P)
      return fail(SMILEHIP_ERR_INVALID, "chroma_filt chain: frame_size_sec and frame_step_sec must both be tonefilt_output_period (blocks of %lld samples; they give %lld / %lld)",
                  (long long)p->tonefilt.P, (long long)p->geo.N, (long long)p->geo.H);
    if (c.chroma_octave_size < 1 || c.chroma_octave_size > chroma::kMaxOctaveSize)
      return fail(SMILEHIP_ERR_INVALID, "chroma_filt chain: chroma_octave_size (cChroma octaveSize) must be 1 .. %d; got %d", chroma::kMaxOctaveSize, c.chroma_octave_size);
    if (p->tonefilt.n_notes % c.chroma_octave_size)
      return fail(SMILEHIP_ERR_INVALID, "chroma_filt chain: tonefilt_n_notes = %d notes are no multiple of chroma_octave_size %d (cChroma writes no values then)",
                  p->tonefilt.n_notes, c.chroma_octave_size);
    if (!(c.chroma_sil_thresh == c.chroma_sil_thresh)) return fail(SMILEHIP_ERR_INVALID, "chroma_filt chain: chroma_sil_thresh is not a number");
  } else if (p->cfg.chain_kind == SMILEHIP_CHAIN_SPECTROGRAM) {
    // everything the chain cannot express is refused with the parameter named
    const smilehip_lld_config &c = p->cfg;
    if (mask != SMILEHIP_STAGE_ALL) return fail(SMILEHIP_ERR_INVALID, "spectrogram chain: stage_mask must be all stages");
    if (c.n_delta != 0) return fail(SMILEHIP_ERR_INVALID, "spectrogram chain: n_delta must be 0 (the file has no cDeltaRegression); got %d", c.n_delta);
    if (c.preemph) return fail(SMILEHIP_ERR_INVALID, "spectrogram chain: preemph must be 0 (the file has no cVectorPreemphasis)");
    if (c.append_log_energy) return fail(SMILEHIP_ERR_INVALID, "spectrogram chain: append_log_energy must be 0 (the file has no cEnergy)");
    if (c.cms) return fail(SMILEHIP_ERR_INVALID, "spectrogram chain: cms must be 0 (the file has no cFullinputMean)");
    if (p->geo.Nfft < 64 || p->geo.Nfft > 8192)
      return fail(SMILEHIP_ERR_INVALID, "spectrogram chain: the transform length must be 64 .. 8192 points; frame_size_sec at this sample_rate gives %lld",
                  (long long)p->geo.Nfft);
    p->spg_form = spectrogram::form_consts(spectrogram::kMagnitude, p->geo.Nfft, (float)90.302, (float)-102.0);
  } else if (is_aud) {
    // everything the chain cannot express is refused with the parameter named
    const smilehip_lld_config &c = p->cfg;
    if (mask != SMILEHIP_STAGE_ALL) return fail(SMILEHIP_ERR_INVALID, "audspec chain: stage_mask must be all stages");
    if (!c.use_power) return fail(SMILEHIP_ERR_INVALID, "audspec chain: use_power must be 1 (cPlp reads a power mel spectrum)");
    if (!c.mel_htk_compatible) return fail(SMILEHIP_ERR_INVALID, "audspec chain: mel_htk_compatible must be 1 (cPlp's htkcompatible floor is that of HTK-scaled bands)");
    if (!(c.plp_compression >= 0.0f)) return fail(SMILEHIP_ERR_INVALID, "audspec chain: plp_compression (cPlp compression) must be >= 0; got %g", (double)c.plp_compression);
    if (c.append_log_energy) return fail(SMILEHIP_ERR_INVALID, "audspec chain: append_log_energy must be 0 (cEnergy is not built for this chain)");
    if (c.cms) return fail(SMILEHIP_ERR_INVALID, "audspec chain: cms must be 0 (cFullinputMean is not built for this chain)");
    if (p->geo.Nfft < 64 || p->geo.Nfft > 8192)
      return fail(SMILEHIP_ERR_INVALID, "audspec chain: the transform length must be 64 .. 8192 points; frame_size_sec at this sample_rate gives %lld",
                  (long long)p->geo.Nfft);
    for (int b = 0; b < p->mel.n_bands; ++b)               // what the band's lane walks lies in the spectrum
      if (p->mel.rise_lo[b] < 0 || p->mel.rise_hi[b] > p->geo.K || p->mel.fall_lo[b] < 0 || p->mel.fall_hi[b] > p->geo.K)
        return fail(SMILEHIP_ERR_INVALID, "audspec chain: n_bands / lofreq / hifreq: band %d reaches outside the %lld bins", b, (long long)p->geo.K);
    p->dct.melfloor = 1.0f;                               // htkcompatible forces melfloor = 1.0 (plp.cpp:153-163)
  } else if (p->cfg.chain_kind != SMILEHIP_CHAIN_MFCC) {
    return fail(SMILEHIP_ERR_INVALID, "unknown chain_kind %d", p->cfg.chain_kind);
  }
  if (p->cfg.n_delta > 0 && (p->cfg.delta_win < 1 || p->cfg.delta_win > 4))
    return fail(SMILEHIP_ERR_INVALID, "delta_win must be 1..4");

  std::vector<int32_t> rng((tmask & SMILEHIP_STAGE_MEL) ? size_t(4) * p->mel.n_bands : 0);
  for (int b = 0; b < p->mel.n_bands && (tmask & SMILEHIP_STAGE_MEL); ++b) {
    rng[4 * b + 0] = p->mel.rise_lo[b];
    rng[4 * b + 1] = p->mel.rise_hi[b];
    rng[4 * b + 2] = p->mel.fall_lo[b];
    rng[4 * b + 3] = p->mel.fall_hi[b];
  }
  // PLP chain: cPlp::initTables (plp.cpp:288-357): IDFT cosine table, lifter table, HTK equal-loudness weights at
  // the band centres cMelspec publishes (melspec.cpp:408-412)
  std::vector<float> plp_eql(32, 0.0f), plp_sin(16, 1.0f);
  const bool is_plp = p->cfg.chain_kind == SMILEHIP_CHAIN_PLP;
  if (is_plp) {
    const int nB = p->mel.n_bands, nFreq = nB + 2, nAuto = p->cfg.plp_lp_order + 1;
    p->h_plp_cos.assign(size_t(nAuto) * nFreq, 0.0f);
    const float a = (float)M_PI / (float)(nFreq - 1);
    for (int i = 0; i < nAuto; i++) {
      const int ib = i * nFreq;
      int m;
      p->h_plp_cos[ib] = 1.0f;
      for (m = 1; m < (nFreq - 1); m++) p->h_plp_cos[m + ib] = (float)(2.0 * std::cos(a * (double)i * (double)m));
      p->h_plp_cos[m + ib] = (float)(std::cos(a * (double)i * (double)m));
    }
    const float L = (float)(int)p->cfg.cep_lifter;      // cepLifter is read with getInt (plp.cpp:142)
    for (int i = 0; i < nAuto; i++)
      plp_sin[i] = (L > 0.0f) ? ((float)1.0 + L / (float)2.0 * std::sin((float)M_PI * ((float)(i)) / L)) : 1.0f;
    for (int m = 1; m <= nB; ++m) {
      const double hz = 700.0 * (std::exp(double(p->mel.centres[m]) / 1127.0) - 1.0);
      const double f2 = hz * hz, fs = f2 / (f2 + 1.6e5);
      plp_eql[m - 1] = (float)(fs * fs * ((f2 + 1.44e6) / (f2 + 9.61e6)));   // smileDsp_equalLoudnessWeight_htk
    }
  }
  if (is_aud) {                                           // the same weights (smileDsp_equalLoudnessWeight_htk), a lane per band: up to 64
    plp_eql.assign(audspec::kMaxBands, 0.0f);
    for (int m = 1; m <= p->mel.n_bands; ++m) plp_eql[m - 1] = audspec::eql_htk(p->mel.centres[m]);
  }
  // fast Nfft=512 kernel if the geometry allows it (SMILEHIP_FORCE_GENERIC=1 disables it)
  p->use_fast = false;
  if (mask == SMILEHIP_STAGE_ALL && (p->cfg.chain_kind == SMILEHIP_CHAIN_MFCC || (is_plp && p->mel.n_bands == 26 && p->cfg.use_power)) &&
      !p->force_generic && fast512_applicable((int)p->geo.Nfft, (int)p->geo.N)) {
    p->use_fast = fast512_build_host(p->cfg, p->geo, p->h_window, p->mel, p->dct, p->fast) == 0;
    if (p->use_fast && is_plp) {                          // the DCT rows' place holds the IDFT cosine rows (28 floats each)
      p->fast.dct28.assign(16 * 28, 0.0f);
      std::copy(p->h_plp_cos.begin(), p->h_plp_cos.end(), p->fast.dct28.begin());
    }
    if (p->ctx) p->fast.max_blocks = 2 * p->ctx->prop.multiProcessorCount;
  }
  if (!upload) return SMILEHIP_OK;
  if ((rc = p->d_window.upload(p->h_window))) return rc;
  if ((rc = p->d_mel_coef.upload(p->mel.coef))) return rc;
  if ((rc = p->d_mel_rng.upload(rng))) return rc;
  if ((rc = p->d_dct_rows.upload(p->dct.cos_rows))) return rc;
  if ((rc = p->d_dct_gain.upload(p->dct.gain))) return rc;
  // (shorter frames: a plan that windows, frames or pre-emphasises only; what would transform refuses it, require_transform)
  if (p->geo.Nfft >= 64 && (rc = p->oo.build((int)p->geo.Nfft, true))) return rc;
  if (is_plp && ((rc = p->d_plp_eql.upload(plp_eql)) || (rc = p->d_plp_cos.upload(p->h_plp_cos)) || (rc = p->d_plp_sin.upload(plp_sin))))
    return rc;
  if (is_aud && (rc = p->d_plp_eql.upload(plp_eql))) return rc;
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FFT && ((rc = p->d_ts_fmap.upload(p->tonespec.filter_map)) || (rc = p->d_ts_rec.upload(p->tonespec.rec))))
    return rc;
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FILT && (rc = p->d_tf_tab.upload(p->tonefilt.tab))) return rc;
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_EMOBASE && ((rc = p->d_window40.upload(p->h_window40)) || (rc = p->oo40.build((int)p->geo40.Nfft, true)))) return rc;
  if (f0_front_chain(p->cfg.chain_kind) &&
      ((rc = p->d_f0_rec.upload(p->f0.sp_rec)) || (rc = p->d_f0_d1.upload(p->f0.sp_d1)) || (rc = p->d_f0_d2.upload(p->f0.sp_d2)) ||
       (rc = p->d_f0_co.upload(p->f0.ip_co)) || (rc = p->d_f0_audw.upload(p->f0.audw)) || (rc = p->d_f0_k.upload(p->f0.ip_k)) ||
       (rc = p->d_f0_iprec.upload(p->f0.ip_rec)) || (rc = p->d_f0_swrec.upload(p->f0.sw_rec)) || (rc = p->d_f0_ipcnt.upload(p->f0.ip_cnt))))
    return rc;
  if (p->cfg.vit_buffer_len < 0 || p->cfg.vit_buffer_len == 1 || p->cfg.vit_buffer_len > 128)
    return fail(SMILEHIP_ERR_INVALID, "vit_buffer_len must be 0 (= 30) or 2..128");
  if (p->cfg.jitter_search_range < 0.0 || p->cfg.jitter_search_range >= 1.0)
    return fail(SMILEHIP_ERR_INVALID, "jitter_search_range must be in [0, 1)");
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_EGEMAPS) {
    // [gemapsv01b_audspec]: equal-loudness weights at the band centres (plp.cpp:335-357)
    std::vector<float> eql(26);
    for (int m = 1; m <= 26; ++m) {
      const double hz = 700.0 * (std::exp(double(p->mel.centres[m]) / 1127.0) - 1.0);
      const double w = 2.0 * M_PI * hz, w2 = w * w, c = w2 + 6300000.0;
      eql[m - 1] = float((c > 0.0) ? (1e32 * ((w2 + 56.8e6) * w2 * w2) / (c * c * (w2 + 0.38e9) * (w2 * w2 * w2 * w + 1.7e31))) : 0.0);
    }
    if ((rc = p->d_eql.upload(eql))) return rc;
    // [gemapsv01b_logSpectral]: slopes 0-500 and 500-1500 Hz of the log spectrum (spectral.cpp:872-946), freqRange 0-5000
    // (:625-644), specFloor 1e-7 squared and its log (:228-235)
    const int Nsrc = (int)p->geo.K;
    const double F0 = 1.0 / p->geo.fft_frame_size_sec;
    const int lo_hz[2] = {0, 500}, hi_hz[2] = {500, 1500};
    for (int b = 0; b < 2; ++b) {
      int ii;
      double wghtL, wghtR, idxL, idxR;
      for (ii = 0; ii < Nsrc; ii++) if (F0 * ii > (double)lo_hz[b]) break;
      if ((ii < Nsrc) && (ii > 0)) wghtL = (F0 * ii - (double)lo_hz[b]) / (F0 * ii - F0 * (ii - 1)); else wghtL = 1.0;
      idxL = (double)ii - 1.0;
      if (idxL < 0) idxL = 0;
      if (idxL >= Nsrc) idxL = Nsrc;
      if (wghtL == 0.0) wghtL = 1.0;
      for (ii = 0; ii < Nsrc; ii++) if (F0 * ii >= (float)hi_hz[b]) break;
      if ((ii < Nsrc) && (ii > 0)) wghtR = ((double)hi_hz[b] - F0 * (ii - 1)) / (F0 * ii - F0 * (ii - 1)); else wghtR = 1.0;
      if ((ii < Nsrc) && (F0 * ii == (float)hi_hz[b])) idxR = (double)ii; else idxR = (double)ii - 1.0;
      if (idxR >= Nsrc) idxR = Nsrc - 1;
      if (wghtR == 0.0) wghtR = 1.0;
      int iL = (int)std::floor(idxL), iR = (int)std::floor(idxR);
      if (iL >= Nsrc) { iL = iR = Nsrc - 1; wghtR = 0.0; wghtL = 0.0; }
      if (iR >= Nsrc) { iR = Nsrc - 1; wghtR = 1.0; }
      if (iL < 0) iL = 0;
      if (iR < 0) iR = 0;
      if (iR - iL >= 64 || iR >= 64) return fail(SMILEHIP_ERR_INVALID, "eGeMAPS chain: slope band wider than the kernel's 64 bins");
      p->gm_sl_iL[b] = iL; p->gm_sl_iR[b] = iR; p->gm_sl_wL[b] = wghtL; p->gm_sl_wR[b] = wghtR; p->gm_sl_Nind[b] = idxR - idxL;
    }
    int lo = -1, hi = -1;
    for (int i = 0; i < Nsrc; i++) {
      if ((double)0 >= F0 * i) lo = i;
      if ((double)5000 > F0 * i) hi = i;
    }
    if (hi == -1 || hi >= Nsrc) hi = Nsrc - 1;
    if (lo < 0) lo = 0;
    p->gm_rng_lo = lo; p->gm_rng_hi = hi;
    {                                                     // the alpha ratio's two bands (spectral.cpp:997-1022), the kernel's own expressions
      int n1 = 0, n2 = 0;
      while (n1 < Nsrc && F0 * (double)n1 < 1000.0) ++n1;
      n2 = n1;
      while (n2 < Nsrc && !(F0 * (double)n2 > 5000.0)) ++n2;
      p->gm_ar_n1 = n1; p->gm_ar_n2 = n2;
    }
    float specFloor = (float)0.0000001;
    specFloor = specFloor * specFloor;
    p->gm_spec_floor = specFloor;
    p->gm_log_spec_floor = (float)(10.0 * (double)std::log(specFloor) / std::log(10.0));
    p->gm_log_spec_factor = (float)(10.0 / std::log(10.0));
    // [gemapsv01b_resampLpc]: cSpecResample::setupNewNames (specResample.cpp:117-172) + smileDsp_initIrdft
    // (smileUtil.c:1752-1786) for the Nfft-value complex spectrum, targetFs = 11000; the tables transposed to [k/2 - 1][i]
    {
      const long n_in = (long)p->geo.Nfft;
      const double fs_sec = p->geo.fft_frame_size_sec, last_fs_sec = (double)p->geo.N * p->geo.period, bT = p->geo.period;
      const double sr = 1.0 / bT;
      double target_fs = 11000.0, ratio = target_fs / sr, nd;
      long n_out;
      if ((fs_sec != last_fs_sec) && (last_fs_sec != 0.0) && (last_fs_sec != bT)) {
        const double nout0 = std::round((double)n_in * ratio * last_fs_sec / fs_sec);
        const double new_ratio = nout0 / ((double)n_in * (last_fs_sec / fs_sec));
        n_out = (long)nout0;
        if (new_ratio != ratio) { target_fs = sr * new_ratio; ratio = new_ratio; }
        nd = (double)n_in * ratio;
      } else {
        const double nout0 = std::round((double)n_in * ratio);
        const double new_ratio = nout0 / (double)n_in;
        n_out = (long)nout0;
        if (new_ratio != ratio) { target_fs = sr * new_ratio; ratio = new_ratio; }
        nd = nout0;
      }
      long kMax = n_in > n_out ? n_out : n_in;
      if (kMax & 1) kMax--;
      if (n_out != 220 || kMax / 2 - 1 != 109 || n_out >= n_in)
        return fail(SMILEHIP_ERR_INVALID, "eGeMAPS chain: cSpecResample geometry %ld -> %ld is not the one the kernel is built for", n_in, n_out);
      p->gm_target_fs = target_fs;
      std::vector<float> ct(size_t(109) * 220), st(size_t(109) * 220);
      const double pi2 = 2.0 * M_PI;
      for (long i = 0; i < n_out; i++)
        for (long k = 2; k < kMax; k += 2) {
          const double kn = pi2 * (double)(k / 2 * i) / nd;
          ct[size_t(k / 2 - 1) * 220 + i] = (float)std::cos(kn);
          st[size_t(k / 2 - 1) * 220 + i] = (float)std::sin(kn);
        }
      if ((rc = p->d_rs_cos.upload(ct)) || (rc = p->d_rs_sin.upload(st))) return rc;
    }
  }
  if (is_compare_ab_like(p->cfg)) {
    // cPlp::initTables (plp.cpp:335-402): equal-loudness weights at the band centres cMelspec
    // publishes as metadata (melspec.cpp:408-412), and the newRASTA filter coefficients
    std::vector<float> eql(26), eqll(26);
    for (int m = 1; m <= 26; ++m) {
      const double hz = 700.0 * (std::exp(double(p->mel.centres[m]) / 1127.0) - 1.0);
      const double w = 2.0 * M_PI * hz, w2 = w * w, c = w2 + 6300000.0;
      const double e = (c > 0.0) ? (1e32 * ((w2 + 56.8e6) * w2 * w2) / (c * c * (w2 + 0.38e9) * (w2 * w2 * w2 * w + 1.7e31))) : 0.0;
      eql[m - 1] = float(e);
      eqll[m - 1] = std::log(eql[m - 1]);
    }
    const double Tl = p->geo.frame_period;
    const float lower = 1.0f, upper = 29.0f;
    p->rasta_iir = float(1.0 - std::sin(2.0 * M_PI * lower * Tl));
    const float om = float(std::cos(2.0 * M_PI * upper * Tl));
    const float norm = float(std::sqrt(10.0 * (32.0 * om * om + 8.0)));
    p->rasta_fir[0] = float(2.0 / norm);
    p->rasta_fir[1] = float(-4.0 * om / norm);
    p->rasta_fir[2] = 0.0f;
    p->rasta_fir[3] = -p->rasta_fir[1];
    p->rasta_fir[4] = -p->rasta_fir[0];
    if ((rc = p->d_eql.upload(eql)) || (rc = p->d_eql_log.upload(eqll))) return rc;
  }
  if (is_compare_ab_like(p->cfg) || (mask & SMILEHIP_STAGE_SPECTRAL)) {
    // sharpness weights (spectral.cpp:1440-1455): bark(f) * g(bark(f)) for bins 1..K-1
    std::vector<double> sw(size_t(p->geo.K - 1));
    const double F0 = 1.0 / p->geo.fft_frame_size_sec;
    for (int64_t j = 1; j < p->geo.K; ++j) {
      const double x = F0 * double(j);
      double zz = 0.0;
      if (x > 0) {
        zz = (26.81 / (1.0 + 1960.0 / x)) - 0.53;
        if (zz < 2) zz = 0.85 * zz + 0.3;
        else if (zz > 20.1) zz = 1.22 * zz - 0.22 * 20.1;
      }
      const double g = (zz <= 16.0) ? 1.0 : std::pow((zz - 16.0) / 4.0, 1.5849625) + 1.0;
      sw[size_t(j - 1)] = zz * g;
    }
    // band edges of [is13_spectral] bands 250-650 and 1000-4000 (spectral.cpp:779-853)
    int band_lo[2] = {250, 1000}, band_hi[2] = {650, 4000};
    if (p->cfg.spectral_band_lo[0] || p->cfg.spectral_band_lo[1] || p->cfg.spectral_band_hi[0] || p->cfg.spectral_band_hi[1])
      for (int b = 0; b < 2; ++b) {
        band_lo[b] = p->cfg.spectral_band_lo[b];
        band_hi[b] = p->cfg.spectral_band_hi[b];
        if (band_lo[b] < 0 || band_hi[b] <= band_lo[b]) return fail(SMILEHIP_ERR_INVALID, "cSpectral bands[%d] = %d-%d", b, band_lo[b], band_hi[b]);
      }
    const int Nsrc = (int)p->geo.K;
    for (int b = 0; b < 2; ++b) {
      int ii;
      double wghtL, wghtR, idxL, idxR;
      for (ii = 0; ii < Nsrc; ii++) if (F0 * ii > (double)band_lo[b]) break;
      if ((ii < Nsrc) && (ii > 0)) wghtL = (F0 * ii - (double)band_lo[b]) / (F0 * ii - F0 * (ii - 1)); else wghtL = 1.0;
      idxL = (double)ii - 1.0;
      if (idxL < 0) idxL = 0;
      if (idxL >= Nsrc) idxL = Nsrc;
      if (wghtL == 0.0) wghtL = 1.0;
      for (ii = 0; ii < Nsrc; ii++) if (F0 * ii >= (float)band_hi[b]) break;
      if ((ii < Nsrc) && (ii > 0)) wghtR = ((double)band_hi[b] - F0 * (ii - 1)) / (F0 * ii - F0 * (ii - 1)); else wghtR = 1.0;
      if ((ii < Nsrc) && (F0 * ii == (float)band_hi[b])) idxR = (double)ii; else idxR = (double)ii - 1.0;
      if (idxR >= Nsrc) idxR = Nsrc - 1;
      if (wghtR == 0.0) wghtR = 1.0;
      int iL = (int)std::floor(idxL), iR = (int)std::floor(idxR);
      if (iL >= Nsrc) { iL = iR = Nsrc - 1; wghtR = 0.0; wghtL = 0.0; }
      if (iR >= Nsrc) { iR = Nsrc - 1; wghtR = 1.0; }
      if (iL < 0) iL = 0;
      if (iR < 0) iR = 0;
      p->band_iL[b] = iL; p->band_iR[b] = iR; p->band_wL[b] = wghtL; p->band_wR[b] = wghtR;
    }
    double Sf = 0.0, S2f = 0.0;
    for (int64_t i = 1; i < p->geo.K; ++i) { S2f += (F0 * i) * (F0 * i); Sf += F0 * i; }
    p->slope_Sf = Sf;
    p->slope_S2f = S2f;
    if ((rc = p->d_sharp.upload(sw))) return rc;
  }
  if (p->use_fast) {
    if ((rc = p->d_tw256.upload(p->fast.tw256))) return rc;
    if ((rc = p->d_tw512.upload(p->fast.tw512))) return rc;
    if ((rc = p->d_fwin.upload(p->fast.win))) return rc;
    if ((rc = p->d_melw.upload(p->fast.melw))) return rc;
    if ((rc = p->d_melo.upload(p->fast.melo))) return rc;
    if ((rc = p->d_dct28.upload(p->fast.dct28))) return rc;
    if ((rc = p->d_lane_bands.upload(p->fast.lane_bands))) return rc;
  }
  return SMILEHIP_OK;
}

extern "C" int smilehip_plan_create(smilehip_context *ctx, const smilehip_lld_config *cfg, smilehip_plan **out) {
  if (!ctx || !cfg || !out) return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_create: null argument");
  *out = nullptr;
  if (!config_size_known(cfg->struct_size))
    return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size,
                sizeof(smilehip_lld_config));
  HIP_TRY(hipSetDevice(ctx->device));
  auto *p = new (std::nothrow) smilehip_plan();
  if (!p) return fail(SMILEHIP_ERR_NOMEM, "out of host memory");
  p->ctx = ctx;
  copy_config(p->cfg, cfg);
  const char *fg = getenv("SMILEHIP_FORCE_GENERIC");
  p->force_generic = (fg && fg[0] == '1') ? 1 : 0;
  int rc = build_tables(p);
  if (rc == SMILEHIP_OK && cfg->chain_kind == SMILEHIP_CHAIN_COMPARE) {      // the 60 ms sub-chain
    smilehip_lld_config c60;
    smilehip_config_compare16_f0(&c60);
    c60.sample_rate = cfg->sample_rate;
    c60.frame_step_sec = cfg->frame_step_sec;
    c60.zero_pad_symmetric = cfg->zero_pad_symmetric;     // both cTransformFFT instances carry the set's value
    c60.jitter_broken_thresh = cfg->jitter_broken_thresh;
    if (cfg->pitch_max > 0.0) {                           // the F0 group's parameters (an edited ComParE_2016.conf; 0 = a config struct from before they were forwarded)
      c60.pitch_min = cfg->pitch_min; c60.pitch_max = cfg->pitch_max; c60.voicing_cutoff = cfg->voicing_cutoff;
      c60.shs_n_harmonics = cfg->shs_n_harmonics; c60.shs_compression = cfg->shs_compression;
      c60.f0_min_energy = cfg->f0_min_energy;
      if (cfg->vit_buffer_len > 0) c60.vit_buffer_len = cfg->vit_buffer_len;
      if (cfg->jitter_search_range > 0.0) c60.jitter_search_range = cfg->jitter_search_range;
    }
    rc = smilehip_plan_create(ctx, &c60, &p->f0_plan);
    if (rc == SMILEHIP_OK && (hipStreamCreateWithFlags(&p->side_stream, hipStreamNonBlocking) != hipSuccess ||
                              hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming) != hipSuccess ||
                              hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming) != hipSuccess))
      rc = fail(SMILEHIP_ERR_HIP, "could not create the side stream of the ComParE chain");
  }
  if (rc == SMILEHIP_OK && cfg->chain_kind == SMILEHIP_CHAIN_EGEMAPS) {      // the 60 ms sub-chain of GeMAPSv01b_core.lld.conf.inc
    smilehip_lld_config c60;
    smilehip_config_compare16_f0(&c60);
    c60.sample_rate = cfg->sample_rate;
    c60.frame_step_sec = cfg->frame_step_sec;
    c60.zero_pad_symmetric = cfg->zero_pad_symmetric;
    c60.pitch_min = cfg->pitch_min; c60.pitch_max = cfg->pitch_max; c60.voicing_cutoff = cfg->voicing_cutoff;
    c60.shs_n_harmonics = cfg->shs_n_harmonics; c60.shs_compression = cfg->shs_compression;
    c60.f0_min_energy = cfg->f0_min_energy;
    c60.vit_buffer_len = cfg->vit_buffer_len;
    c60.jitter_search_range = cfg->jitter_search_range;
    c60.jitter_broken_thresh = cfg->jitter_broken_thresh;
    rc = smilehip_plan_create(ctx, &c60, &p->f0_plan);
    if (rc == SMILEHIP_OK && (hipStreamCreateWithFlags(&p->side_stream, hipStreamNonBlocking) != hipSuccess ||
                              hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming) != hipSuccess ||
                              hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming) != hipSuccess))
      rc = fail(SMILEHIP_ERR_HIP, "could not create the side stream of the eGeMAPS chain");
    int prio_least = 0, prio_greatest = 0;
    if (rc == SMILEHIP_OK && (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess ||
                              hipStreamCreateWithPriority(&p->bg_stream, hipStreamNonBlocking, prio_least) != hipSuccess ||
                              hipEventCreateWithFlags(&p->ev_bg_fork, hipEventDisableTiming) != hipSuccess ||
                              hipEventCreateWithFlags(&p->ev_bg_join, hipEventDisableTiming) != hipSuccess))
      rc = fail(SMILEHIP_ERR_HIP, "could not create the background stream of the eGeMAPS chain");
  }
  if (rc != SMILEHIP_OK) {
    delete p;
    return rc;
  }
  *out = p;
  return SMILEHIP_OK;
}

extern "C" int smilehip_plan_create_host_only(const smilehip_lld_config *cfg, smilehip_plan **out) {
  if (!cfg || !out) return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_create_host_only: null argument");
  *out = nullptr;
  if (!config_size_known(cfg->struct_size))
    return fail(SMILEHIP_ERR_INVALID, "smilehip_lld_config.struct_size %u != %zu (ABI mismatch)", cfg->struct_size,
                sizeof(smilehip_lld_config));
  auto *p = new (std::nothrow) smilehip_plan();
  if (!p) return fail(SMILEHIP_ERR_NOMEM, "out of host memory");
  copy_config(p->cfg, cfg);
  int rc = build_tables(p, false);
  if (rc != SMILEHIP_OK) {
    delete p;
    return rc;
  }
  *out = p;
  return SMILEHIP_OK;
}

extern "C" void smilehip_plan_destroy(smilehip_plan *plan) { delete plan; }

// cFFTmagphase's form of a spectrogram plan: the flag bits as the component orders its branches, the mindBp clamp as it applies it
static const int32_t kSpgFormFlags[5] = {SMILEHIP_MAGPHASE_MAGNITUDE, SMILEHIP_MAGPHASE_MAGNITUDE | SMILEHIP_MAGPHASE_NORMALISE,
                                         SMILEHIP_MAGPHASE_MAGNITUDE | SMILEHIP_MAGPHASE_POWER,
                                         SMILEHIP_MAGPHASE_MAGNITUDE | SMILEHIP_MAGPHASE_NORMALISE | SMILEHIP_MAGPHASE_POWER,
                                         SMILEHIP_MAGPHASE_MAGNITUDE | SMILEHIP_MAGPHASE_NORMALISE | SMILEHIP_MAGPHASE_DBPSD};
extern "C" int smilehip_plan_set_spectrum_form(smilehip_plan *plan, int32_t flags, float dbp_norm, float min_dbp) {
  if (!plan) return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_set_spectrum_form: null plan");
  if (plan->cfg.chain_kind != SMILEHIP_CHAIN_SPECTROGRAM)
    return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_set_spectrum_form: not a spectrogram plan (chain_kind %d)", plan->cfg.chain_kind);
  if (flags & SMILEHIP_MAGPHASE_PHASE)
    return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_set_spectrum_form: SMILEHIP_MAGPHASE_PHASE (cFFTmagphase phase) is not built for the spectrogram chain");
  if (!(flags & SMILEHIP_MAGPHASE_MAGNITUDE))
    return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_set_spectrum_form: SMILEHIP_MAGPHASE_MAGNITUDE must be set (cFFTmagphase magnitude = 0 is not built)");
  const int form = spectrogram::form_of_flags(flags);
  if (form < 0) return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_set_spectrum_form: unknown flag bits 0x%x", (unsigned)flags);
  if (form == spectrogram::kDbPsd && (!(dbp_norm == dbp_norm) || !(min_dbp == min_dbp)))
    return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_set_spectrum_form: dbp_norm / min_dbp is not a number");
  plan->spg_form = spectrogram::form_consts(form, plan->geo.Nfft, dbp_norm, min_dbp);
  return SMILEHIP_OK;
}
extern "C" int smilehip_plan_get_spectrum_form(const smilehip_plan *plan, int32_t *flags, float *dbp_norm, float *min_dbp) {
  if (!plan) return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_get_spectrum_form: null plan");
  if (plan->cfg.chain_kind != SMILEHIP_CHAIN_SPECTROGRAM)
    return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_get_spectrum_form: not a spectrogram plan (chain_kind %d)", plan->cfg.chain_kind);
  if (flags) *flags = kSpgFormFlags[plan->spg_form.form];
  if (dbp_norm) *dbp_norm = plan->spg_form.dbp_norm;
  if (min_dbp) *min_dbp = plan->spg_form.min_dbp;
  return SMILEHIP_OK;
}

extern "C" int smilehip_plan_set_lpc_order(smilehip_plan *plan, int32_t p) {
  if (!plan) return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_set_lpc_order: null plan");
  if (plan->cfg.chain_kind != SMILEHIP_CHAIN_EMOBASE)
    return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_set_lpc_order: not an emobase plan (chain_kind %d)", plan->cfg.chain_kind);
  if (p < 2 || p > emobase::kMaxLpcOrder || (p & 1))
    return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_set_lpc_order: cLpc p must be even, 2 .. %d; got %d", emobase::kMaxLpcOrder, p);
  plan->emo_lpc_order = p;
  return SMILEHIP_OK;
}
extern "C" int smilehip_plan_get_lpc_order(const smilehip_plan *plan, int32_t *p) {
  if (!plan || plan->cfg.chain_kind != SMILEHIP_CHAIN_EMOBASE)
    return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_get_lpc_order: not an emobase plan");
  if (p) *p = plan->emo_lpc_order;
  return SMILEHIP_OK;
}

extern "C" int smilehip_plan_emobase_frame40(const smilehip_plan *plan, int64_t *frame_size, int64_t *fft_size) {
  if (!plan || plan->cfg.chain_kind != SMILEHIP_CHAIN_EMOBASE)
    return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_emobase_frame40: not an emobase plan");
  if (frame_size) *frame_size = plan->geo40.N;
  if (fft_size) *fft_size = plan->geo40.Nfft;
  return SMILEHIP_OK;
}

int plan_n_static(const smilehip_plan *p) {
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_EMOBASE) return emobase::n_lld(p->emo_lpc_order);
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_COMPARE_F0) return 2;
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_PROSODY_SHS || p->cfg.chain_kind == SMILEHIP_CHAIN_PROSODY_ACF) return 3;
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FFT || p->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FILT) return p->cfg.chroma_octave_size;
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_AUDSPEC) return p->mel.n_bands;
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_SPECTROGRAM) return (int)p->geo.K;
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_COMPARE) return 65;
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_EGEMAPS) return 25;
  return p->cfg.chain_kind == SMILEHIP_CHAIN_IS09 ? 16
         : (p->cfg.chain_kind == SMILEHIP_CHAIN_COMPARE_AB ? 59 : p->dct.n_mfcc + (p->cfg.append_log_energy ? 1 : 0));
}
int plan_n_out(const smilehip_plan *p) { return plan_n_static(p) * (1 + p->cfg.n_delta); }
int plan_row_extra(const smilehip_plan *p) {
  return (p->cfg.chain_kind == SMILEHIP_CHAIN_IS09 || p->cfg.chain_kind == SMILEHIP_CHAIN_PROSODY_SHS ||
          p->cfg.chain_kind == SMILEHIP_CHAIN_PROSODY_ACF || p->cfg.chain_kind == SMILEHIP_CHAIN_EMOBASE) ? p->cfg.sma_win / 2 : 0;
}

extern "C" int smilehip_plan_geometry(const smilehip_plan *p, smilehip_geometry *g) {
  if (!p || !g) return fail(SMILEHIP_ERR_INVALID, "smilehip_plan_geometry: null argument");
  g->frame_size = p->geo.N;
  g->frame_step = p->geo.H;
  g->fft_size = p->geo.Nfft;
  g->n_bins = p->geo.K;
  g->n_static = plan_n_static(p);
  g->n_out = plan_n_out(p);
  g->frame_period = p->geo.frame_period;
  g->fft_frame_size_sec = p->geo.fft_frame_size_sec;
  return SMILEHIP_OK;
}

extern "C" int64_t smilehip_num_frames(const smilehip_plan *p, int64_t n_samples) {
  if (!p) return fail(SMILEHIP_ERR_INVALID, "smilehip_num_frames: null plan");
  if (p->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FILT) return tonefilt::rows_of(n_samples, p->tonefilt.P);   // blocks, the last one padded
  if (n_samples < p->geo.N) return 0;
  return (n_samples - p->geo.N) / p->geo.H + 1;
}

extern "C" double smilehip_frame_time(const smilehip_plan *p, int64_t t) {
  // vIdx * level period; the framer's level period is frameStep
  // (winToVecProcessor.cpp:562-568), time = vIdx*T via squashTimeMeta
  return p ? double(t) * p->geo.frame_period : 0.0;
}

extern "C" double smilehip_row_time(const smilehip_plan *plan, int64_t n_frames, int64_t row) {
  if (!plan || row < 0) return 0.0;
  // prosodyShs: the rows carry the time stamps of cPitchSmoother's level, whose frame j has that of input frame j + 1
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_PROSODY_SHS)
    return smilehip_frame_time(plan, n_frames >= 2 ? (row < n_frames - 2 ? row : n_frames - 2) + 1 : 0);
  // spectrogram: as measured on the binary's CSV sink, row t carries the time of its first sample, t * H / sample_rate -- t * frameStep
  // where frameStep is a whole number of samples, 0.009977 t at 11.025 kHz and 0.010023 t at 22.05 kHz (the HTK header keeps frameStep)
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_SPECTROGRAM) return double(row * plan->geo.H) / plan->cfg.sample_rate;
  // emobase (lld_emobase_ops.hpp: row_time_frame; n_frames = the utterance's 25 ms frames): the left-padding rows carry their own index
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_EMOBASE) return smilehip_frame_time(plan, emobase::row_time_frame(n_frames, 0, plan->cfg.sma_win / 2, row));
  if (plan->cfg.chain_kind == SMILEHIP_CHAIN_MFCC || plan->cfg.chain_kind == SMILEHIP_CHAIN_PLP || plan->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FFT ||
      plan->cfg.chain_kind == SMILEHIP_CHAIN_CHROMA_FILT || plan->cfg.chain_kind == SMILEHIP_CHAIN_AUDSPEC ||
      plan->cfg.chain_kind == SMILEHIP_CHAIN_COMPARE_F0 || plan->cfg.chain_kind == SMILEHIP_CHAIN_EGEMAPS || n_frames <= 1)
    return smilehip_frame_time(plan, row);
  // IS09 and prosodyAcf (lld_prosody_acf_ops.hpp: row_time_frame): the smoother's end-of-input rows repeat the last frame's time
  return smilehip_frame_time(plan, row < n_frames - 1 ? row : n_frames - 1);
}

template <typename T>
static int64_t copy_out(const std::vector<T> &v, T *out, int64_t cap) {
  if (out) {
    if (cap < (int64_t)v.size()) return fail(SMILEHIP_ERR_INVALID, "output buffer too small");
    std::memcpy(out, v.data(), v.size() * sizeof(T));
  }
  return (int64_t)v.size();
}
extern "C" int64_t smilehip_plan_get_window(const smilehip_plan *p, float *o, int64_t cap) { return copy_out(p->h_window, o, cap); }
extern "C" int64_t smilehip_plan_get_mel_weights(const smilehip_plan *p, float *o, int64_t cap) { return copy_out(p->mel.coef, o, cap); }
extern "C" int64_t smilehip_plan_get_mel_chanmap(const smilehip_plan *p, int32_t *o, int64_t cap) { return copy_out(p->mel.chan, o, cap); }
extern "C" int64_t smilehip_plan_get_dct(const smilehip_plan *p, float *o, int64_t cap) { return copy_out(p->dct.cos_rows, o, cap); }
extern "C" int64_t smilehip_plan_get_lifter(const smilehip_plan *p, float *o, int64_t cap) { return copy_out(p->dct.lifter, o, cap); }
