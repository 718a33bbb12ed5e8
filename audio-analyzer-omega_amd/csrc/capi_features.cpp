// libomega.so host side: the per-frame feature families over a spectrum and its audio -- harmonic
// analysis, genre features and hip-hop features.

#include "host.hpp"

namespace {

// The spectrum's frequency table of a configure call (after the caller's NULL check): at least two
// bins, a built bin count, finite and strictly increasing.
int check_freq_table(omega_ctx* c, const char* who, int n_bins, const double* freqs) {
  if (n_bins < 2) return fail(c, OMEGA_EINVAL, "%s: n_bins %d", who, n_bins);
  if (n_bins < kHarmonicMinBins || n_bins > kHarmonicMaxBins)
    return fail(c, OMEGA_EUNSUP, "%s: %d spectrum bins (%d..%d are built)", who, n_bins, kHarmonicMinBins,
                kHarmonicMaxBins);
  for (int i = 0; i < n_bins; ++i)
    if (!std::isfinite(freqs[i]) || (i && !(freqs[i] > freqs[i - 1])))
      return fail(c, OMEGA_EINVAL, "%s: freqs must be finite and strictly increasing (entry %d)", who, i);
  return 0;
}

// (Re)configures a stream: table uploaded, both spectra allocated; *set goes false once old ones are freed.
int configure_stream(omega_ctx* c, PrevSpectrum& s, const double* freqs, int n_bins, bool* set) {
  if (s.freqs) {  // a reconfiguration: work already enqueued may still read the old tables
    HIPC(c, hipStreamSynchronize(c->stream));
    for (void* q : {(void*)s.freqs, (void*)s.prev[0], (void*)s.prev[1]}) release(c, q);
    s.freqs = nullptr;
    s.prev[0] = s.prev[1] = nullptr;
    *set = false;
  }
  const std::vector<double> tab(freqs, freqs + n_bins);
  int e = upload(c, &s.freqs, tab);
  for (int b = 0; b < 2 && !e; ++b) e = dalloc(c, &s.prev[b], (size_t)n_bins);
  if (e) return e;
  s.cur = 0;
  s.has_prev = false;
  return 0;
}

}  // namespace

extern "C" {

void omega_harmonic_config_default(omega_harmonic_config* cfg) {
  if (!cfg) return;
  *cfg = omega_harmonic_config{};
  cfg->sample_rate = 48000;
  cfg->n_bins = 512;
  cfg->max_series = 16;
}

int omega_harmonic_configure(omega_ctx* c, const omega_harmonic_config* cfg, const double* freqs) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (!freqs) return fail(c, OMEGA_EINVAL, "harmonic: freqs is NULL");
  if (cfg->sample_rate <= 0) return fail(c, OMEGA_EINVAL, "harmonic: need sample_rate > 0");
  if (cfg->max_series < 1 || cfg->max_series > 1024)
    return fail(c, OMEGA_EINVAL, "harmonic: max_series %d outside 1..1024", cfg->max_series);
  if (int e = check_freq_table(c, "harmonic", cfg->n_bins, freqs)) return e;
  HIPC(c, hipSetDevice(c->device));
  if (int e = configure_stream(c, c->harm.stream, freqs, cfg->n_bins, &c->harm.set)) return e;
  HarmonicParams p{};
  p.n_bins = cfg->n_bins;
  p.freqs = c->harm.stream.freqs;
  p.fs = cfg->sample_rate;
  p.nyquist = cfg->sample_rate / 2.0;
  p.max_series = cfg->max_series;
  c->harm.p = p;
  c->harm.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_harmonic_reset(omega_ctx* c) try {
  if (!c) return OMEGA_EINVAL;
  c->harm.stream.has_prev = false;
  return 0;
} catch (...) {
  return guard_fail(c);
}

namespace {
// np.hamming(m) on the device, cached per audio length: at most kHarmonicWindows tables (a caller that
// varies m does not grow device memory; past the cap the cache is emptied once the stream is idle). m is any
// length in 15..8192 and the pointer is fetched per call, so this is the one evicting cache: omega_ctx::tables
// never frees an entry and must not absorb these.
constexpr size_t kHarmonicWindows = 8;
int harmonic_window(omega_ctx* c, int m, double** out) {
  auto it = c->harm.ham.find(m);
  if (it == c->harm.ham.end()) {
    if (c->harm.ham.size() >= kHarmonicWindows) {
      HIPC(c, hipStreamSynchronize(c->stream));
      for (auto& kv : c->harm.ham) release(c, kv.second);
      c->harm.ham.clear();
    }
    double* d = nullptr;
    if (int e = upload(c, &d, np_window64(OMEGA_WIN_HAMMING, m))) return e;
    it = c->harm.ham.emplace(m, d).first;
  }
  *out = it->second;
  return 0;
}
}  // namespace

int omega_harmonic_analyze(omega_ctx* c, const float* spectra, int64_t spec_stride, const void* audio, int32_t f64,
                           int32_t m, int64_t audio_stride, int64_t n_frames, double* out, int32_t* series_bins,
                           double* series_strength, int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!c->harm.set) return fail(c, OMEGA_EINVAL, "harmonic: omega_harmonic_configure has not been called");
  const int K = c->harm.p.n_bins, S = c->harm.p.max_series;
  if (!spectra || n_frames < 0 || spec_stride < 1) return fail(c, OMEGA_EINVAL, "harmonic: bad spectrum layout");
  if (audio && (m <= 0 || audio_stride < 1)) return fail(c, OMEGA_EINVAL, "harmonic: bad audio layout");
  if (audio && (m < kHarmonicMinAudio || m > kHarmonicMaxAudio))
    return fail(c, OMEGA_EUNSUP, "harmonic: %d audio samples per frame (%d..%d are built)", m, kHarmonicMinAudio,
                kHarmonicMaxAudio);
  if (n_frames == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  double* dham = nullptr;
  if (audio)
    if (int e = harmonic_window(c, m, &dham)) return e;
  HostCall h(c, mem);
  const Rows32 dspec = h.rows32(spectra, spec_stride, K, n_frames);
  const Rows daudio = h.rows(audio, audio_stride, m, f64, n_frames);
  double* dout = h.out(out, (size_t)n_frames * kHarmonicCols);
  int32_t* dbins = h.out(series_bins, (size_t)n_frames * S * (1 + kHarmonicMaxHarm));
  double* dstr = h.out(series_strength, (size_t)n_frames * S);
  if (h.err) return h.err;
  HarmonicParams p = c->harm.p;
  p.m = audio ? m : 0;
  p.ham = dham;
  // one launch covers at most 2^30 workgroups (two per frame)
  if (int e = for_frame_chunks(n_frames, (int64_t)1 << 29, [&](int64_t f0, int64_t count) -> int {
    HarmonicParams q = p;
    q.n_frames = count;
    q.spec = dspec.from(f0);
    q.audio = daudio.from(f0);
    c->harm.stream.chunk(dspec, f0, count, n_frames, &q.prev_in, &q.prev_out);
    q.out = dout + f0 * kHarmonicCols;
    q.series_bins = dbins ? dbins + f0 * S * (1 + kHarmonicMaxHarm) : nullptr;
    q.series_strength = dstr ? dstr + f0 * S : nullptr;
    HIPC(c, launch_harmonic(q, c->stream));
    return 0;
  }))
    return e;
  c->harm.stream.advance();
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_harmonic_metrics(omega_ctx* c, const float* spectrum, const float* previous, const void* audio, int32_t f64,
                           int32_t m, double fundamental, double* out, int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!c->harm.set) return fail(c, OMEGA_EINVAL, "harmonic: omega_harmonic_configure has not been called");
  if (!spectrum) return fail(c, OMEGA_EINVAL, "harmonic: spectrum is NULL");
  if (audio && m <= 0) return fail(c, OMEGA_EINVAL, "harmonic: bad audio layout");
  if (audio && (m < kHarmonicMinAudio || m > kHarmonicMaxAudio))
    return fail(c, OMEGA_EUNSUP, "harmonic: %d audio samples per frame (%d..%d are built)", m, kHarmonicMinAudio,
                kHarmonicMaxAudio);
  HIPC(c, hipSetDevice(c->device));
  double* dham = nullptr;
  if (audio)
    if (int e = harmonic_window(c, m, &dham)) return e;
  const int K = c->harm.p.n_bins;
  HostCall h(c, mem);
  HarmonicParams p = c->harm.p;  // (the stream state -- the stored previous spectrum -- is neither read nor written)
  p.spec = h.rows32(spectrum, K, K, 1);
  p.audio = h.rows(audio, m > 0 ? m : 1, m, f64, 1);
  p.prev_in = h.in(previous, (size_t)K * sizeof(float));
  p.out = h.out(out, (size_t)kHarmonicCols);
  if (h.err) return h.err;
  p.m = audio ? m : 0;
  p.ham = dham;
  p.n_frames = 1;
  p.ungated = 1;
  p.f0 = fundamental;
  p.prev_out = nullptr;
  HIPC(c, launch_harmonic(p, c->stream));
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

void omega_genre_config_default(omega_genre_config* cfg) {
  if (!cfg) return;
  *cfg = omega_genre_config{};
  cfg->sample_rate = 48000;
  cfg->n_bins = 512;
}

int omega_genre_configure(omega_ctx* c, const omega_genre_config* cfg, const double* freqs) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (!freqs) return fail(c, OMEGA_EINVAL, "genre: freqs is NULL");
  if (cfg->sample_rate <= 0) return fail(c, OMEGA_EINVAL, "genre: need sample_rate > 0");
  const int K = cfg->n_bins;
  if (int e = check_freq_table(c, "genre", K, freqs)) return e;
  HIPC(c, hipSetDevice(c->device));
  if (int e = configure_stream(c, c->genre.stream, freqs, K, &c->genre.set)) return e;
  GenreParams p{};
  p.n_bins = K;
  p.freqs = c->genre.stream.freqs;
  // the reference's masks, with its own comparisons in float64; over an increasing table each is one range
  auto in_band = [](int b, double f) {
    switch (b) {
      case 0: return f >= 20 && f <= 250;      // compute_bass_emphasis: bass
      case 1: return f > 250 && f <= 2000;     //                        mid
      case 2: return f >= 200 && f <= 4000;    // compute_vocal_presence: vocal
      case 3: return f >= 300 && f <= 3000;    //                         core
      case 4: return f >= 4000 && f <= 10000;  // compute_high_freq_energy: high
      case 5: return f <= 10000;               //                           total
      case 6: return f >= 20 && f < 500;       // compute_mid_frequency_dominance: low
      case 7: return f >= 500 && f <= 2000;    //                                  mid
      case 8: return f > 2000 && f <= 8000;    //                                  high
      default: return f >= 100 && f <= 4000;   // compute_spectral_complexity
    }
  };
  for (int b = 0; b < kGenreBands; ++b)
    mask_range(K, [&](int i) { return freqs[i]; }, [&](double f) { return in_band(b, f); }, &p.band_lo[b], &p.band_n[b]);
  c->genre.p = p;
  c->genre.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_genre_reset(omega_ctx* c) try {
  if (!c) return OMEGA_EINVAL;
  c->genre.stream.has_prev = false;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_genre_features(omega_ctx* c, const float* spectra, int64_t spec_stride, const void* audio, int32_t f64,
                         int32_t m, int64_t audio_stride, int64_t n_frames, double* out, int32_t* peak_bins,
                         int mem) try {
  if (!c || !out || !peak_bins) return OMEGA_EINVAL;
  if (!c->genre.set) return fail(c, OMEGA_EINVAL, "genre: omega_genre_configure has not been called");
  const int K = c->genre.p.n_bins;
  if (!spectra || n_frames < 0 || spec_stride < 1) return fail(c, OMEGA_EINVAL, "genre: bad spectrum layout");
  if (!audio || m <= 0 || audio_stride < 1) return fail(c, OMEGA_EINVAL, "genre: bad audio layout");
  if (m < kHarmonicMinAudio || m > kHarmonicMaxAudio)
    return fail(c, OMEGA_EUNSUP, "genre: %d audio samples per frame (%d..%d are built)", m, kHarmonicMinAudio,
                kHarmonicMaxAudio);
  if (n_frames == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  HostCall h(c, mem);
  const Rows32 dspec = h.rows32(spectra, spec_stride, K, n_frames);
  const Rows daudio = h.rows(audio, audio_stride, m, f64, n_frames);
  double* dout = h.out(out, (size_t)n_frames * kGenreCols);
  int32_t* dbins = h.out(peak_bins, (size_t)n_frames * kGenrePeaks);
  if (h.err) return h.err;
  GenreParams p = c->genre.p;
  p.m = m;
  // np.percentile's virtual index (m - 1) q with q = 95 / 100 and 20 / 100 in the audio's precision
  if (f64) {
    const double v95 = (double)(m - 1) * (95.0 / 100.0), v20 = (double)(m - 1) * (20.0 / 100.0);
    p.rank95 = (int)std::floor(v95), p.gamma95 = v95 - std::floor(v95);
    p.rank20 = (int)std::floor(v20), p.gamma20 = v20 - std::floor(v20);
  } else {
    const volatile float q95 = 95.0f / 100.0f, q20 = 20.0f / 100.0f;
    const volatile float v95 = (float)(m - 1) * q95, v20 = (float)(m - 1) * q20;
    p.rank95 = (int)std::floor(v95), p.gamma95 = (double)v95 - std::floor((double)v95);
    p.rank20 = (int)std::floor(v20), p.gamma20 = (double)v20 - std::floor((double)v20);
  }
  if (p.rank95 + 1 >= m || p.rank20 + 1 >= m) return fail(c, OMEGA_EINVAL, "genre: percentile rank outside the frame");
  // one launch covers at most 2^30 workgroups (two per frame)
  if (int e = for_frame_chunks(n_frames, (int64_t)1 << 29, [&](int64_t f0, int64_t count) -> int {
    GenreParams q = p;
    q.n_frames = count;
    q.spec = dspec.from(f0);
    q.audio = daudio.from(f0);
    c->genre.stream.chunk(dspec, f0, count, n_frames, &q.prev_in, &q.prev_out);
    q.out = dout + f0 * kGenreCols;
    q.peak_bins = dbins + f0 * kGenrePeaks;
    HIPC(c, launch_genre(q, c->stream));
    return 0;
  }))
    return e;
  c->genre.stream.advance();
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

void omega_hiphop_config_default(omega_hiphop_config* cfg) {
  if (!cfg) return;
  *cfg = omega_hiphop_config{};
  cfg->sample_rate = 48000;
  cfg->n_bins = 512;
}

namespace {
// the reference's filter bank (hip_hop_detector.py:70-92; bass_sos is never used): 0 sub-bass, 1 kick, 2 hi-hat
void hiphop_design(int sample_rate, int which, double out[4][6]) {
  const double nyquist = sample_rate / 2.0;
  const double lo = which == 0 ? 20.0 : which == 1 ? 40.0 : 3000.0;
  const double hi = which == 0 ? 60.0 : which == 1 ? 100.0 : std::min(10000.0, nyquist * 0.9);
  butter4_bandpass_sos(lo, hi, (double)sample_rate, out);
}
}  // namespace

int omega_hiphop_design_sos(int32_t sample_rate, int32_t which, double* out) try {
  if (!out || which < 0 || which > 2 || sample_rate < kHipHopMinRate) return OMEGA_EINVAL;
  double sos[4][6];
  hiphop_design(sample_rate, which, sos);
  std::memcpy(out, sos, sizeof sos);
  return 0;
} catch (...) {
  return guard_fail(nullptr);
}

int omega_hiphop_configure(omega_ctx* c, const omega_hiphop_config* cfg, const double* freqs) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (!freqs) return fail(c, OMEGA_EINVAL, "hiphop: freqs is NULL");
  if (cfg->sample_rate <= 0) return fail(c, OMEGA_EINVAL, "hiphop: need sample_rate > 0");
  if (cfg->sample_rate < kHipHopMinRate)
    return fail(c, OMEGA_EUNSUP, "hiphop: sample rate %d (%d Hz and above are built)", cfg->sample_rate, kHipHopMinRate);
  const int K = cfg->n_bins;
  if (int e = check_freq_table(c, "hiphop", K, freqs)) return e;
  HipHopParams p{};
  p.n_bins = K;
  const double nyquist = cfg->sample_rate / 2.0;
  // the reference's masks, with its own comparisons in float64; over an increasing table each is one range
  auto in_band = [nyquist](int b, double f) {
    switch (b) {
      case 0: return f >= 20 && f <= 60;      // _detect_sub_bass: sub-bass
      case 1: return f >= 60 && f <= 250;     //                   bass
      case 2: return f < nyquist;             //                   total (the Nyquist bin is left out)
      case 3: return f >= 20 && f <= 500;     // _analyze_spectral_tilt: low
      case 4: return f >= 500 && f <= 2000;   //                         mid
      case 5: return f >= 2000 && f <= 8000;  //                         high
      case 6: return f >= 200 && f <= 3000;   // _detect_rap_vocals: vocal
      case 7: return f >= 300 && f <= 2000;   //                     core
      default: return true;                   //                     every bin
    }
  };
  for (int b = 0; b < kHipHopBands; ++b)
    mask_range(K, [&](int i) { return freqs[i]; }, [&](double f) { return in_band(b, f); }, &p.band_lo[b], &p.band_n[b]);
  for (int w = 0; w < 3; ++w) {
    hiphop_design(cfg->sample_rate, w, c->hiphop.sos[w]);
    for (int s = 0; s < 4; ++s) {
      const double* q = c->hiphop.sos[w][s];
      W64Stage& st = p.sos[w][s];
      st.b0 = q[0], st.b1 = q[1], st.b2 = q[2], st.a1 = q[4], st.a2 = q[5];
    }
  }
  p.distance = (int)(0.1 * cfg->sample_rate);
  c->hiphop.p = p;
  c->hiphop.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_hiphop_get_sos(omega_ctx* c, int32_t which, double* out) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!c->hiphop.set) return fail(c, OMEGA_EINVAL, "hiphop: omega_hiphop_configure has not been called");
  if (which < 0 || which > 2) return fail(c, OMEGA_EINVAL, "hiphop: filter %d (0 sub-bass, 1 kick, 2 hi-hat)", which);
  std::memcpy(out, c->hiphop.sos[which], sizeof c->hiphop.sos[which]);
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_hiphop_features(omega_ctx* c, const float* spectra, int64_t spec_stride, const void* audio, int32_t f64,
                          int32_t m, int64_t audio_stride, int64_t n_frames, double* out, int32_t* kick_peaks,
                          int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!c->hiphop.set) return fail(c, OMEGA_EINVAL, "hiphop: omega_hiphop_configure has not been called");
  const int K = c->hiphop.p.n_bins;
  if (!spectra || n_frames < 0 || spec_stride < 1) return fail(c, OMEGA_EINVAL, "hiphop: bad spectrum layout");
  if (!audio || m <= 0 || audio_stride < 1) return fail(c, OMEGA_EINVAL, "hiphop: bad audio layout");
  if (!is_pow2_in(m, kHipHopMinAudio, kHipHopMaxAudio))
    return fail(c, OMEGA_EUNSUP, "hiphop: %d audio samples per frame (the powers of two %d..%d are built)", m,
                kHipHopMinAudio, kHipHopMaxAudio);
  if (n_frames == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  HipHopParams p = c->hiphop.p;
  if (int e = get_twiddles64(c, m, m / 2 + 1, &p.tw)) return e;
  HostCall h(c, mem);
  const Rows32 dspec = h.rows32(spectra, spec_stride, K, n_frames);
  const Rows daudio = h.rows(audio, audio_stride, m, f64, n_frames);
  double* dout = h.out(out, (size_t)n_frames * kHipHopCols);
  int32_t* dpeaks = h.out(kick_peaks, (size_t)n_frames * kHipHopPeaks);
  if (h.err) return h.err;
  p.m = m;
  // one launch covers at most 2^30 workgroups (two per frame)
  if (int e = for_frame_chunks(n_frames, (int64_t)1 << 29, [&](int64_t f0, int64_t count) -> int {
    HipHopParams q = p;
    q.n_frames = count;
    q.spec = dspec.from(f0);
    q.audio = daudio.from(f0);
    q.out = dout + f0 * kHipHopCols;
    q.kick_peaks = dpeaks ? dpeaks + f0 * kHipHopPeaks : nullptr;
    HIPC(c, launch_hiphop(q, c->stream));
    return 0;
  }))
    return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
