// libomega.so host side: the time-domain entry points -- VU meters, transients, pitch detection and
// stereo phase correlation.

#include "host.hpp"

namespace omega_host {

// the float64 tables of hilbert64.hpp's n-point real transform (n a power of two): e^{-2 pi i m / (n / 2)} for
// m < n / 4 and e^{-2 pi i q / n} for q <= n / 2, each asked for as its period's common table (period / 2 + 1)
int tr_pow2_tables(omega_ctx* c, int n, const double2** tw, const double2** tw2) {
  if (int e = get_twiddles64(c, n / 2, n / 4 + 1, tw)) return e;
  return get_twiddles64(c, n, n / 2 + 1, tw2);
}

}  // namespace omega_host

extern "C" {

int omega_vu_reset(omega_ctx* c) try {
  if (!c) return OMEGA_EINVAL;
  c->vu.total = 0;
  if (!c->vu.st[0]) return 0;
  HIPC(c, hipSetDevice(c->device));
  const int C = c->cfg.n_channels;
  std::vector<double> st((size_t)C * 3);
  for (int i = 0; i < C; ++i) {  // vu_meters.py:33-42: display and peak at -60, hold time 0
    st[i * 3] = -60.0;
    st[i * 3 + 1] = -60.0;
    st[i * 3 + 2] = 0.0;
  }
  for (int b = 0; b < 2; ++b)
    HIPC(c, hipMemcpyAsync(c->vu.st[b], st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_vu_update(omega_ctx* c, const void* x, int32_t f64, int64_t n_updates, int32_t chunk, int64_t update_stride,
                    int64_t channel_stride, const double* dt, double* out, int mem) try {
  if (!c || !out || !dt) return OMEGA_EINVAL;
  if (!x || n_updates < 0 || chunk < 1) return fail(c, OMEGA_EINVAL, "vu update: bad input layout");
  if (n_updates == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  const int C = c->cfg.n_channels;
  const int64_t Wv = (int64_t)(0.3 * c->cfg.sample_rate);  // vu_meters.py:28-30
  if (!c->vu.st[0]) {
    for (int b = 0; b < 2; ++b) {
      int e = dalloc(c, &c->vu.hist[b], (size_t)C * Wv);
      if (!e) e = dalloc(c, &c->vu.st[b], (size_t)C * 3);
      if (e) return e;
    }
    if (int e = omega_vu_reset(c)) return e;
  }
  if (int e = grow(c, &c->vu.ms, &c->vu.ms_cap, n_updates * C)) return e;
  HostCall h(c, mem);
  VuParams p{};
  p.x = h.rows(x, update_stride, (C - 1) * channel_stride + chunk, f64, n_updates);  // (a row: every channel's chunk)
  p.dt = h.in(dt, (size_t)n_updates * sizeof(double));
  p.out = h.out(out, (size_t)n_updates * C * 3);
  if (h.err) return h.err;
  p.n = n_updates;
  p.chunk = chunk;
  p.channel_stride = channel_stride;
  p.C = C;
  const int a = c->vu.cur, b = a ^ 1;
  p.hist_in = c->vu.hist[a];
  p.hist_out = c->vu.hist[b];
  p.hist_n = std::min(c->vu.total, Wv);
  p.Wv = Wv;
  p.ms = c->vu.ms;
  p.st_in = c->vu.st[a];
  p.st_out = c->vu.st[b];
  HIPC(c, launch_vu(p, c->stream));
  c->vu.cur = b;
  c->vu.total += n_updates * chunk;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_transients(omega_ctx* c, const void* x, int32_t f64, int64_t n_frames, int32_t n, int64_t frame_stride,
                     double* out, int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!x || n_frames < 0 || frame_stride < n) return fail(c, OMEGA_EINVAL, "transients: bad frame layout");
  if (n < 64) return fail(c, OMEGA_EINVAL, "transients: frame length %d below 64 (transient.py:21)", n);
  const bool pow2 = n <= 8192 && !(n & (n - 1));
  if (n_frames == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  TransientParams p{};
  if (int e = get_savgol(c, 21, &p.sg)) return e;
  if (!pow2) {  // other lengths: the complex mixed-radix transform (transient_any_kernel)
    auto ia = c->tr.any.find(n);
    if (ia == c->tr.any.end()) {
      const std::vector<int> rad = fft_radices(n);
      if ((int)rad.size() > kTrMaxStages) return fail(c, OMEGA_EUNSUP, "transients: length %d: too many factors", n);
      double2* d = nullptr;
      if (int e = upload(c, &d, twiddles64(n, n))) return e;
      ia = c->tr.any.emplace(n, std::make_pair(rad, d)).first;
    }
    p.n_stages = (int)ia->second.first.size();
    for (int i = 0; i < p.n_stages; ++i) p.radix[i] = ia->second.first[i];
    p.twn = ia->second.second;
  }
  // frames too long for LDS work in global buffers (2 n double2 per frame), launched in slices of
  // frames whose buffers stay within 64 MiB
  int64_t per = n_frames;
  if (!pow2 && (size_t)n * 2 * sizeof(double2) > 160 * 1024 - 64) {
    per = std::max<int64_t>(1, std::min<int64_t>(n_frames, (int64_t)(64 << 20) / (2 * (int64_t)n * (int64_t)sizeof(double2))));
    if (int e = grow(c, &c->tr.scratch, &c->tr.scratch_cap, per * 2 * (int64_t)n)) return e;
    p.scratch = c->tr.scratch;
  }
  if (pow2)
    if (int e = tr_pow2_tables(c, n, &p.tw, &p.tw2)) return e;
  HostCall h(c, mem);
  const Rows dx = h.rows(x, frame_stride, n, f64, n_frames);
  double* dout = h.out(out, (size_t)n_frames * kTransientCols);
  if (h.err) return h.err;
  p.n = n;
  p.fs = c->cfg.sample_rate;
  if (pow2) {
    p.x = dx;
    p.n_frames = n_frames;
    p.out = dout;
    HIPC(c, launch_transients(p, c->stream));
  } else {
    if (int e = for_frame_chunks(n_frames, per, [&](int64_t f0, int64_t count) -> int {
      TransientParams q = p;
      q.x = dx.from(f0);
      q.n_frames = count;
      q.out = dout + f0 * kTransientCols;
      HIPC(c, launch_transients_any(q, c->stream));
      return 0;
    }))
      return e;
  }
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

void omega_pitch_config_default(omega_pitch_config* cfg) {
  if (!cfg) return;
  // PitchDetectionConfig's defaults at 48 kHz after adjust_for_sample_rate (pitch_detection_config.py:13-121)
  *cfg = omega_pitch_config{};
  cfg->sample_rate = 48000;
  cfg->min_pitch = 50.0;
  cfg->max_pitch = 2000.0;
  cfg->yin_threshold = 0.15;
  cfg->yin_window_size = 1920;
  cfg->enable_preprocessing = 1;
  cfg->highpass_frequency = 80.0;
  cfg->highpass_order = 4;
  cfg->enable_compression = 1;
  cfg->compression_threshold = 0.1;
  cfg->compression_ratio = 0.5;
}

int omega_pitch_configure(omega_ctx* c, const omega_pitch_config* cfg) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (cfg->sample_rate <= 0 || !(cfg->min_pitch > 0.0) || !(cfg->max_pitch > cfg->min_pitch))
    return fail(c, OMEGA_EINVAL, "pitch: need sample_rate > 0 and 0 < min_pitch < max_pitch");
  if (!(cfg->yin_threshold > 0.0 && cfg->yin_threshold < 1.0) || cfg->yin_window_size <= 0)
    return fail(c, OMEGA_EINVAL, "pitch: need 0 < yin_threshold < 1 and yin_window_size > 0");
  const int min_period = (int)(cfg->sample_rate / cfg->max_pitch), max_period = (int)(cfg->sample_rate / cfg->min_pitch);
  if (min_period < 1) return fail(c, OMEGA_EINVAL, "pitch: max_pitch %g above the sample rate", cfg->max_pitch);
  PitchParams p{};
  if (cfg->enable_preprocessing) {
    if (!(cfg->highpass_frequency > 0.0) || !(cfg->highpass_frequency < cfg->sample_rate / 2.0))
      return fail(c, OMEGA_EINVAL, "pitch: high-pass frequency %g outside (0, fs/2)", cfg->highpass_frequency);
    if (cfg->highpass_order != 4)
      return fail(c, OMEGA_EUNSUP, "pitch: high-pass order %d (every preset's order 4 is built)", cfg->highpass_order);
    BiquadCoef sos[2];
    butter4_highpass_sos(cfg->highpass_frequency, cfg->sample_rate, sos);
    for (int s = 0; s < 2; ++s) {
      W64Stage& q = p.hp[s];
      q.b0 = sos[s].b[0], q.b1 = sos[s].b[1], q.b2 = sos[s].b[2];
      q.a1 = sos[s].a[1], q.a2 = sos[s].a[2];
    }
  }
  p.fs = cfg->sample_rate;
  p.min_pitch = cfg->min_pitch;
  p.max_pitch = cfg->max_pitch;
  p.min_period = min_period;
  p.max_period = max_period;
  p.yin_threshold = cfg->yin_threshold;
  p.yin_window = cfg->yin_window_size;
  p.preprocess = cfg->enable_preprocessing ? 1 : 0;
  p.compress = cfg->enable_compression ? 1 : 0;
  p.comp_threshold = cfg->compression_threshold;
  p.comp_ratio = cfg->compression_ratio;
  c->pitch.p = p;
  c->pitch.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_pitch_detect(omega_ctx* c, const void* x, int32_t f64, int64_t n_frames, int32_t n, int64_t frame_stride,
                       double* out, int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!c->pitch.set) return fail(c, OMEGA_EINVAL, "pitch: omega_pitch_configure has not been called");
  if (!x || n_frames < 0 || n <= 0 || frame_stride < 1) return fail(c, OMEGA_EINVAL, "pitch: bad frame layout");
  if (n_frames == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  if (n < c->pitch.p.yin_window) {  // detect_pitch_advanced's all-zero result (:487-495)
    if (mem == OMEGA_MEM_HOST) {
      std::memset(out, 0, (size_t)n_frames * kPitchCols * sizeof(double));
      return 0;
    }
    HIPC(c, hipMemsetAsync(out, 0, (size_t)n_frames * kPitchCols * sizeof(double), c->stream));
    return 0;
  }
  if (n != 2048 && n != 4096 && n != 8192)
    return fail(c, OMEGA_EUNSUP, "pitch: frame length %d (2048, 4096 and 8192 are built)", n);
  PitchParams p = c->pitch.p;
  if (int e = get_twiddles64(c, 2 * n, n + 1, &p.tw)) return e;
  if (int e = get_window64(c, OMEGA_WIN_HANN, n, &p.win)) return e;
  HostCall h(c, mem);
  const Rows dx = h.rows(x, frame_stride, n, f64, n_frames);
  double* dout = h.out(out, (size_t)n_frames * kPitchCols);
  if (h.err) return h.err;
  p.n = n;
  // one launch covers at most 2^30 workgroups (three per frame)
  if (int e = for_frame_chunks(n_frames, (int64_t)1 << 28, [&](int64_t f0, int64_t count) -> int {
    PitchParams q = p;
    q.x = dx.from(f0);
    q.n_frames = count;
    q.out = dout + f0 * kPitchCols;
    HIPC(c, launch_pitch(q, c->stream));
    return 0;
  }))
    return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

void omega_phase_config_default(omega_phase_config* cfg) {
  if (!cfg) return;
  *cfg = omega_phase_config{};
  cfg->sample_rate = 48000;
  cfg->m = 2048;
}

// np.hanning(m) by numpy's own route (design.cpp np_window64), as omega_phase_configure uploads it
int omega_phase_hanning(int32_t m, double* out) try {
  if (!out || m < 2) return OMEGA_EINVAL;
  const std::vector<double> w = np_window64(OMEGA_WIN_HANN, m);
  std::memcpy(out, w.data(), w.size() * sizeof(double));
  return 0;
} catch (...) {
  return guard_fail(nullptr);
}

int omega_phase_band_ranges(int32_t sample_rate, int32_t m, const double* edges, int32_t* ranges) try {
  if (!edges || !ranges || sample_rate <= 0 || m < 2) return OMEGA_EINVAL;
  for (int i = 0; i <= kPhaseBands; ++i)
    if (!std::isfinite(edges[i])) return OMEGA_EINVAL;
  // np.fft.rfftfreq(m, 1 / fs) in its own arithmetic: val = 1.0 / (m * d), f_k = k * val. The table increases,
  // so the mask (freqs >= lo) & (freqs < hi) is one range.
  const double d = 1.0 / (double)sample_rate, val = 1.0 / ((double)m * d);
  const int nb = m / 2 + 1;
  for (int b = 0; b < kPhaseBands; ++b) {
    int lo = 0, n = 0;
    mask_range(nb, [&](int k) { return (double)k * val; }, [&](double f) { return f >= edges[b] && f < edges[b + 1]; },
               &lo, &n);
    ranges[2 * b] = lo;
    ranges[2 * b + 1] = lo + n;
  }
  return 0;
} catch (...) {
  return guard_fail(nullptr);
}

int omega_phase_configure(omega_ctx* c, const omega_phase_config* cfg, const double* edges) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (!edges) return fail(c, OMEGA_EINVAL, "phase: edges is NULL");
  if (cfg->sample_rate <= 0) return fail(c, OMEGA_EINVAL, "phase: need sample_rate > 0");
  const int m = cfg->m;
  if (m <= 0) return fail(c, OMEGA_EINVAL, "phase: frame length %d", m);
  if (!is_pow2_in(m, kPhaseMinFrame, kPhaseMaxFrame))
    return fail(c, OMEGA_EUNSUP, "phase: %d samples per frame (the powers of two %d..%d are built)", m, kPhaseMinFrame,
                kPhaseMaxFrame);
  int32_t ranges[2 * kPhaseBands];
  if (omega_phase_band_ranges(cfg->sample_rate, m, edges, ranges))
    return fail(c, OMEGA_EINVAL, "phase: the band edges must be finite");
  HIPC(c, hipSetDevice(c->device));
  PhaseParams p{};
  if (int e = get_twiddles64(c, m, m / 2 + 1, &p.tw)) return e;  // (the kernel reads q < m / 2)
  if (int e = get_window64(c, OMEGA_WIN_HANN, m, &p.hann)) return e;
  p.m = m;
  while ((1 << p.bits) < m) ++p.bits;
  for (int b = 0; b < kPhaseBands; ++b) p.first[b] = ranges[2 * b], p.last[b] = ranges[2 * b + 1];
  c->phase.p = p;
  c->phase.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_phase_correlation(omega_ctx* c, const void* left, const void* right, int32_t f64, int64_t frame_stride,
                            int64_t n_frames, double* out, double* points, int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!c->phase.set) return fail(c, OMEGA_EINVAL, "phase: omega_phase_configure has not been called");
  if (!left || !right || n_frames < 0 || frame_stride < 1) return fail(c, OMEGA_EINVAL, "phase: bad frame layout");
  if (n_frames == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  const int m = c->phase.p.m;
  HostCall h(c, mem);
  const Rows dl = h.rows(left, frame_stride, m, f64, n_frames);
  const Rows dr = h.rows(right, frame_stride, m, f64, n_frames);
  double* dout = h.out(out, (size_t)n_frames * kPhaseCols);
  double* dpts = h.out(points, (size_t)n_frames * kPhasePoints * 2);
  if (h.err) return h.err;
  // one launch covers at most 2^30 workgroups
  if (int e = for_frame_chunks(n_frames, (int64_t)1 << 30, [&](int64_t f0, int64_t count) -> int {
    PhaseParams q = c->phase.p;
    q.n_frames = count;
    q.left = dl.from(f0);
    q.right = dr.from(f0);
    q.out = dout + f0 * kPhaseCols;
    q.points = dpts ? dpts + f0 * kPhasePoints * 2 : nullptr;
    HIPC(c, launch_phase(q, c->stream));
    return 0;
  }))
    return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
