// libomega.so host side: the bass zoom panel -- the 20..200 Hz bars of consecutive frames of a stream with their
// smoothing and peak hold (basszoom.hip). The panel's state travels with the caller as a blob; the context keeps
// only tables.

#include "host.hpp"

namespace {

struct BzMapping {
  int n_bars = 0, first_bin = 0, bins_per_bar = 0, n_valid = 0;
  double ranges[2 * kBzMaxBars] = {};
  double comp[kBzMaxBars] = {};
};

// setup_bass_mapping (bass_zoom.py:51-97). 0, or OMEGA_EUNSUP where there is no valid bin or a cap is passed
int bz_mapping(double fs, BzMapping* m) {
  int lo = 0, n = 0;
  mask_range(kBzFft / 2 + 1, [&](int k) { return rfreq(k, kBzFft, fs); },
             [](double f) { return 20 <= f && f <= 200; }, &lo, &n);
  if (n == 0 || n > kBzMaxBins) return OMEGA_EUNSUP;
  const int per = std::max(1, n / 31);
  const int bars = (n + per - 1) / per;
  if (bars > kBzMaxBars) return OMEGA_EUNSUP;
  m->n_bars = bars;
  m->first_bin = lo;
  m->bins_per_bar = per;
  m->n_valid = n;
  for (int i = 0; i < bars; ++i) {
    const int b0 = lo + i * per, b1 = lo + std::min((i + 1) * per, n) - 1;
    double f0 = rfreq(b0, kBzFft, fs);
    const double f1 = rfreq(b1, kBzFft, fs);
    if (i > 0) f0 = std::max(f0, m->ranges[2 * i - 1]);  // :85-86
    m->ranges[2 * i] = f0;
    m->ranges[2 * i + 1] = f1;
    const double centre = (f0 + f1) / 2;
    m->comp[i] = centre < 60 ? 0.3 : (centre < 100 ? 0.6 : (centre < 150 ? 1.0 : 0.8));  // :178-185
  }
  return 0;
}

bool bz_rate_ok(double fs) { return fs > 0.0 && std::isfinite(fs); }

}  // namespace

extern "C" {

void omega_basszoom_config_default(omega_basszoom_config* cfg) {
  if (!cfg) return;
  *cfg = omega_basszoom_config{};
  cfg->sample_rate = 48000.0;
  cfg->frame_len = kBzFft;
}

int64_t omega_basszoom_state_size(void) { return kBzStateLen; }

int omega_basszoom_mapping(double sample_rate, int32_t* n_bars, int32_t* first_bin, int32_t* bins_per_bar,
                           int32_t* n_valid, double* freq_ranges, double* compensation) try {
  if (!bz_rate_ok(sample_rate)) return OMEGA_EINVAL;
  BzMapping m;
  if (int e = bz_mapping(sample_rate, &m)) return e;
  if (n_bars) *n_bars = m.n_bars;
  if (first_bin) *first_bin = m.first_bin;
  if (bins_per_bar) *bins_per_bar = m.bins_per_bar;
  if (n_valid) *n_valid = m.n_valid;
  for (int i = 0; i < m.n_bars; ++i) {
    if (freq_ranges) {
      freq_ranges[2 * i] = m.ranges[2 * i];
      freq_ranges[2 * i + 1] = m.ranges[2 * i + 1];
    }
    if (compensation) compensation[i] = m.comp[i];
  }
  return 0;
} catch (...) {
  return guard_fail(nullptr);
}

int omega_basszoom_configure(omega_ctx* c, const omega_basszoom_config* cfg) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (!bz_rate_ok(cfg->sample_rate) || cfg->frame_len < 0)
    return fail(c, OMEGA_EINVAL, "basszoom: need a positive, finite sample rate and a frame length");
  // (every size is refused before the configured shape is touched)
  BzMapping m;
  if (cfg->frame_len == 0 || bz_mapping(cfg->sample_rate, &m))
    return fail(c, OMEGA_EUNSUP, "basszoom: %d samples per frame at %g Hz (frames of 1 sample and more are built, at "
                "rates with 1..%d bins of the %d-point transform in 20..200 Hz)", cfg->frame_len, cfg->sample_rate,
                kBzMaxBins, kBzFft);
  HIPC(c, hipSetDevice(c->device));
  BassZoomState& v = c->basszoom;
  const int nw = std::min(cfg->frame_len, kBzFft);
  BassZoomParams p{};
  if (int e = get_twiddles64(c, kBzFft, kBzFft, &p.tw)) return e;
  if (int e = get_window64(c, OMEGA_WIN_HANN, nw, &p.win)) return e;  // (np.hanning(1) is [1.])
  p.nw = nw;
  p.first_bin = m.first_bin;
  p.n_valid = m.n_valid;
  p.bins_per_bar = m.bins_per_bar;
  p.n_bars = m.n_bars;
  for (int i = 0; i < m.n_bars; ++i) p.comp[i] = m.comp[i];
  v.p = p;
  v.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_basszoom_features(omega_ctx* c, const void* frames, int64_t frame_stride, int32_t f64, const double* times,
                            int64_t n_frames, const double* state_in, double* rows, double* bars, double* peaks,
                            double* peak_times, double* state_out, int mem) try {
  if (!c) return OMEGA_EINVAL;
  BassZoomState& v = c->basszoom;
  if (!v.set) return fail(c, OMEGA_EINVAL, "basszoom: omega_basszoom_configure has not been called");
  const BassZoomParams& cp = v.p;
  if (n_frames < 0 || n_frames > INT32_MAX ||
      (n_frames > 0 && (!frames || !times || !rows || !bars || !peaks || !peak_times || frame_stride < 1)))
    return fail(c, OMEGA_EINVAL, "basszoom: bad frame layout, or an output or the times missing");
  HIPC(c, hipSetDevice(c->device));
  const size_t sbytes = (size_t)kBzStateLen * sizeof(double), nb = (size_t)cp.n_bars;
  HostCall h(c, mem);
  BassZoomParams p = cp;
  p.frames = n_frames ? h.rows(frames, frame_stride, cp.nw, f64, n_frames) : Rows{};
  p.times = n_frames ? h.in(times, (size_t)n_frames * sizeof(double)) : nullptr;
  p.state_in = h.in(state_in, sbytes);
  p.rows = n_frames ? h.out(rows, (size_t)n_frames * (kBzRowHead + nb)) : nullptr;
  p.bars = n_frames ? h.out(bars, (size_t)n_frames * nb) : nullptr;
  p.peaks = n_frames ? h.out(peaks, (size_t)n_frames * nb) : nullptr;
  p.peak_times = n_frames ? h.out(peak_times, (size_t)n_frames * nb) : nullptr;
  p.state_out = h.out(state_out, (size_t)kBzStateLen);
  if (h.err) return h.err;
  p.n_frames = n_frames;
  // the bars past n_bars: zero in a new panel's blob, else carried (the track kernel writes the first n_bars of
  // each third; it reads its own entries before it writes them, so one buffer may serve as both blobs)
  if (int e = pass_state_through(c, p.state_in, p.state_out, sbytes)) return e;
  if (n_frames > 0) {
    HIPC(c, launch_basszoom_frames(p, c->stream));
    HIPC(c, launch_basszoom_track(p, c->stream));
  }
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
