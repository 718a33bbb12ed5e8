// libomega.so host side: room acoustics -- the room modes of a batch of spectra and the decay fit of a batch
// of sample histories (room.hip).

#include "host.hpp"

extern "C" {

void omega_room_config_default(omega_room_config* cfg) {
  if (!cfg) return;
  *cfg = omega_room_config{};
  cfg->sample_rate = 48000.0;  // room_mode_config.py:13-25
  cfg->min_frequency = 30.0;
  cfg->max_frequency = 300.0;
  cfg->peak_threshold_multiplier = 2.0;
  cfg->minimum_prominence_std = 1.0;
  cfg->min_q_factor = 0.5;
  cfg->max_q_factor = 100.0;
  cfg->minimum_severity = 0.3;
}

int omega_room_bin_range(const double* freqs, int32_t n_bins, double min_f, double max_f, int32_t* range) try {
  if (!freqs || !range || n_bins < 1 || std::isnan(min_f) || std::isnan(max_f)) return OMEGA_EINVAL;
  for (int i = 1; i < n_bins; ++i)
    if (!(freqs[i] > freqs[i - 1])) return OMEGA_EINVAL;
  if (std::isnan(freqs[0])) return OMEGA_EINVAL;
  // room_modes.py:74-75 over an increasing table: one range
  int lo = 0, n = 0;
  mask_range(n_bins, [&](int i) { return freqs[i]; }, [&](double f) { return f >= min_f && f <= max_f; }, &lo, &n);
  range[0] = lo;
  range[1] = lo + n;
  return 0;
} catch (...) {
  return guard_fail(nullptr);
}

int omega_room_configure(omega_ctx* c, const omega_room_config* cfg, const double* freqs, int32_t n_bins,
                         const double* hints) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (!freqs || n_bins < 1) return fail(c, OMEGA_EINVAL, "room: need a frequency table of at least one bin");
  // room_mode_config.py:44-59 (NaN fails every test)
  if (!(cfg->sample_rate > 0.0) || !(cfg->min_frequency < cfg->max_frequency) ||
      !(cfg->peak_threshold_multiplier > 0.0) || !(cfg->minimum_prominence_std >= 0.0) ||
      !(cfg->min_q_factor < cfg->max_q_factor) || !(cfg->minimum_severity >= 0.0 && cfg->minimum_severity <= 1.0))
    return fail(c, OMEGA_EINVAL, "room: the configuration fails RoomModeConfig's validation");
  int32_t range[2];
  if (omega_room_bin_range(freqs, n_bins, cfg->min_frequency, cfg->max_frequency, range))
    return fail(c, OMEGA_EINVAL, "room: freqs must be strictly increasing");
  if (range[1] - range[0] > kRoomMaxBins)
    return fail(c, OMEGA_EUNSUP, "room: %d bins in [%g, %g] Hz (at most %d are built)", range[1] - range[0],
                cfg->min_frequency, cfg->max_frequency, kRoomMaxBins);
  HIPC(c, hipSetDevice(c->device));
  RoomState& r = c->room;
  if (int e = grow(c, &r.freqs, &r.freqs_cap, (int64_t)n_bins)) return e;
  // (an earlier call's kernels may still read the table)
  HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, hipMemcpy(r.freqs, freqs, (size_t)n_bins * sizeof(double), hipMemcpyHostToDevice));
  RoomModesParams p{};
  p.n_bins = n_bins;
  p.first = range[0];
  p.last = range[1];
  p.freqs = r.freqs;
  for (int i = 0; i < n_bins; ++i)
    if (!std::isfinite(freqs[i])) p.freqs_bad = 1;
  p.height_mult = cfg->peak_threshold_multiplier;
  p.prom_std = cfg->minimum_prominence_std;
  p.min_q = cfg->min_q_factor;
  p.max_q = cfg->max_q_factor;
  p.min_sev = cfg->minimum_severity;
  bool all = hints != nullptr;
  for (int i = 0; all && i < 6; ++i) all = hints[i] > 0.0 && std::isfinite(hints[i]);
  for (int i = 0; i < 6; ++i) p.hints[i] = all ? hints[i] : 0.0;
  r.p = p;
  r.fs = cfg->sample_rate;
  r.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_room_modes(omega_ctx* c, const void* spectra, int32_t f64, int64_t spec_stride, int64_t n_frames, double* out,
                     int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!c->room.set) return fail(c, OMEGA_EINVAL, "room: omega_room_configure has not been called");
  if (!spectra || n_frames < 0 || spec_stride < 1) return fail(c, OMEGA_EINVAL, "room: bad spectrum layout");
  if (n_frames == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  const int nb = c->room.p.n_bins;
  HostCall h(c, mem);
  const Rows ds = h.rows(spectra, spec_stride, nb, f64, n_frames);
  double* dout = h.out(out, (size_t)n_frames * kRoomRows * kRoomCols);
  if (h.err) return h.err;
  // one launch covers at most 2^30 workgroups
  if (int e = for_frame_chunks(n_frames, (int64_t)1 << 30, [&](int64_t f0, int64_t count) -> int {
    RoomModesParams q = c->room.p;
    q.n_frames = count;
    q.spec = ds.from(f0);
    q.out = dout + f0 * (kRoomRows * kRoomCols);
    HIPC(c, launch_room_modes(q, c->stream));
    return 0;
  }))
    return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_room_decay(omega_ctx* c, const void* audio, int32_t f64, int64_t stream_stride, int64_t L, int64_t W,
                    int64_t n_streams, double* out, double* energies, int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!c->room.set) return fail(c, OMEGA_EINVAL, "room: omega_room_configure has not been called");
  if (!audio || n_streams < 0 || stream_stride < 1 || L < 2 || W < 0 || (W > 0 && L % W != 0))
    return fail(c, OMEGA_EINVAL, "room: bad history layout (need L >= 2 and W dividing L)");
  if (L > kRt60MaxLen) return fail(c, OMEGA_EUNSUP, "room: %lld samples per history (at most %d)", (long long)L, kRt60MaxLen);
  if (n_streams == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  const int64_t nf = W > 0 ? L / W : 0;
  HostCall h(c, mem);
  const Rows da = h.rows(audio, stream_stride, L, f64, n_streams);
  double* dout = h.out(out, (size_t)n_streams * kRt60Cols);
  double* den = W > 0 ? h.out(energies, (size_t)(n_streams * nf)) : nullptr;
  if (h.err) return h.err;
  if (int e = for_frame_chunks(n_streams, (int64_t)1 << 30, [&](int64_t s0, int64_t count) -> int {
    RoomRt60Params q{};
    q.audio = da.from(s0);
    q.n_streams = count;
    q.L = (int)L;
    q.W = (int)W;
    q.fs = c->room.fs;
    q.out = dout + s0 * kRt60Cols;
    q.energies = den ? den + s0 * nf : nullptr;
    HIPC(c, launch_room_rt60(q, c->stream));
    return 0;
  }))
    return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
