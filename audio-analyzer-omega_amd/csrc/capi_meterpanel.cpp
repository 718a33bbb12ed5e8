// libomega.so host side: the professional meters panel -- what ProfessionalMetersPanel.update does with a frame and
// with calculate_lufs' values for it (meterpanel.hip). The panel's state travels with the caller as a blob; the
// context keeps only the configured shape, the uploaded edges and the frame kernel's per-call records.

#include "host.hpp"

namespace {

// 0, or the code a config is refused with (msg: why)
int mp_check(const omega_meterpanel_config* cfg, const char** msg) {
  const char* dummy;
  if (!msg) msg = &dummy;
  *msg = "meterpanel: no config";
  if (!cfg) return OMEGA_EINVAL;
  *msg = "meterpanel: need a positive, finite sample rate and a frame length";
  if (!(cfg->sample_rate > 0.0) || !std::isfinite(cfg->sample_rate) || cfg->frame_len < 0) return OMEGA_EINVAL;
  *msg = "meterpanel: level_len, peak_len and range_len are 1..4096 each";
  for (int32_t len : {cfg->level_len, cfg->peak_len, cfg->range_len})
    if (len < 1 || len > kMpMaxHist) return OMEGA_EINVAL;
  *msg = "meterpanel: n_bins is 1..62";
  if (cfg->n_bins < 1 || cfg->n_bins > kMpMaxBins) return OMEGA_EINVAL;
  *msg = "meterpanel: hist_lo < hist_hi, both finite, with strictly increasing edges between them";
  if (!std::isfinite(cfg->hist_lo) || !std::isfinite(cfg->hist_hi) || !(cfg->hist_lo < cfg->hist_hi)) return OMEGA_EINVAL;
  for (int k = 0; k < cfg->n_bins; ++k)
    if (!(np_linspace(k, cfg->n_bins + 1, cfg->hist_lo, cfg->hist_hi) <
          np_linspace(k + 1, cfg->n_bins + 1, cfg->hist_lo, cfg->hist_hi)))
      return OMEGA_EINVAL;
  *msg = "meterpanel: frames of 1..16384 samples are built";
  if (cfg->frame_len == 0 || cfg->frame_len > kMpMaxFrame) return OMEGA_EUNSUP;
  return 0;
}

int64_t mp_state_len(const omega_meterpanel_config* cfg) {
  return (int64_t)kMpHead + cfg->level_len + cfg->peak_len + cfg->range_len;
}

std::vector<double> mp_edges(int n_bins, double lo, double hi) {
  std::vector<double> e((size_t)n_bins + 1);
  for (int k = 0; k <= n_bins; ++k) e[k] = np_linspace(k, n_bins + 1, lo, hi);
  return e;
}

// a ring of the blob oldest first; false where the blob's fill and position are not a ring's
bool mp_unring(const double* ring, int len, double fill_v, double pos_v, double* out, int32_t* n) {
  if (!(fill_v >= 0 && fill_v <= len && pos_v >= 0 && pos_v < len)) return false;
  const int fill = (int)fill_v, pos = (int)pos_v;
  if (fill != fill_v || pos != pos_v || (fill < len && pos != fill)) return false;
  if (out)
    for (int i = 0; i < fill; ++i) out[i] = ring[fill < len ? i : (pos + i) % len];
  if (n) *n = fill;
  return true;
}

}  // namespace

extern "C" {

void omega_meterpanel_config_default(omega_meterpanel_config* cfg) {
  if (!cfg) return;
  *cfg = omega_meterpanel_config{};
  cfg->sample_rate = 48000.0;
  cfg->frame_len = 2048;
  cfg->level_len = 600;
  cfg->peak_len = 300;
  cfg->range_len = 300;
  cfg->n_bins = 60;
  cfg->hist_lo = -60.0;
  cfg->hist_hi = 0.0;
}

int64_t omega_meterpanel_state_size(const omega_meterpanel_config* cfg) {
  if (int e = mp_check(cfg, nullptr)) return e;
  return mp_state_len(cfg);
}

int omega_meterpanel_edges(const omega_meterpanel_config* cfg, double* out) try {
  if (int e = mp_check(cfg, nullptr)) return e;
  if (!out) return OMEGA_EINVAL;
  const std::vector<double> e = mp_edges(cfg->n_bins, cfg->hist_lo, cfg->hist_hi);
  std::copy(e.begin(), e.end(), out);
  return 0;
} catch (...) {
  return guard_fail(nullptr);
}

int omega_meterpanel_unpack(const omega_meterpanel_config* cfg, const double* state, double* level, int32_t* n_level,
                            double* peaks, int32_t* n_peaks, double* ranges, int32_t* n_ranges, double* hold,
                            double* transient) {
  if (int e = mp_check(cfg, nullptr)) return e;
  if (!state) return OMEGA_EINVAL;
  const double* ring = state + kMpHead;
  // (every ring is checked before anything is written)
  if (!mp_unring(ring, cfg->level_len, state[kMpLevelFill], state[kMpLevelPos], nullptr, nullptr) ||
      !mp_unring(ring + cfg->level_len, cfg->peak_len, state[kMpPeakFill], state[kMpPeakPos], nullptr, nullptr) ||
      !mp_unring(ring + cfg->level_len + cfg->peak_len, cfg->range_len, state[kMpRangeFill], state[kMpRangePos], nullptr,
                 nullptr))
    return OMEGA_EINVAL;
  mp_unring(ring, cfg->level_len, state[kMpLevelFill], state[kMpLevelPos], level, n_level);
  mp_unring(ring + cfg->level_len, cfg->peak_len, state[kMpPeakFill], state[kMpPeakPos], peaks, n_peaks);
  mp_unring(ring + cfg->level_len + cfg->peak_len, cfg->range_len, state[kMpRangeFill], state[kMpRangePos], ranges,
            n_ranges);
  if (hold) {
    hold[0] = state[kMpHold];
    hold[1] = state[kMpCounter];
  }
  if (transient) {
    transient[0] = state[kMpAttack];
    transient[1] = state[kMpPunch];
    transient[2] = state[kMpCount];
  }
  return 0;
}

int omega_meterpanel_configure(omega_ctx* c, const omega_meterpanel_config* cfg) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  // (every refusal comes before the configured shape is touched)
  const char* msg = nullptr;
  if (int e = mp_check(cfg, &msg)) return fail(c, e, "%s (%d samples per frame at %g Hz)", msg, cfg->frame_len, cfg->sample_rate);
  HIPC(c, hipSetDevice(c->device));
  MeterPanelState& v = c->meterpanel;
  // the edges' place in the table cache: (kind 4, n_bins, the index of this [lo, hi] among those seen); kinds 0..3 are
  // the twiddles, the windows, the Savitzky-Golay weights and the tonal tables
  const std::pair<double, double> range(cfg->hist_lo, cfg->hist_hi);
  size_t ri = std::find(v.ranges.begin(), v.ranges.end(), range) - v.ranges.begin();
  if (ri == v.ranges.size()) v.ranges.push_back(range);
  const double* edges = nullptr;
  if (int e = host_table(c, 4, cfg->n_bins, (int)ri, &edges, [&] { return mp_edges(cfg->n_bins, range.first, range.second); }))
    return e;
  MeterPanelParams p{};
  p.frame_len = cfg->frame_len;
  p.sample_rate = cfg->sample_rate;
  p.level_len = cfg->level_len;
  p.peak_len = cfg->peak_len;
  p.range_len = cfg->range_len;
  p.n_bins = cfg->n_bins;
  p.edges = edges;
  v.p = p;
  v.state_len = mp_state_len(cfg);
  v.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_meterpanel_update(omega_ctx* c, const void* frames, int64_t frame_stride, int32_t f64, const double* meters,
                            int64_t n_frames, int64_t peak_hold_samples, int32_t reset_hold, const double* state_in,
                            double* rows, int32_t* hist, double* state_out, int mem) try {
  if (!c) return OMEGA_EINVAL;
  MeterPanelState& v = c->meterpanel;
  if (!v.set) return fail(c, OMEGA_EINVAL, "meterpanel: omega_meterpanel_configure has not been called");
  if (n_frames < 0 || n_frames > INT32_MAX || (n_frames > 0 && (!frames || !meters || !rows || frame_stride < 1)))
    return fail(c, OMEGA_EINVAL, "meterpanel: bad frame layout, or the frames, the meters or the rows missing");
  if (n_frames == 0 && !state_out) return 0;
  HIPC(c, hipSetDevice(c->device));
  if (int e = grow(c, &v.ws, &v.ws_cap, n_frames * kMpWsCols)) return e;
  const size_t slen = (size_t)v.state_len, nf = (size_t)n_frames;
  HostCall h(c, mem);
  MeterPanelParams p = v.p;
  p.frames = n_frames ? h.rows(frames, frame_stride, p.frame_len, f64, n_frames) : Rows{};
  p.meters = n_frames ? h.in(meters, nf * 5 * sizeof(double)) : nullptr;
  p.state_in = h.in(state_in, slen * sizeof(double));
  p.rows = n_frames ? h.out(rows, nf * kMpRowCols) : nullptr;
  p.hist = n_frames ? h.out(hist, nf * (size_t)p.n_bins) : nullptr;
  p.state_out = h.out(state_out, slen);
  if (h.err) return h.err;
  p.n_frames = n_frames;
  p.hold_samples = peak_hold_samples;
  p.reset_hold = reset_hold != 0;
  p.ws = v.ws;
  // the same launches whatever n_frames is: the track kernel walks the call's frames itself, reads each state entry
  // before it writes it (one buffer may serve as both blobs) and writes a new panel's blob where state_in is null,
  // with no frames too
  HIPC(c, launch_meterpanel_frames(p, kMpWaveMax, c->stream));
  HIPC(c, launch_meterpanel_track(p, kMpTrackWalk, c->stream));
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
