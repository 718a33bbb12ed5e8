// libomega.so host side: the spectrogram waterfall -- the dB rows of consecutive frames of a stream with their
// auto-range, normalisation and colours, and the colour map alone (waterfall.hip). The panel's state travels with
// the caller as a blob; the context keeps only the configured shape.

#include "host.hpp"

namespace {

constexpr int64_t kWfChunk = 65536;  // frames per launch pair

bool wf_shape_ok(const omega_waterfall_config& g) {
  return g.n_bins >= 1 && g.n_bins <= kWfMaxBins && g.n_cells >= 1 && g.first_bin >= 0 &&
         (int64_t)g.first_bin + g.n_cells <= g.n_bins;
}

}  // namespace

extern "C" {

void omega_waterfall_config_default(omega_waterfall_config* cfg) {
  if (!cfg) return;
  *cfg = omega_waterfall_config{};
  cfg->n_bins = 1025;
  cfg->first_bin = 1;
  cfg->n_cells = 853;
}

int64_t omega_waterfall_state_size(void) { return kWfStateLen; }

int omega_waterfall_mapping(double sample_rate, int32_t fft_size, double min_freq, double max_freq, int32_t* first_bin,
                            int32_t* end_bin) try {
  if (!(sample_rate > 0.0) || !std::isfinite(sample_rate) || fft_size < 2 || std::isnan(min_freq) || std::isnan(max_freq))
    return OMEGA_EINVAL;
  // _setup_frequency_mapping (spectrogram_waterfall.py:56-69)
  const int n = fft_size / 2 + 1;
  const double nyquist = sample_rate / 2;
  const int lo = linspace0_argmax_ge(n, nyquist, min_freq);
  int hi = linspace0_argmax_ge(n, nyquist, max_freq);
  if (hi == 0) hi = n - 1;
  if (first_bin) *first_bin = lo;
  if (end_bin) *end_bin = hi;
  return 0;
} catch (...) {
  return guard_fail(nullptr);
}

int omega_waterfall_configure(omega_ctx* c, const omega_waterfall_config* cfg) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  // (every shape is refused before the configured one is touched)
  if (!wf_shape_ok(*cfg))
    return fail(c, OMEGA_EUNSUP, "waterfall: %d bins, cells [%d, %d + %d) (1..%d bins and a slice of 1 cell and more "
                "inside them are built)", cfg->n_bins, cfg->first_bin, cfg->first_bin, cfg->n_cells, kWfMaxBins);
  WaterfallState& v = c->waterfall;
  v.n_bins = cfg->n_bins;
  v.first_bin = cfg->first_bin;
  v.n_cells = cfg->n_cells;
  v.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_waterfall_rows(omega_ctx* c, const void* spectra, int64_t spec_stride, int32_t f64, int64_t n_frames,
                         int32_t auto_gain, double gain_db, int32_t scheme, const double* state_in, double* state_out,
                         double* stats, void* rows, uint8_t* rgb, int mem) try {
  if (!c) return OMEGA_EINVAL;
  WaterfallState& v = c->waterfall;
  if (!v.set) return fail(c, OMEGA_EINVAL, "waterfall: omega_waterfall_configure has not been called");
  if (n_frames < 0 || !std::isfinite(gain_db) || (n_frames > 0 && (!spectra || !stats || !rows || spec_stride < 1)))
    return fail(c, OMEGA_EINVAL, "waterfall: bad spectrum layout or gain, or an output missing");
  HIPC(c, hipSetDevice(c->device));
  f64 = f64 ? 1 : 0;
  // a stream has one precision: the blob's head (valid, dtype tag) is read before anything is staged or written
  if (state_in) {
    double head[2] = {0.0, 0.0};
    if (mem == OMEGA_MEM_HOST) {
      std::memcpy(head, state_in, sizeof head);
    } else {
      HIPC(c, hipMemcpyAsync(head, state_in, sizeof head, hipMemcpyDeviceToHost, c->stream));
      HIPC(c, hipStreamSynchronize(c->stream));
    }
    if (head[0] != 0.0 && head[1] != (double)f64)
      return fail(c, OMEGA_EUNSUP, "waterfall: the state was recorded on float%d spectra, this call brings float%d "
                  "(a stream has one precision; start a new panel with state_in NULL)", head[1] != 0.0 ? 64 : 32,
                  f64 ? 64 : 32);
  }
  const size_t K = (size_t)v.n_cells, el = f64 ? 8 : 4, sbytes = (size_t)kWfStateLen * sizeof(double);
  HostCall h(c, mem);
  const Rows dspec = n_frames ? h.rows(spectra, spec_stride, v.n_bins, f64, n_frames) : Rows{};
  const double* dsin = h.in(state_in, sbytes);
  double* dstats = n_frames ? h.out(stats, (size_t)n_frames * kWfCols) : nullptr;
  char* drows = n_frames ? h.out(static_cast<char*>(rows), (size_t)n_frames * K * el) : nullptr;
  uint8_t* drgb = n_frames ? h.out(rgb, (size_t)n_frames * K * 3) : nullptr;
  double* dsout = h.out(state_out, (size_t)kWfStateLen);
  if (h.err) return h.err;
  if (n_frames == 0) {
    if (int e = pass_state_through(c, dsin, dsout, sbytes)) return e;
    return h.finish();
  }
  if (int e = chained_frame_chunks(c, v.chain, (size_t)kWfStateLen, (size_t)kWfStateLen, n_frames, kWfChunk, dsin, dsout,
                                   [&](int64_t f0, int64_t count, const double* sin, double* sout) -> int {
        WaterfallParams q{};
        q.spec = dspec.from(f0);
        q.n_frames = count;
        q.n_bins = v.n_bins;
        q.first_bin = v.first_bin;
        q.n_cells = v.n_cells;
        q.auto_gain = auto_gain ? 1 : 0;
        q.gain_db = gain_db;
        q.scheme = scheme;
        q.state_in = sin;
        q.state_out = sout;
        q.stats = dstats + f0 * kWfCols;
        q.rows = drows + (size_t)f0 * K * el;
        q.rgb = drgb ? drgb + (size_t)f0 * K * 3 : nullptr;
        HIPC(c, launch_waterfall(q, c->stream));
        return 0;
      }))
    return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_waterfall_colors(omega_ctx* c, const void* intensity, int64_t row_stride, int32_t f64, int64_t n_rows,
                           int32_t n_cells, int32_t scheme, uint8_t* rgb, int mem) try {
  if (!c) return OMEGA_EINVAL;
  if (n_rows < 0 || n_rows > INT32_MAX || n_cells < 0 || (n_rows > 0 && n_cells > 0 && (!intensity || !rgb || row_stride < 1)))
    return fail(c, OMEGA_EINVAL, "waterfall: bad intensity layout, or the output missing");
  if (n_rows == 0 || n_cells == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  HostCall h(c, mem);
  WaterfallColorParams p{};
  p.in = h.rows(intensity, row_stride, n_cells, f64, n_rows);
  p.rgb = h.out(rgb, (size_t)n_rows * (size_t)n_cells * 3);
  if (h.err) return h.err;
  p.n_rows = n_rows;
  p.n_cells = n_cells;
  p.scheme = scheme;
  HIPC(c, launch_waterfall_colors(p, c->stream));
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
