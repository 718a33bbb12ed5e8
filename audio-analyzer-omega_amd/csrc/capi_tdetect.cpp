// libomega.so host side: transient detection -- the envelope, level, flux, novelty, high-frequency, attack /
// decay and classification features of consecutive frames of a stream (tdetect.hip). The stream's state travels
// with the caller as a blob; the context keeps only tables and the per-call workspace.

#include "host.hpp"

namespace {

constexpr int64_t kTdChunk = 65536;  // frames per launch pair (the workspace's rows)

// np.searchsorted(freqs, [0, 100, 250, 2000, fs / 2]) over the K bins of np.fft.rfftfreq(2 (K - 1), 1 / fs)
void td_band_indices(double fs, int K, int* idx) {
  const double step = np_rfftfreq_step(2 * (K - 1), fs);
  const double lim[5] = {0.0, 100.0, 250.0, 2000.0, fs / 2};
  for (int b = 0; b < 5; ++b) idx[b] = searchsorted_left_uniform(step, K, lim[b]);
}

bool td_shape_ok(double fs, int K, int m) {
  return std::isfinite(fs) && fs >= kTdMinRate && K >= 2 && K <= kTdMaxBins && is_pow2_in(m, kTdMinFrame, kTdMaxFrame);
}

}  // namespace

extern "C" {

void omega_tdetect_config_default(omega_tdetect_config* cfg) {
  if (!cfg) return;
  *cfg = omega_tdetect_config{};
  cfg->sample_rate = 48000.0;
  cfg->n_bins = 513;
  cfg->frame_len = 2048;
}

int64_t omega_tdetect_state_size(void) { return kTdStateLen; }

int omega_tdetect_band_indices(double sample_rate, int32_t n_bins, int32_t* idx) try {
  if (!idx || !(sample_rate > 0.0) || !std::isfinite(sample_rate) || n_bins < 2) return OMEGA_EINVAL;
  int v[5];
  td_band_indices(sample_rate, n_bins, v);
  for (int b = 0; b < 5; ++b) idx[b] = v[b];
  return 0;
} catch (...) {
  return guard_fail(nullptr);
}

int omega_tdetect_configure(omega_ctx* c, const omega_tdetect_config* cfg) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (!(cfg->sample_rate > 0.0) || cfg->n_bins < 1 || cfg->frame_len < 1)
    return fail(c, OMEGA_EINVAL, "tdetect: need a positive sample rate, bin count and frame length");
  // (every size is refused before the configured shape is touched)
  if (!td_shape_ok(cfg->sample_rate, cfg->n_bins, cfg->frame_len))
    return fail(c, OMEGA_EUNSUP, "tdetect: %d bins, %d samples per frame at %g Hz (2..%d bins and the powers of two "
                "%d..%d at %g Hz and above are built)", cfg->n_bins, cfg->frame_len, cfg->sample_rate, kTdMaxBins,
                kTdMinFrame, kTdMaxFrame, kTdMinRate);
  HIPC(c, hipSetDevice(c->device));
  TdetectState& v = c->tdetect;
  const double fs = cfg->sample_rate;
  const int K = cfg->n_bins, m = cfg->frame_len;
  TdetectParams p{};
  if (int e = get_savgol(c, 11, &p.sg)) return e;
  if (int e = get_window64(c, OMEGA_WIN_HANN, kTdFluxLen, &p.han_f)) return e;
  if (int e = get_window64(c, OMEGA_WIN_HANN, kTdNovLen, &p.han_n)) return e;
  if (int e = tr_pow2_tables(c, m, &p.tw_m, &p.tw2_m)) return e;
  if (int e = tr_pow2_tables(c, kTdFluxLen, &p.tw_f, &p.tw2_f)) return e;
  if (int e = tr_pow2_tables(c, kTdNovLen, &p.tw_n, &p.tw2_n)) return e;
  p.n_bins = K;
  p.m = m;
  p.hf = m > 256 && 5000.0 / (fs / 2) < 1.0;  // :191, :196
  p.nov = m >= kTdNovLen;                     // :324
  p.bin_hz = np_rfftfreq_step(2 * (K - 1), fs);
  td_band_indices(fs, K, p.band_idx);
  if (p.hf) {
    butter4_highpass_ba(5000.0, fs, p.b, p.a);
    lfilter_zi4(p.b, p.a, p.zi);
    TdScan* scan = nullptr;
    if (int e = cached(v.scans, std::make_pair(fs, m), &scan, [&](TdScan** d) -> int {
          std::vector<TdScan> t(1);
          lfilter4_scan(p.a, (m + 2 * kTdPad + kTdThreads - 1) / kTdThreads, t.data());
          return upload(c, d, t);
        }))
      return e;
    p.scan = scan;
  }
  // the heavier roles first in the grid
  p.n_roles = 0;
  if (p.hf) p.roles[p.n_roles++] = kTdHf;
  p.roles[p.n_roles++] = kTdEnvelope;
  if (p.nov) p.roles[p.n_roles++] = kTdNovelty;
  p.roles[p.n_roles++] = kTdFlux;
  p.roles[p.n_roles++] = kTdScalar;
  v.p = p;
  v.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_tdetect_features(omega_ctx* c, const float* spectra, int64_t spec_stride, const void* frames, int32_t f64,
                           int64_t n_frames, int64_t frame_stride, const double* state_in, double* state_out,
                           double* out, int mem) try {
  if (!c) return OMEGA_EINVAL;
  TdetectState& v = c->tdetect;
  if (!v.set) return fail(c, OMEGA_EINVAL, "tdetect: omega_tdetect_configure has not been called");
  const TdetectParams& cp = v.p;
  if (n_frames < 0 || (n_frames > 0 && (!out || !spectra || !frames || spec_stride < 1 || frame_stride < 1)))
    return fail(c, OMEGA_EINVAL, "tdetect: bad spectrum or audio layout");
  HIPC(c, hipSetDevice(c->device));
  const size_t slen = (size_t)kTdStateLen;
  HostCall h(c, mem);
  const Rows32 dspec = n_frames ? h.rows32(spectra, spec_stride, cp.n_bins, n_frames) : Rows32{};
  const Rows daudio = n_frames ? h.rows(frames, frame_stride, cp.m, f64, n_frames) : Rows{};
  const double* dsin = h.in(state_in, slen * sizeof(double));
  double* dout = n_frames ? h.out(out, (size_t)n_frames * kTdCols) : nullptr;
  double* dsout = h.out(state_out, slen);
  if (h.err) return h.err;
  if (n_frames == 0) {
    if (int e = pass_state_through(c, dsin, dsout, slen * sizeof(double))) return e;
    return h.finish();
  }
  const int64_t per = std::min(n_frames, kTdChunk);
  if (int e = grow(c, &v.ws, &v.ws_cap, per * kTdWsStride)) return e;
  if (int e = chained_frame_chunks(c, v.chain, slen, slen, n_frames, per, dsin, dsout,
                                   [&](int64_t f0, int64_t count, const double* sin, double* sout) -> int {
        TdetectParams q = cp;
        q.n_frames = count;
        q.spec = dspec.from(f0);
        q.audio = daudio.from(f0);
        q.ws = v.ws;
        q.state_in = sin;
        q.state_out = sout;
        q.out = dout + f0 * kTdCols;
        HIPC(c, launch_tdetect(q, c->stream));
        return 0;
      }))
    return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
