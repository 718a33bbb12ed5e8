// libomega.so host side: transient detection -- the envelope, level, flux, novelty, high-frequency, attack /
// decay and classification features of consecutive frames of a stream (tdetect.hip). The stream's state travels
// with the caller as a blob; the context keeps only tables and the per-call workspace.

#include "host.hpp"

namespace {

constexpr int64_t kTdChunk = 65536;  // frames per launch pair (the workspace's rows)

// np.fft.rfftfreq(2 (K - 1), 1 / fs) as numpy evaluates it: val = 1.0 / (n * d), results = arange * val
double td_bin_hz(double fs, int K) {
  const double d = 1.0 / fs;
  return 1.0 / ((double)(2 * (K - 1)) * d);
}

// np.searchsorted(freqs, [0, 100, 250, 2000, fs / 2]) (side 'left') over the K bins
void td_band_indices(double fs, int K, int* idx) {
  const double step = td_bin_hz(fs, K);
  const double lim[5] = {0.0, 100.0, 250.0, 2000.0, fs / 2};
  for (int b = 0; b < 5; ++b) {
    int k = 0;
    while (k < K && (double)k * step < lim[b]) ++k;
    idx[b] = k;
  }
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
  p.bin_hz = td_bin_hz(fs, K);
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
  const size_t el = f64 ? 8 : 4, sbytes = (size_t)kTdStateLen * sizeof(double);
  HostCall h(c, mem);
  const float* dspec = n_frames ? h.in(spectra, (size_t)((n_frames - 1) * spec_stride + cp.n_bins) * sizeof(float)) : nullptr;
  const void* daudio = n_frames ? h.in(frames, (size_t)((n_frames - 1) * frame_stride + cp.m) * el) : nullptr;
  const double* dsin = h.in(state_in, sbytes);
  double* dout = n_frames ? h.out(out, (size_t)n_frames * kTdCols) : nullptr;
  double* dsout = h.out(state_out, (size_t)kTdStateLen);
  if (h.err) return h.err;
  if (n_frames == 0) {  // the state passes through
    if (dsout && dsout != dsin) {
      if (dsin)
        HIPC(c, hipMemcpyAsync(dsout, dsin, sbytes, hipMemcpyDefault, c->stream));
      else
        HIPC(c, hipMemsetAsync(dsout, 0, sbytes, c->stream));
    }
    return h.finish();
  }
  const int64_t per = std::min(n_frames, kTdChunk);
  if (int e = grow(c, &v.ws, &v.ws_cap, per * kTdWsStride)) return e;
  for (double*& b : v.chain)
    if (!b)
      if (int e = dalloc(c, &b, (size_t)kTdStateLen)) return e;
  // a call's launches chain through the context's two blobs; the last writes the caller's (through a blob
  // where the caller's in and out are one buffer: the cross kernel reads the one while it writes the other)
  const double* sin = dsin;
  int k = 0;
  if (int e = for_frame_chunks(n_frames, per, [&](int64_t f0, int64_t count) -> int {
        const bool last = f0 + count == n_frames;
        double* sout = last && dsout != dsin ? dsout : (last && !dsout ? nullptr : v.chain[k]);
        TdetectParams q = cp;
        q.f64 = f64 ? 1 : 0;
        q.spec_stride = spec_stride;
        q.audio_stride = frame_stride;
        q.n_frames = count;
        q.spec = dspec + f0 * spec_stride;
        q.audio = static_cast<const char*>(daudio) + (size_t)(f0 * frame_stride) * el;
        q.ws = v.ws;
        q.state_in = sin;
        q.state_out = sout;
        q.out = dout + f0 * kTdCols;
        HIPC(c, launch_tdetect(q, c->stream));
        if (last && dsout && sout != dsout) HIPC(c, hipMemcpyAsync(dsout, sout, sbytes, hipMemcpyDeviceToDevice, c->stream));
        sin = sout;
        k ^= 1;
        return 0;
      }))
    return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
