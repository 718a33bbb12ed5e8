// libomega.so host side: beat detection and band tracking -- the flux, band, kick, centroid and spread sums of
// consecutive frames of a stream (rhythm.hip). The stream's state travels with the caller as a blob; the context
// keeps only the frequency table, the edges and the per-call workspace.

#include "host.hpp"

namespace {

constexpr int64_t kRhChunk = 65536;  // frames per launch pair (the workspace's entries)

bool rh_shape_ok(int K, int m) { return K >= kRhMinBins && K <= kRhMaxBins && m >= 1 && m <= kRhMaxFrame; }

}  // namespace

extern "C" {

void omega_rhythm_config_default(omega_rhythm_config* cfg) {
  if (!cfg) return;
  *cfg = omega_rhythm_config{};
  cfg->n_bins = 513;
  cfg->frame_len = 2048;
}

int64_t omega_rhythm_state_size(int32_t n_bins) { return n_bins < 1 ? 0 : rh_state_len(n_bins); }

int omega_rhythm_configure(omega_ctx* c, const omega_rhythm_config* cfg, const double* freqs, const int32_t* edges) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (!freqs || !edges) return fail(c, OMEGA_EINVAL, "rhythm: need a frequency table and the %d edges", kRhEdges);
  // (every size is refused before the configured shape is touched)
  if (!rh_shape_ok(cfg->n_bins, cfg->frame_len))
    return fail(c, OMEGA_EUNSUP, "rhythm: %d bins, %d samples per frame (%d..%d bins and 1..%d samples are built)",
                cfg->n_bins, cfg->frame_len, kRhMinBins, kRhMaxBins, kRhMaxFrame);
  const int K = cfg->n_bins;
  for (int i = 0; i < kRhEdges; ++i)
    if (edges[i] < 0 || edges[i] > K)
      return fail(c, OMEGA_EINVAL, "rhythm: edge %d is bin %d of %d", i, edges[i], K);
  HIPC(c, hipSetDevice(c->device));
  RhythmState& v = c->rhythm;
  const bool same = v.set && (int)v.freqs_host.size() == K && !std::memcmp(v.freqs_host.data(), freqs, (size_t)K * sizeof(double));
  if (!same) {
    std::vector<double> host(freqs, freqs + K);
    if (int e = grow(c, &v.freqs, &v.freqs_cap, (int64_t)K)) return e;
    // (an earlier call's kernels may still read the table)
    HIPC(c, hipStreamSynchronize(c->stream));
    v.set = false;  // (a failed upload leaves no half-written table configured)
    HIPC(c, hipMemcpy(v.freqs, freqs, (size_t)K * sizeof(double), hipMemcpyHostToDevice));
    v.freqs_host.swap(host);
  }
  RhythmParams p{};
  p.n_bins = K;
  p.m = cfg->frame_len;
  p.freqs = v.freqs;
  for (int i = 0; i < kRhEdges; ++i) p.edge[i] = edges[i];
  v.p = p;
  v.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_rhythm_features(omega_ctx* c, const float* spectra, int64_t spec_stride, const void* frames, int32_t f64,
                          int64_t n_frames, int64_t frame_stride, const double* state_in, double* state_out,
                          double* out, int mem) try {
  if (!c) return OMEGA_EINVAL;
  RhythmState& v = c->rhythm;
  if (!v.set) return fail(c, OMEGA_EINVAL, "rhythm: omega_rhythm_configure has not been called");
  const RhythmParams& cp = v.p;
  if (n_frames < 0 || (n_frames > 0 && (!out || !spectra || spec_stride < 1 || (frames && frame_stride < 1))))
    return fail(c, OMEGA_EINVAL, "rhythm: bad spectrum or audio layout");
  HIPC(c, hipSetDevice(c->device));
  const size_t slen = (size_t)rh_state_len(cp.n_bins);
  HostCall h(c, mem);
  const Rows32 dspec = n_frames ? h.rows32(spectra, spec_stride, cp.n_bins, n_frames) : Rows32{};
  const Rows daudio = n_frames && frames ? h.rows(frames, frame_stride, cp.m, f64, n_frames) : Rows{};
  const double* dsin = h.in(state_in, slen * sizeof(double));
  double* dout = n_frames ? h.out(out, (size_t)n_frames * kRhCols) : nullptr;
  double* dsout = h.out(state_out, slen);
  if (h.err) return h.err;
  if (n_frames == 0) {
    if (int e = pass_state_through(c, dsin, dsout, slen * sizeof(double))) return e;
    return h.finish();
  }
  const int64_t per = std::min(n_frames, kRhChunk);
  if (int e = grow(c, &v.ws, &v.ws_cap, per)) return e;
  if (int e = chained_frame_chunks(c, v.chain, (size_t)rh_state_len(kRhMaxBins), slen, n_frames, per, dsin, dsout,
                                   [&](int64_t f0, int64_t count, const double* sin, double* sout) -> int {
        RhythmParams q = cp;
        q.n_frames = count;
        q.spec = dspec.from(f0);
        q.audio = daudio.from(f0);
        q.ws = v.ws;
        q.state_in = sin;
        q.state_out = sout;
        q.out = dout + f0 * kRhCols;
        HIPC(c, launch_rhythm(q, c->stream));
        return 0;
      }))
    return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
