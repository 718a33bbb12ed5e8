// libomega.so host side: voice detection -- the voice-band energies, the formant peaks and the pitch
// autocorrelation of a batch of frames (voice.hip).

#include "host.hpp"

namespace {

bool voice_shape_ok(double fs, int m) {
  return std::isfinite(fs) && fs >= kVoiceMinRate && is_pow2_in(m, kVoiceMinFrame, kVoiceMaxFrame);
}

}  // namespace

extern "C" {

void omega_voice_config_default(omega_voice_config* cfg) {
  if (!cfg) return;
  *cfg = omega_voice_config{};
  cfg->sample_rate = 48000.0;
  cfg->n_bins = 1025;
  cfg->frame_len = 2048;
}

int omega_voice_bin_range(double sample_rate, int32_t frame_len, int32_t* range) try {
  if (!range || !(sample_rate > 0.0) || !std::isfinite(sample_rate) || frame_len < 1) return OMEGA_EINVAL;
  const double step = np_rfftfreq_step(frame_len, sample_rate);
  range[0] = searchsorted_left_uniform(step, frame_len / 2 + 1, 85.0);   // voice_detection.py:63-67
  range[1] = searchsorted_left_uniform(step, frame_len / 2 + 1, 255.0);
  return 0;
} catch (...) {
  return guard_fail(nullptr);
}

int omega_voice_configure(omega_ctx* c, const omega_voice_config* cfg) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (!(cfg->sample_rate > 0.0) || cfg->n_bins < 1 || cfg->frame_len < 1)
    return fail(c, OMEGA_EINVAL, "voice: need a positive sample rate, bin count and frame length");
  // (every size is refused before the configured table is touched)
  if (cfg->n_bins > kVoiceMaxBins)
    return fail(c, OMEGA_EUNSUP, "voice: %d spectrum bins (1..%d are built)", cfg->n_bins, kVoiceMaxBins);
  if (!voice_shape_ok(cfg->sample_rate, cfg->frame_len))
    return fail(c, OMEGA_EUNSUP, "voice: %d samples per frame at %g Hz (the powers of two %d..%d at %g Hz and above "
                "are built)", cfg->frame_len, cfg->sample_rate, kVoiceMinFrame, kVoiceMaxFrame, kVoiceMinRate);
  HIPC(c, hipSetDevice(c->device));
  VoiceState& v = c->voice;
  const int K = cfg->n_bins, m = cfg->frame_len;
  const int w = K > 10 ? std::min(11, K / 4 * 2 + 1) : 0;  // :95-97
  const double* sg = nullptr;
  if (w)
    if (int e = get_savgol(c, w, &sg)) return e;
  VoiceParams p{};
  p.n_bins = K;
  p.m = m;
  p.n_freq = m / 2 + 1;
  p.bin_hz = np_rfftfreq_step(m, cfg->sample_rate);
  p.voice_start = searchsorted_left_uniform(p.bin_hz, p.n_freq, 85.0);
  p.voice_end = searchsorted_left_uniform(p.bin_hz, p.n_freq, 255.0);
  p.sg_w = w;
  p.sg = sg;
  p.lag_lo = (int)std::min(cfg->sample_rate / 400.0, (double)m);  // :182-183 (Python's int() truncates)
  const double hi = cfg->sample_rate / 80.0;
  p.lag_hi = hi < (double)m ? (int)hi : m;
  p.pitch = m >= kVoicePitchFrame && p.lag_hi < m;  // :174, :185
  v.p = p;
  v.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_voice_features(omega_ctx* c, const float* spectra, int64_t spec_stride, const void* frames, int32_t f64,
                         int32_t m, int64_t frame_stride, int64_t n_frames, double* out, int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!c->voice.set) return fail(c, OMEGA_EINVAL, "voice: omega_voice_configure has not been called");
  const VoiceParams& cp = c->voice.p;
  if (!spectra || n_frames < 0 || spec_stride < 1) return fail(c, OMEGA_EINVAL, "voice: bad spectrum layout");
  if (m != cp.m) return fail(c, OMEGA_EINVAL, "voice: %d samples per frame, configured for %d", m, cp.m);
  // (a shape that gives no pitch never reads the audio)
  if (cp.pitch && (!frames || frame_stride < 1)) return fail(c, OMEGA_EINVAL, "voice: bad audio layout");
  if (n_frames == 0) return 0;
  HIPC(c, hipSetDevice(c->device));
  HostCall h(c, mem);
  const Rows32 dspec = h.rows32(spectra, spec_stride, cp.n_bins, n_frames);
  const Rows daudio = cp.pitch ? h.rows(frames, frame_stride, m, f64, n_frames) : Rows{};
  double* dout = h.out(out, (size_t)n_frames * kVoiceCols);
  if (h.err) return h.err;
  // one launch covers at most 2^30 workgroups (two per frame)
  if (int e = for_frame_chunks(n_frames, (int64_t)1 << 29, [&](int64_t f0, int64_t count) -> int {
    VoiceParams q = cp;
    q.n_frames = count;
    q.spec = dspec.from(f0);
    q.audio = daudio.from(f0);
    q.out = dout + f0 * kVoiceCols;
    HIPC(c, launch_voice(q, c->stream));
    return 0;
  }))
    return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
