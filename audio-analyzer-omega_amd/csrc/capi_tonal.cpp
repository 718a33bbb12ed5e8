// libomega.so host side: key, alternative-key, chord and mode scores of consecutive chroma rows of a stream
// (tonal.hip), from the raw rows or, fused behind omega_chroma's kernel, from the spectra. The stream's state
// travels with the caller as a blob; the context keeps only the configured genre.

#include "host.hpp"

namespace {

constexpr int64_t kTnChunk = 65536;  // frames per launch

// every roll must lie in -11..11: checked on the host before anything is staged or launched (a host array needs no
// device; a device array is read back, which waits for the context's stream)
int check_rolls(omega_ctx* c, const int32_t* roll, int64_t n_frames, int mem) {
  if (!roll || n_frames <= 0) return 0;
  std::vector<int32_t> back;
  const int32_t* r = roll;
  if (mem != OMEGA_MEM_HOST) {
    HIPC(c, hipSetDevice(c->device));
    back.resize((size_t)n_frames);
    HIPC(c, hipMemcpyAsync(back.data(), roll, back.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    r = back.data();
  }
  for (int64_t f = 0; f < n_frames; ++f)
    if (r[f] < -11 || r[f] > 11)
      return fail(c, OMEGA_EINVAL, "tonal: roll[%lld] = %d (-11..11 semitones)", (long long)f, (int)r[f]);
  return 0;
}

struct TonalOut {
  double *rows, *key_corr, *alt_corr, *chord, *mode;
};

// the launches over raw rows already on the device
int run_tonal(omega_ctx* c, const double* draw, int64_t n_frames, const int32_t* droll, const int32_t* dfirst,
              const double* dsin, double* dsout, const TonalOut& o) {
  TonalState& v = c->tonal;
  const double* tab = nullptr;
  if (int e = host_table(c, 3, v.genre, 0, &tab, [&] { return tonal_table(v.genre); })) return e;
  return chained_frame_chunks(c, v.chain, (size_t)kTnStateLen, (size_t)kTnStateLen, n_frames, kTnChunk, dsin, dsout,
                              [&](int64_t f0, int64_t count, const double* sin, double* sout) -> int {
    TonalParams q{};
    q.raw = draw + f0 * 12;
    q.n_frames = count;
    q.roll = droll ? droll + f0 : nullptr;
    q.first = dfirst ? dfirst + f0 : nullptr;
    q.genre = v.genre;
    q.blend = tonal_blend(v.genre);
    q.tolerance = tonal_tolerance(v.genre);
    q.tab = tab;
    q.state_in = sin;
    q.state_out = sout;
    q.rows = o.rows + f0 * kTnCols;
    q.key_corr = o.key_corr ? o.key_corr + f0 * kTnKeys : nullptr;
    q.alt_corr = o.alt_corr ? o.alt_corr + f0 * kTnKeys : nullptr;
    q.chord = o.chord ? o.chord + f0 * 2 * kTnCells : nullptr;
    q.mode = o.mode ? o.mode + f0 * 12 * kTnModes : nullptr;
    HIPC(c, launch_tonal(q, c->stream));
    return 0;
  });
}

// what both entry points stage after their input, in one order
struct TonalCall {
  const int32_t *roll, *first;
  const double* sin;
  double* sout;
  TonalOut o;
};
TonalCall stage_tonal(HostCall& h, int64_t n, const int32_t* roll, const int32_t* first, const double* state_in,
                      double* state_out, double* rows, double* key_corr, double* alt_corr, double* chord, double* mode) {
  TonalCall t{};
  t.roll = h.in(roll, (size_t)n * sizeof(int32_t));
  t.first = h.in(first, (size_t)n * sizeof(int32_t));
  t.sin = h.in(state_in, (size_t)kTnStateLen * sizeof(double));
  t.o.rows = n ? h.out(rows, (size_t)n * kTnCols) : nullptr;
  t.o.key_corr = n ? h.out(key_corr, (size_t)n * kTnKeys) : nullptr;
  t.o.alt_corr = n ? h.out(alt_corr, (size_t)n * kTnKeys) : nullptr;
  t.o.chord = n ? h.out(chord, (size_t)n * 2 * kTnCells) : nullptr;
  t.o.mode = n ? h.out(mode, (size_t)n * 12 * kTnModes) : nullptr;
  t.sout = h.out(state_out, (size_t)kTnStateLen);
  return t;
}

}  // namespace

extern "C" {

void omega_tonal_config_default(omega_tonal_config* cfg) {
  if (!cfg) return;
  *cfg = omega_tonal_config{};
  cfg->genre = OMEGA_TONAL_POP;
}

int64_t omega_tonal_state_size(void) { return kTnStateLen; }

int omega_tonal_configure(omega_ctx* c, const omega_tonal_config* cfg) try {
  if (!c || !cfg) return OMEGA_EINVAL;
  if (cfg->genre < 0 || cfg->genre >= kTnGenres)
    return fail(c, OMEGA_EINVAL, "tonal: genre %d (omega_tonal_genre: 0..%d)", (int)cfg->genre, kTnGenres - 1);
  c->tonal.genre = cfg->genre;
  c->tonal.set = true;
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_tonal_features(omega_ctx* c, const double* raw_chroma, int64_t n_frames, const int32_t* roll,
                         const int32_t* first, const double* state_in, double* state_out, double* rows,
                         double* key_corr, double* alt_corr, double* chord, double* mode, int mem) try {
  if (!c) return OMEGA_EINVAL;
  if (!c->tonal.set) return fail(c, OMEGA_EINVAL, "tonal: omega_tonal_configure has not been called");
  if (n_frames < 0 || (n_frames > 0 && (!raw_chroma || !rows)))
    return fail(c, OMEGA_EINVAL, "tonal: a negative frame count, or the chroma rows or the output rows missing");
  if (int e = check_rolls(c, roll, n_frames, mem)) return e;
  HIPC(c, hipSetDevice(c->device));
  HostCall h(c, mem);
  const double* draw = h.in(raw_chroma, (size_t)n_frames * 12 * sizeof(double));
  const TonalCall t = stage_tonal(h, n_frames, roll, first, state_in, state_out, rows, key_corr, alt_corr, chord, mode);
  if (h.err) return h.err;
  if (n_frames == 0) {
    if (int e = pass_state_through(c, t.sin, t.sout, (size_t)kTnStateLen * sizeof(double))) return e;
    return h.finish();
  }
  if (int e = run_tonal(c, draw, n_frames, t.roll, t.first, t.sin, t.sout, t.o)) return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_tonal_spectra(omega_ctx* c, const float* spectra, int64_t n_frames, int32_t n_bins, double df,
                        const int32_t* roll, const int32_t* first, const double* state_in, double* state_out,
                        double* rows, double* key_corr, double* alt_corr, double* chord, double* mode, int mem) try {
  if (!c) return OMEGA_EINVAL;
  TonalState& v = c->tonal;
  if (!v.set) return fail(c, OMEGA_EINVAL, "tonal: omega_tonal_configure has not been called");
  if (n_frames < 0 || n_bins < 3 || !(df > 0) || (n_frames > 0 && (!spectra || !rows)))
    return fail(c, OMEGA_EINVAL, "tonal: a negative frame count, fewer than 3 bins, a bin width that is not positive, "
                "or the spectra or the output rows missing");
  if (int e = check_rolls(c, roll, n_frames, mem)) return e;
  HIPC(c, hipSetDevice(c->device));
  ChromaMat m{};
  if (n_frames)
    if (int e = get_chroma_mat(c, n_bins, df, &m)) return e;
  if (int e = grow(c, &v.raw, &v.raw_cap, n_frames * 12)) return e;
  HostCall h(c, mem);
  const float* dspec = h.in(spectra, (size_t)n_frames * n_bins * sizeof(float));
  const TonalCall t = stage_tonal(h, n_frames, roll, first, state_in, state_out, rows, key_corr, alt_corr, chord, mode);
  if (h.err) return h.err;
  if (n_frames == 0) {
    if (int e = pass_state_through(c, t.sin, t.sout, (size_t)kTnStateLen * sizeof(double))) return e;
    return h.finish();
  }
  HIPC(c, launch_chroma(dspec, n_frames, n_bins, m.lo, m.hi, m.mat, v.raw, c->stream));
  if (int e = run_tonal(c, v.raw, n_frames, t.roll, t.first, t.sin, t.sout, t.o)) return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
