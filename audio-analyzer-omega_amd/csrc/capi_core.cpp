// libomega.so host side: the C ABI declared in include/omega.h. Here: the context's life cycle, the table
// builders, error reporting and the queue probes (entry points: capi_*.cpp; shared: host.hpp, design.cpp).
//
// The context precomputes (in float64, cast like the reference casts) every table the kernels read:
// windows (np.blackman/np.hanning/np.hamming), psychoacoustic weights (multi_resolution_fft.py:304-329,
// float32 compounding), the combine plan (multi_resolution_fft.py:353-395), FFT twiddles, the
// true-peak rotation table, the two K-weighting biquads in state-space form with their chunk-scan
// tables (professional_meters.py:48-72, scipy.signal.butter/lfilter_zi closed forms), and owns the
// per-channel meter state (professional_meters.py:19-25) on the device, double-buffered.

#include "host.hpp"

namespace omega_host __attribute__((visibility("hidden"))) {

int fail(omega_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) {
    std::memcpy(c->err, buf, sizeof buf);
    c->zc_ok = false;  // (a host call that fails before finish_host)
  }
  return code;
}

// The ABI contract (omega.h: no C++ exception and no abort crosses it): every extern "C" entry point
// is a function-try-block whose handler maps what escaped -- std::bad_alloc from a host container, or
// anything else -- to a status code and omega_last_error. Called only from inside a catch clause.
int guard_fail(omega_ctx* c) noexcept {
  try {
    throw;
  } catch (const std::bad_alloc&) {
    return fail(c, OMEGA_ENOMEM, "out of host memory");
  } catch (const std::exception& e) {
    return fail(c, OMEGA_EHIP, "internal error: %s", e.what());
  } catch (...) {
    return fail(c, OMEGA_EHIP, "internal error: unknown exception");
  }
}

void release(omega_ctx* c, void* p) {
  auto it = std::find(c->allocs.begin(), c->allocs.end(), p);
  if (it != c->allocs.end()) c->allocs.erase(it);
  if (p) (void)hipFree(p);
}

void drop_graphs(omega_ctx* c) {
  for (auto& g : c->graphs) {
    (void)hipGraphExecDestroy(g.exec);
    (void)hipGraphDestroy(g.graph);
  }
  c->graphs.clear();
}

static int build_twiddles(omega_ctx* c) {
  for (int l = 1; l < kMaxLog2; ++l) {
    const int N = 1 << l;
    std::vector<float2> t(N);
    for (int m = 0; m < N; ++m) {
      const double a = 2.0 * kPi * (double)m / (double)N;
      t[m] = make_float2((float)std::cos(a), (float)-std::sin(a));
    }
    int r = upload(c, &c->d_tw[l], t);
    if (r) return r;
  }
  return 0;
}

int get_window(omega_ctx* c, int m, int kind, float** out) {
  return cached(c->windows, std::make_pair(m, kind), out, [&](float** d) { return upload(c, d, make_window(m, kind)); });
}

// true-peak rotation e^{2 pi i k / (4M)}, k <= M/2
int get_rot(omega_ctx* c, int M, float2** out) {
  return cached(c->rots, M, out, [&](float2** d) {
    std::vector<float2> rot(M / 2 + 1);
    for (int k = 0; k <= M / 2; ++k) {
      const double a = 2.0 * kPi * (double)k / (4.0 * M);
      rot[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    return upload(c, d, rot);
  });
}

}  // namespace omega_host

namespace {

int validate(omega_ctx* c, const omega_config* cfg) {
  // MultiResolutionFFT.__init__ (multi_resolution_fft.py:139-142) and FFTConfig.__post_init__ (:35-44)
  if (cfg->sample_rate <= 0) return fail(c, OMEGA_EINVAL, "Sample rate must be positive");
  if (cfg->max_freq <= 0 || cfg->max_freq > cfg->sample_rate / 2.0)
    return fail(c, OMEGA_EINVAL, "Max frequency must be positive and <= Nyquist");
  if (cfg->n_res < 1 || cfg->n_res > OMEGA_MAX_RES) return fail(c, OMEGA_EINVAL, "n_res must be 1..%d", OMEGA_MAX_RES);
  for (int r = 0; r < cfg->n_res; ++r) {
    const omega_resolution& q = cfg->res[r];
    if (q.freq_lo >= q.freq_hi) return fail(c, OMEGA_EINVAL, "Invalid frequency range: (%g, %g)", q.freq_lo, q.freq_hi);
    if (q.fft_size <= 0 || (q.fft_size & (q.fft_size - 1)) != 0)
      return fail(c, OMEGA_EINVAL, "FFT size must be power of 2: %d", q.fft_size);
    if (q.hop_size <= 0) return fail(c, OMEGA_EINVAL, "Hop size must be positive: %d", q.hop_size);
    if (!(q.weight > 0)) return fail(c, OMEGA_EINVAL, "Weight must be positive: %g", q.weight);
  }
  if (!is_pow2_in(cfg->frame_size, 512, 16384))
    return fail(c, OMEGA_EUNSUP, "frame_size %d: power of two 512..16384 required", cfg->frame_size);
  for (int r = 0; r < cfg->n_res; ++r) {
    const omega_resolution& q = cfg->res[r];
    if (q.fft_size < 2 || q.fft_size > cfg->frame_size)
      return fail(c, OMEGA_EUNSUP, "fft_size %d: 2..frame_size(%d) supported", q.fft_size, cfg->frame_size);
  }
  if (cfg->target_bins < 1 || cfg->target_bins > (1 << 24)) return fail(c, OMEGA_EINVAL, "target_bins out of range");
  if (cfg->n_channels < 1) return fail(c, OMEGA_EINVAL, "n_channels must be >= 1");
  if (cfg->integrated_len < 1 || cfg->integrated_len > 4096)
    return fail(c, OMEGA_EUNSUP, "integrated_len %d: 1..4096 supported", cfg->integrated_len);
  if (cfg->momentary_len < 1 || cfg->short_len < 1 || cfg->peak_len < 1)
    return fail(c, OMEGA_EINVAL, "deque lengths must be >= 1");
  return 0;
}

int build_spectral_tables(omega_ctx* c) {
  const omega_config& cfg = c->cfg;
  const double fs = cfg.sample_rate;
  std::vector<std::vector<float>> wg(cfg.n_res);  // host copies of the weight tables
  for (int r = 0; r < cfg.n_res; ++r) {
    const omega_resolution& q = cfg.res[r];
    const int N = q.fft_size;
    int e = get_window(c, N, q.window, &c->d_win[r]);
    if (e) return e;
    // multi_resolution_fft.py:310-326 -- float32 weights, float32 compounding
    std::vector<float> w(N / 2 + 1);
    for (int k = 0; k <= N / 2; ++k) {
      const double f = rfreq(k, N, fs);
      float v = (float)q.weight;
      if (cfg.apply_weighting) {
        const bool in = f >= q.freq_lo && f <= q.freq_hi;
        if (in && f >= 60 && f <= 120) v = v * 1.8f;
        if (in && f >= 200 && f <= 400) v = v * 1.4f;
        if (in && f >= 2000 && f <= 5000) v = v * 1.2f;
        if (in && f >= 20 && f <= 80) v = v * 1.6f;
      } else {
        v = 1.0f;
      }
      w[k] = v;
    }
    e = upload(c, &c->d_wgt[r], w);
    if (e) return e;
    wg[r] = std::move(w);
  }
  // combine plan (multi_resolution_fft.py:353-395)
  const int T = cfg.target_bins;
  const double mf = std::min(cfg.max_freq, fs / 2);
  std::vector<double> tgt(T);
  const double step = T > 1 ? mf / (T - 1) : 0.0;  // np.linspace(0, mf, T)
  for (int t = 0; t < T; ++t) tgt[t] = t * step;
  if (T > 1) tgt[T - 1] = mf;
  struct Ent {
    int r, j;
    float fr;
  };
  std::vector<std::vector<Ent>> own(T);
  for (int r = 0; r < cfg.n_res; ++r) {
    const omega_resolution& q = cfg.res[r];
    const int N = q.fft_size;
    std::vector<int> vidx;
    for (int k = 0; k <= N / 2; ++k) {
      const double f = rfreq(k, N, fs);
      if (f >= q.freq_lo && f <= q.freq_hi) vidx.push_back(k);
    }
    if (vidx.size() < 2) continue;  // :367-374
    for (int t = 0; t < T; ++t) {
      const double x = tgt[t];
      if (!(x >= q.freq_lo && x <= q.freq_hi)) continue;
      const double f0 = rfreq(vidx.front(), N, fs), f1 = rfreq(vidx.back(), N, fs);
      Ent en{r, 0, 0.f};
      if (x <= f0) {
        en.j = vidx.front();
      } else if (x >= f1) {
        en.j = vidx.back();
      } else {
        // vidx is contiguous: x in [f_j, f_{j+1})
        const double val = rfreq(1, N, fs);
        int j = (int)std::floor(x / val);
        j = std::max(vidx.front(), std::min(j, vidx.back() - 1));
        while (j > vidx.front() && rfreq(j, N, fs) > x) --j;
        while (j + 1 < vidx.back() && rfreq(j + 1, N, fs) <= x) ++j;
        const double fa = rfreq(j, N, fs), fb = rfreq(j + 1, N, fs);
        en.j = j;
        en.fr = (float)((x - fa) / (fb - fa));
      }
      own[t].push_back(en);
    }
  }
  c->res_independent = true;
  for (int t = 0; t < T; ++t)
    if (own[t].size() > 1) c->res_independent = false;
  // per-resolution combine entries (see CombEnt): the interpolation of weighted magnitudes
  // m_j + fr (m_{j+1} - m_j), m = |X| * wgt, times cw / sum of the target's owner weights
  std::vector<std::vector<CombEnt>> er(cfg.n_res);
  for (int t = 0; t < T; ++t) {
    const auto& o = own[t];
    if (o.empty()) {
      er[0].push_back(CombEnt{t | (2 << 24), 0, 0.f, 0.f});
      continue;
    }
    double ws = 0.0;
    for (const Ent& en : o) ws += (double)(float)cfg.res[en.r].weight;
    for (size_t q = 0; q < o.size(); ++q) {
      const Ent& en = o[q];
      const double s = (double)(float)cfg.res[en.r].weight / ws;
      const double fr = en.fr;
      const int op = (q == 0 ? 0 : 1) << 24;
      if (en.fr == 0.f && en.j == cfg.res[en.r].fft_size / 2)  // last bin: keep j + 1 in range
        er[en.r].push_back(CombEnt{t | op, en.j - 1, 0.f, (float)(wg[en.r][en.j] * s)});
      else
        er[en.r].push_back(CombEnt{t | op, en.j, (float)((1.0 - fr) * wg[en.r][en.j] * s),
                                   (float)(en.fr != 0.f ? fr * wg[en.r][en.j + 1] * s : 0.0)});
    }
  }
  std::vector<CombEnt> all;
  for (int r = 0; r < cfg.n_res; ++r) {
    c->ent_begin[r] = (int)all.size();
    all.insert(all.end(), er[r].begin(), er[r].end());
    c->ent_end[r] = (int)all.size();
    c->ent_jmax[r] = 0;
    for (const CombEnt& en : er[r]) c->ent_jmax[r] = std::max(c->ent_jmax[r], en.j + 1);
    // the magnitude pairs (k, K - k) holding every bin an entry reads (j and j + 1): one untangle per
    // pair instead of two per entry, where that is fewer (ResParam::pair_lo / pair_hi)
    const int K = cfg.res[r].fft_size / 2;
    int plo = K, phi = -1;
    for (const CombEnt& en : er[r]) {
      if ((en.tm >> 24) == 2) continue;
      for (int b = en.j; b <= en.j + 1; ++b) {
        const int k = (b == K || b == K / 2) ? 0 : std::min(b, K - b);
        plo = std::min(plo, k);
        phi = std::max(phi, k);
      }
    }
    c->pair_lo[r] = c->pair_hi[r] = 0;
    if (phi >= 0 && K >= 2 && (phi + 1 - plo) < 2 * (int)er[r].size()) {
      c->pair_lo[r] = plo;
      c->pair_hi[r] = phi + 1;
    }
  }
  std::vector<int> ooff(1, 0), orj;
  std::vector<float> ofr;
  for (int t = 0; t < T; ++t) {
    for (const Ent& en : own[t]) {
      orj.push_back((en.r << 24) | en.j);
      ofr.push_back(en.fr);
    }
    ooff.push_back((int)orj.size());
  }
  int e = upload(c, &c->d_own_off, ooff);
  if (!e) e = upload(c, &c->d_own_rj, orj);
  if (!e) e = upload(c, &c->d_own_frac, ofr);
  if (!e) e = upload(c, &c->d_ent, all);
  if (e) return e;
  return get_rot(c, cfg.frame_size, &c->d_rot);
}

int build_meter_state(omega_ctx* c) {
  const int C = c->cfg.n_channels;
  c->HL = std::max(1, c->cfg.integrated_len - 1);
  c->HT = std::max(1, c->cfg.peak_len - 1);
  for (int b = 0; b < 2; ++b) {
    int e = dalloc(c, &c->d_hist_l[b], (size_t)C * c->HL);
    if (!e) e = dalloc(c, &c->d_hist_t[b], (size_t)C * c->HT);
    if (!e) e = dalloc(c, &c->d_nl[b], C);
    if (!e) e = dalloc(c, &c->d_nt[b], C);
    if (e) return e;
  }
  int e = 0;
  for (int b = 0; b < 2 && !e; ++b) {
    e = dalloc(c, &c->d_skeys[b], (size_t)C * c->HL);
    if (!e) e = dalloc(c, &c->d_ns[b], C);
    if (!e) e = dalloc(c, &c->d_t0[b], C);
  }
  for (int b = 0; b < 2; ++b) {
    if (!e) e = dalloc(c, &c->d_core[b], (size_t)C * kMeterSeqCap);
    if (!e) e = dalloc(c, &c->d_ext[b], (size_t)C * kMeterSeqCap);
    if (!e) e = dalloc(c, &c->d_ncore[b], C);
    if (!e) e = dalloc(c, &c->d_next[b], C);
    if (!e) e = dalloc(c, &c->d_gcount[b], (size_t)C * (kMeterSeqCap + 1));
    if (!e) e = dalloc(c, &c->d_gsum[b], (size_t)C * (kMeterSeqCap + 1));
  }
  if (!e) e = dalloc(c, &c->d_ctr, kCtrWords);
  if (e) return e;
  if (!c->h_err) {
    HIPC(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_err), 2 * sizeof(unsigned),
                          hipHostMallocMapped | hipHostMallocCoherent));
    c->h_err[0] = c->h_err[1] = 0;
    HIPC(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_err), c->h_err, 0));
  }
  HIPC(c, hipMemset(c->d_ctr, 0, kCtrWords * sizeof(unsigned)));
  c->ms = MeterSync{};
  return omega_meter_reset(c);
}

// fork[0] carries the latency-bound meter kernels beside full-chip work, at the default priority: a
// high-priority side stream measured the same on the cfg2 step (pipelined 65.7-68.7 vs 65.5-67.8 us,
// profiles/r05_ab_side_priority.txt) and made the event-joined paths 2-4x slower per call with one
// other context alive in the process (profiles/r05_side_order.txt)
hipError_t create_side_stream(hipStream_t* st) { return hipStreamCreateWithFlags(st, hipStreamNonBlocking); }

// The meter ordering needs the context's stream and fork[0] on different hardware queues (omega.h,
// omega_set_stream), and HIP deals streams out over GPU_MAX_HW_QUEUES (4) queues per process, so with
// other contexts or streams alive the two can share one: the batch path's device waits then run into
// their bound (OMEGA_EHIP), and the event-joined paths serialise (bench.py's cfg1 line measured 0.28 ms
// per call instead of 0.07 with one other context alive, tools/side_order_probe.py). Probe the pair
// (a waiter on fork[0], then a setter on the stream: the waiter sees the value only if they run at
// once); on a shared queue keep that side stream as a spare and take a new one -- the next queue -- and
// probe again (three times at most). Run at creation and on a stream switch.
// A stream already probed against the current side stream is not probed again (a caller alternating
// streams keeps its host/GPU overlap); force re-probes the pair (omega_check_queues: streams created
// since, e.g. an RCCL communicator's, may have been dealt onto the side stream's queue).
constexpr int kProbePolls = 2048;  // x ~0.3 us: the waiter's bound (paid only on a shared queue)
constexpr size_t kMaxSpare = 6;
// `*st` shares a hardware queue it should not: keep it as a spare (so the next stream created lands on
// another queue) and take a new one. The replacement is created BEFORE the oldest spare beyond
// kMaxSpare is destroyed: destroying first could free the very queue that was found shared and put
// the new stream back on it.
int replace_side_stream(omega_ctx* c, hipStream_t* st) {
  hipStream_t fresh = nullptr;
  HIPC(c, create_side_stream(&fresh));
  c->spare.push_back(*st);
  *st = fresh;
  if (c->spare.size() > kMaxSpare) {
    HIPC(c, hipStreamDestroy(c->spare.front()));
    c->spare.erase(c->spare.begin());
  }
  return 0;
}

int probe_words(omega_ctx* c) {  // omega_ctx::d_probe, on first use
  if (c->d_probe) return 0;
  HIPC(c, hipMalloc(&c->d_probe, 2 * sizeof(unsigned)));
  HIPC(c, hipMemset(c->d_probe, 0, 2 * sizeof(unsigned)));
  return 0;
}

// One probe of a pair of idle streams: *ind = a kernel on `setter` ran beside a waiting one on `waiter`.
int probe_pair(omega_ctx* c, hipStream_t waiter, hipStream_t setter, bool* ind) {
  const unsigned target = ++c->probe_seq;  // (w[0] holds the previous one: never equal)
  HIPC(c, launch_queue_probe(c->d_probe, target, kProbePolls, waiter, setter));
  HIPC(c, hipStreamSynchronize(waiter));
  HIPC(c, hipStreamSynchronize(setter));
  unsigned r[2] = {0u, 0u};
  HIPC(c, hipMemcpy(r, c->d_probe, sizeof r, hipMemcpyDeviceToHost));
  *ind = r[1] == target;
  return 0;
}

// The batch streams of overlapped pipelined calls (omega_ctx::bs), probed like the side stream: each
// against fork[0] (the meter prep polls beside the batch, and the batch's meter segment polls the prep's
// count), against the context's stream (an entry event recorded behind a batch on a shared queue would
// hold the next batch until this one ends) and against each other (the overlap itself). A batch stream
// on a shared queue is replaced, three times at most; after that the calls serialise on that queue
// (every stream wait follows the work it waits for) and the device waits stay bounded.
int batch_stream_check(omega_ctx* c) {
  c->bs_shared = false;
  if (!c->bs[0]) return 0;
  if (int e = probe_words(c)) return e;
  HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, hipStreamSynchronize(c->fork[0]));
  for (int k = 0; k < 2; ++k) {
    HIPC(c, hipStreamSynchronize(c->bs[k]));
    bool ind = false;
    for (int attempt = 0;; ++attempt) {  // (the last replacement is probed too)
      if (int e = probe_pair(c, c->fork[0], c->bs[k], &ind)) return e;
      if (ind)
        if (int e = probe_pair(c, c->bs[k], c->stream, &ind)) return e;
      if (ind && k == 1)
        if (int e = probe_pair(c, c->bs[0], c->bs[1], &ind)) return e;
      if (ind || attempt == 3) break;
      if (int e = replace_side_stream(c, &c->bs[k])) return e;
    }
    if (!ind) c->bs_shared = true;
  }
  // Not an error and not what omega_check_queues returns (that is the side stream's queue, on which the
  // device waits depend): overlapped calls then serialise, and omega_last_error says so.
  if (c->bs_shared && !c->queue_shared)
    std::snprintf(c->err, sizeof c->err,
                  "batch streams: no hardware queues independent of the context's stream, the side stream and "
                  "each other found after 3 attempts (more streams than GPU_MAX_HW_QUEUES?): consecutive "
                  "pipelined batch calls serialise instead of overlapping");
  return 0;
}

int side_stream_check(omega_ctx* c, bool force = false) {
  if (!force && std::find(c->checked.begin(), c->checked.end(), c->stream) != c->checked.end()) return 0;
  if (int e = probe_words(c)) return e;
  // both streams idle first: a setter queued behind earlier work on the caller's stream would read as
  // a shared queue (a rocprofv3 trace of bench.py showed probe waiters running to their bound)
  HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, hipStreamSynchronize(c->fork[0]));
  for (int attempt = 0; attempt < 3; ++attempt) {
    bool ind = false;
    if (int e = probe_pair(c, c->fork[0], c->stream, &ind)) return e;
    if (ind) {
      c->queue_shared = false;
      c->checked.push_back(c->stream);
      return batch_stream_check(c);
    }
    // a new side stream: what was checked against the old one no longer holds
    c->checked.clear();
    if (int e = replace_side_stream(c, &c->fork[0])) return e;
  }
  // No independent queue found: not an error (the device waits stay bounded, omega.h), but reported --
  // omega_check_queues returns it, and omega_last_error says why the batch path may return OMEGA_EHIP.
  // The stream is not marked checked: the next switch to it probes again.
  c->queue_shared = true;
  if (int e = batch_stream_check(c)) return e;  // (the batch streams against this side stream all the same)
  std::snprintf(c->err, sizeof c->err,
                "side stream: no hardware queue independent of the context's stream found after 3 attempts "
                "(more streams than GPU_MAX_HW_QUEUES?): batch-path device waits may run to their bound "
                "(OMEGA_POLL_LIMIT) and return OMEGA_EHIP%s",
                c->bs_shared ? "; the batch streams share queues too: pipelined batch calls serialise" : "");
  return 0;
}

}  // namespace

extern "C" {

const char* omega_version(void) { return "omega-mi355x 0.5 (gfx950, ABI 5)"; }

void omega_config_default(omega_config* cfg) try {
  std::memset(cfg, 0, sizeof *cfg);
  cfg->sample_rate = 48000;
  cfg->max_freq = 20000;
  cfg->n_res = 4;
  const omega_resolution def[4] = {{20, 200, 4096, 1024, 1.5, OMEGA_WIN_BLACKMAN},
                                   {200, 1000, 2048, 512, 1.2, OMEGA_WIN_BLACKMAN},
                                   {1000, 5000, 1024, 256, 1.0, OMEGA_WIN_BLACKMAN},
                                   {5000, 20000, 1024, 256, 1.5, OMEGA_WIN_BLACKMAN}};
  std::memcpy(cfg->res, def, sizeof def);
  cfg->apply_weighting = 1;
  cfg->target_bins = 1024;
  cfg->frame_size = 4096;
  cfg->n_channels = 1;
  cfg->gate_lufs = -70.0;
  cfg->momentary_len = 24;
  cfg->short_len = 180;
  cfg->integrated_len = 3600;
  cfg->peak_len = 60;
} catch (...) {
}

int omega_create(const omega_config* cfg, int device, omega_ctx** out) try {
  if (!cfg || !out) return OMEGA_EINVAL;
  *out = nullptr;
  omega_ctx* c = new (std::nothrow) omega_ctx();
  if (!c) return OMEGA_ENOMEM;
  int e = validate(c, cfg);
  if (e) {
    // surface the message through a throwaway context: callers read it via omega_last_error(*out)
    *out = c;
    return e;
  }
  c->cfg = *cfg;
  c->device = device;
  hipError_t he = hipSetDevice(device);
  if (he == hipSuccess) he = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking);
  if (he != hipSuccess) {
    *out = c;
    return fail(c, OMEGA_EHIP, "device %d: %s", device, hipGetErrorString(he));
  }
  c->stream = c->own;
  // the one environment variable the library reads: the device-wait bound of the meter ordering
  // (a test knob: tests/test_gpu_parity.py test_meter_ordering_expiry_is_reported)
  if (const char* pl = std::getenv("OMEGA_POLL_LIMIT")) c->poll_limit = std::atoi(pl) > 0 ? std::atoi(pl) : 1;
  // (the graph-capture stream is created on the first capture: a context holds two streams --
  // the hardware has GPU_MAX_HW_QUEUES = 4 queues per process, see omega.h on the meter ordering)
  if (he == hipSuccess) he = create_side_stream(&c->fork[0]);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&c->ev_join[0], hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&c->ev_join[1], hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&c->ev_kw, hipEventDisableTiming);
  if (he != hipSuccess) {
    *out = c;
    return fail(c, OMEGA_EHIP, "streams/events: %s", hipGetErrorString(he));
  }
  e = build_twiddles(c);
  if (!e) e = build_spectral_tables(c);
  if (!e) e = build_meter_state(c);
  if (!e) e = side_stream_check(c);
  *out = c;
  return e;
} catch (...) {
  return guard_fail(out ? *out : nullptr);
}

void omega_destroy(omega_ctx* c) try {
  if (!c) return;
  if (c->device >= 0) (void)hipSetDevice(c->device);
  if ((c->ms.pend || c->unjoined) && !flush_meters(c)) (void)hipStreamSynchronize(c->stream);  // (the last call's meters)
  for (hipStream_t st : c->bs)
    if (st) (void)hipStreamSynchronize(st);
  if (c->own) (void)hipStreamSynchronize(c->own);
  if (c->fork[0]) (void)hipStreamSynchronize(c->fork[0]);
  for (void* p : c->allocs) (void)hipFree(p);
  for (auto& kv : c->chroma_mats) (void)hipFree(kv.second.first);
  for (void* q : {(void*)c->ctab.w4, (void*)c->ctab.w1, (void*)c->ctab.perm, (void*)c->ctab.goff,
                  (void*)c->ctab.rec})
    if (q) (void)hipFree(q);
  for (DevBuf& b : c->stage)
    if (b.p) (void)hipFree(b.p);
  for (DevBuf& b : c->pin)
    if (b.p) (void)hipHostFree(b.p);
  if (c->oarena.p) (void)hipFree(c->oarena.p);
  if (c->oarena_pin.p) (void)hipHostFree(c->oarena_pin.p);
  if (c->zc_pin.p) (void)hipHostFree(c->zc_pin.p);
  drop_graphs(c);
  if (c->h_err) (void)hipHostFree(c->h_err);
  if (c->d_tail) (void)hipFree(c->d_tail);
  if (c->d_mirror) (void)hipFree(c->d_mirror);
  for (hipStream_t st : {c->cap, c->fork[0], c->bs[0], c->bs[1]})
    if (st) (void)hipStreamDestroy(st);
  for (hipStream_t st : c->spare) (void)hipStreamDestroy(st);
  if (c->d_probe) (void)hipFree(c->d_probe);
  for (hipEvent_t ev : {c->ev_fork, c->ev_join[0], c->ev_join[1], c->ev_kw, c->ev_in, c->ev_done[0], c->ev_done[1]})
    if (ev) (void)hipEventDestroy(ev);
  if (c->own) (void)hipStreamDestroy(c->own);
  delete c;
} catch (...) {
}

const char* omega_last_error(const omega_ctx* c) { return c ? c->err : "null context"; }

int omega_set_stream(omega_ctx* c, void* s) try {
  if (!c) return OMEGA_EINVAL;
  const hipStream_t ns = static_cast<hipStream_t>(s);  // NULL = the null (default) stream, e.g. torch's
  if (ns != c->stream) {
    if (c->ms.pend || c->unjoined) {  // (a pending meter segment runs on its batch's stream)
      HIPC(c, hipSetDevice(c->device));
      if (int e = flush_meters(c)) return e;
    }
    // The work already enqueued on the old stream -- a batch's meter segment still reading the
    // per-context prep scratch and history, a query kernel -- must finish before the next call's work:
    // on one stream that is stream order, and the next meter prep on fork[0] waits for the next
    // batch's K-weighting count, i.e. for a batch that started after the previous one ended. Across a
    // stream switch nothing orders them, so the new stream and fork[0] wait once for the old stream.
    HIPC(c, hipSetDevice(c->device));
    if (int e = after_main(c, ns)) return e;
    HIPC(c, hipStreamWaitEvent(side_stream(c), c->ev_fork, 0));
    c->stream = ns;
    if (int e = side_stream_check(c)) return e;
  }
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_check_queues(omega_ctx* c, int* shared) try {
  if (!c) return OMEGA_EINVAL;
  HIPC(c, hipSetDevice(c->device));
  if (c->ms.pend || c->unjoined) {  // (the probe synchronises the streams; a pending segment launches first)
    if (int e = flush_meters(c)) return e;
  }
  if (int e = side_stream_check(c, true)) return e;
  if (shared) *shared = c->queue_shared ? 1 : 0;
  return 0;
} catch (...) {
  return guard_fail(c);
}

void* omega_get_stream(const omega_ctx* c) { return c ? static_cast<void*>(c->stream) : nullptr; }

int omega_get_config(const omega_ctx* c, omega_config* cfg, int* device) {
  if (!c) return OMEGA_EINVAL;
  if (cfg) *cfg = c->cfg;
  if (device) *device = c->device;
  return 0;
}

int omega_set_graphs(omega_ctx* c, int enable) try {
  if (!c) return OMEGA_EINVAL;
  if (c->ms.pend || c->unjoined) {
    HIPC(c, hipSetDevice(c->device));
    if (int e = flush_meters(c)) return e;
  }
  c->use_graph = (enable & 1) != 0;
  // bits 1-2: 0 default (one batch launch where eligible), else the full-chip kernels back to back with
  // the meters on a side stream
  c->layout = ((enable >> 1) & 3) ? 2 : 3;
  drop_graphs(c);
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_synchronize(omega_ctx* c) try {
  if (!c) return OMEGA_EINVAL;
  if (c->ms.pend || c->unjoined) {
    HIPC(c, hipSetDevice(c->device));
    if (int e = flush_meters(c)) return e;
  }
  HIPC(c, hipStreamSynchronize(c->stream));
  return check_device_err(c);
} catch (...) {
  return guard_fail(c);
}

int omega_set_meter_pipelining(omega_ctx* c, int enable) try {
  if (!c) return OMEGA_EINVAL;
  if (!enable && (c->ms.pend || c->unjoined)) {
    HIPC(c, hipSetDevice(c->device));
    if (int e = flush_meters(c)) return e;
  }
  c->pipe = enable != 0;
  if (c->pipe && !c->bs[0]) {
    HIPC(c, hipSetDevice(c->device));
    for (int k = 0; k < 2; ++k) {
      HIPC(c, create_side_stream(&c->bs[k]));
      HIPC(c, hipEventCreateWithFlags(&c->ev_done[k], hipEventDisableTiming));
    }
    HIPC(c, hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
    if (int e = batch_stream_check(c)) return e;
  }
  return 0;
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
