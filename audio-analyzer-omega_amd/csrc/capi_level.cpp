// libomega.so host side: the entry points that measure level without the batch kernel -- the true peak
// (power-of-two frames and, with the any-length plan and run_any, every other length), the K-weighting scan
// and the float64 weighting cascade, the meter aggregates (update, load, reset) and omega_calculate_lufs,
// which runs the three in one call: the true peak on the side stream beside the weighting. The device-side
// bodies of the true peak and the weighting take the stream they enqueue on; the entry points validate and
// stage. The ordering of the side stream against the caller's is host.hpp's named helpers, and whether a
// join is owed is the ledger's (meter_sync.hpp: MeterSync::side, step_lufs_tp, step_join).

#include "host.hpp"

extern "C" {

// Plan of the any-length transform: radices (4s, then 2, 3, 5, 7, then the remaining primes) and the
// tables e^{-2 pi i m / N}, e^{2 pi i m / (4N)} in float64 rounded to float32
int get_any_plan(omega_ctx* c, int N, omega_ctx::AnyPlan** out) {
  auto it = c->any_plans.find(N);
  if (it == c->any_plans.end()) {
    omega_ctx::AnyPlan pl;
    pl.radix = fft_radices(N);
    if ((int)pl.radix.size() > kAnyMaxStages) return fail(c, OMEGA_EUNSUP, "length %d: too many factors", N);
    std::vector<float2> tw(N), rot(3 * (N / 2) + 1);
    for (int m = 0; m < N; ++m) tw[m] = make_float2((float)std::cos(2 * kPi * m / N), (float)-std::sin(2 * kPi * m / N));
    for (size_t m = 0; m < rot.size(); ++m)
      rot[m] = make_float2((float)std::cos(2 * kPi * (double)m / (4.0 * N)), (float)std::sin(2 * kPi * (double)m / (4.0 * N)));
    int e = upload(c, &pl.tw, tw);
    if (!e) e = upload(c, &pl.rot, rot);
    if (!e && !pl.radix.empty() && pl.radix.back() > kAnyF32Radix) {
      // a stage of R terms summed in float64 keeps its precision only with unrounded factors: the rounding
      // errors of the float32 table add up over the R terms to the same offset in every output
      e = upload(c, &pl.tw64, twiddles64(N, N));
    }
    if (e) return e;
    it = c->any_plans.emplace(N, std::move(pl)).first;
  }
  *out = &it->second;
  return 0;
}

// launches the any-length kernel on `s` over n frames in slices whose global scratch (N > kAnyLdsMax) stays
// within 64 MiB; p.x / outputs advanced per slice
int run_any(omega_ctx* c, AnyFftParams p, int truepeak, hipStream_t s) {
  omega_ctx::AnyPlan* pl = nullptr;
  if (int e = get_any_plan(c, p.N, &pl)) return e;
  p.n_stages = (int)pl->radix.size();
  for (int i = 0; i < p.n_stages; ++i) p.radix[i] = pl->radix[i];
  p.tw = pl->tw;
  p.tw64 = pl->tw64;
  p.rot = pl->rot;
  for (int ph = 0; ph < 4; ++ph) p.nyq_cos[ph] = (float)std::cos(kPi * ph / 4.0);
  const int64_t n = p.n;
  int64_t per = n;
  if (p.N > kAnyLdsMax) {
    per = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(8 << 20) / (3 * (int64_t)p.N)));
    if (int e = grow(c, &c->d_any, &c->any_cap, per * 3 * p.N)) return e;
    p.scratch = c->d_any;
  }
  const int nb = p.N / 2 + 1;
  for (int64_t f0 = 0; f0 < n; f0 += per) {
    AnyFftParams q = p;
    q.x = p.x + f0 * p.frame_stride;
    q.n = std::min(per, n - f0);
    if (q.tp_out) q.tp_out = p.tp_out + f0;
    if (q.mag) q.mag = p.mag + f0 * nb;
    if (q.cplx) q.cplx = p.cplx + f0 * nb * 2;
    HIPC(c, launch_any(q, truepeak, s));
  }
  return 0;
}

// The float64 filter cascade of a weighting mode for the context's sample rate
// (professional_meters.py:48-72, :74-127): K = {butter(2, 38 Hz, high), iirfilter(2, 1500 Hz, high)}
// blended 0.3; A = {butter(2, 20.598997, high), butter(1, 107.65265, high), butter(1, 737.86223, low),
// butter(2, min(12194.217 / nyq, 0.99), low)} x 2.5; C = {butter(2, 20.598997, high), butter(2, 12194.217, low)}.
W64Stage w64_stage(const BiquadCoef& q, int order) {
  W64Stage s{};
  s.b0 = q.b[0];
  s.b1 = q.b[1];
  s.b2 = q.b[2];
  s.a1 = q.a[1];
  s.a2 = q.a[2];
  // scipy.signal.lfilter_zi: solve (I - companion(a).T) zi = b[1:] - a[1:] b[0]
  const double B0 = s.b1 - s.a1 * s.b0, B1 = s.b2 - s.a2 * s.b0;
  s.zi0 = (B0 + B1) / (1.0 + s.a1 + s.a2);
  s.zi1 = B1 - s.a2 * s.zi0;
  s.E = 3 * (order + 1);  // filtfilt's default padlen 3 max(len(a), len(b))
  return s;
}

int get_w64_stages(omega_ctx* c, int mode, W64Stage** out) {
  if (c->w64[mode]) {
    *out = c->w64[mode];
    return 0;
  }
  const double fs = c->cfg.sample_rate, nyq = fs / 2;
  const double f1 = 20.598997, f2 = 107.65265, f3 = 737.86223, f4 = 12194.217;
  const double f4c = std::min(f4 / nyq, 0.99) * nyq;
  std::vector<W64Stage> t;
  if (mode == OMEGA_WEIGHT_K)
    t = {w64_stage(butter2(38.0, fs, true), 2), w64_stage(butter2(1500.0, fs, true), 2)};
  else if (mode == OMEGA_WEIGHT_A)
    t = {w64_stage(butter2(f1, fs, true), 2), w64_stage(butter1(f2, fs, true), 1),
         w64_stage(butter1(f3, fs, false), 1), w64_stage(butter2(f4c, fs, false), 2)};
  else
    t = {w64_stage(butter2(f1, fs, true), 2), w64_stage(butter2(f4c, fs, false), 2)};
  if (int e = upload(c, &c->w64[mode], t)) return e;
  *out = c->w64[mode];
  return 0;
}

}  // extern "C"

namespace {

int true_peak_check(omega_ctx* c, int32_t m, int32_t oversampling) {
  if (oversampling != 1 && oversampling != 2 && oversampling != 4)
    return fail(c, OMEGA_EUNSUP, "true peak: oversampling %d unsupported (1, 2, 4)", oversampling);
  if (m < 1) return fail(c, OMEGA_EINVAL, "true peak: frame length %d", m);
  return 0;
}

// omega_true_peak_os on device memory, enqueued on `s`; count_to: the word the workgroups count in on
// (power-of-two frames: omega_calculate_lufs' kCtrLufsTp), or null
int true_peak_dev(omega_ctx* c, const float* dx, int64_t n, int32_t m, int32_t oversampling, float* dout,
                  hipStream_t s, unsigned* count_to) {
  const int phases = oversampling == 4 ? 0xE : (oversampling == 2 ? 0x4 : 0);
  if (!is_pow2_in(m, 512, 16384)) {  // frames of other lengths (anyfft.hip)
    AnyFftParams ap{};
    ap.x = dx;
    ap.frame_stride = m;
    ap.n = n;
    ap.N = m;
    ap.phases = phases;
    ap.tp_out = dout;
    return run_any(c, ap, 1, s);
  }
  SpectralParams sp = spectral_params(c);
  sp.x = dx;
  sp.C = 1;
  sp.frame_stride = m;
  sp.chan_stride = 0;
  sp.n_cf = n;
  sp.comb_out = nullptr;
  for (int r = 0; r < kMaxRes; ++r) sp.res[r].mag_out = nullptr;
  sp.n_res = 0;
  sp.tp_out = dout;
  float2* rot = nullptr;
  if (int e = get_rot(c, m, &rot)) return e;
  sp.rot = rot;
  sp.tp_phases = phases;
  sp.tp_done = count_to;
  HIPC(c, tp_launch(m, sp, s));
  return 0;
}

int weighting_check(omega_ctx* c, int32_t m, int32_t mode) {
  if (mode < OMEGA_WEIGHT_K || mode > OMEGA_WEIGHT_Z) return fail(c, OMEGA_EINVAL, "weighting mode %d", mode);
  // scipy's filtfilt needs more samples than its padlen (9 for the first section of K, A and C)
  if (m < 1 || (mode != OMEGA_WEIGHT_Z && m <= 9))
    return fail(c, OMEGA_EINVAL, "weighting: the length of the input (%d) must be greater than padlen (9)", m);
  return 0;
}

// omega_weighting on device memory, enqueued on `s`
int weighting_dev(omega_ctx* c, const float* dx, int64_t n, int32_t m, int32_t mode, float* dw, float* dl,
                  hipStream_t s) {
  Weight64Params p{};
  p.M = m;
  p.mode = mode;
  if (mode != OMEGA_WEIGHT_Z) {
    if (int e = get_w64_stages(c, mode, &p.st)) return e;
    p.n_st = mode == OMEGA_WEIGHT_A ? 4 : 2;
  }
  // float64 working buffers per frame: the signal and its odd extension (at most 64 MiB per launch)
  p.scratch_stride = 2 * (int64_t)m + 32;
  const int64_t per_launch = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(8 << 20) / p.scratch_stride));
  if (int e = grow(c, &c->d_w64, &c->w64_cap, per_launch * p.scratch_stride)) return e;
  p.scratch = c->d_w64;
  for (int64_t f0 = 0; f0 < n; f0 += per_launch) {
    p.x = dx + f0 * m;
    p.n = std::min(per_launch, n - f0);
    p.weighted_out = dw ? dw + f0 * m : nullptr;
    p.lufs_out = dl ? dl + f0 : nullptr;
    HIPC(c, launch_weight64(p, s));
  }
  return 0;
}

// All meter chunks on one stream.
int meters_enqueue(omega_ctx* c, const float* lufs, const float* tp, int64_t n_frames, double* out,
                   hipStream_t stream, unsigned* wait_ctr = nullptr, unsigned wait_target = 0) {
  bool first = true;
  const SyncStep st = step_state_chunks(c->ms, chunk_frames(n_frames));
  c->ms = st.ok;
  for (MeterPrepParams p : meter_chunks(c, st.chunks, lufs, tp, out)) {
    // (wait_ctr: the first chunk's prep polls it before reading the batch's values -- the true peaks
    // of omega_calculate_lufs on the side stream counting in, instead of an event join)
    if (first && wait_ctr) {
      p.wait_ctr = wait_ctr;
      p.wait_target = wait_target;
    }
    HIPC(c, launch_meter_prep(p, stream));
    HIPC(c, launch_meter_query(p, stream));
    first = false;
  }
  return 0;
}

}  // namespace

extern "C" {

int omega_true_peak(omega_ctx* c, const float* x, int64_t n, int32_t m, float* out_db, int mem) try {
  return omega_true_peak_os(c, x, n, m, 4, out_db, mem);
} catch (...) {
  return guard_fail(c);
}

int omega_true_peak_os(omega_ctx* c, const float* x, int64_t n, int32_t m, int32_t oversampling, float* out_db,
                       int mem) try {
  if (!c || !x || !out_db) return OMEGA_EINVAL;
  if (int e = true_peak_check(c, m, oversampling)) return e;
  if (n <= 0) return n == 0 ? 0 : fail(c, OMEGA_EINVAL, "negative count");
  HIPC(c, hipSetDevice(c->device));
  HostCall h(c, mem);  // (omega_process_frames' slots for the same data)
  const float* dx = h.in(x, (size_t)n * m * sizeof(float));
  float* dout = h.out(out_db, n, 3);
  if (h.err) return h.err;
  if (int e = true_peak_dev(c, dx, n, m, oversampling, dout, c->stream, nullptr)) return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

// the batch kernel's float32 K-weighting (kweight_kernel) on its own, for power-of-two frames
int omega_k_weighting(omega_ctx* c, const float* x, int64_t n, int32_t m, float* weighted, float* lufs_inst,
                      int mem) try {
  if (!c || !x) return OMEGA_EINVAL;
  if (!is_pow2_in(m, 512, 16384)) return fail(c, OMEGA_EUNSUP, "k-weighting: frame length %d unsupported", m);
  if (n <= 0) return n == 0 ? 0 : fail(c, OMEGA_EINVAL, "negative count");
  HIPC(c, hipSetDevice(c->device));
  HostCall h(c, mem);  // (omega_process_frames' slots for the same data)
  const float* dx = h.in(x, (size_t)n * m * sizeof(float));
  float* dw = h.out(weighted, (size_t)n * m, 5);
  float* dl = h.out(lufs_inst, n, 2);
  if (h.err) return h.err;
  BiquadTab* tabs = nullptr;
  if (int e = get_kw_tab(c, m, &tabs)) return e;
  KWeightParams kp{dx, m, 0, 1, n, tabs, tabs + 1, dl, dw, OMEGA_WEIGHT_K};
  HIPC(c, launch_kweight(m, kp, c->stream));
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_weighting(omega_ctx* c, const float* x, int64_t n, int32_t m, int32_t mode, float* weighted,
                    float* lufs_inst, int mem) try {
  if (!c || !x) return OMEGA_EINVAL;
  if (int e = weighting_check(c, m, mode)) return e;
  if (n <= 0) return n == 0 ? 0 : fail(c, OMEGA_EINVAL, "negative count");
  HIPC(c, hipSetDevice(c->device));
  HostCall h(c, mem);  // (omega_process_frames' slots for the same data)
  const float* dx = h.in(x, (size_t)n * m * sizeof(float));
  float* dw = h.out(weighted, (size_t)n * m, 5);
  float* dl = h.out(lufs_inst, n, 2);
  if (h.err) return h.err;
  if (int e = weighting_dev(c, dx, n, m, mode, dw, dl, c->stream)) return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_meter_reset(omega_ctx* c) try {
  if (!c) return OMEGA_EINVAL;
  if (int e = flush_meters(c)) return e;  // (the pending segment reads the state being reset)
  // a meter prep on the side stream may still be writing the next state after its count-in
  if (side_stream(c)) HIPC(c, hipStreamSynchronize(side_stream(c)));
  const int C = c->cfg.n_channels;
  for (int b = 0; b < 2; ++b) {
    HIPC(c, hipMemsetAsync(c->d_nl[b], 0, C * sizeof(int), c->stream));
    HIPC(c, hipMemsetAsync(c->d_nt[b], 0, C * sizeof(int), c->stream));
    HIPC(c, hipMemsetAsync(c->d_ns[b], 0, C * sizeof(int), c->stream));
    HIPC(c, hipMemsetAsync(c->d_t0[b], 0, C * sizeof(uint32_t), c->stream));
  }
  HIPC(c, hipStreamSynchronize(c->stream));
  return 0;
} catch (...) {
  return guard_fail(c);
}

// The meter aggregates on the caller's stream from device inputs. join_side: these kernels read the
// state a meter prep on the side stream may still be writing (after its count-in), so the caller's
// stream first waits for the side stream (a caller that has just joined it skips the second wait);
// order_side: the next batch's meter prep runs on the side stream and reads, before its K-weighting
// count, the state these kernels write, so the side stream is ordered after them (a host-memory
// caller does it after its copies back, which then follow the kernels without an event between).
int meter_update_dev(omega_ctx* c, const float* dl, const float* dt, int64_t n_frames, double* dm, bool join_side,
                     bool order_side, unsigned* wait_ctr = nullptr, unsigned wait_target = 0) {
  if (join_side)
    if (int e = main_after_side(c, 1)) return e;
  if (int e = meters_enqueue(c, dl, dt, n_frames, dm, c->stream, wait_ctr, wait_target)) return e;
  return order_side ? side_after_main(c) : 0;
}

int omega_meter_update(omega_ctx* c, const float* lufs_inst, const float* tp_db, int64_t n_frames, double* meters,
                       int mem) try {
  if (!c || !lufs_inst || !tp_db || !meters) return OMEGA_EINVAL;
  if (n_frames <= 0) return n_frames == 0 ? 0 : fail(c, OMEGA_EINVAL, "negative count");
  if (int e = check_device_err(c)) return e;
  HIPC(c, hipSetDevice(c->device));
  if (int e = flush_meters(c)) return e;
  const int64_t ncf = n_frames * c->cfg.n_channels;
  HostCall h(c, mem);  // (omega_process_frames' slots for the same data)
  const float* dl = h.in(lufs_inst, ncf * sizeof(float), 2);
  const float* dt = h.in(tp_db, ncf * sizeof(float));
  double* dm = h.out(meters, ncf * 5);
  if (h.err) return h.err;
  if (int e = meter_update_dev(c, dl, dt, n_frames, dm, true, true)) return e;
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_meter_load_history(omega_ctx* c, const float* lufs_inst, int64_t n_l, const float* tp_db, int64_t n_t,
                             int mem) try {
  if (!c) return OMEGA_EINVAL;
  if (n_l < 0 || n_t < 0 || n_t > n_l) return fail(c, OMEGA_EINVAL, "need 0 <= n_t <= n_l");
  if ((n_l && !lufs_inst) || (n_t && !tp_db)) return fail(c, OMEGA_EINVAL, "null history");
  // rows older than the windows hold (integrated_len - 1 LUFS values, peak_len - 1 true peaks) leave no
  // trace in the state a replay of them would build: keep the last ones (a time-shard exchange hands over
  // up to 3599 / 59 rows whatever this context's window lengths are)
  if (n_l > c->HL) {
    lufs_inst += (n_l - c->HL) * (int64_t)c->cfg.n_channels;
    n_l = c->HL;
  }
  if (n_t > std::min<int64_t>(c->HT, n_l)) {
    const int64_t k = std::min<int64_t>(c->HT, n_l);
    tp_db += (n_t - k) * (int64_t)c->cfg.n_channels;
    n_t = k;
  }
  if (int e = check_device_err(c)) return e;
  HIPC(c, hipSetDevice(c->device));
  if (int e = flush_meters(c)) return e;  // (a pending segment reads the state being replaced)
  const int C = c->cfg.n_channels;
  const float* dl = lufs_inst;
  const float* dt = tp_db;
  if (mem == OMEGA_MEM_HOST) {  // (raw staging: a null history of no rows still gets its slot's pointer)
    int e = stage_in(c, 2, lufs_inst, (size_t)n_l * C * sizeof(float), reinterpret_cast<const void**>(&dl));
    if (!e) e = stage_in(c, 3, tp_db, (size_t)n_t * C * sizeof(float), reinterpret_cast<const void**>(&dt));
    if (e) return e;
  }
  // as omega_meter_update: after the side stream's last writes of the state, and before its next reads
  if (int e = main_after_side(c, 1)) return e;
  const int a = c->ms.cur;
  MeterLoadParams p{dl, dt, (int)n_l, (int)n_t, C, c->HL, c->HT, (float)c->cfg.gate_lufs, c->d_hist_l[a],
                    c->d_hist_t[a], c->d_nl[a], c->d_nt[a], c->d_skeys[a], c->d_ns[a], c->d_t0[a]};
  HIPC(c, launch_meter_load(p, c->stream));
  if (int e = side_after_main(c)) return e;
  if (mem == OMEGA_MEM_HOST) HIPC(c, hipStreamSynchronize(c->stream));
  return 0;
} catch (...) {
  return guard_fail(c);
}

int omega_calculate_lufs(omega_ctx* c, const float* x, int64_t n_frames, int32_t m, int32_t mode, int32_t oversampling,
                         float* lufs_inst, float* tp_db, double* meters, int mem) try {
  if (!c || !x || !meters) return OMEGA_EINVAL;
  if (n_frames <= 0) return n_frames == 0 ? 0 : fail(c, OMEGA_EINVAL, "negative count");
  if (int e = check_device_err(c)) return e;
  HIPC(c, hipSetDevice(c->device));
  const int64_t ncf = n_frames * c->cfg.n_channels;
  HostCall h(c, mem);  // (omega_process_frames' slots for the same data)
  const float* dx = h.in(x, (size_t)ncf * m * sizeof(float));
  float* dl = h.out(lufs_inst, ncf, 2);
  float* dt = h.out(tp_db, ncf);
  double* dm = h.out(meters, ncf * 5);
  if (h.err) return h.err;
  int e = 0;
  // device scratch for the instantaneous values the caller does not want back
  if (!dl || !dt) {
    if ((e = grow(c, &c->d_lufs_scr, &c->lufs_scr_cap, 2 * ncf))) return e;
    if (!dl) dl = c->d_lufs_scr;
    if (!dt) dt = c->d_lufs_scr + ncf;
  }
  if ((e = true_peak_check(c, m, oversampling))) return e;
  if ((e = weighting_check(c, m, mode))) return e;
  // The weighting and the true peak read the same input and write different outputs: the true peak
  // runs on the side stream beside the weighting's latency-bound float64 scans (per-call metering of
  // the app's 2048-sample frames: 37 + 14 us of kernels in sequence before). The aggregates read the
  // meter state, which a meter prep on the side stream may still be writing, and the true peaks.
  // Joining the side stream by an event costs ~5-10 us of idle GPU between kernels, so: when no meter
  // kernel went to the side stream since the last join (the app's steady state: nothing but these
  // calls; MeterSync::side) there is nothing to join before, and the true peaks (power-of-two frames,
  // direct launches) count themselves in on a device counter that the first meter prep polls before it
  // reads them; otherwise events, as omega_meter_update. Only an enqueued join clears the flag (step_join).
  const bool capture = c->cap && c->stream == c->cap;
  const bool counted = !capture && is_pow2_in(m, 512, 16384);
  unsigned* const count_to = counted ? c->d_ctr + kCtrLufsTp : nullptr;
  if (step_lufs_tp(c->ms, ncf, counted).join_side) {
    if ((e = main_after_side(c, 1))) return e;
    c->ms = step_join(c->ms).ok;
  }
  if ((e = side_after_main(c))) return e;
  if ((e = true_peak_dev(c, dx, ncf, m, oversampling, dt, side_stream(c), count_to))) return e;
  const SyncStep st = step_lufs_tp(c->ms, ncf, counted);  // (the true peaks are enqueued: they will count in)
  c->ms = st.ok;
  if ((e = weighting_dev(c, dx, ncf, m, mode, nullptr, dl, c->stream))) return e;
  if (!counted) {
    // the side stream's last work is the true peak, behind any earlier meter prep: one join serves
    // both (omega_meter_update's second wait is skipped)
    if ((e = main_after_side(c, 0))) return e;
    c->ms = step_join(c->ms).ok;
  }
  if ((e = flush_meters(c))) return e;
  // for a host-memory call the side stream is ordered after the copies back (no event between the
  // aggregates and the copies)
  const bool host = mem == OMEGA_MEM_HOST;
  if ((e = meter_update_dev(c, dl, dt, n_frames, dm, false, !host, count_to, st.wait_target))) return e;
  if (!host) return 0;
  if ((e = h.finish())) return e;
  return side_after_main(c);
} catch (...) {
  return guard_fail(c);
}

}  // extern "C"
