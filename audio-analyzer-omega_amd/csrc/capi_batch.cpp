// libomega.so host side: the batch launch path -- omega_process_frames down to launch_batch, with the
// meter segments and the stream layout. (The entry points that measure level without the batch kernel
// are capi_level.cpp's; what both files use is in omega_host below, declared in host.hpp.) This file
// enqueues; the arithmetic is in two pure headers: batch_plan.hpp's plan_batch lays
// out the grid of a call's shape, and meter_sync.hpp's step functions give every counter target of a
// transition and the ledger (omega_ctx::ms) it leaves, on success and on a failed launch. enqueue_frames
// decides the call's shape once (batch layout, meters in the grid, pipelined, overlapped) and hands the
// batch to one of three enqueue functions: enqueue_batch_chunks (no meters, or a batch longer than
// kChunkFrames: meter query kernels), enqueue_batch_direct (this call's meter segment as the grid's last)
// and enqueue_batch_pipelined (the previous call's segment in the grid, this call's left pending). Each
// takes its step, copies the targets into the params, enqueues, and assigns one of the step's ledgers.

#include "batch_plan.hpp"
#include "host.hpp"

namespace omega_host __attribute__((visibility("hidden"))) {

constexpr int kChunkFrames = kMeterChunk;

int get_kw_tab(omega_ctx* c, int M, int L, BiquadTab** out) {
  return cached(c->kw_tabs, std::make_pair(M, L), out, [&](BiquadTab** d) {
    const double fs = c->cfg.sample_rate;
    const std::vector<BiquadTab> t = {make_biquad_tab(butter2(38.0, fs, true), L),
                                      make_biquad_tab(butter2(1500.0, fs, true), L)};
    return upload(c, d, t);
  });
}
int get_kw_tab(omega_ctx* c, int M, BiquadTab** out) { return get_kw_tab(c, M, kw_chunk(M), out); }

// True-peak kernel choice: the register-FFT kernel for 8192- and 16384-sample frames, the LDS-pass
// kernel for the other powers of two.
hipError_t tp_launch(int W, const SpectralParams& sp, hipStream_t s) {
  if (W == 16384 || W == 8192) return launch_truepeak_rf(W, sp, s);
  return launch_truepeak(W, sp, s);
}

SpectralParams spectral_params(omega_ctx* c) {
  SpectralParams p{};
  p.tp_phases = 0xE;
  p.C = c->cfg.n_channels;
  p.n_res = c->cfg.n_res;
  p.rf_sizes = c->rf_sizes;
  for (int r = 0; r < p.n_res; ++r) {
    ResParam& q = p.res[r];
    q.n = c->cfg.res[r].fft_size;
    q.offset = c->cfg.frame_size - q.n;
    q.win = c->d_win[r];
    q.wgt = c->d_wgt[r];
    q.ent_begin = c->ent_begin[r];
    q.ent_end = c->ent_end[r];
    q.cw = (float)c->cfg.res[r].weight;
    q.low_band = c->ent_jmax[r] < 256;
    q.pair_lo = c->pair_lo[r];
    q.pair_hi = c->pair_hi[r];
  }
  p.ent = c->d_ent;
  p.T = c->cfg.target_bins;
  p.rot = c->d_rot;
  for (int l = 0; l < kMaxLog2; ++l) p.tw[l] = c->d_tw[l];
  return p;
}

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// Meter aggregates over n_frames x C values go in chunks of at most kChunkFrames frames: their frame counts
std::vector<int64_t> chunk_frames(int64_t n_frames) {
  std::vector<int64_t> v;
  for (int64_t f0 = 0; f0 < n_frames; f0 += kChunkFrames) v.push_back(std::min<int64_t>(kChunkFrames, n_frames - f0));
  return v;
}

// The params of a step's chunks, consecutive in lufs / tp / out; each reads the state buffers of its
// parity and writes the other's.
std::vector<MeterPrepParams> meter_chunks(const omega_ctx* c, const std::vector<ChunkSync>& chunks, const float* lufs,
                                          const float* tp, double* out) {
  const int C = c->cfg.n_channels;
  std::vector<MeterPrepParams> v;
  int64_t f0 = 0;
  for (const ChunkSync& ch : chunks) {
    const int a = ch.par, b = ch.par ^ 1;
    MeterPrepParams p{};
    p.lufs = lufs + f0 * C;
    p.tp = tp + f0 * C;
    p.n_frames = ch.n_frames;
    p.C = C;
    p.hist_l_in = c->d_hist_l[a];
    p.hist_t_in = c->d_hist_t[a];
    p.n_l_in = c->d_nl[a];
    p.n_t_in = c->d_nt[a];
    p.skeys_in = c->d_skeys[a];
    p.n_s_in = c->d_ns[a];
    p.t0_in = c->d_t0[a];
    p.hist_l_out = c->d_hist_l[b];
    p.hist_t_out = c->d_hist_t[b];
    p.n_l_out = c->d_nl[b];
    p.n_t_out = c->d_nt[b];
    p.skeys_out = c->d_skeys[b];
    p.n_s_out = c->d_ns[b];
    p.t0_out = c->d_t0[b];
    p.HL = c->HL;
    p.HT = c->HT;
    p.mom_len = c->cfg.momentary_len;
    p.short_len = c->cfg.short_len;
    p.int_len = c->cfg.integrated_len;
    p.peak_len = c->cfg.peak_len;
    p.poll_limit = c->poll_limit;
    p.err_word = c->d_err;
    p.gate = (float)c->cfg.gate_lufs;
    p.core = c->d_core[a];
    p.ext = c->d_ext[a];
    p.n_core = c->d_ncore[a];
    p.n_ext = c->d_next[a];
    p.gcount = c->d_gcount[a];
    p.gsum = c->d_gsum[a];
    p.out = out + f0 * C * OMEGA_N_METERS;
    p.parts = 3;
    p.seg_ctr = c->d_ctr + kCtrSeg;
    p.seg_pre_target = ch.seg_pre_target;
    p.seg_post_target = ch.seg_post_target;
    v.push_back(p);
    f0 += ch.n_frames;
  }
  return v;
}

// Overlapped pipelined batches: order the last call's batch stream (batch, then meter segment) into the
// context's stream. (The call before it was joined when the last one was enqueued.)
int join_batches(omega_ctx* c) {
  if (!c->unjoined) return 0;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamWaitEvent(c->stream, c->ev_done[c->last_bs], 0));
  c->unjoined = false;
  c->prev_span.clear();
  return 0;
}

// Meter pipelining: the pending meter segment as a launch of its own on the context's stream (the
// stream of the batch it belongs to: omega_set_stream flushes before switching), or on `on` (an
// overlapped call's batch stream); an overlapped call still on its batch stream is joined first.
int flush_meters(omega_ctx* c, hipStream_t on) {
  if (!on)
    if (int e = join_batches(c)) return e;
  if (!c->ms.pend) return 0;
  HIPC(c, hipSetDevice(c->device));
  const SyncStep st = step_flush(c->ms);
  SpectralParams sp{};
  KWeightParams kp{};
  const hipError_t le = launch_batch(sp, kp, plan_segment_only(st.q_n), c->pend_mq, st.q_n, on ? on : c->stream);
  if (le != hipSuccess) {
    c->ms = st.fail;
    return fail(c, OMEGA_EHIP, "meter segment launch: %s", hipGetErrorString(le));
  }
  c->ms = st.ok;
  return 0;
}
}  // namespace omega_host

namespace {

// The signal-memory word of omega_ctx::d_tail, on first use (tail_ok: 1 ready, -1 no stream-wait-value
// support on this device).
int tail_init(omega_ctx* c) {
  if (c->tail_ok != 0) return 0;
  int ok = 0;
  HIPC(c, hipDeviceGetAttribute(&ok, hipDeviceAttributeCanUseStreamWaitValue, c->device));
  c->tail_ok = -1;
  if (ok && hipExtMallocWithFlags(reinterpret_cast<void**>(&c->d_tail), 8, hipMallocSignalMemory) == hipSuccess) {
    HIPC(c, hipMemset(c->d_tail, 0, 8));
    c->tail_ok = 1;
  }
  return 0;
}

// Layout 3 applies to 16384-sample frames on direct launches (a captured graph would freeze the
// kw_done target) when every requested stage has a 512-thread batch role: the register-FFT true peak,
// at most one 16384-point resolution (on the register FFT), the others at most 8192 points, and
// resolutions that commute (no combine target with several owners). *mr: the 16384-point resolution.
bool batch_eligible(omega_ctx* c, const SpectralParams& sp, const KWeightParams& kp, int W, bool do_res, hipStream_t s,
                    int* mr) {
  *mr = -1;
  if (W != 16384 || (c->cap && s == c->cap)) return false;  // (graph capture: the other layout)
  if ((kp.lufs_out || kp.weighted_out) && kp.mode != 0) return false;
  if (!do_res) return true;
  if (!c->res_independent) return false;
  for (int r = 0; r < sp.n_res; ++r) {
    if (!sp.comb_out && !sp.res[r].mag_out) continue;
    const int n = sp.res[r].n;
    if (n == 16384) {
      if (*mr >= 0 || !((sp.rf_sizes >> 14) & 1)) return false;
      *mr = r;
    } else if (n < 512 || n > 8192) {
      return false;
    }
  }
  return true;
}

// The default layout for 16384-sample frames. On `s`: one batch_kernel launch (plan_batch: K-weighting
// and 16384-point-resolution workgroups mixed, then the true peaks, then the small resolutions, then --
// for a batch of at most kChunkFrames frames per channel -- the meter aggregates as the grid's last
// segment; pipelined, the previous call's, between the true peaks and the small resolutions). On
// fork[0]: the meter prep (it waits on the K-weighting count, kw_done, and counts itself
// in). The meter workgroups wait for the prep's count and for the true peaks' count, so `s` completes
// only after fork[0]'s work: no stream events and no kernel after the batch (each event record / wait
// cost ~7-13 us of idle GPU between kernels). Longer batches (chunks chained through the per-context
// scratch) keep the meter query kernels: the LUFS query on fork[0] counting itself in, the true-peak
// query after the batch on `s` joining that count. Mixing the latency-bound K-weighting scans with
// transform work is what pays (K-weighting alone 25.7 us, the true peak 37, the resolutions 26.5; one
// batch launch of all three 73.9). Measured and rejected on MI355X (rounds 1-3): other role
// orders (K-weighting as its own kernel 110.4 us per step; mixed with the true peaks 85.2; the true
// peaks first ~equal; role chunks of one workgroup per CU), the meter queries after the batch (88 vs
// 81-82), the true-peak query on the side stream joined in the batch's last workgroup (85-87), the
// true-peak meter as a batch role (86-88), the true-peak meter by the batch's last true-peak workgroup,
// joined there (86.2 vs 81.1, round 3). The in-grid meter segment measured even with the query kernels
// (step 79.4-80.6 vs 79.0-79.4 us) at two fewer launches per call (host enqueue 13-17 vs 22-27 us).

// What plan_batch reads of the call; the meter segment (q_n, q_before_multi) is the enqueue function's.
BatchShape batch_shape(const SpectralParams& sp, int mr, bool do_tp, bool do_kw) {
  BatchShape sh{};
  sh.n_cf = sp.n_cf;
  sh.n_res = sp.n_res;
  for (int r = 0; r < sp.n_res; ++r) sh.res[r] = {sp.res[r].n, sp.comb_out || sp.res[r].mag_out};
  sh.mr = mr;
  sh.do_kw = do_kw;
  sh.do_tp = do_tp;
  return sh;
}

int plan_or_fail(omega_ctx* c, const BatchShape& sh, BatchPlan* bp, int* grid) {
  if (plan_batch(sh, bp, grid))
    return fail(c, OMEGA_EINVAL, "batch of %lld channel-frames too large", (long long)sh.n_cf);
  return 0;
}

// The batch without a meter segment: no meters, or a batch longer than kChunkFrames, whose chunks chain
// through the per-context scratch and keep the query kernels. Before the batch, per chunk on fork[0]: the
// prep (the first waits for the K-weighting count) and the LUFS query, counting itself in; the batch on
// `s`; behind it on `s` the true-peak queries, the last joining the LUFS queries' count.
int enqueue_batch_chunks(omega_ctx* c, const SpectralParams& sp, KWeightParams kp, const BatchShape& sh,
                         int64_t n_frames, const float* lufs, const float* tp, double* meters, hipStream_t s) {
  BatchPlan bp{};
  int grid = 0;
  if (int e = plan_or_fail(c, sh, &bp, &grid)) return e;
  // (no meters: no chunk, and the ledger stays)
  const SyncStep st = meters ? step_chunks(c->ms, sp.n_cf, sp.C, chunk_frames(n_frames)) : step_state_chunks(c->ms, {});
  const std::vector<MeterPrepParams> mc = meter_chunks(c, st.chunks, lufs, tp, meters);
  if (meters) {
    kp.kw_done = c->d_ctr + kCtrKw;
    for (size_t i = 0; i < mc.size(); ++i) {
      MeterPrepParams p = mc[i];
      if (i == 0) {
        p.wait_ctr = c->d_ctr + kCtrKw;
        p.wait_target = st.wait_target;
      }
      HIPC(c, launch_meter_prep(p, side_stream(c)));
      p.parts = 1;
      p.q_done = c->d_ctr + kCtrQuery;
      HIPC(c, launch_meter_query(p, side_stream(c)));
    }
  }
  if (grid > 0) {
    const hipError_t le = launch_batch(sp, kp, bp, MeterPrepParams{}, grid, s);
    if (le != hipSuccess) {
      c->ms = st.fail;
      // the prep kernel already waits for this batch's count: publish it, so that it (and every later
      // call's target) stays in step with the device counter instead of timing out
      if (meters) (void)hipMemcpy(c->d_ctr + kCtrKw, &c->ms.kw, sizeof(unsigned), hipMemcpyHostToDevice);
      return fail(c, OMEGA_EHIP, "batch launch: %s", hipGetErrorString(le));
    }
  }
  c->ms = st.ok;
  for (size_t i = 0; i < mc.size(); ++i) {
    MeterPrepParams p = mc[i];
    p.parts = 2;
    if (i + 1 == mc.size()) {
      p.join_ctr = c->d_ctr + kCtrQuery;
      p.join_target = st.join_target;
    }
    HIPC(c, launch_meter_query(p, s));
  }
  return 0;
}

// The meter aggregates of a one-chunk batch as the grid's last segment (batch_meter_role), this call's own:
// the prep kernel on fork[0] (it waits for the K-weighting count) counts itself in, the true-peak
// workgroups count themselves in, the meter workgroups wait for both. The prep goes before the batch: it
// must be resident while the batch runs (its segment waits for it).
int enqueue_batch_direct(omega_ctx* c, SpectralParams sp, KWeightParams kp, BatchShape sh, int64_t n_frames,
                         const float* lufs, const float* tp, double* meters, hipStream_t s) {
  const SyncStep st = step_direct(c->ms, sp.n_cf, sp.C);
  sh.q_n = st.q_n;
  sh.q_before_multi = false;
  BatchPlan bp{};
  int grid = 0;
  if (int e = plan_or_fail(c, sh, &bp, &grid)) return e;
  const MeterPrepParams m0 = meter_chunks(c, st.chunks, lufs, tp, meters)[0];
  // the prep on the side stream, waiting for this batch's K-weighting count
  MeterPrepParams p = m0;
  p.q_done = c->d_ctr + kCtrPrep;
  kp.kw_done = c->d_ctr + kCtrKw;
  p.wait_ctr = c->d_ctr + kCtrKw;
  p.wait_target = st.wait_target;
  HIPC(c, launch_meter_prep(p, side_stream(c)));
  MeterPrepParams mq = m0;
  mq.start_ctr = c->d_ctr + kCtrPrep;
  mq.start_target = st.start_target;
  // the meter segment's wait for the true peaks (each true-peak workgroup stores its value write-through
  // and counts in)
  sp.tp_done = c->d_ctr + kCtrTp;
  mq.join_ctr = c->d_ctr + kCtrTp;
  mq.join_target = st.join_target;
  const hipError_t le = launch_batch(sp, kp, bp, mq, grid, s);
  if (le != hipSuccess) {
    c->ms = st.fail;
    // the prep kernel already waits for this batch's count: publish it, so that it (and every later
    // call's target) stays in step with the device counter instead of timing out
    (void)hipMemcpy(c->d_ctr + kCtrKw, &c->ms.kw, sizeof(unsigned), hipMemcpyHostToDevice);
    return fail(c, OMEGA_EHIP, "batch launch: %s", hipGetErrorString(le));
  }
  c->ms = st.ok;
  return 0;
}

// Meter pipelining: this launch runs the PREVIOUS call's meter segment in its grid (its inputs are
// complete: that batch ended before this one starts, so it waits for nothing) and leaves its own
// pending. The prep that reads this batch's values runs beside it on the side stream: it polls
// generation-tagged words the K-weighting workgroups store without a drain or a count,
// and goes AFTER the batch, behind the stream wait for the grid's last workgroup -- enqueued before the
// batch, a wait whose stream shared a hardware queue with the batch's would block the batch behind it
// for ever. `s`: the caller's stream, or an overlapped call's batch stream (nothing is pending there:
// enqueue_frames launches each call's segment behind its batch).
int enqueue_batch_pipelined(omega_ctx* c, const SpectralParams& sp, KWeightParams kp, BatchShape sh,
                            int64_t n_frames, const float* lufs, const float* tp, double* meters, hipStream_t s) {
  // first use: the mirror words and the tail word
  const size_t mir_n = (size_t)kChunkFrames * c->cfg.n_channels;
  if (!c->d_mirror) {
    HIPC(c, hipMalloc(&c->d_mirror, 2 * mir_n * sizeof(unsigned long long)));
    HIPC(c, hipMemset(c->d_mirror, 0, 2 * mir_n * sizeof(unsigned long long)));
  }
  if (int e = tail_init(c)) return e;
  const bool tail = c->tail_ok > 0;
  const SyncStep st = step_pipelined(c->ms, sp.n_cf, sp.C, tail);
  sh.q_n = st.q_n;
  sh.q_before_multi = true;
  BatchPlan bp{};
  int grid = 0;
  if (int e = plan_or_fail(c, sh, &bp, &grid)) return e;
  const MeterPrepParams m0 = meter_chunks(c, st.chunks, lufs, tp, meters)[0];
  MeterPrepParams p = m0;
  p.q_done = c->d_ctr + kCtrPrep;
  // consecutive launches alternate parity: a prep still reading one parity while the next launch's
  // K-weighting writes the other (it waits for nothing), and done before the launch after that
  // (whose predecessor's segment waits for it)
  kp.lufs_mirror = c->d_mirror + (st.mirror_gen & 1) * mir_n;
  kp.mirror_gen = st.mirror_gen;
  p.lufs_mirror = kp.lufs_mirror;
  p.mirror_gen = st.mirror_gen;
  if (tail) bp.tail_ctr = c->d_tail;
  // this call's segment, for the launch that runs it: it starts once the prep has counted in (its batch
  // has ended by then: no wait for the true peaks)
  MeterPrepParams mq = m0;
  mq.start_ctr = c->d_ctr + kCtrPrep;
  mq.start_target = st.start_target;
  const hipError_t le = launch_batch(sp, kp, bp, c->pend_mq, grid, s);
  if (le != hipSuccess) {
    // (no prep waits for this launch: nothing was enqueued, the pending segment stays pending and the
    // next launch takes this one's generation and parities)
    c->ms = st.fail;
    return fail(c, OMEGA_EHIP, "batch launch: %s", hipGetErrorString(le));
  }
  c->ms = st.launched;
  if (tail) {
    HIPC(c, hipStreamWaitValue32(side_stream(c), c->d_tail, st.tail_target, hipStreamWaitValueGte, 0xFFFFFFFFu));
    c->ms = st.waited;
  }
  HIPC(c, launch_meter_prep(p, side_stream(c)));
  c->ms = st.ok;
  c->pend_mq = mq;
  return 0;
}

// The per-batch work: layout 3 (the enqueue_batch_* functions) where eligible, otherwise the full-chip
// kernels back to back on `s` (K-weighting first); the meter aggregates' prep and LUFS query kernels (one or two
// workgroups per channel: latency-bound) run on fork[0] beside the resolution and true-peak kernels,
// the true-peak meter after the true peaks on `s`. (Concurrent full-chip kernels lose to this: 512
// channel-frames are exactly two rounds of 256 CUs, and a CU held by another kernel pushes a third.)
// lufs_st / tp_st: the context's staging slots of a pipelined call with meters (omega_process_frames).
int enqueue_frames(omega_ctx* c, SpectralParams sp, KWeightParams kp, int W, int64_t n_frames, const float* lufs,
                   const float* tp, double* meters, hipStream_t s, bool pipe = false, float* lufs_st = nullptr,
                   float* tp_st = nullptr, bool serial = false) {
  const bool do_tp = sp.tp_out != nullptr, do_kw = kp.lufs_out || kp.weighted_out;
  const bool do_res = sp.comb_out != nullptr || sp.res[0].mag_out || sp.res[1].mag_out || sp.res[2].mag_out ||
                      sp.res[3].mag_out;
  int mr = -1;
  const bool batch = c->layout == 3 && batch_eligible(c, sp, kp, W, do_res, s, &mr);
  // the meter aggregates in the batch's grid: a one-chunk batch with both of their inputs
  const bool in_grid = batch && meters && do_tp && do_kw && n_frames > 0 && n_frames <= kChunkFrames;
  // a pending meter segment goes first: folded into this batch's launch when it has an in-grid meter
  // segment of its own, else on its own
  const bool fold = pipe && in_grid;
  const BatchShape sh = batch ? batch_shape(sp, mr, do_tp, do_kw) : BatchShape{};
  // overlapped (omega_ctx::bs): the batch and, behind it, its own meter segment on a batch stream
  if (fold && c->bs[0])
    if (int e = tail_init(c)) return e;
  const bool ovl = fold && c->bs[0] && c->tail_ok > 0;
  if ((c->ms.pend && (!fold || ovl)) || (c->unjoined && !ovl))
    if (int e = flush_meters(c)) return e;
  if (fold && lufs_st && tp_st) {
    // the segment and the prep read the staging slots; the caller's buffers get copies
    if (kp.lufs_out != lufs_st) kp.lufs_copy = kp.lufs_out;
    if (sp.tp_out != tp_st) sp.tp_copy = sp.tp_out;
    kp.lufs_out = lufs_st;
    sp.tp_out = tp_st;
    lufs = lufs_st;
    tp = tp_st;
  }
  if (ovl) {
    const int k = (int)(c->bs_idx & 1);
    hipStream_t b = c->bs[k];
    // serial: this call touches memory the unjoined call reads or writes -- that one first
    if (serial)
      if (int e = join_batches(c)) return e;
    // the input dependency: what the caller enqueued so far, before anything of this call
    HIPC(c, hipEventRecord(c->ev_in, s));
    HIPC(c, hipStreamWaitEvent(b, c->ev_in, 0));
    // the gate: batch i starts placing workgroups once batch i - 1 has none left to place (its
    // last-dispatched workgroup has bumped the tail count) and fills the slots its drain frees. The
    // wait follows the launch it waits for (the previous call's): shared hardware queues serialise
    if (c->ms.tail)
      HIPC(c, hipStreamWaitValue32(b, c->d_tail, c->ms.tail, hipStreamWaitValueGte, 0xFFFFFFFFu));
    const int err = [&]() -> int {
      if (int e = enqueue_batch_pipelined(c, sp, kp, sh, n_frames, lufs, tp, meters, b)) return e;
      // this call's meter segment, a launch of its own behind its batch: it polls the prep's count (the
      // prep is enqueued: fork[0], behind the tail wait) and runs beside the next call's batch. Segments
      // run in call order (each reads the true-peak history the one before rolled)
      if (c->unjoined) HIPC(c, hipStreamWaitEvent(b, c->ev_done[k ^ 1], 0));
      if (int e = flush_meters(c, b)) return e;
      HIPC(c, hipEventRecord(c->ev_done[k], b));
      // the deferred join: the caller's stream waits for the PREVIOUS call here, for this one in the
      // next call (or a flush), so the next call's input dependency does not hold this batch's drain
      if (c->unjoined) HIPC(c, hipStreamWaitEvent(s, c->ev_done[k ^ 1], 0));
      return 0;
    }();
    if (err) {
      // a step failed, possibly with the batch already on its stream: order whatever runs on both batch
      // streams into the caller's stream now (a segment left pending is then launched there, behind
      // its batch, by the next flush) and leave nothing unjoined
      (void)hipEventRecord(c->ev_done[k], b);
      if (c->unjoined) (void)hipStreamWaitEvent(s, c->ev_done[k ^ 1], 0);
      (void)hipStreamWaitEvent(s, c->ev_done[k], 0);
      c->unjoined = false;
      c->prev_span.clear();
      return err;
    }
    c->unjoined = true;
    c->last_bs = k;
    ++c->bs_idx;
    return 0;
  }
  if (fold) return enqueue_batch_pipelined(c, sp, kp, sh, n_frames, lufs, tp, meters, s);
  if (in_grid) return enqueue_batch_direct(c, sp, kp, sh, n_frames, lufs, tp, meters, s);
  if (batch) return enqueue_batch_chunks(c, sp, kp, sh, n_frames, lufs, tp, meters, s);
  if (do_kw) HIPC(c, launch_kweight(W, kp, s));
  std::vector<MeterPrepParams> mc;
  if (meters) {
    const SyncStep st = step_state_chunks(c->ms, chunk_frames(n_frames), true);
    // (a graph capture runs nothing: the chunks' step is omega_process_frames', at each replay; the flag is set)
    c->ms = c->cap && s == c->cap ? step_state_chunks(c->ms, {}, true).ok : st.ok;
    mc = meter_chunks(c, st.chunks, lufs, tp, meters);
    HIPC(c, hipEventRecord(c->ev_kw, s));
    HIPC(c, hipStreamWaitEvent(side_stream(c), c->ev_kw, 0));
    for (MeterPrepParams p : mc) {
      HIPC(c, launch_meter_prep(p, side_stream(c)));
      p.parts = 1;
      HIPC(c, launch_meter_query(p, side_stream(c)));
    }
    if (int e = side_join_record(c, 0)) return e;
  }
  if (do_res) HIPC(c, c->res_independent ? launch_mrfft_independent(sp, s) : launch_mrfft(sp, s));
  if (do_tp) HIPC(c, tp_launch(W, sp, s));
  for (MeterPrepParams p : mc) {
    p.parts = 2;
    HIPC(c, launch_meter_query(p, s));
  }
  if (meters) return side_join_wait(c, 0, s);  // (the flag stays: the next counted omega_calculate_lufs joins again)
  return 0;
}

}  // namespace

extern "C" {

#ifdef OMEGA_STAMPS
// Development build only (make dev): one kernel variant over n_cf channel-frames of the context's
// frames x (device memory, frame stride W, channel stride W * ... as omega_process_frames with
// frame_stride = C * W, channel_stride = W), outputs to device buffers. which: 0 the 16384-point
// resolution kernel, 2 the true-peak kernel (aux: [n_cf] true peaks), 3 the same at one workgroup per
// CU (dynamic LDS padded past half the CU's 160 KiB). (Two frames per workgroup
// through one exchange buffer -- the 16384-point resolution interleaved, and a true peak with its
// spectrum parked in L2 between phases -- measured no faster at 8192 channel-frames (true peak 614 vs
// 621 us at a shader clock of 1773 vs 1897 MHz): the extra frames in flight bought activity and the
// clock gave it back; both were deleted.)
int omega_dev_probe(omega_ctx* c, int which, const float* x, int64_t n_frames, float* comb, float* aux) {
  SpectralParams sp = spectral_params(c);
  const int W = c->cfg.frame_size;
  sp.x = x;
  sp.frame_stride = (int64_t)c->cfg.n_channels * W;
  sp.chan_stride = W;
  sp.n_cf = n_frames * c->cfg.n_channels;
  sp.comb_out = comb;
  (void)aux;
  for (int r = 0; r < kMaxRes; ++r) sp.res[r].mag_out = nullptr;
  hipError_t e = hipErrorInvalidValue;
  sp.tp_out = aux;
  float2* rot = nullptr;
  if (int r = get_rot(c, W, &rot)) return r;
  sp.rot = rot;
  if (which == 0) e = launch_mrfft_rf(16384, sp, 0, c->stream);
  if (which == 2) e = launch_truepeak_rf(16384, sp, c->stream);
  // 3: the true-peak kernel at one workgroup per CU (extra dynamic LDS), the occupancy probe
  if (which == 3) e = launch_truepeak_rf(16384, sp, c->stream, 16 * 1024);
  return e == hipSuccess ? 0 : fail(c, OMEGA_EHIP, "probe %d: %s", which, hipGetErrorString(e));
}
#endif

int omega_process_frames(omega_ctx* c, const float* x, int64_t n_frames, int64_t frame_stride, int64_t channel_stride,
                         const omega_outputs* out, int mem) try {
  if (!c || !out) return OMEGA_EINVAL;
  if (!x || n_frames < 0) return fail(c, OMEGA_EINVAL, "null input or negative frame count");
  if (int e = check_device_err(c)) return e;
  if (n_frames == 0) return 0;
  const int C = c->cfg.n_channels, W = c->cfg.frame_size, T = c->cfg.target_bins;
  const int64_t ncf = n_frames * C;
  if ((frame_stride & 1) || (channel_stride & 1))
    return fail(c, OMEGA_EINVAL, "frame_stride and channel_stride must be even (8-byte aligned frames)");
  if (ncf > 0x7FFFFFFF) return fail(c, OMEGA_EINVAL, "too many channel-frames");
  HIPC(c, hipSetDevice(c->device));
  // meter pipelining applies to direct device-memory calls; any other call runs a pending meter
  // segment first (before its staging buffers are touched)
  const bool pipe = c->pipe && mem == OMEGA_MEM_DEVICE && !c->use_graph;
  if (!pipe)
    if (int e = flush_meters(c)) return e;
  SpectralParams sp = spectral_params(c);
  sp.frame_stride = frame_stride;
  sp.chan_stride = channel_stride;
  sp.n_cf = ncf;
  float* mags[kMaxRes] = {};
  const size_t span = (size_t)((n_frames - 1) * frame_stride + (C - 1) * channel_stride + W);
  // when every kernel of a host-memory call only stores its outputs, small ones go straight to page-locked
  // memory: not with meters (the meter path's true peaks are re-read across workgroups) nor with combine
  // targets owned by several resolutions (their o[t] += v reads back across kernels): device staging
  if (mem == OMEGA_MEM_HOST) c->zc_ok = !out->meters && (!out->combined || c->res_independent);
  HostCall h(c, mem);
  const float* dx = h.in(x, span * sizeof(float));
  float* comb = h.out(out->combined, ncf * T);
  float* lufs = h.out(out->lufs_inst, ncf);
  float* tp = h.out(out->true_peak_db, ncf);
  double* meters = h.out(out->meters, ncf * 5);
  float* weighted = h.out(out->weighted, ncf * W);
  for (int r = 0; r < c->cfg.n_res; ++r) mags[r] = h.out(out->mag[r], ncf * (c->cfg.res[r].fft_size / 2 + 1));
  if (h.err) return h.err;
  if (mem != OMEGA_MEM_HOST && !aligned8(x)) return fail(c, OMEGA_EINVAL, "input must be 8-byte aligned");
  int e = 0;
  // meters need the instantaneous values even when the caller does not ask for them. Pipelined, the
  // meter prep and the deferred meter segment read them during the next call, so they read the
  // context's staging slots (two sets in turn) and never the caller's buffers, which the next call may
  // overwrite (the usual preallocated outputs): enqueue_frames points the batch's K-weighting and
  // true-peak roles at the slots and hands them the caller's buffers as copies.
  const int sl = pipe ? 2 * c->stage_par : 0;
  if (pipe && meters) c->stage_par ^= 1;
  float* lufs_st = nullptr;
  float* tp_st = nullptr;
  if (meters && (pipe || !lufs)) {
    e = stage_buf(c, 10 + sl, ncf * sizeof(float), reinterpret_cast<void**>(&lufs_st));
    if (e) return e;
    if (!lufs) lufs = lufs_st;
  }
  if (meters && (pipe || !tp)) {
    e = stage_buf(c, 11 + sl, ncf * sizeof(float), reinterpret_cast<void**>(&tp_st));
    if (e) return e;
    if (!tp) tp = tp_st;
  }
  sp.x = dx;
  sp.comb_out = comb;
  sp.tp_out = tp;
  for (int r = 0; r < c->cfg.n_res; ++r) sp.res[r].mag_out = mags[r];
  BiquadTab* tabs = nullptr;
  if (lufs || weighted) {
    e = get_kw_tab(c, W, &tabs);
    if (e) return e;
  }
  KWeightParams kp{dx, frame_stride, channel_stride, C, ncf, tabs, tabs ? tabs + 1 : nullptr, lufs, weighted, 0};
  if (mem == OMEGA_MEM_DEVICE && c->use_graph) {
    // replay a captured graph of this exact call (pointers, sizes, meter-state parity), capturing it on
    // first use: removes the per-launch host cost and runs the three branches concurrently
    const std::vector<uint64_t> key = {(uint64_t)dx, (uint64_t)n_frames, (uint64_t)frame_stride,
                                       (uint64_t)channel_stride, (uint64_t)comb, (uint64_t)lufs, (uint64_t)tp,
                                       (uint64_t)meters, (uint64_t)weighted, (uint64_t)mags[0], (uint64_t)mags[1],
                                       (uint64_t)mags[2], (uint64_t)mags[3], (uint64_t)c->ms.cur};
    hipGraphExec_t exec = nullptr;
    for (auto& g : c->graphs)
      if (g.key == key) exec = g.exec;
    if (!exec) {
      if (c->graphs.size() >= 16) drop_graphs(c);
      if (!c->cap) HIPC(c, hipStreamCreateWithFlags(&c->cap, hipStreamNonBlocking));
      HIPC(c, hipStreamBeginCapture(c->cap, hipStreamCaptureModeThreadLocal));
      e = enqueue_frames(c, sp, kp, W, n_frames, lufs, tp, meters, c->cap);
      hipGraph_t graph = nullptr;
      const hipError_t ce = hipStreamEndCapture(c->cap, &graph);
      if (e) return e;
      if (ce != hipSuccess) return fail(c, OMEGA_EHIP, "graph capture: %s", hipGetErrorString(ce));
      HIPC(c, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      c->graphs.push_back({key, graph, exec});
    }
    HIPC(c, hipGraphLaunch(exec, c->stream));
    if (meters) c->ms = step_state_chunks(c->ms, chunk_frames(n_frames)).ok;  // (the captured call's step)
    return 0;
  }
  // overlapped pipelined calls: what this call reads ([0]) and writes; one that touches what the call
  // still on its batch stream writes, or writes what that one reads, waits for it (two overlapped
  // launches never write the same bytes, and an output passed on as input is complete)
  std::vector<std::pair<const char*, size_t>> span_now;
  bool serial = false;
  if (pipe) {
    auto add = [&](const void* p, size_t bytes) {
      if (p) span_now.emplace_back(static_cast<const char*>(p), bytes);
    };
    span_now.emplace_back(reinterpret_cast<const char*>(x), span * sizeof(float));
    add(comb, (size_t)ncf * T * sizeof(float));
    add(out->lufs_inst, (size_t)ncf * sizeof(float));
    add(out->true_peak_db, (size_t)ncf * sizeof(float));
    add(meters, (size_t)ncf * OMEGA_N_METERS * sizeof(double));
    add(weighted, (size_t)ncf * W * sizeof(float));
    for (int r = 0; r < c->cfg.n_res; ++r) add(mags[r], (size_t)ncf * (c->cfg.res[r].fft_size / 2 + 1) * sizeof(float));
    if (c->unjoined)
      for (size_t i = 0; i < span_now.size() && !serial; ++i)
        for (size_t j = 0; j < c->prev_span.size() && !serial; ++j)
          serial = (i || j) && span_now[i].first < c->prev_span[j].first + c->prev_span[j].second &&
                   c->prev_span[j].first < span_now[i].first + span_now[i].second;
  }
  e = enqueue_frames(c, sp, kp, W, n_frames, lufs, tp, meters, c->stream, pipe, lufs_st, tp_st, serial);
  if (e) {
    if (pipe && meters) c->stage_par ^= 1;  // (a still-pending segment reads the slots of the other parity)
    return e;
  }
  if (c->unjoined) c->prev_span.swap(span_now);
  return h.finish();
} catch (...) {
  return guard_fail(c);
}

int omega_flush_meters(omega_ctx* c) try {
  if (!c) return OMEGA_EINVAL;
  if (!c->ms.pend && !c->unjoined) return 0;
  HIPC(c, hipSetDevice(c->device));
  return flush_meters(c);
} catch (...) {
  return guard_fail(c);
}

int omega_process_stream(omega_ctx* c, const float* x, int64_t n_samples, int32_t hop, int64_t channel_stride,
                         const omega_outputs* out, int mem, int64_t* n_frames_out) try {
  if (!c) return OMEGA_EINVAL;
  if (n_frames_out) *n_frames_out = 0;
  if (hop < 1 || n_samples < 0) return fail(c, OMEGA_EINVAL, "hop must be >= 1 and n_samples >= 0");
  const int W = c->cfg.frame_size;
  const int64_t nf = n_samples < W ? 0 : (n_samples - W) / hop + 1;
  if (n_frames_out) *n_frames_out = nf;
  return omega_process_frames(c, x, nf, hop, channel_stride, out, mem);
} catch (...) {
  return guard_fail(c);
}
}  // extern "C"
