// The grid of one batch_kernel launch (BatchPlan, params.hpp) as a pure function of the call's shape:
// integer arithmetic only -- no context, no device, no HIP call -- so a plan can be evaluated, and a change
// to it stated, on the CPU (tests/test_batch_plan.py against tools/model/batch_plan_model.py). Host only:
// capi_batch.cpp enqueues what plan_batch lays out. The measured-and-rejected orders are recorded beside
// the decisions they belong to.
#pragma once

#include <algorithm>

#include "params.hpp"

namespace omega {

constexpr int kBatchWaves = 8;  // waves of a batch_kernel workgroup (rfkern.hip kBatchThreads / 64)
// meter workgroups of the batch grid at most: they wait (spinning) for the meter prep kernel, which
// may be dispatched after them and needs a CU with at most one batch workgroup resident (1024 threads
// and 72.6 KiB of LDS beside one 512-thread, 71.9 KiB batch workgroup). 64 waiting workgroups hold at
// most 64 of the 512 batch slots, so at least 192 CUs keep a slot that other roles free as they
// finish. (Round 1: one meter workgroup per 8 outputs of a 4096-frame batch took every slot and waited
// until the poll bound expired.)
#ifndef OMEGA_METER_WGS
#define OMEGA_METER_WGS 64  // (measured: 16 and 32 slower, profiles/r04_ab_meter_wgs.txt)
#endif
constexpr int kMeterWgs = OMEGA_METER_WGS;

// What the grid arithmetic reads of a call.
struct BatchShape {
  int64_t n_cf;  // channel-frames
  int n_res;
  struct {
    int n;        // FFT size
    bool wanted;  // it has an output (its magnitudes or the combined spectrum)
  } res[kMaxRes];
  int mr;  // the 16384-point resolution (it runs as role 2 of segment 0), or -1
  bool do_kw, do_tp;
  // the meter segment this launch runs: its workgroup count (unpipelined this call's own,
  // meter_segment_wgs; pipelined the pending one's, omega_ctx::pend_nq; 0: none) and whether it goes
  // before the small resolutions (pipelined) or last
  int q_n;
  bool q_before_multi;
};

constexpr int kPlanSegmentTooLarge = 1, kPlanGridTooLarge = 2;  // plan_batch: past INT32_MAX

// The workgroups of the meter segment over n_cf outputs: one wave per output, at most kMeterWgs.
inline int meter_segment_wgs(int64_t n_cf) {
  return (int)std::min<int64_t>((n_cf + kBatchWaves - 1) / kBatchWaves, kMeterWgs);
}

// A grid of nq meter workgroups and nothing else (a pending segment launched on its own).
inline BatchPlan plan_segment_only(int nq) {
  BatchPlan bp{};
  bp.q_begin = 0;
  bp.q_n = nq;
  bp.seg_start[0] = bp.seg_start[1] = bp.multi_start = nq;  // (no other workgroups)
  return bp;
}

// Every field of *bp but tail_ctr (a device pointer: the caller's), and the grid size. 0, or which of the
// two ends passed INT32_MAX (nothing is to be launched then).
inline int plan_batch(const BatchShape& sh, BatchPlan* out, int* grid_out) {
  const int64_t n = sh.n_cf;
  BatchPlan bp{};
  int seg[2][3], ns[2] = {0, 0};
  auto add = [&](int sg, int role, bool on) {
    if (on) seg[sg][ns[sg]++] = role;
  };
  // (measured: the true peaks in segment 0 beside the K-weighting, the 16384-point resolution in
  // segment 1, with or without the small resolutions before it: step 73.5-75.1 vs 68.8-70.5 us)
  // (measured, round 5, pipelined step on one box: the K-weighting beside the true peaks with the
  // 16384-point resolution after them, or the true peaks beside the 16384-point resolution with the
  // K-weighting after them, 65.3-67.3 us against 65.3-67.1 for this order: the same)
  add(0, 0, sh.do_kw);     // segment 0: K-weighting and the 16384-point resolution, groups of 8 frames
  add(0, 2, sh.mr >= 0);
  add(1, 1, sh.do_tp);     // segment 1: the true peaks
  const int64_t groups = (n + 7) / 8;
  int64_t end = 0;
  for (int sg = 0; sg < 2; ++sg) {
    bp.n_roles[sg] = ns[sg] ? ns[sg] : 1;
    for (int i = 0; i < 3; ++i) bp.roles[sg][i] = i < ns[sg] ? seg[sg][i] : 0;
    end += ns[sg] ? 8 * ns[sg] * groups : 0;
    if (end > 0x7FFFFFFF) return kPlanSegmentTooLarge;
    bp.seg_begin[sg + 1] = (int)end;
  }
  bp.mr_res = sh.mr < 0 ? 0 : sh.mr;
  int64_t nwg = 0;
  for (int r = 0; r < sh.n_res; ++r) {
    if (r == sh.mr || !sh.res[r].wanted) continue;
    const int K = sh.res[r].n / 2;
    const int G = K / 16 < 64 ? 64 : K / 16;  // threads_for<K>() for K <= 4096
    const int fpw = 512 / G;
    bp.multi.res[bp.multi.n_seg] = r;
    bp.multi.wg_begin[bp.multi.n_seg] = (int)nwg;
    ++bp.multi.n_seg;
    nwg += (n + fpw - 1) / fpw;
  }
  // grid order: segment 0 | segment 1 | small resolutions (measured: the small resolutions between the
  // segments, step 80.4-81.3 vs 76.6-77.5 us, round 4); segment 0 in the period-8 role order
  // (BatchPlan::pat: batch kernel 65.7-66.1 vs 70.9-71.5 us)
  bp.pat = 1;
  bp.multi_n = (int)nwg;
  bp.seg_start[0] = 0;
  bp.seg_start[1] = bp.seg_begin[1];
  bp.multi_start = bp.seg_begin[2];
  const int64_t body_end = end + nwg;
  // the grid's last segment unpipelined (measured: placed before the small resolutions it holds 64
  // slots from ~50 us on while it waits and the step is no shorter, 77.4-79.2 vs 77.0-78.0 us);
  // pipelined, it waits for nothing (first in the grid it delayed the true peaks: step 68-69 vs 64-65
  // us without meters)
  bp.q_begin = (int)body_end;
  bp.q_n = sh.q_n;
  // pipelined (the previous call's segment: it waits for nothing), the segment goes after the true peaks
  // and before the small resolutions instead: longest-first in the tail, its ~9-10 us workgroups ahead
  // of the 7-12 us resolution ones (pipelined step 63.5-64.4 vs 64.9-65.2 us last, four alternations on
  // one box, tools/ab.sh, outputs bitwise equal direct and pipelined; on a second box 62.8-64.7 vs
  // 64.6-65.1 last and 62.8-64.4 after the 8192-point resolution).
  // Unpipelined it stays last: before the small resolutions its waiting workgroups cost the in-call
  // step 70.4-73.1 vs 66.9-67.6 us
  if (sh.q_before_multi) bp.q_begin = bp.multi_start;
  // (measured, round 5: the pipelined segment between segment 0 and the true peaks instead, step
  // 65.3-67.1 vs 66.5-66.6 us on one box: no difference)
  const int64_t grid = body_end + sh.q_n;
  if (grid > 0x7FFFFFFF) return kPlanGridTooLarge;
  *out = bp;
  *grid_out = (int)grid;
  return 0;
}

}  // namespace omega
