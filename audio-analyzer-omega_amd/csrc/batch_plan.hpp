// The grid of one batch_kernel launch, both directions, as pure functions: plan_batch lays the workgroups
// of a call's shape out (BatchPlan), decode_block maps a blockIdx back to the work it does. Integer
// arithmetic only -- no context, no device memory, no HIP call -- so a plan and its decode can be evaluated,
// and a change to them stated, on the CPU (tests/test_batch_plan.py against tools/model/batch_plan_model.py).
// plan_batch and its helpers are host code: capi_batch.cpp enqueues what they lay out. decode_block and the
// pieces it is made of compile for host and device: rfkern.hip's batch_body runs the pieces, the CPU test
// runs decode_block. The measured-and-rejected orders are recorded beside the decisions they
// belong to.
#pragma once

#include "params.hpp"

namespace omega {

constexpr int kBatchThreads = 512;               // one batch_kernel workgroup
constexpr int kBatchWaves = kBatchThreads / 64;

// The thread group that transforms one frame of an at most 8192-point resolution (threads_for<K>() of
// fft.hpp for K = fft_size / 2 <= 4096; rfkern.hip batch_multi holds the two to each other): a workgroup
// of T threads runs T / small_res_group(fft_size) frames of it.
constexpr int small_res_group(int fft_size) { return fft_size / 32 < 64 ? 64 : fft_size / 32; }

// Segments of one mrfft_multi_kernel launch: resolution res[s] owns workgroups
// [wg_begin[s], wg_begin[s+1]) (the last one up to the grid end).
struct MultiPlan {
  int n_seg;
  int res[4];
  int wg_begin[4];
};

// One launch for the per-channel-frame work of a batch of 16384-sample frames (rfkern.hip
// batch_kernel), 512-thread workgroups. Roles: 0 K-weighting + LUFS_inst, 1 true peak, 2 the
// 16384-point resolution (mr_res). Two segments of role groups, the small resolutions (multi) and the
// meter segment [q_begin, q_begin + q_n); decode_block below is the map from a blockIdx to its work.
//   [seg_begin[s], seg_begin[s + 1])  the length of segment s: groups of 8 workgroups, one role and 8
//       consecutive channel-frames each, so the roles of a frame land on one XCD (blockIdx % 8). (The
//       hardware places an XCD's workgroups in blockIdx order round-robin over its 4 shader engines and
//       holds the next one until its engine has room, so with two roles each engine runs one role and
//       the engines of the short 16384-point-resolution workgroups idle ~5 us behind the K-weighting
//       ones: 80 % of the slot-time used, tools/wgtrace.py. Role chunks of one workgroup per CU fill
//       90 % of it, but the shader clock drops from ~2120 to ~1890 MHz and the launch takes longer: the
//       batch runs at the chip's power limit, so idle slots are not free time. DESIGN.md §8.)
//   pat: the group order of a two-role segment: 0 alternating groups (each shader engine runs one
//       role), 1 the period-8 order A B A B B A B A (seen by one XCD through blockIdx % 8, its engines
//       get the roles in turn, so an engine's short workgroups do not wait behind another's long
//       ones; the product's order, round 4: batch kernel 71.3 -> 65.9 us).
//   seg_start / multi_start / multi_n: where segment s and the small resolutions begin in the grid.
struct BatchPlan {
  int seg_begin[3];
  int n_roles[2];
  int roles[2][3];
  int mr_res;
  MultiPlan multi;
  int q_begin, q_n;
  unsigned* tail_ctr;  // (meter pipelining) the last workgroup adds 1 at its start: see host.hpp omega_ctx::d_tail
  int pat;
  int seg_start[2];
  int multi_start, multi_n;
};

// What one workgroup of the grid does.
enum BatchWorkKind : int {
  kBatchNothing,  // past every range
  kBatchMeter,    // workgroup `index` of the q_n of the meter segment
  kBatchRole,     // role `which` (0, 1, 2) of channel-frame `index`; in the last group of 8 it may be past n_cf
  kBatchSmallRes  // workgroup `index` of resolution `which`
};
struct BatchWork {
  int kind, which;
  int64_t index;
};

// blockIdx b of a grid laid out by plan_batch or plan_segment_only -> its work (decode_block): three range
// tests in this order, each answering "which of mine, or -1", and for the roles and the small resolutions
// the work of a block that passed its test. Only operations that mean the same on host and device.
// batch_body runs the same pieces in the same order, each test with its own early exit: called as one
// function there, the compiler keeps the merged result and dispatches on it a second time, which costs the
// kernel spilled SGPRs and a measurable part of its speed.

// the meter segment: workgroup q of q_n, or -1
__host__ __device__ __forceinline__ int meter_index(const BatchPlan& bp, int b) {
  return b >= bp.q_begin && b < bp.q_begin + bp.q_n ? b - bp.q_begin : -1;
}

// the role segment b lies in, or -1
__host__ __device__ __forceinline__ int role_segment(const BatchPlan& bp, int b) {
  const int len0 = bp.seg_begin[1], len1 = bp.seg_begin[2] - bp.seg_begin[1];
  return (b >= bp.seg_start[0] && b < bp.seg_start[0] + len0) ? 0
         : (b >= bp.seg_start[1] && b < bp.seg_start[1] + len1) ? 1 : -1;
}

// block b of role segment sg: role 0, 1 or 2 of a channel-frame (past n_cf in the last group of 8, perhaps)
__host__ __device__ __forceinline__ BatchWork role_work(const BatchPlan& bp, int sg, int b) {
  // workgroup j of the segment: group j / 8 of 8 channel-frames, frame j % 8 of it
  const int j = b - bp.seg_start[sg], nr = bp.n_roles[sg];
  int role;
  int64_t cf;
  if (nr == 2 && bp.pat == 1) {
    // period-8 group order A B A B B A B A (0x5A: the B positions); a group's index among its role's
    // groups = 4 per period + the same-role positions before it
    const int g = j >> 3, per = g & 7, rb = (0x5A >> per) & 1;
    role = bp.roles[sg][rb];
    const int idx = 4 * (g >> 3) + __builtin_popcount((rb ? 0x5A : 0xA5) & ((1 << per) - 1));
    cf = (int64_t)idx * 8 + (j & 7);
  } else {  // the roles in turn, group by group
    role = bp.roles[sg][(j >> 3) % nr];
    cf = (int64_t)(j / (8 * nr)) * 8 + (j & 7);
  }
  return {kBatchRole, role, cf};
}

// b's index among the small resolutions' workgroups, or -1
__host__ __device__ __forceinline__ int small_res_index(const BatchPlan& bp, int b) {
  // (the meter segment may sit before or inside the small resolutions: the workgroups after it shift by
  // q_n)
  const int w = b - bp.multi_start -
                (b >= bp.q_begin + bp.q_n && bp.q_begin < bp.multi_start + bp.multi_n ? bp.q_n : 0);
  return w < 0 || w >= bp.multi_n ? -1 : w;
}

// small-resolution workgroup w: which resolution's, and which of that resolution's
__host__ __device__ __forceinline__ BatchWork small_res_work(const BatchPlan& bp, int w) {
  const MultiPlan& mp = bp.multi;
  int s = 0;
  while (s + 1 < mp.n_seg && w >= mp.wg_begin[s + 1]) ++s;
  return {kBatchSmallRes, mp.res[s], w - mp.wg_begin[s]};
}

__host__ __device__ __forceinline__ BatchWork decode_block(const BatchPlan& bp, int b) {
  const int q = meter_index(bp, b);
  if (q >= 0) return {kBatchMeter, 0, q};
  const int sg = role_segment(bp, b);
  if (sg >= 0) return role_work(bp, sg, b);
  const int w = small_res_index(bp, b);
  if (w < 0) return {kBatchNothing, 0, 0};
  return small_res_work(bp, w);
}

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
  const int64_t wgs = (n_cf + kBatchWaves - 1) / kBatchWaves;
  return wgs < kMeterWgs ? (int)wgs : kMeterWgs;
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
    const int fpw = kBatchThreads / small_res_group(sh.res[r].n);
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
