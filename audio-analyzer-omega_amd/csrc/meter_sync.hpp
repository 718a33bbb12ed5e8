// The meter pipeline's ledger, host only: the device counter words by name, the host's running counts
// of what was launched to count into them, and one pure function per transition -- ledger and the call's
// integers in; the targets the enqueue code writes into MeterPrepParams / KWeightParams / SpectralParams
// and the stream wait, and the ledger after each outcome, out. No HIP call and no pointer: the enqueue
// functions of capi_batch.cpp and capi_level.cpp assign one of the returned ledgers to omega_ctx::ms and
// touch the state in no other way. tools/model/meter_sync_model.py states the same rules independently and
// tests/test_meter_sync.py holds this header to it (tests/abi/meter_sync_dump.cpp), failure branches and
// 2^32 wrap-around included. The table of who adds and who waits: DESIGN.md §4, "The meter counters".
//
// All counts are unsigned and wrap; the device compares (int)(word - target) >= 0.
//
// Which ledger a path is left with (the enqueue functions assign, the rules are here):
//   - a step whose batch launch fails gets `fail`: the ledger that came in (pipelined, flush), kw and prep
//     advanced with the parity flipped (direct: the prep is enqueued and will count in), everything
//     advanced (chunks); direct and chunks then publish kw to the device word, which the prep waits for;
//   - a HIP call that fails BEFORE the batch launch leaves the ledger that came in;
//   - after a successful pipelined launch the tail wait and the prep launch can still fail: `launched`
//     (the parity flipped, seg_par of the segment the grid ran, the generation) resp. `waited` (and the
//     tail count) stay, with the segment still marked pending -- as before this header, no recovery;
//   - on the chunk paths everything is advanced once the step is taken, whichever later launch fails;
//   - `side` (a meter kernel went to the side stream and the caller's stream has not joined it since) is
//     set in every ledger of a step that enqueues a prep or a LUFS query there -- chunks, direct, the
//     back-to-back layout: ok and fail; pipelined: launched, waited and ok, not fail (nothing has reached
//     the side stream) -- and cleared by step_join alone, which the enqueue code assigns once the event
//     record and the stream wait of a join have both succeeded: a call that fails before leaves it set.
#pragma once

#include <cstdint>
#include <vector>

#include "batch_plan.hpp"  // meter_segment_wgs

namespace omega_host __attribute__((visibility("hidden"))) {

// The words of omega_ctx::d_ctr. Who counts in: K-weighting workgroups of a batch with the count on;
// LUFS-meter query workgroups (one per 4 frames x channel); batch true-peak workgroups with the count on;
// meter prep workgroups (one per channel) that a segment waits for; meter-segment workgroups, when their
// reads are done; omega_calculate_lufs' true-peak workgroups.
enum MeterCounter { kCtrKw = 0, kCtrQuery, kCtrTp, kCtrPrep, kCtrSeg, kCtrLufsTp, kCtrWords = 8 };

struct MeterSync {
  unsigned kw = 0, query = 0, tp = 0, prep = 0, seg = 0, lufs_tp = 0;  // launched to count in, per word
  // `seg` once the last segment reading parity p's scratch / state has counted in: what a prep waits
  // for before it overwrites them (MeterPrepParams::seg_pre_target / seg_post_target)
  unsigned seg_par[2] = {0, 0};
  int cur = 0;  // parity of the current meter state
  // the meter segment of the last pipelined batch, not yet launched: its workgroups and its parity
  bool pend = false;
  int pend_nq = 0, pend_par = 0;
  unsigned mirror_gen = 0;  // generation tag of the last pipelined launch's LUFS mirror (never 0 once used)
  unsigned tail = 0;        // pipelined launches whose last workgroup bumps omega_ctx::d_tail
  bool side = false;        // a meter kernel was enqueued on the side stream since the caller's stream last joined it
};

// One meter chunk: it reads the state and scratch of parity `par` and writes `par ^ 1`.
struct ChunkSync {
  int64_t n_frames;
  int par;
  unsigned seg_pre_target, seg_post_target;
};

struct SyncStep {
  std::vector<ChunkSync> chunks;
  unsigned wait_target = 0;   // the first prep's: kw (chunks, direct) or lufs_tp
  unsigned start_target = 0;  // the segment's, on prep (direct, pipelined)
  unsigned join_target = 0;   // the segment's on tp (direct); the last true-peak query's on query (chunks)
  unsigned tail_target = 0;   // the side stream's wait on d_tail (pipelined with the tail)
  unsigned mirror_gen = 0;    // this launch's generation; the mirror's parity is mirror_gen & 1 (pipelined)
  int q_n = 0;                // segment workgroups this launch runs: its own (direct), the pending one's
  bool join_side = false;     // the caller's stream joins the side stream before the aggregates (lufs_tp)
  MeterSync ok, fail;
  MeterSync launched, waited;  // pipelined only (see the file comment)
};

// The one parity rule: a chunk reads parity a = cur and writes a ^ 1, waits for the segments that read
// either, and cur flips.
inline ChunkSync take_chunk(MeterSync& s, int64_t n_frames) {
  const int a = s.cur;
  s.cur = a ^ 1;
  return {n_frames, a, s.seg_par[a], s.seg_par[a ^ 1]};
}

// Chunks that touch no counter: the back-to-back layout (on_side: its preps and LUFS queries go to the side
// stream), meters_enqueue, a graph replay (both on the caller's stream). `frames`: the frame count of each
// chunk.
inline SyncStep step_state_chunks(const MeterSync& m, const std::vector<int64_t>& frames, bool on_side = false) {
  SyncStep r;
  MeterSync s = m;
  s.side = s.side || on_side;
  for (int64_t f : frames) r.chunks.push_back(take_chunk(s, f));
  r.ok = r.fail = s;
  return r;
}

// A batch with query kernels: n_cf K-weighting workgroups count in, the first prep waits for them; every
// chunk's LUFS query counts in, the last chunk's true-peak query joins them.
inline SyncStep step_chunks(const MeterSync& m, int64_t n_cf, int C, const std::vector<int64_t>& frames) {
  SyncStep r = step_state_chunks(m, frames, !frames.empty());
  MeterSync s = r.ok;
  s.kw += (unsigned)n_cf;
  r.wait_target = s.kw;
  for (int64_t f : frames) s.query += (unsigned)(((f + 3) / 4) * C);
  r.join_target = s.query;
  r.ok = r.fail = s;
  return r;
}

// A one-chunk batch with its own meter segment last in the grid.
inline SyncStep step_direct(const MeterSync& m, int64_t n_cf, int C) {
  SyncStep r;
  MeterSync s = m;
  r.chunks.push_back(take_chunk(s, n_cf / C));
  r.q_n = omega::meter_segment_wgs(n_cf);
  s.side = true;  // (the prep goes before the batch launch)
  s.kw += (unsigned)n_cf;
  r.wait_target = s.kw;
  s.prep += (unsigned)C;
  r.start_target = s.prep;
  r.join_target = s.tp + (unsigned)n_cf;
  r.fail = s;
  s.tp += (unsigned)n_cf;
  s.seg_par[r.chunks[0].par] = s.seg + (unsigned)r.q_n;
  s.seg += (unsigned)r.q_n;
  r.ok = s;
  return r;
}

// A one-chunk batch that runs the pending segment in its grid and leaves its own pending. tail: the side
// stream waits for the grid's last workgroup before the prep.
inline SyncStep step_pipelined(const MeterSync& m, int64_t n_cf, int C, bool tail) {
  SyncStep r;
  r.fail = m;
  MeterSync s = m;
  r.q_n = m.pend ? m.pend_nq : 0;
  // the pending segment is enqueued by this launch: the chunk's targets count it
  if (m.pend) s.seg_par[m.pend_par] = s.seg + (unsigned)m.pend_nq;
  r.chunks.push_back(take_chunk(s, n_cf / C));
  s.mirror_gen = s.mirror_gen == 0xFFFFFFFFu ? 2u : s.mirror_gen + 1;  // (never 0, and the parity alternates)
  r.mirror_gen = s.mirror_gen;
  r.start_target = s.prep + (unsigned)C;
  r.tail_target = s.tail + 1;
  s.side = true;  // (from the launch on: the tail wait and the prep follow it on the side stream)
  r.launched = s;
  if (tail) s.tail += 1;
  r.waited = s;
  s.prep += (unsigned)C;
  s.seg += (unsigned)r.q_n;
  s.pend = true;
  s.pend_nq = omega::meter_segment_wgs(n_cf);
  s.pend_par = r.chunks[0].par;
  r.ok = s;
  return r;
}

// The pending segment as a launch of its own (nothing pending: nothing changes, q_n = 0).
inline SyncStep step_flush(const MeterSync& m) {
  SyncStep r;
  r.ok = r.fail = m;
  if (!m.pend) return r;
  r.q_n = m.pend_nq;
  r.ok.seg_par[m.pend_par] = m.seg + (unsigned)m.pend_nq;
  r.ok.seg += (unsigned)m.pend_nq;
  r.ok.pend = false;
  return r;
}

// omega_calculate_lufs' true peaks on the side stream. counted: n_cf workgroups count in and the first prep
// waits for them instead of an event join -- sound only while no meter kernel is on the side stream, so
// join_side says that the caller's stream joins it first (step_join). Not counted: nothing changes, the
// call joins by an event behind its true peak.
inline SyncStep step_lufs_tp(const MeterSync& m, int64_t n_cf, bool counted) {
  SyncStep r;
  r.ok = r.fail = m;
  r.join_side = counted && m.side;
  if (counted) r.ok.lufs_tp += (unsigned)n_cf;
  r.wait_target = r.ok.lufs_tp;
  return r;
}

// The caller's stream has joined the side stream: an event recorded there and waited for here.
inline SyncStep step_join(const MeterSync& m) {
  SyncStep r;
  r.ok = r.fail = m;
  r.ok.side = false;
  return r;
}

}  // namespace omega_host
