// The meter pipeline's ledger on the CPU (tests/test_meter_sync.py): reads one step per line from standard
// input, takes it with csrc/meter_sync.hpp from the ledger the line before left, and prints the step's
// targets and the whole ledger after the outcome the line names, one step per line.
//   Z                                     -> MeterSync{} (configure)
//   S v                                   -> every count := v (the six, seg_par, mirror_gen, tail)
//   B k f1..fk ok                         -> step_state_chunks (meters_enqueue, graph replay)
//   E k f1..fk ok                         -> step_state_chunks, on the side stream (back-to-back layout)
//   K n_cf C k f1..fk ok|fail             -> step_chunks
//   D n_cf C ok|fail                      -> step_direct
//   P n_cf C tail ok|fail|launched|waited -> step_pipelined
//   F ok|fail                             -> step_flush
//   L n_cf counted ok|fail                -> step_lufs_tp
//   J ok|fail                             -> step_join
// No device and no context: the header is integer arithmetic only.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../audio-analyzer-omega_amd/csrc/meter_sync.hpp"

using namespace omega_host;

static std::vector<int64_t> read_frames() {
  int k = 0;
  std::vector<int64_t> v;
  if (std::scanf("%d", &k) != 1 || k < 0 || k > 64) std::exit(2);
  for (int i = 0; i < k; ++i) {
    int64_t f = 0;
    if (std::scanf("%" SCNd64, &f) != 1) std::exit(2);
    v.push_back(f);
  }
  return v;
}

template <class F>
static void list(const char* name, const std::vector<ChunkSync>& ch, F field) {
  std::printf(" %s=", name);
  if (ch.empty()) std::printf("-");
  for (size_t i = 0; i < ch.size(); ++i) std::printf(i ? ",%" PRId64 : "%" PRId64, (int64_t)field(ch[i]));
}

int main() {
  MeterSync m;
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    SyncStep st;
    st.ok = st.fail = st.launched = st.waited = m;
    int64_t n = 0;
    int C = 0, tail = 0;
    bool outcome = true;
    if (kind == 'Z') {
      st.ok = MeterSync{};
      outcome = false;
    } else if (kind == 'S') {
      unsigned v = 0;
      if (std::scanf("%u", &v) != 1) return 2;
      MeterSync& s = st.ok;
      s.kw = s.query = s.tp = s.prep = s.seg = s.lufs_tp = s.seg_par[0] = s.seg_par[1] = s.mirror_gen = s.tail = v;
      outcome = false;
    } else if (kind == 'B') {
      st = step_state_chunks(m, read_frames());
    } else if (kind == 'E') {
      st = step_state_chunks(m, read_frames(), true);
    } else if (kind == 'K') {
      if (std::scanf("%" SCNd64 " %d", &n, &C) != 2) return 2;
      st = step_chunks(m, n, C, read_frames());
    } else if (kind == 'D') {
      if (std::scanf("%" SCNd64 " %d", &n, &C) != 2) return 2;
      st = step_direct(m, n, C);
    } else if (kind == 'P') {
      if (std::scanf("%" SCNd64 " %d %d", &n, &C, &tail) != 3) return 2;
      st = step_pipelined(m, n, C, tail != 0);
    } else if (kind == 'F') {
      st = step_flush(m);
    } else if (kind == 'L') {
      if (std::scanf("%" SCNd64 " %d", &n, &C) != 2) return 2;
      st = step_lufs_tp(m, n, C != 0);
    } else if (kind == 'J') {
      st = step_join(m);
    } else {
      return 2;
    }
    m = st.ok;
    if (outcome) {
      char word[16];
      if (std::scanf("%15s", word) != 1) return 2;
      if (!std::strcmp(word, "fail"))
        m = st.fail;
      else if (kind == 'P' && !std::strcmp(word, "launched"))
        m = st.launched;
      else if (kind == 'P' && !std::strcmp(word, "waited"))
        m = st.waited;
      else if (std::strcmp(word, "ok"))
        return 2;
    }
    std::printf("wait=%u start=%u join=%u tail_target=%u gen=%u q_n=%d join_side=%d", st.wait_target, st.start_target,
                st.join_target, st.tail_target, st.mirror_gen, st.q_n, st.join_side ? 1 : 0);
    list("frames", st.chunks, [](const ChunkSync& c) { return c.n_frames; });
    list("par", st.chunks, [](const ChunkSync& c) { return c.par; });
    list("seg_pre", st.chunks, [](const ChunkSync& c) { return c.seg_pre_target; });
    list("seg_post", st.chunks, [](const ChunkSync& c) { return c.seg_post_target; });
    std::printf(" kw=%u query=%u tp=%u prep=%u seg=%u lufs_tp=%u seg_par=%u,%u cur=%d pend=%d pend_nq=%d pend_par=%d"
                " mirror_gen=%u tail=%u side=%d\n",
                m.kw, m.query, m.tp, m.prep, m.seg, m.lufs_tp, m.seg_par[0], m.seg_par[1], m.cur, m.pend ? 1 : 0,
                m.pend_nq, m.pend_par, m.mirror_gen, m.tail, m.side ? 1 : 0);
  }
  return 0;
}
