// The batch grid on the CPU (tests/test_batch_plan.py): reads one shape per line from standard input,
// evaluates csrc/batch_plan.hpp on it and prints every BatchPlan field and the grid, one case per line.
//   P n_cf do_kw do_tp mr q_n q_before_multi n_res {fft_size wanted} x n_res   -> plan_batch
//   S nq                                                                       -> plan_segment_only
//   M n_cf                                                                     -> meter_segment_wgs
// A D before a P or S case prints, instead of the fields, what decode_block (the pieces batch_body runs,
// composed) makes of every block of the planned grid: numbers only, "code grid" and then "kind which index" per block 0..grid-1 (none
// for a refused plan), all on the case's line.
// No device and no context: the header is integer arithmetic only.
#include <cinttypes>
#include <cstdio>

#include "../../audio-analyzer-omega_amd/csrc/batch_plan.hpp"

using namespace omega;

static void list(const char* name, const int* v, int n) {
  std::printf(" %s=", name);
  for (int i = 0; i < n; ++i) std::printf(i ? ",%d" : "%d", v[i]);
}

static void dump(int code, const BatchPlan& bp, int grid) {
  std::printf("code=%d grid=%d", code, grid);
  list("seg_begin", bp.seg_begin, 3);
  list("n_roles", bp.n_roles, 2);
  list("roles", &bp.roles[0][0], 6);
  std::printf(" mr_res=%d multi_n_seg=%d", bp.mr_res, bp.multi.n_seg);
  list("multi_res", bp.multi.res, 4);
  list("multi_wg_begin", bp.multi.wg_begin, 4);
  std::printf(" q_begin=%d q_n=%d tail_ctr=%d pat=%d", bp.q_begin, bp.q_n, bp.tail_ctr ? 1 : 0, bp.pat);
  list("seg_start", bp.seg_start, 2);
  std::printf(" multi_start=%d multi_n=%d\n", bp.multi_start, bp.multi_n);
}

static void dump_decode(int code, const BatchPlan& bp, int grid) {
  std::printf("%d %d", code, grid);
  for (int b = 0; code == 0 && b < grid; ++b) {
    const BatchWork wk = decode_block(bp, b);
    std::printf(" %d %d %" PRId64, wk.kind, wk.which, wk.index);
  }
  std::printf("\n");
}

int main() {
  char kind;
  bool decode = false;
  while (std::scanf(" %c", &kind) == 1) {
    if (kind == 'D') {
      decode = true;
      continue;
    }
    if (kind == 'M') {
      int64_t n = 0;
      if (std::scanf("%" SCNd64, &n) != 1) return 2;
      std::printf("wgs=%d\n", meter_segment_wgs(n));
    } else if (kind == 'S') {
      int nq = 0;
      if (std::scanf("%d", &nq) != 1) return 2;
      (decode ? dump_decode : dump)(0, plan_segment_only(nq), nq);
    } else if (kind == 'P') {
      BatchShape sh{};
      int kw = 0, tp = 0, first = 0;
      if (std::scanf("%" SCNd64 " %d %d %d %d %d %d", &sh.n_cf, &kw, &tp, &sh.mr, &sh.q_n, &first, &sh.n_res) != 7)
        return 2;
      if (sh.n_res < 0 || sh.n_res > kMaxRes) return 2;
      sh.do_kw = kw != 0;
      sh.do_tp = tp != 0;
      sh.q_before_multi = first != 0;
      for (int r = 0; r < sh.n_res; ++r) {
        int wanted = 0;
        if (std::scanf("%d %d", &sh.res[r].n, &wanted) != 2) return 2;
        sh.res[r].wanted = wanted != 0;
      }
      BatchPlan bp{};
      int grid = -1;
      const int code = plan_batch(sh, &bp, &grid);
      (decode ? dump_decode : dump)(code, bp, grid);
    } else {
      return 2;
    }
    decode = false;
  }
  return 0;
}
