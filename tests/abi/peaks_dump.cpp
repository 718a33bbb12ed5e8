// The shared find_peaks pieces on the CPU (tests/test_peaks.py): reads one case per line from standard input
// (or from the file named as the first argument), evaluates csrc/peaks.hpp on it and prints one line of numbers.
//   f|d n d lo hi x[0] ... x[n-1]      f: the array as float32, d: as float64; distance d over [lo, hi)
//   -> P p[0..P) prom[0..P) K k[0..K) rounds
// p: local_max_at from every i of 1..n-2, ascending; prom: prominence of each (%.17g: float64 round trip);
// k: the peaks of [lo, hi) that the distance rule keeps, run as the device loop runs it -- a sweep of
// distance_top over the undecided peaks, then a sweep of distance_decided, until none is undecided -- and the
// number of rounds that took. The flags are bytes for f and ints for d, as in the kernels.
#include <cstdio>
#include <vector>

#include "../../audio-analyzer-omega_amd/csrc/peaks.hpp"

using namespace omega;

template <class T, class F>
static bool run(std::FILE* in, int n, int d, int lo, int hi) {
  if (n < 1 || d < 1 || lo < 0 || hi > n) return false;
  std::vector<T> x(n);
  for (int i = 0; i < n; ++i) {
    double v = 0.0;
    if (std::fscanf(in, "%lf", &v) != 1) return false;
    x[i] = (T)v;
  }
  std::vector<int> pk;
  for (int i = 1; i < n - 1; ++i) {
    const int p = local_max_at(x.data(), n, i);
    if (p >= 0) pk.push_back(p);
  }
  std::printf("%zu", pk.size());
  for (int p : pk) std::printf(" %d", p);
  for (int p : pk) std::printf(" %.17g", prominence(x.data(), n, p));

  std::vector<F> und(n, 0), kept(n, 0);
  bool any = false;
  for (int p : pk)
    if (p >= lo && p < hi) und[p] = 1, any = true;
  int rounds = 0;
  for (; rounds < hi - lo && any; ++rounds) {
    for (int i = lo; i < hi; ++i)  // (kept is written, und only read: the sweep's order does not matter)
      if (und[i] && distance_top(x.data(), und.data(), lo, hi, d, i)) kept[i] = 1;
    any = false;
    for (int i = lo; i < hi; ++i) {  // (und[i] alone is written, kept only read)
      if (!und[i]) continue;
      if (distance_decided(kept.data(), lo, hi, d, i)) und[i] = 0;
      else any = true;
    }
  }
  int nk = 0;
  for (int i = lo; i < hi; ++i) nk += kept[i] != 0;
  std::printf(" %d", nk);
  for (int i = lo; i < hi; ++i)
    if (kept[i]) std::printf(" %d", i);
  std::printf(" %d\n", rounds);
  return true;
}

int main(int argc, char** argv) {
  std::FILE* in = argc > 1 ? std::fopen(argv[1], "r") : stdin;
  if (!in) return 2;
  char type;
  int n, d, lo, hi;
  while (std::fscanf(in, " %c", &type) == 1) {
    if (std::fscanf(in, "%d %d %d %d", &n, &d, &lo, &hi) != 4) return 2;
    const bool ok = type == 'f'   ? run<float, unsigned char>(in, n, d, lo, hi)
                    : type == 'd' ? run<double, int>(in, n, d, lo, hi)
                                  : false;
    if (!ok) return 2;
  }
  return 0;
}
