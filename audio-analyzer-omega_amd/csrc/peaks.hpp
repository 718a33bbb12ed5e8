// The pieces of scipy.signal.find_peaks that the feature kernels share (harmonic, hip-hop, pitch, voice, room),
// once: _local_maxima_1d, _peak_prominences with wlen=None, and _select_by_peak_distance in a parallel form.
// The per-index functions are pure and compile for host and device, so tests/test_peaks.py holds them to
// tools/model/peaks_model.py and to scipy on the CPU (tests/abi/peaks_dump.cpp); select_by_distance is the
// workgroup loop over the same two predicates. Like wg64.hpp this header sets no contraction pragma and takes
// the including file's state; nothing here multiplies.
//
// THE DISTANCE RULE. scipy keeps peaks greedily, highest first, each kept peak removing those nearer than d.
// Here that runs in rounds over flags: an UNDECIDED peak that is top among the undecided peaks within d - 1
// of it is kept (distance_top); then every undecided peak that is kept, or has a kept peak within d - 1, is
// decided (distance_decided). The highest undecided peak, the latest of them on a tie, is always top, so every
// round decides at least one peak and the rounds number at most the candidates. A peak is top only when all
// higher peaks in its window are already decided -- removed, since a kept one would have removed it too --
// which is the moment the greedy order reaches it: without equal heights the result is scipy's.
// EQUAL HEIGHTS: the later index wins here. scipy orders equal priorities by an unstable argsort, so it has
// no such rule: scipy 1.15.3 differs from this one on 4 of 59,022 arrays of length 3..9 over three values
// (d = 2, 3) and on 1,338 of 2,000 random arrays over four values. The kernels' results follow this rule.
#pragma once

#include <hip/hip_runtime.h>

namespace omega {

// scipy's _local_maxima_1d at plateau start i (0 < i < n - 1): the peak's index (the plateau's middle,
// (left + right) // 2), or -1. A plateau that runs into the array's end is no peak.
template <class T>
__host__ __device__ __forceinline__ int local_max_at(const T* x, int n, int i) {
  const T v = x[i];
  if (!(x[i - 1] < v)) return -1;
  int j = i + 1;
  while (j < n - 1 && x[j] == v) ++j;
  return x[j] < v ? (i + j - 1) / 2 : -1;
}

// scipy's _peak_prominences (wlen=None) of the peak at p: each side's minimum out to the next higher sample or
// the array's end, in the element type; the difference in float64 (exact for float32). No NaN reaches the
// minima (x[j] <= x[p] ends the scan), and the sign of a zero minimum does not reach the value's comparisons.
template <class T>
__host__ __device__ __forceinline__ double prominence(const T* x, int n, int p) {
  const T h = x[p];
  T lmin = h, rmin = h;
  for (int j = p; j >= 0 && x[j] <= h; --j) lmin = x[j] < lmin ? x[j] : lmin;
  for (int j = p; j < n && x[j] <= h; ++j) rmin = x[j] < rmin ? x[j] : rmin;
  return (double)h - (double)(lmin > rmin ? lmin : rmin);
}

// the undecided peak i of [lo, hi) is top among the undecided peaks within d - 1: none is higher, none of
// equal height comes later
template <class T, class F>
__host__ __device__ __forceinline__ bool distance_top(const T* x, const F* und, int lo, int hi, int d, int i) {
  const T v = x[i];
  const int a = i - d + 1 > lo ? i - d + 1 : lo, b = i + d < hi ? i + d : hi;
  bool top = true;
  for (int j = a; j < b; ++j)
    if (j != i && und[j] && (x[j] > v || (x[j] == v && j > i))) top = false;
  return top;
}

// peak i of [lo, hi) is kept or has a kept peak within d - 1
template <class F>
__host__ __device__ __forceinline__ bool distance_decided(const F* kept, int lo, int hi, int d, int i) {
  const int a = i - d + 1 > lo ? i - d + 1 : lo, b = i + d < hi ? i + d : hi;
  bool gone = kept[i] != 0;
  for (int j = a; j < b && !gone; ++j)
    if (kept[j]) gone = true;
  return gone;
}

#ifdef __HIPCC__
// The rounds over [lo, hi) for a workgroup of T threads. On entry und marks the candidates, kept is clear and
// `any` says whether this thread marked one; no barrier is needed in between (the loop's condition is one).
// On return kept marks find_peaks(distance = d)'s survivors and every thread has passed the last barrier.
template <int T, class X, class F>
__device__ __forceinline__ void select_by_distance(const X* x, F* und, F* kept, int lo, int hi, int d, int any) {
  for (int round = 0; round < hi - lo && __syncthreads_or(any); ++round) {
    for (int i = lo + threadIdx.x; i < hi; i += T)
      if (und[i] && distance_top(x, und, lo, hi, d, i)) kept[i] = 1;
    __syncthreads();
    any = 0;
    for (int i = lo + threadIdx.x; i < hi; i += T) {
      if (!und[i]) continue;
      if (distance_decided(kept, lo, hi, d, i)) und[i] = 0;
      else any = 1;
    }
  }
}
#endif

}  // namespace omega
