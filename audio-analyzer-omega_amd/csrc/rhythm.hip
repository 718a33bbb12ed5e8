// BeatDetector / BeatDetectionPanel (omega4/panels/beat_detection.py) and FrequencyBandTracker
// (omega4/panels/frequency_band_tracker.py) on the device: the sums both panels take over one frame's spectrum, in
// float64 over the float32 bins (widened exactly). The panels' scalar logic stays on the host.
//
//   rhythm_flags_kernel, one 256-thread workgroup per frame: the frame's samples and bins are scanned for non-finite
//     values, sum x^2 is formed, and the panel's silence gate (:338-349, sqrt(mean(x^2)) < 0.001) is decided. Flag
//     bits 0 and 1 go to the workspace, sum x^2 to the row.
//   rhythm_kernel, behind it on the same stream, one 256-thread workgroup per frame: the predecessor -- the nearest
//     earlier frame with neither bit set, else the carried state's -- is found by walking the workspace flags
//     backwards, 256 frames per step. The frame's row is read once, coalesced, into LDS beside the predecessor's
//     values (the neighbouring workgroup read that row as its own a moment earlier: it comes from the cache), and one
//     pass forms
//       :71, :74       flux = sum max(0, float32(s - p)), the difference rounded to float32 as numpy rounds it, and
//                      spec_sum = sum s
//       :85-92, :143-149 and frequency_band_tracker.py:118-130   the kick band and the seven band sums
//       frequency_band_tracker.py:81   spec_fsum = sum freqs s
//     eleven sums reduced at once (wg64.hpp block_sums). The centroid c = spec_fsum / (double)(float)spec_sum comes
//     out of that reduction on every thread; the spread pass sum (freqs - c)^2 s (:155-156) reads the spectrum from
//     LDS, not from memory again. Workgroup n_frames writes the outgoing state.
//
// Every sum has a fixed order that does not depend on the number of frames in the call: F frames in one call equal
// F chained calls bit for bit. No workgroup waits for another; the two launches are ordered by the stream.
#include <hip/hip_runtime.h>

#include "params.hpp"
#include "wg64.hpp"

namespace omega {

namespace {

constexpr int kT = kRhThreads;

// The nearest live frame before `before` (uniform; -1: none in this launch), 256 frames per step
__device__ __forceinline__ int64_t rh_predecessor(const RhythmParams& p, int64_t before, double* red) {
  for (int64_t base = before - 1; base >= 0; base -= kT) {
    const int64_t g = base - threadIdx.x;
    const double cand = g >= 0 && p.ws[g] == 0 ? (double)g : -1.0;
    const double best = block_max(cand, red);
    if (best >= 0.0) return (int64_t)best;
  }
  return -1;
}

}  // namespace

__global__ __launch_bounds__(kT) void rhythm_flags_kernel(RhythmParams p) {
  __shared__ double red[2 * (kT / 64)];
  const int t = threadIdx.x;
  const int64_t f = blockIdx.x;
  double v[2] = {0.0, 0.0};  // non-finite count, sum x^2
  if (p.audio.base)
    for (int i = t; i < p.m; i += kT) {
      const double x = p.audio.at(f, i);
      if (!isfinite(x)) v[0] = 1.0;
      v[1] = fma(x, x, v[1]);
    }
  const float* g = p.spec.row(f);
  for (int i = t; i < p.n_bins; i += kT)
    if (!isfinite(g[i])) v[0] = 1.0;
  block_sums<2, kT / 64>(v, red);
  if (t == 0) {
    const bool bad = v[0] > 0.0;
    const bool gated = !bad && p.audio.base && sqrt(v[1] / (double)p.m) < kRhGate;
    p.ws[f] = bad ? kRhNonFinite : (gated ? kRhGated : 0);
    p.out[f * kRhCols + 1] = bad ? 0.0 : v[1];
  }
}

// Workgroup f < n_frames: frame f's row. Workgroup n_frames: the outgoing state.
__global__ __launch_bounds__(kT) void rhythm_kernel(RhythmParams p) {
  extern __shared__ __attribute__((aligned(16))) float rh_s[];  // [n_bins] the frame's spectrum
  __shared__ double red[kRhSums * (kT / 64)];
  const int t = threadIdx.x, K = p.n_bins;
  const int64_t f = blockIdx.x, F = p.n_frames;
  const double* sin = p.state_in;
  const bool has_state = sin && sin[0] != 0.0 && sin[1] == (double)K;
  if (f == F) {
    double* so = p.state_out;
    if (!so) return;
    const int64_t last = rh_predecessor(p, F, red);
    if (last >= 0) {
      const float* g = p.spec.row(last);
      for (int i = t; i < K; i += kT) so[kRhStateHead + i] = (double)g[i];
    } else {
      for (int i = t; i < K; i += kT) so[kRhStateHead + i] = has_state ? sin[kRhStateHead + i] : 0.0;
    }
    if (t == 0) {
      so[0] = last >= 0 || has_state ? 1.0 : 0.0;
      so[1] = (double)K;
    }
    return;
  }
  double* o = p.out + f * kRhCols;
  const int flags = p.ws[f];
  if (flags & kRhNonFinite) {  // (uniform) the flag alone
    if (t == 0) o[0] = (double)kRhNonFinite;
    if (t >= 2 && t < kRhCols) o[t] = 0.0;
    return;
  }
  const int64_t prev = rh_predecessor(p, f, red);
  const float* pg = prev >= 0 ? p.spec.row(prev) : nullptr;
  const bool has_prev = pg || has_state;
  const float* g = p.spec.row(f);
  // a band's upper edge 0 is the reference's "beyond the spectrum": the band runs to the last bin
  auto upper = [&](int e) { return p.edge[e] == 0 ? K : p.edge[e]; };
  const int kick_lo = p.edge[1], kick_hi = upper(3);
  const int lo[kRhBands] = {p.edge[0], p.edge[2], p.edge[4], p.edge[5], p.edge[6], p.edge[7], p.edge[8]};
  const int hi[kRhBands] = {upper(2), upper(4), upper(5), upper(6), upper(7), upper(8), upper(9)};
  double v[kRhSums];
#pragma unroll
  for (int n = 0; n < kRhSums; ++n) v[n] = 0.0;
  for (int i = t; i < K; i += kT) {
    const float s = g[i];
    rh_s[i] = s;
    const double sd = (double)s;
    v[0] += sd;
    if (has_prev) {
      const float q = pg ? pg[i] : (float)sin[kRhStateHead + i];
      const float d = s - q;  // (one float32 rounding, as numpy's float32 subtraction)
      v[1] += (double)fmaxf(0.0f, d);
    }
    if (i >= kick_lo && i < kick_hi) v[2] += sd;
#pragma unroll
    for (int b = 0; b < kRhBands; ++b)
      if (i >= lo[b] && i < hi[b]) v[3 + b] += sd;
    v[3 + kRhBands] = fma(p.freqs[i], sd, v[3 + kRhBands]);
  }
  block_sums<kRhSums, kT / 64>(v, red);  // (its barriers publish rh_s)
  const double total = (double)(float)v[0];  // the reference's total_energy is a float32
  const double c = total > 0.0 ? v[3 + kRhBands] / total : 0.0;
  double spread = 0.0;
  if (total > 0.0 && c > 0.0) {  // (uniform)
    for (int i = t; i < K; i += kT) {
      const double d = p.freqs[i] - c;
      spread = fma(d * d, (double)rh_s[i], spread);
    }
    spread = block_sum(spread, red);  // (its first barrier stands between the reads of red above and its writes)
  }
  if (t == 0) {
    o[0] = (double)(flags | (has_prev ? 0 : kRhNoFlux));
    o[2] = v[0];
    o[3] = v[1];
    o[4] = v[2];
    for (int b = 0; b < kRhBands; ++b) o[5 + b] = v[3 + b];
    o[12] = v[3 + kRhBands];
    o[13] = spread;
  }
}

hipError_t launch_rhythm(const RhythmParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  hipLaunchKernelGGL(rhythm_flags_kernel, dim3((unsigned)p.n_frames), dim3(kT), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rhythm_kernel, dim3((unsigned)(p.n_frames + 1)), dim3(kT), (size_t)p.n_bins * sizeof(float), s, p);
  return hipGetLastError();
}

}  // namespace omega
