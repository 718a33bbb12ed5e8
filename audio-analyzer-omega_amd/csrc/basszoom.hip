// BassZoomPanel (omega4/panels/bass_zoom.py) on the device, in float64 like the reference's numpy path (float32
// frames are widened exactly on load), 256 threads per workgroup.
//
// basszoom_frame_kernel, one workgroup per frame (:141-196, :204-210): abs(rfft(x[:nw] * hanning(nw), 8192)) at the
// 20..200 Hz bins only, the bar means, the compensation, bass_max, scale_factor and the compressed values, one row
// per frame. The staging loop scans the frame's samples for non-finite values.
//
// The transform: of the two designs that fit (the packed 4096-point Stockham transform of hilbert64.hpp, or a
// direct evaluation of the wanted bins) this is the direct one. The panel wants 8 to 184 of the 4097 bins (31 at
// 48 kHz); the Stockham route costs 128 KiB of LDS, so one workgroup per CU, and twelve barrier-separated passes
// that each move the whole 64 KiB frame through LDS, whatever the number of bins; the direct sum costs
// 2 * bins * 8192 float64 FMAs (0.5 M at 48 kHz, 3 M at 8 kHz) with one barrier, and a short frame costs
// proportionally less. A plain gather of e^{-2 pi i k n / 8192} per term would be bound by the table reads, so
// the sum is split as n = 64 a + b: lane b of a wave accumulates S_b = sum_a xw[64 a + b] e^{-2 pi i k a / 128},
// where the twiddle is the same for the whole wave (a scalar load; its index (k a) mod 128 is kept in integers), a
// wave holds eight bins at once so that one LDS read of xw feeds sixteen FMAs, and the 64 partial sums are rotated
// by e^{-2 pi i k b / 8192} (one table read per lane and bin, index (k b) mod 8192 in integers) and added by a
// shuffle tree. Every bin's summation order is fixed by (a, b) alone: the result does not depend on the number of
// frames in the call, nor on the bin's place in the mapping. LDS: 8 B per staged sample (64 KiB at 8192) plus 2.6
// KiB static. Neither design has been timed against the other.
//
// basszoom_track_kernel, behind it on the same stream, one workgroup, thread i = bar i (:212-226): the rising /
// falling smoothing, the clamp and the peak hold over the call's frames in order, on float32 state with numpy
// 2.x's types -- float32(bar) * float32(0.1) rounded to float32, the float64 product c * 0.9 rounded to float64,
// their float64 sum rounded to float32 on store, peak *= float32(0.95) -- every step an explicitly rounded
// operation, so that nothing is contracted into an FMA. The caller gives each frame's time; frames flagged
// non-finite are passed over and their output rows repeat the state.
#include <hip/hip_runtime.h>

#include "params.hpp"
#include "wg64.hpp"

namespace omega {

namespace {

constexpr int kT = kBzThreads;
static_assert(kBzThreads == 4 * 64, "block_sum's default is four waves");
constexpr int kBzGroup = 8;  // bins a wave holds at once

// the row's tail from the magnitudes (:168-210), in the reference's operation order and without contraction
__device__ __forceinline__ void bz_bars(const BassZoomParams& p, const double* mag, double* raw, double* row) {
#pragma clang fp contract(off)
  const int t = threadIdx.x, nb = p.n_bars;
  if (t < nb) {
    const int lo = t * p.bins_per_bar, hi = min(lo + p.bins_per_bar, p.n_valid);
    double s = 0.0;
    for (int i = lo; i < hi; ++i) s += mag[i];
    raw[t] = s / (double)(hi - lo) * p.comp[t];
  }
  __syncthreads();
  double bmax = 0.0;
  for (int i = 0; i < nb; ++i) bmax = fmax(bmax, raw[i]);
  double scale = 1.0;
  if (bmax > 0.0) scale = 0.85 / bmax * (log10(fmax(1.0, bmax * 10.0)) / 2.0);
  if (t == 0) {
    row[0] = 0.0;
    row[1] = bmax;
    row[2] = scale;
  }
  if (t < nb) {
    const double v = raw[t] * scale;
    row[kBzRowHead + t] = v > 0.7 ? 0.7 + (v - 0.7) * 0.3 : v;
  }
}

}  // namespace

__global__ __launch_bounds__(kT) void basszoom_frame_kernel(BassZoomParams p) {
  extern __shared__ __attribute__((aligned(16))) double bz_xw[];  // [64 A] the windowed samples, zero-padded
  __shared__ double red[4];
  __shared__ double mag[kBzMaxBins];
  __shared__ double raw[kBzMaxBars];
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t f = blockIdx.x;
  const int A = (p.nw + 63) / 64;
  double* row = p.rows + f * (kBzRowHead + p.n_bars);
  double bad = 0.0;
  for (int i = t; i < 64 * A; i += kT) {
    double v = 0.0;
    if (i < p.nw) {
      v = p.frames.at(f, i);
      if (!isfinite(v)) bad = 1.0;
      v *= p.win[i];
    }
    bz_xw[i] = v;
  }
  if (block_sum(bad, red) > 0.0) {  // (uniform; the barriers publish bz_xw)
    if (t < kBzRowHead + p.n_bars) row[t] = t == 0 ? 1.0 : 0.0;
    return;
  }
  const int n_groups = (p.n_valid + kBzGroup - 1) / kBzGroup;
  for (int g = wv; g < n_groups; g += kT / 64) {
    int k[kBzGroup], ph[kBzGroup];
    double sr[kBzGroup], si[kBzGroup];
#pragma unroll
    for (int j = 0; j < kBzGroup; ++j) {
      k[j] = p.first_bin + min(g * kBzGroup + j, p.n_valid - 1);  // (the last group's spare slots repeat a bin)
      ph[j] = 0;
      sr[j] = si[j] = 0.0;
    }
    for (int a = 0; a < A; ++a) {
      const double v = bz_xw[64 * a + lane];
#pragma unroll
      for (int j = 0; j < kBzGroup; ++j) {
        const double2 w = p.tw[ph[j] * (kBzFft / 128)];  // e^{-2 pi i (k a mod 128) / 128}, wave-uniform
        sr[j] = fma(v, w.x, sr[j]);
        si[j] = fma(v, w.y, si[j]);
        ph[j] = (ph[j] + k[j]) & 127;
      }
    }
#pragma unroll
    for (int j = 0; j < kBzGroup; ++j) {
      const double2 r = zmul(make_double2(sr[j], si[j]), p.tw[(k[j] * lane) & (kBzFft - 1)]);
      const double re = wave_sum(r.x), im = wave_sum(r.y);
      const int q = g * kBzGroup + j;
      if (lane == 0 && q < p.n_valid) mag[q] = hypot(re, im);
    }
  }
  __syncthreads();
  bz_bars(p, mag, raw, row);
}

__global__ __launch_bounds__(64) void basszoom_track_kernel(BassZoomParams p) {
  const int i = threadIdx.x, nb = p.n_bars;
  if (i >= nb) return;
  const double* sin = p.state_in;
  float bar = sin ? (float)sin[i] : 0.0f, peak = sin ? (float)sin[kBzMaxBars + i] : 0.0f;
  double ts = sin ? sin[2 * kBzMaxBars + i] : 0.0;
  for (int64_t f = 0; f < p.n_frames; ++f) {
    const double* row = p.rows + f * (kBzRowHead + nb);
    if (row[0] == 0.0) {
      const double c = row[kBzRowHead + i], now = p.times[f];
      double v;
      if (c > (double)bar)
        v = __dadd_rn((double)__fmul_rn(bar, 0.1f), __dmul_rn(c, 0.9));
      else
        v = __dadd_rn((double)__fmul_rn(bar, 0.6f), __dmul_rn(c, 0.4));
      bar = (float)v;
      bar = bar < 1.0f ? bar : 1.0f;  // max(0.0, min(1.0, bar))
      bar = bar > 0.0f ? bar : 0.0f;
      if (bar > peak) {
        peak = bar;
        ts = now;
      } else if (__dsub_rn(now, ts) > 3.0) {
        peak = __fmul_rn(peak, 0.95f);
      }
    }
    p.bars[f * nb + i] = (double)bar;
    p.peaks[f * nb + i] = (double)peak;
    p.peak_times[f * nb + i] = ts;
  }
  if (double* so = p.state_out) {
    so[i] = (double)bar;
    so[kBzMaxBars + i] = (double)peak;
    so[2 * kBzMaxBars + i] = ts;
  }
}

size_t basszoom_lds_bytes(int nw) { return (size_t)((nw + 63) / 64) * 64 * sizeof(double); }

hipError_t launch_basszoom_frames(const BassZoomParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const size_t lds = basszoom_lds_bytes(p.nw);
  if (lds + 4 * 1024 > 64 * 1024) {  // (the kernel's static arrays take under 4 KiB)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&basszoom_frame_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(basszoom_frame_kernel, dim3((unsigned)p.n_frames), dim3(kT), lds, s, p);
  return hipGetLastError();
}

hipError_t launch_basszoom_track(const BassZoomParams& p, hipStream_t s) {
  hipLaunchKernelGGL(basszoom_track_kernel, dim3(1), dim3(64), 0, s, p);
  return hipGetLastError();
}

}  // namespace omega
