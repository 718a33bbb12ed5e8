// VoiceDetectionPanel (omega4/panels/voice_detection.py) on the device: detect_voice :57-87 with
// _detect_formant_structure :89-122 and the autocorrelation of detect_pitch :169-192, for a batch of independent
// frames. One launch, the role split by blockIdx as in hiphop_kernel: workgroup b < F is frame b's spectrum side,
// workgroup F + b its audio side (launched only where the configured shape can give a pitch at all). Each side
// also scans the other side's input for non-finite values, so that both know the frame's flag and write their own
// columns without a join. Contraction is off: freq_bins[peak] is numpy's k * (1.0 / (m * (1 / fs))) bit for bit.
//
// spectrum side -- the K <= 8193 float32 magnitudes and their smoothed copy in LDS, 8 bytes per bin:
//   :66-71    voice_start / voice_end come from the host (omega_voice_bin_range); the range check :69; the two
//             sums as float64 block sums of the float32 inputs (the facade rounds them to the reference's float32)
//   :97       savgol_filter(spectrum, w, 3), mode 'interp': scipy correlates in float64 and stores float32, and
//             fits the w // 2 edge points with a float64 cubic; here every output is the float64 dot product of
//             the host-designed weights of its window position, rounded to float32 once
//   :98       find_peaks(smoothed, prominence=max * 0.1): _local_maxima_1d from every rising edge at once (a
//             plateau gives (left + right) // 2), _peak_prominences with wlen=None on the owning lane; scipy
//             widens x to float64 there, so a prominence is the exact difference of two float32 values; the
//             threshold is the float32 product numpy >= 2 forms
//   :101-115  the first kept peak of each range in ascending order is the lowest kept bin that satisfies the
//             range: an LDS atomicMin per range (integer, so the order of arrival does not matter)
// audio side -- the m <= 8192 samples as float64 in LDS with kVoicePad zeros behind them, 8 bytes per sample,
// and direct sums: c[l] for the at most m - 1 lags of [lag_lo, lag_hi), kVoiceLagBlock consecutive lags per
// thread sharing every x[n] load (16 fused multiply-adds per 11 LDS reads); where the lag blocks number fewer
// than the threads, the sample range is split over the spare threads and the parts added in a fixed order. The
// packed float64 FFT of pitch.hip would need 16 bytes per sample and its twiddle tables for 481 of 2048 lags;
// at the app's shape the direct sums are 1M multiply-adds per frame.
#include <hip/hip_runtime.h>

#include <algorithm>

#pragma clang fp contract(off)  // (above the project headers: peaks.hpp and wg64.hpp take this state)

#include "params.hpp"
#include "peaks.hpp"
#include "wg64.hpp"

namespace omega {

namespace {

constexpr int kVT = kVoiceThreads, kVW = kVoiceThreads / 64;

// 1.0 where frame f's audio holds a non-finite sample (this thread's share)
__device__ __forceinline__ double vc_audio_bad(const VoiceParams& p, int64_t f) {
  const Row a = p.audio.row(f);
  double bad = 0.0;
  for (int i = threadIdx.x; i < p.m; i += kVT)
    if (!isfinite(a[i])) bad = 1.0;
  return bad;
}

__device__ __forceinline__ void voice_spectrum(const VoiceParams& p, int64_t f, unsigned char* smem, double* red,
                                               int* first) {
  const int t = threadIdx.x, K = p.n_bins;
  float* s = reinterpret_cast<float*>(smem);  // [K] the spectrum
  float* sm = s + K;                          // [K] savgol_filter's result
  const float* g = p.spec.row(f);
  double* o = p.out + f * kVoiceCols;
  const int vs = p.voice_start, ve = p.voice_end;
  if (t < 4) first[t] = K;

  double a[3] = {0.0, 0.0, 0.0};  // non-finite, voice_energy, total_energy
  for (int i = t; i < K; i += kVT) {
    const float v = g[i];
    s[i] = v;
    if (!isfinite(v)) a[0] = 1.0;
    a[2] += (double)v;
    if (i >= vs && i < ve) a[1] += (double)v;
  }
  if (p.pitch) a[0] += vc_audio_bad(p, f);
  block_sums<3, kVW>(a, red);  // (the barriers publish s and first)
  const int pitch_flag = p.pitch ? 0 : 8;
  if (a[0] > 0.0) {  // (uniform) a non-finite input: the flag alone
    if (t < 14) o[t] = t == 0 ? 4.0 : 0.0;
    if (!p.pitch && t >= 14 && t < kVoiceCols) o[t] = 0.0;
    return;
  }
  const bool range_ok = vs < K && ve < K;  // :69
  const bool positive = a[2] > 0.0;        // :74
  if (!range_ok || !positive || p.sg_w == 0) {  // (uniform) no formant search
    if (t < kVoiceCols && (t < 14 || !p.pitch)) {
      double v = 0.0;
      if (t == 0) v = (double)((range_ok ? (positive ? 0 : 2) : 1) | pitch_flag);
      if (t == 1) v = (double)vs;
      if (t == 2) v = (double)ve;
      if (t == 3 && range_ok) v = a[1];
      if (t == 4 && range_ok) v = a[2];
      o[t] = v;
    }
    return;
  }

  // :97 every output from its window [w0, w0 + w) and the weights of its position there
  const int w = p.sg_w, half = w / 2;
  float mx = -INFINITY;
  for (int n = t; n < K; n += kVT) {
    const int w0 = n < half ? 0 : (n >= K - half ? K - w : n - half);
    const double* wt = p.sg + w * (n - w0);
    double acc = 0.0;
    for (int j = 0; j < w; ++j) acc = fma(wt[j], (double)s[w0 + j], acc);
    const float r = (float)acc;
    sm[n] = r;
    mx = fmaxf(mx, r);
  }
  double m1[1] = {(double)mx};
#pragma unroll
  for (int q = 32; q > 0; q >>= 1) m1[0] = fmax(m1[0], __shfl_xor(m1[0], q, 64));
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = m1[0];
  __syncthreads();  // (publishes sm)
  double top = red[0];
#pragma unroll
  for (int q = 1; q < kVW; ++q) top = fmax(top, red[q]);
  const double thr = (double)((float)top * 0.1f);  // np.max(smoothed) * 0.1 in float32

  // :98 the local maxima, their prominences, and :101-115 the lowest kept bin of each range
  for (int i = t + 1; i < K - 1; i += kVT) {
    const int pk = local_max_at(sm, K, i);
    if (pk < 0 || !(prominence(sm, K, pk) >= thr) || pk >= p.n_freq) continue;
    const double fr = (double)pk * p.bin_hz;
    if (200.0 <= fr && fr <= 900.0) atomicMin(&first[0], pk);
    if (800.0 <= fr && fr <= 2500.0) atomicMin(&first[1], pk);
    if (2000.0 <= fr && fr <= 3500.0) atomicMin(&first[2], pk);
    if (3000.0 <= fr && fr <= 4500.0) atomicMin(&first[3], pk);
  }
  __syncthreads();
  if (t < kVoiceCols && (t < 14 || !p.pitch)) {
    double v = 0.0;
    if (t == 0) v = (double)pitch_flag;
    if (t == 1) v = (double)vs;
    if (t == 2) v = (double)ve;
    if (t == 3) v = a[1];
    if (t == 4) v = a[2];
    if (t == 5) v = (double)((first[0] < K) + (first[1] < K) + (first[2] < K) + (first[3] < K));
    if (t >= 6 && t < 10 && first[t - 6] < K) v = (double)first[t - 6];
    if (t >= 10 && t < 14 && first[t - 10] < K) v = (double)first[t - 10] * p.bin_hz;
    o[t] = v;
  }
}

__device__ __forceinline__ void voice_audio(const VoiceParams& p, int64_t f, unsigned char* smem, double* red,
                                            double* part) {
  constexpr int B = kVoiceLagBlock;
  const int t = threadIdx.x, m = p.m;
  double* x = reinterpret_cast<double*>(smem);  // [m + kVoicePad]
  const Row au = p.audio.row(f);
  double* o = p.out + f * kVoiceCols;

  double a[2] = {0.0, 0.0};  // non-finite, c[0]
  for (int i = t; i < m + kVoicePad; i += kVT) {
    double v = 0.0;
    if (i < m) v = au[i];
    if (!isfinite(v)) a[0] = 1.0;
    x[i] = v;
    a[1] = fma(v, v, a[1]);
  }
  {
    const float* g = p.spec.row(f);
    for (int i = t; i < p.n_bins; i += kVT)
      if (!isfinite(g[i])) a[0] = 1.0;
  }
  block_sums<2, kVW>(a, red);  // (the barriers publish x)
  if (a[0] > 0.0) {  // (uniform)
    if (t < 3) o[14 + t] = 0.0;
    return;
  }

  // c[l] over [lag_lo, lag_hi) in blocks of B lags; G blocks a pass, the samples split `ns` ways
  const int nl = p.lag_hi - p.lag_lo, G = (nl + B - 1) / B;
  const int per = min(G, kVT), ns = kVT / per;
  double best = -INFINITY;
  int best_lag = 0x7fffffff;
  for (int g0 = 0; g0 < G; g0 += per) {  // (uniform trip count)
    const int gi = t % per, sp = t / per, g = g0 + gi;
    if (sp < ns) {
      double acc[B];
#pragma unroll
      for (int r = 0; r < B; ++r) acc[r] = 0.0;
      if (g < G) {
        const int l0 = p.lag_lo + g * B;
        const int len = (m - l0 + 3) & ~3;                   // lag l0's m - l0 products, in fours
        const int chunk = (((len + ns - 1) / ns) + 3) & ~3;
        const int n0 = min(sp * chunk, len), n1 = min(n0 + chunk, len);
        for (int n = n0; n < n1; n += 4) {
          double u[4], v[B + 3];
#pragma unroll
          for (int j = 0; j < 4; ++j) u[j] = x[n + j];
#pragma unroll
          for (int j = 0; j < B + 3; ++j) v[j] = x[n + l0 + j];  // (at most x[m + 5]: the zeros)
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < B; ++r) acc[r] = fma(u[j], v[j + r], acc[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < B; ++r) part[(sp * per + gi) * B + r] = acc[r];
    }
    __syncthreads();
    for (int k = t; k < per * B; k += kVT) {
      const int lag = p.lag_lo + g0 * B + k;
      if (lag >= p.lag_hi) continue;
      double c = part[k];
      for (int q = 1; q < ns; ++q) c += part[q * per * B + k];
      if (c > best) {  // (ascending lags on a thread: the first of equal values stays)
        best = c;
        best_lag = lag;
      }
    }
    __syncthreads();
  }
  // np.argmax: the greatest value, the lowest lag among equal ones
#pragma unroll
  for (int q = 32; q > 0; q >>= 1) {
    const double ob = __shfl_xor(best, q, 64);
    const int ol = __shfl_xor(best_lag, q, 64);
    if (ob > best || (ob == best && ol < best_lag)) {
      best = ob;
      best_lag = ol;
    }
  }
  if ((t & 63) == 0) {
    red[t >> 6] = best;
    red[kVW + (t >> 6)] = (double)best_lag;
  }
  __syncthreads();
  if (t == 0) {
    for (int q = 1; q < kVW; ++q) {
      const double ob = red[q];
      const int ol = (int)red[kVW + q];
      if (ob > best || (ob == best && ol < best_lag)) {
        best = ob;
        best_lag = ol;
      }
    }
    o[14] = a[1];
    o[15] = (double)best_lag;
    o[16] = best;
  }
}

}  // namespace

__global__ __launch_bounds__(kVT) void voice_kernel(VoiceParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vc_smem[];
  __shared__ double red[kVW * 3];
  __shared__ double part[kVT * kVoiceLagBlock];
  __shared__ int first[4];
  const int64_t b = blockIdx.x;
  if (b < p.n_frames)
    voice_spectrum(p, b, vc_smem, red, first);
  else
    voice_audio(p, b - p.n_frames, vc_smem, red, part);
}

size_t voice_lds_bytes(int n_bins, int m, int pitch) {
  const size_t spec = (size_t)n_bins * 2 * sizeof(float);
  const size_t audio = pitch ? (size_t)(m + kVoicePad) * sizeof(double) : 0;
  return std::max(spec, audio);
}

hipError_t launch_voice(const VoiceParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const size_t lds = voice_lds_bytes(p.n_bins, p.m, p.pitch);
  if (lds + 9 * 1024 > 64 * 1024) {  // (the kernel's static arrays take under 9 KiB)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&voice_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(voice_kernel, dim3((unsigned)(p.n_frames * (p.pitch ? 2 : 1))), dim3(kVT), lds, s, p);
  return hipGetLastError();
}

}  // namespace omega
