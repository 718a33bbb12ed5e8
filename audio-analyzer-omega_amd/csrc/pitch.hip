// CepstralAnalyzer.detect_pitch_advanced (omega4/panels/pitch_detection.py:485-556) for a batch of
// frames of n = 2048 / 4096 / 8192 samples: pitch_kernel runs three 256-thread workgroups per frame,
// one per method, and pitch_combine_kernel (same stream, one thread per frame) weighs their estimates.
// No workgroup waits for another: stream order is the only dependency.
//
//   role 0, cepstrum, float64 like the reference's scipy path
//     :497-525  order-4 Butterworth high-pass as two DF2T sections from the zero state (sosfilt), the
//               RMS compression gain, or the "too quiet, use the original" branch
//     :132-144  np.hanning window, rfft, log(|X| + 1e-10), irfft, first n/2 values
//     :146-174  highest strict local maximum of c[min_period : min(max_period, n/2 - 1)] that reaches
//               0.3 x the range's maximum (find_peaks' strongest peak always survives its distance
//               rule); confidence min(1, height / std(c))
//     :64-93    the frame's non-finite flag and RMS (validate_audio_input)
//   role 1, autocorrelation (:176-227): x - float32 mean, zero-padded to 2n, rfft, |X|^2, irfft,
//     r / (r[0] + 1e-10); find_peaks(height = 0.3, distance = 20)'s FIRST surviving peak; confidence
//     r[period] rounded to float32 (the reference's autocorrelation is a float32 array). The
//     transforms run in float64 -- closer to the exact value than numpy's complex64 pocketfft.
//   role 2, YIN (:229-316, the vectorised path): the difference function over the first
//     yin_window samples in both of the reference's definitions -- the overlapping n - tau samples
//     below tau = min(100, max_tau), all n samples of the zero-padded signal from there on (what its
//     three-dot-product form equals) -- as direct sums of squared float32 differences accumulated in
//     float64, the cumulative mean normalised difference, the first strict local minimum below the
//     threshold and the parabolic refinement (:363-371).
//
// Real transforms of N points run as N/2-point complex FFTs in place in LDS (decimation in frequency,
// natural -> bit-reversed order; the real-even spectrum g(|X|) is packed for the inverse pair-wise in
// bit-reversed order; decimation in time back to natural order), so a frame needs n x 16 bytes for
// the autocorrelation's 2n-point transform and half that for the cepstrum's.
//
// The transform pair, the block reductions and the high-pass sections' chunked scan are wg64.hpp's,
// compiled here with the default contraction (fused multiply-adds).
//
// Flat tops: scipy's find_peaks takes the middle of a plateau; here a peak is a strict local maximum
// (x[i-1] < x[i] > x[i+1]). Float data does not produce plateaus above the height thresholds; a frame
// of equal samples is silent and gives the zero row.
#include <hip/hip_runtime.h>

#include "params.hpp"
#include "peaks.hpp"
#include "wg64.hpp"

namespace omega {

namespace {

constexpr int kPT = kPitchThreads;
constexpr int kPeakDistance = 20;  // find_peaks(distance=20): a kept peak removes those < 20 lags away

// irfft(g(|rfft(x)|^2)) of the 2K real samples held as a[j] = x[2j] + i x[2j+1]: on return
// a[m] = (y[2m], y[2m+1]) of the 2K-point real result y. g maps |X_q|^2 to the real, even spectrum.
template <class G>
__device__ void pt_real_even_roundtrip(double2* a, int K, int bits, const double2* __restrict__ tw, int tws, G g) {
  fft_dif<kPT>(a, K, tw, 2 * tws);
  // X_q (q = 0..K) from the packed spectrum Z: X_q = (Z_q + conj Z_{K-q}) / 2 + e^{-2 pi i q / 2K} (Z_q - conj Z_{K-q}) / 2i.
  // With L_q = g(|X_q|^2) the packed inverse spectrum is Z'_k = (L_k + L_{K-k}) + i e^{2 pi i k / 2K} (L_k - L_{K-k}),
  // stored conjugated so that the forward transform returns conj(K ifft). Bins k and K - k read and
  // write the same two slots, so one thread does the pair.
  for (int k = threadIdx.x; k <= K / 2; k += kPT) {
    const int m = (K - k) & (K - 1);
    const int pk = brev(k, bits), pm = brev(m, bits);
    const double2 zk = a[pk], zm = a[pm];
    auto L = [&](double2 za, double2 zb, int q) {  // g(|X_q|^2), za = Z_q, zb = Z_{K-q}
      const double2 e = make_double2(0.5 * (za.x + zb.x), 0.5 * (za.y - zb.y));
      const double2 o = make_double2(0.5 * (za.y + zb.y), -0.5 * (za.x - zb.x));
      const double2 ow = zmul(o, tw[q * tws]);
      const double re = e.x + ow.x, im = e.y + ow.y;
      return g(re * re + im * im);
    };
    const double Lk = L(zk, zm, k);
    const double Lm = k == 0 ? L(zk, zk, K) : L(zm, zk, K - k);  // (k = 0: X_K from Z_0 alone)
    auto pack = [&](double la, double lb, int q) {  // conj Z'_q, la = L_q, lb = L_{K-q}
      const double2 w = tw[q * tws];                 // e^{-2 pi i q / 2K}; i conj(w) (la - lb)
      const double d = la - lb;
      return make_double2((la + lb) + w.y * d, -(w.x * d));
    };
    a[pk] = pack(Lk, Lm, k);
    if (m != k) a[pm] = pack(Lm, Lk, m);
  }
  __syncthreads();
  fft_dit<kPT>(a, K, tw, 2 * tws);
  const double sc = 0.5 / K;
  for (int m = threadIdx.x; m < K; m += kPT) {
    const double2 v = a[m];
    a[m] = make_double2(v.x * sc, -v.y * sc);
  }
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(kPT) void pitch_kernel(PitchParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pt_smem[];
  const int t = threadIdx.x;
  const int n = p.n;
  const int64_t f = blockIdx.x / 3;
  const int role = blockIdx.x % 3;
  double* buf = reinterpret_cast<double*>(pt_smem);                        // [2 n]
  double2* sc = reinterpret_cast<double2*>(pt_smem + (size_t)n * 16);     // [kPT]
  double* red = reinterpret_cast<double*>(sc + kPT);                       // [4]
  double* o = p.out + f * kPitchCols;
  auto raw = [&](int i) { return p.x.at(f, i); };
  auto xin = [&](int i) -> float { return (float)raw(i); };  // the reference's astype(np.float32) (:587-588)
  int bits = 0;
  while ((1 << bits) < n) ++bits;  // log2 n

  if (role == 0) {
    // validation (:64-93) and the frame as float64
    double ss = 0.0, bad = 0.0;
    for (int i = t; i < n; i += kPT) {
      const double r = raw(i);
      if (!isfinite(r)) bad = 1.0;
      const double v = (double)(float)r;
      buf[i] = v;
      ss += v * v;
    }
    const double nbad = block_sum(bad, red);
    const double rms_in = sqrt(block_sum(ss, red) / n);
    if (t == 0) {
      o[8] = nbad > 0.0 ? 0.0 : rms_in;
      o[9] = (nbad > 0.0 ? 1.0 : 0.0) + (rms_in < 1e-6 ? 2.0 : 0.0);
    }
    __syncthreads();
    if (p.preprocess) {
      auto section = [&](const W64Stage& q) { sos_section_scan<kPT>(buf, n, q.b0, q.b1, q.b2, q.a1, q.a2, sc); };
      section(p.hp[0]);
      section(p.hp[1]);
      double fs2 = 0.0;
      for (int i = t; i < n; i += kPT) fs2 += buf[i] * buf[i];
      const double rms = sqrt(block_sum(fs2, red) / n);
      if (p.compress) {
        if (rms > 0.01 && rms > p.comp_threshold) {
          const double gain = p.comp_threshold + (rms - p.comp_threshold) * p.comp_ratio;
          const double gr = gain / rms;
          for (int i = t; i < n; i += kPT) buf[i] *= gr;
        }
      } else if (rms < 0.01) {
        for (int i = t; i < n; i += kPT) buf[i] = (double)xin(i);
      }
    }
    for (int i = t; i < n; i += kPT) buf[i] *= p.win[i];
    __syncthreads();
    const int K = n / 2;
    pt_real_even_roundtrip(reinterpret_cast<double2*>(buf), K, bits - 1, p.tw, 2,
                           [](double m2) { return log(sqrt(m2) + 1e-10); });
    // c = buf[0..K): np.std, the range's maximum, the highest strict local maximum
    double s1 = 0.0;
    for (int i = t; i < K; i += kPT) s1 += buf[i];
    const double mean = block_sum(s1, red) / K;
    double s2 = 0.0;
    for (int i = t; i < K; i += kPT) {
      const double d = buf[i] - mean;
      s2 += d * d;
    }
    const double sd = sqrt(block_sum(s2, red) / K);
    const int lo = p.min_period, hi = min(p.max_period, K - 1);
    double vmax = -INFINITY;
    for (int i = lo + t; i < hi; i += kPT) vmax = fmax(vmax, buf[i]);
    vmax = block_max(vmax, red);
    const double hmin = vmax * 0.3;
    double best = -INFINITY;
    for (int i = lo + 1 + t; i < hi - 1; i += kPT) {
      const double v = buf[i];
      if (buf[i - 1] < v && v > buf[i + 1] && v >= hmin) best = fmax(best, v);
    }
    best = block_max(best, red);
    int at = 0x7fffffff;
    for (int i = lo + 1 + t; i < hi - 1; i += kPT) {
      const double v = buf[i];
      if (buf[i - 1] < v && v > buf[i + 1] && v >= hmin && v == best) at = min(at, i);
    }
    at = block_min_i(at, red);
    if (t == 0) {
      const bool found = hi > lo && best > -INFINITY && at < hi;
      o[2] = found ? p.fs / at : 0.0;
      o[3] = found ? fmin(1.0, best / sd) : 0.0;
    }
  } else if (role == 1) {
    // :179: x - np.mean(x) in float32, zero-padded to 2n, packed two samples per complex value
    double s = 0.0;
    for (int i = t; i < n; i += kPT) s += (double)xin(i);
    const float mean = (float)(block_sum(s, red) / n);
    double2* a = reinterpret_cast<double2*>(buf);
    for (int j = t; j < n; j += kPT)
      a[j] = 2 * j < n ? make_double2((double)(xin(2 * j) - mean), (double)(xin(2 * j + 1) - mean)) : make_double2(0.0, 0.0);
    __syncthreads();
    pt_real_even_roundtrip(a, n, bits, p.tw, 1, [](double m2) { return m2; });
    // r[0..n) = buf[0..n), normalised (:192-193); buf[n..2n) is free from here on
    const double r0 = buf[0] + 1e-10;
    __syncthreads();
    for (int i = t; i < n; i += kPT) buf[i] = buf[i] / r0;
    int* und = reinterpret_cast<int*>(buf + n);  // [n] 1: a peak the distance rule has not decided
    int* kept = und + n;                          // [n] 1: a peak the distance rule keeps
    __syncthreads();
    const int lo = p.min_period, hi = min(p.max_period, n - 1);
    int any = 0;
    for (int i = lo + t; i < hi; i += kPT) {
      const double v = buf[i];
      const int pk = i > lo && i < hi - 1 && buf[i - 1] < v && v > buf[i + 1] && v >= 0.3;
      und[i] = pk;
      kept[i] = 0;
      any |= pk;
    }
    // scipy's _select_by_peak_distance over the candidates of [lo, hi), in the parallel form of peaks.hpp
    select_by_distance<kPT>(buf, und, kept, lo, hi, kPeakDistance, any);
    int first = 0x7fffffff;
    for (int i = lo + t; i < hi; i += kPT)
      if (kept[i]) first = min(first, i);
    first = block_min_i(first, red);
    if (t == 0) {
      const bool found = hi > lo && first < hi;
      o[4] = found ? p.fs / first : 0.0;
      o[5] = found ? (double)(float)buf[first] : 0.0;
    }
  } else {
    const int W = p.yin_window;
    const int max_tau = min(p.max_period, W / 2), small_tau = min(100, max_tau);
    float* xs = reinterpret_cast<float*>(pt_smem);                                              // [W + max_tau]
    double* d = reinterpret_cast<double*>(pt_smem + ((((size_t)(W + max_tau) * 4) + 15) & ~(size_t)15));  // [max_tau]
    for (int i = t; i < W + max_tau; i += kPT) xs[i] = i < W ? xin(i) : 0.f;
    __syncthreads();
    // difference function: four lags per lane, x[j] a broadcast read, x[j + tau] consecutive over lanes
    for (int base = 0; base < max_tau; base += 4 * kPT) {
      int tau[4], lim[4];
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int tk = base + t + k * kPT;
        tau[k] = tk < max_tau ? tk : 0;
        lim[k] = tau[k] < small_tau ? W - tau[k] : W;  // overlap only below small_tau, else the padded sum
      }
      for (int j = 0; j < W; ++j) {
        const float xj = xs[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double df = (double)(xj - xs[j + tau[k]]);
          acc[k] = j < lim[k] ? fma(df, df, acc[k]) : acc[k];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int tk = base + t + k * kPT;
        if (tk < max_tau) d[tk] = tk == 0 ? 0.0 : acc[k];
      }
    }
    __syncthreads();
    // np.cumsum (float64) and the cumulative mean normalised difference d tau / cumsum, in place
    const int C = (max_tau + kPT - 1) / kPT;
    const int c0 = min(t * C, max_tau), c1 = min(c0 + C, max_tau);
    double tot = 0.0;
    for (int i = c0; i < c1; ++i) tot += d[i];
    double* tots = reinterpret_cast<double*>(sc);
    tots[t] = tot;
    __syncthreads();
    double run = 0.0;
    for (int j = 0; j < t; ++j) run += tots[j];
    for (int i = c0; i < c1; ++i) {
      run += d[i];
      d[i] = i == 0 ? 1.0 : d[i] * i / run;
    }
    __syncthreads();
    int first = 0x7fffffff;
    for (int i = p.min_period + t; i < max_tau - 1; i += kPT) {
      const double v = d[i];
      if (i >= 1 && v < p.yin_threshold && v < d[i - 1] && v < d[i + 1]) first = min(first, i);
    }
    first = block_min_i(first, red);
    if (t == 0) {
      const bool found = n >= W && first < max_tau - 1;
      double pitch = 0.0, conf = 0.0;
      if (found) {
        const double y1 = d[first - 1], y2 = d[first], y3 = d[first + 1];
        const double a = (y1 - 2 * y2 + y3) / 2, b = (y3 - y1) / 2;
        const double tf = a != 0.0 ? first + (-b / (2 * a)) : (double)first;
        pitch = p.fs / tf;
        conf = 1.0 - y2;
      }
      o[6] = pitch;
      o[7] = conf;
    }
  }
}

// combine_pitch_estimates (:384-433), its acceptance thresholds and weights as the reference
// hard-codes them, in the reference's operation order (no contraction: __dmul_rn / __dadd_rn); frames
// flagged non-finite or silent give the zero row
__global__ __launch_bounds__(kPT) void pitch_combine_kernel(PitchParams p) {
  const int64_t f = (int64_t)blockIdx.x * kPT + threadIdx.x;
  if (f >= p.n_frames) return;
  double* o = p.out + f * kPitchCols;
  if (o[9] != 0.0) {
    for (int k = 0; k < 8; ++k) o[k] = 0.0;
    return;
  }
  double ep[3], ew[3];
  int ne = 0;
  auto in_range = [&](double v) { return p.min_pitch <= v && v <= p.max_pitch; };
  if (o[3] > 0.15 && in_range(o[2])) ep[ne] = o[2], ew[ne++] = __dmul_rn(o[3], 0.8);
  // the autocorrelation confidence is a float32 scalar: its comparison and its weight are float32 (NEP 50)
  if ((float)o[5] > 0.2f && in_range(o[4])) ep[ne] = o[4], ew[ne++] = (double)__fmul_rn((float)o[5], 0.9f);
  if (o[7] > 0.25 && in_range(o[6])) ep[ne] = o[6], ew[ne++] = __dmul_rn(o[7], 1.1);
  if (ne == 0) {
    o[0] = 0.0;
    o[1] = 0.0;
    return;
  }
  double tw = 0.0, wp = 0.0, ps = 0.0;
  for (int k = 0; k < ne; ++k) {
    tw = __dadd_rn(tw, ew[k]);
    wp = __dadd_rn(wp, __dmul_rn(ep[k], ew[k]));
    ps = __dadd_rn(ps, ep[k]);
  }
  double conf = tw / ne;
  if (ne >= 2) {
    const double mean = ps / ne;
    double var = 0.0;
    for (int k = 0; k < ne; ++k) {
      const double d = __dadd_rn(ep[k], -mean);
      var = __dadd_rn(var, __dmul_rn(d, d));
    }
    const double ratio = sqrt(var / ne) / mean;
    if (ratio < 0.02) conf = fmin(1.0, __dmul_rn(conf, 1.2));
    else if (ratio > 0.05) conf = __dmul_rn(conf, 0.8);
  }
  o[0] = wp / tw;
  o[1] = conf;
}

size_t pitch_lds_bytes(int n) { return (size_t)n * 16 + kPT * sizeof(double2) + 64; }

hipError_t launch_pitch(const PitchParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const size_t lds = pitch_lds_bytes(p.n);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pitch_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pitch_kernel, dim3((unsigned)(3 * p.n_frames)), dim3(kPT), lds, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pitch_combine_kernel, dim3((unsigned)((p.n_frames + kPT - 1) / kPT)), dim3(kPT), 0, s, p);
  return hipGetLastError();
}

}  // namespace omega
