// HarmonicAnalyzer.detect_harmonic_series (omega4/panels/harmonic_analysis.py:193-333) with the
// HarmonicMetrics it calls (omega4/analyzers/harmonic_metrics.py:51-357) for a batch of frames:
// harmonic_kernel runs two 256-thread workgroups per frame, one per role, and harmonic_combine_kernel
// (same stream, one thread per frame) gates the formants on "a series was found". No workgroup waits
// for another: stream order is the only dependency. Every loop has a fixed bound.
//
//   role 0, the spectrum side (n_bins float32 magnitudes in LDS, freqs a float64 table)
//     :199-203  scipy.signal.find_peaks(height = 0.1 max, distance = 10): plateau-aware local maxima
//               (the middle (left + right) // 2 of a flat top whose two sides fall), the float32 height
//               threshold, then scipy's distance rule over ALL peaks, highest first, in the parallel form
//               of peaks.hpp (an undecided peak that no undecided peak within 9 bins exceeds is kept and
//               removes the peaks within 9 bins)
//     :281-333  one lane per (peak, harmonic) for the surviving peaks with 20 <= f <= 2000: the nearest
//               bin (np.argmin's first minimum, by bisection of the increasing table and a comparison
//               of the neighbours' actual distances), the 5 % acceptance, relative_strength and the
//               weighted strength score in float32 operation for operation (NEP 50: the reference's
//               float32 scalars stay float32 against Python floats); series with strength > 0.3 are
//               kept and ranked by strength, descending and stable
//     metrics   for the dominant fundamental (the first series): THD (:51-82), THD+N (:84-113),
//               centroid / spread / rolloff (:198-256), flux against the previous frame (:227-241),
//               inharmonicity (:326-357), HNR (:258-296, the noise bins by a mask test, never by
//               subtracting intervals). Powers and sums accumulate in float64 from the float32 bins;
//               the one float32 sum kept is np.sum(|x|), the float32 pairwise sum that divides the
//               float64 centroid and variance in the reference (numpy_emul.hpp's leaf order).
//   role 1, formants (:115-196), float64: pre-emphasis 0.97, np.hamming, autocorrelation lags 0..14 as
//     direct sums, the reference's recursion AS WRITTEN (every reflection sum is divided by r[0], not by
//     the running prediction error), and the 14 roots of z^14 + a1 z^13 + ... + a14 by the
//     Aberth-Ehrlich simultaneous iteration in complex float64 on 14 lanes of wave 0.
//
// Root iteration. Every lane of the wave runs the same trip count: the largest relative update
// max_j |dz_j| / max(1, |z_j|) is reduced over the wave, the loop ends two iterations after it first
// falls to kHmRootTol = 1e-10, or at kHmMaxIter; a frame that does not get there sets flag 1 and gives no
// formants. Real roots: np.roots returns an exactly zero imaginary part for a real eigenvalue, which
// the reference drops at imag > 0; the complex iteration leaves a rounding residue there instead
// (about 1e-17 on a negative real root, whose angle just under pi would pass as a frequency just under
// Nyquist). A root is therefore REAL, and dropped, when |imag| <= kHmRealTol max(1, |z|) with kHmRealTol =
// 1e-8 = 100 x the convergence tolerance: anything smaller is not distinguishable from the iteration's
// own error.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)  // (above the project headers: numpy_emul.hpp, peaks.hpp and wg64.hpp take this state)

#include "numpy_emul.hpp"
#include "params.hpp"
#include "peaks.hpp"
#include "wg64.hpp"

namespace omega {

namespace {

constexpr int kHT = kHarmonicThreads;
constexpr int kHmDistance = 10;     // find_peaks(distance=10): a kept peak removes those < 10 bins away
constexpr int kHmMaxPeaks = 832;    // kept peaks are >= 10 bins apart: at most ceil(8193 / 10) = 820
constexpr int kHmMaxIter = 200;
constexpr double kHmRootTol = 1e-10;
constexpr double kHmRealTol = 1e-8;
constexpr double kHmTwoPi = 2.0 * 3.14159265358979323846;

// np.argmin(np.abs(freqs - target)) for the strictly increasing table: the first index at or above the
// target by bisection (14 halvings cover 8193 entries), then the actual distances of the entries around
// it compared in ascending order with <, which keeps numpy's first minimum on a tie
__device__ __forceinline__ int hm_nearest(const double* __restrict__ fr, int K, double target) {
  int lo = 0, hi = K;
#pragma unroll 1
  for (int it = 0; it < 14; ++it) {
    if (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (fr[mid] < target) lo = mid + 1;
      else hi = mid;
    }
  }
  int best = max(0, min(K - 1, lo - 2));
  double bd = fabs(fr[best] - target);
#pragma unroll
  for (int d = -1; d <= 1; ++d) {
    const int j = lo + d;
    if (j > best && j < K) {
      const double dj = fabs(fr[j] - target);
      if (dj < bd) bd = dj, best = j;
    }
  }
  return best;
}

__device__ __forceinline__ double2 hm_zdiv(double2 a, double2 b) {
  const double d = b.x * b.x + b.y * b.y;
  return {(a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d};
}

// the harmonic n = h + 1 of the fundamental at bin pb: its bin when accepted (:292-316), else -1
__device__ __forceinline__ int hm_harmonic_bin(const HarmonicParams& p, int pb, int n) {
  const double f0 = p.freqs[pb];
  const double hf = f0 * n;
  if (!(hf <= p.nyquist)) return -1;
  const int idx = hm_nearest(p.freqs, p.n_bins, hf);
  return fabs(p.freqs[idx] - hf) <= f0 * 0.05 ? idx : -1;
}

}  // namespace

__global__ __launch_bounds__(kHT) void harmonic_kernel(HarmonicParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hm_smem[];
  __shared__ double red[8];
  __shared__ double sd[16];
  __shared__ int si[32];
  __shared__ double dv[16];
  __shared__ double tots[kHT];
  __shared__ int icnt[kHT];
  __shared__ unsigned ltab[kNpMaxLeaves];
  __shared__ float lsum[kNpMaxLeaves];
  __shared__ double ca[16], cn[16], rr[16], fmt[4];
  const int t = threadIdx.x;
  const int64_t f = blockIdx.x >> 1;
  const int role = blockIdx.x & 1;
  double* o = p.out + f * kHarmonicCols;

  if (role == 0) {
    const int K = p.n_bins;
    const int Kp = (K + 15) & ~15;
    float* spec = reinterpret_cast<float*>(hm_smem);                    // [Kp]
    unsigned char* und = hm_smem + (size_t)Kp * 4;                      // [Kp] 1: a peak the distance rule has not decided
    unsigned char* kept = und + Kp;                                     // [Kp] 1: a peak the distance rule keeps
    int* pk = reinterpret_cast<int*>(kept + Kp);                        // [kHmMaxPeaks] kept peaks in 20..2000 Hz, ascending
    float* str = reinterpret_cast<float*>(pk + kHmMaxPeaks);            // [kHmMaxPeaks] their strength scores
    int* ord = reinterpret_cast<int*>(str + kHmMaxPeaks);               // [kHmMaxPeaks] rank -> index into pk
    const double* __restrict__ fr = p.freqs;
    const float* sp = p.spec.row(f);
    const float* prev = f > 0 ? p.spec.row(f - 1) : p.prev_in;
    float* keep_out = f == p.n_frames - 1 ? p.prev_out : nullptr;  // :264: stored whatever the frame holds
    int* sb = p.series_bins ? p.series_bins + f * p.max_series * (1 + kHarmonicMaxHarm) : nullptr;
    double* ss = p.series_strength ? p.series_strength + f * p.max_series : nullptr;

    double mx = -INFINITY, bad = 0.0;
    for (int i = t; i < K; i += kHT) {
      const float v = sp[i];
      spec[i] = v;
      und[i] = 0;
      kept[i] = 0;
      if (keep_out) keep_out[i] = v;
      if (!isfinite(v)) bad = 1.0;
      mx = fmax(mx, (double)v);
    }
    const double nbad = block_sum(bad, red);
    mx = block_max(mx, red);
    int count = 0;
    int npk = 0;
    if (nbad == 0.0) {
      // ---- find_peaks ----
      const float hmin = __fmul_rn((float)mx, 0.1f);  // np.float32 max x Python float: float32
      int any = 0;
      for (int i = 1 + t; i < K - 1; i += kHT) {
        const int pkx = local_max_at(spec, K, i);
        if (pkx >= 0 && spec[i] >= hmin) und[pkx] = 1, any = 1;  // (spec[i] is the plateau's height)
      }
      select_by_distance<kHT>(spec, und, kept, 0, K, kHmDistance, any);
      // ---- the kept peaks with 20 <= f <= 2000, in ascending order ----
      const int C = (K + kHT - 1) / kHT;
      const int c0 = min(t * C, K), c1 = min(c0 + C, K);
      int mine = 0;
      for (int i = c0; i < c1; ++i) mine += kept[i] && fr[i] >= 20.0 && fr[i] <= 2000.0;
      icnt[t] = mine;
      __syncthreads();
      int at = 0;
      for (int j = 0; j < kHT; ++j) {
        const int c = icnt[j];
        if (j < t) at += c;
        npk += c;
      }
      npk = min(npk, kHmMaxPeaks);
      for (int i = c0; i < c1; ++i)
        if (kept[i] && fr[i] >= 20.0 && fr[i] <= 2000.0) {
          if (at < kHmMaxPeaks) pk[at] = i;
          ++at;
        }
      __syncthreads();
      // ---- the strength score: 16 lanes per peak, lane h the harmonic h + 1 ----
      const int h = t & 15, gb = t & 48;
      for (int base = 0; base < npk; base += kHT / 16) {
        const int q = base + (t >> 4);
        const bool live = q < npk;
        const int pb = live ? pk[q] : 0;
        const int idx = live ? hm_harmonic_bin(p, pb, h + 1) : -1;
        const bool acc = idx >= 0;
        // :306 in float32: magnitude / (fundamental_magnitude + 1e-10)
        const float rel = acc ? __fdiv_rn(spec[idx], __fadd_rn(spec[pb], 1e-10f)) : 0.f;
        const unsigned mask = (unsigned)((__ballot(acc) >> gb) & 0xFFFFull);
        float s = 0.f;
        int taken = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float v = __shfl(rel, gb + j, 64);
          if (((mask >> j) & 1u) && taken < 8) {  // :322-324, the first eight accepted harmonics
            s = __fadd_rn(s, __fmul_rn(v, (float)(1.0 / (j + 1))));
            ++taken;
          }
        }
        const int cnt = __popc(mask);
        if (cnt >= 2) {
          double den = 0.0;
          for (int n = 1; n <= 8; ++n)
            if (n <= cnt) den += 1.0 / n;
          s = __fdiv_rn(s, (float)den);
        } else {
          s = 0.f;
        }
        if (live && h == 0) str[q] = s;
      }
      __syncthreads();
      // ---- keep strength > 0.3, rank descending and stable ----
      double mykept = 0.0;
      for (int q = t; q < npk; q += kHT) {
        const float s = str[q];
        if (!(s > 0.3f)) continue;
        int rank = 0;
        for (int j = 0; j < npk; ++j) {
          const float sj = str[j];
          rank += sj > 0.3f && (sj > s || (sj == s && j < q));
        }
        ord[rank] = q;
        mykept += 1.0;
      }
      count = (int)block_sum(mykept, red);
    }
    // ---- the series arrays: the top max_series, the rest -1 / 0 ----
    if (sb || ss) {
      const int h = t & 15;
      for (int base = 0; base < p.max_series; base += kHT / 16) {
        const int r = base + (t >> 4);
        if (r >= p.max_series) continue;
        const bool live = r < count;
        const int q = live ? ord[r] : 0;
        const int pb = live ? pk[q] : -1;
        if (sb) {
          sb[r * (1 + kHarmonicMaxHarm) + 1 + h] = live ? hm_harmonic_bin(p, pb, h + 1) : -1;
          if (h == 0) sb[r * (1 + kHarmonicMaxHarm)] = pb;
        }
        if (ss && h == 0) ss[r] = live ? (double)str[q] : 0.0;
      }
    }
    const bool ungated = p.ungated != 0 && nbad == 0.0;  // omega_harmonic_metrics: the caller's fundamental, no series needed
    if (count == 0 && !ungated) {  // no series (or a non-finite spectrum): every metric 0
      if (t < 10) o[t] = 0.0;
      if (t == 0) o[15] = nbad > 0.0 ? 2.0 : 0.0;
      return;
    }
    // ---- metrics for the dominant fundamental ----
    // sd: 0 f0, 1 thd, 2 harmonic energy (HNR)   si: 0 span start, 1 span end, 2 fundamental usable,
    // 3 HNR half width, 4..8 HNR harmonic bins (-1: not accepted)   dv[0..8]: inharmonicity deviations (-1: none)
    const double f0 = p.ungated ? p.f0 : fr[pk[ord[0]]];
    if (t == 0) {
      sd[0] = f0;
      double thd = 0.0;
      int usable = 0;
      if (f0 > 0.0 && f0 <= p.nyquist) {
        const float m = spec[hm_nearest(fr, K, f0)];
        if (!(__fmul_rn(m, m) < 1e-10f)) {  // fund_power, a float32, against the Python float
          usable = 1;
          double hs = 0.0;
          bool open = true;
          for (int n = 2; n <= 5; ++n) {
            const double hf = f0 * n;
            if (hf > p.nyquist) open = false;
            if (open) {
              const int id = hm_nearest(fr, K, hf);
              if (fabs(fr[id] - hf) < f0 * 0.1) hs += (double)spec[id] * (double)spec[id];
            }
          }
          thd = fmin(sqrt(hs / ((double)m * (double)m)) * 100.0, 100.0);
        }
      }
      sd[1] = thd;
      si[2] = usable;
      const double bwf = f0 * 0.05;
      si[0] = hm_nearest(fr, K, f0 - bwf);
      si[1] = hm_nearest(fr, K, f0 + bwf);
      const double bwd = bwf / (fr[1] - fr[0]);
      si[3] = bwd >= (double)K ? K : (int)bwd;
    } else if (t >= 1 && t <= 5) {  // HNR harmonics 1..5 (:271-285)
      const double hf = f0 * t;
      int id = -1;
      if (f0 > 0.0 && hf <= p.nyquist) {
        id = hm_nearest(fr, K, hf);
        if (!(fabs(fr[id] - hf) < f0 * 0.1)) id = -1;
      }
      si[3 + t] = id;
    } else if (t >= 6 && t <= 14) {  // inharmonicity, n = 2..10 (:337-353)
      const int n = t - 4;
      const double ef = f0 * n;
      double d = -1.0;
      if (f0 > 0.0 && ef <= p.nyquist) {
        const double range = f0 * 0.1;
        const int a = hm_nearest(fr, K, ef - range), b = hm_nearest(fr, K, ef + range);
        if (b > a) {
          int at = a;
          float best = spec[a];
          for (int i = a + 1; i < b; ++i)
            if (spec[i] > best) best = spec[i], at = i;
          d = fabs(fr[at] - ef) / ef;
        }
      }
      dv[n - 2] = d;
    }
    __syncthreads();
    const int s0 = si[0], s1 = si[1], bw = si[3];
    int hb[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) hb[k] = si[4 + k];
    double sfx = 0.0, nonf = 0.0, noise = 0.0, flux = 0.0, pbad = 0.0;
    for (int i = t; i < K; i += kHT) {
      const double v = (double)spec[i], a = fabs(v), v2 = v * v;
      sfx += fr[i] * a;
      if (i < s0 || i > s1) nonf += v2;
      bool harm = false;
#pragma unroll
      for (int k = 0; k < 5; ++k) harm = harm || (hb[k] >= 0 && i >= hb[k] - bw && i <= hb[k] + bw);
      if (!harm) noise += v2;
      if (prev) {
        const double pv = (double)prev[i];
        if (isfinite(pv)) flux += fmax(a - fabs(pv), 0.0);
        else pbad = 1.0;  // (a stored non-finite spectrum: its bins are left out and the frame is flagged)
      }
    }
    pbad = block_sum(pbad, red);
    sfx = block_sum(sfx, red);
    nonf = block_sum(nonf, red);
    noise = block_sum(noise, red);
    flux = block_sum(flux, red);
    // np.sum(|x|) in float32, numpy's pairwise order: one leaf per thread, the tree on thread 0
    if (t == 0) {
      int nl = 0;
      np_emit_leaves<7>(0, K, ltab, nl);
      si[16] = nl;
    }
    __syncthreads();
    const int nl = si[16];
    if (t < nl) {
      const float* a = spec + (ltab[t] & 0xFFFFu);
      lsum[t] = np_slice_leaf((int)(ltab[t] >> 16), [&](int i) { return fabsf(a[i]); });
    }
    __syncthreads();
    if (t == 0) {
      int idx = 0;
      sd[3] = (double)np_leaf_combine<7>(K, lsum, idx);
    }
    __syncthreads();
    const double sabs = sd[3];
    const double centroid = sabs > 0.0 ? sfx / sabs : 0.0;
    double var = 0.0;
    for (int i = t; i < K; i += kHT) {
      const double d = fr[i] - centroid;
      var += (d * d) * fabs((double)spec[i]);
    }
    var = block_sum(var, red);
    // rolloff: np.cumsum(|x|) >= 0.85 cumsum[-1], the first index
    const int C = (K + kHT - 1) / kHT;
    const int c0 = min(t * C, K), c1 = min(c0 + C, K);
    double tot = 0.0;
    for (int i = c0; i < c1; ++i) tot += fabs((double)spec[i]);
    tots[t] = tot;
    __syncthreads();
    double run = 0.0, all = 0.0;
    for (int j = 0; j < kHT; ++j) {
      if (j == t) run = all;
      all += tots[j];
    }
    const double thr = 0.85 * all;
    int first = 0x7fffffff;
    for (int i = c0; i < c1; ++i) {
      run += fabs((double)spec[i]);
      if (run >= thr && first == 0x7fffffff) first = i;
    }
    first = block_min_i(first, red);
    if (t == 0) {
      double he = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k)
        if (hb[k] >= 0) he += (double)spec[hb[k]] * (double)spec[hb[k]];
      double hnr = 60.0;
      if (noise > 0.0) hnr = fmax(0.0, fmin(10.0 * log10(he / noise), 60.0));
      if (!(f0 > 0.0)) hnr = 0.0;  // :264-265
      double dsum = 0.0;
      int dn = 0;
      for (int k = 0; k < 9; ++k)
        if (dv[k] >= 0.0) dsum += dv[k], ++dn;
      const double fp = (double)spec[hm_nearest(fr, K, f0)];
      o[0] = (double)count;
      o[1] = f0;
      o[2] = sd[1];
      o[3] = si[2] ? fmin(sqrt(nonf / (fp * fp)) * 100.0, 100.0) : 0.0;
      o[4] = centroid;
      o[5] = sabs > 0.0 ? sqrt(var / sabs) : 0.0;
      o[6] = flux;
      o[7] = all > 0.0 && first < K ? fr[first] : 0.0;
      o[8] = dn ? dsum / dn : 0.0;
      o[9] = hnr;
      o[15] = pbad > 0.0 ? 2.0 : 0.0;
    }
    return;
  }

  // ---- role 1: detect_formants_lpc (:115-196); o[10] = formant count, -1 not converged, -2 non-finite ----
  const int m = p.m;
  double* w = reinterpret_cast<double*>(hm_smem);  // [m]
  if (!p.audio.base) {
    if (t < 5) o[10 + t] = 0.0;
    return;
  }
  auto raw = [&](int i) { return p.audio.at(f, i); };
  double amax = 0.0, bad = 0.0;
  for (int i = t; i < m; i += kHT) {
    const double x = raw(i);
    if (!isfinite(x)) bad = 1.0;
    amax = fmax(amax, fabs(x));
    w[i] = (i ? x - 0.97 * raw(i - 1) : x) * p.ham[i];
  }
  bad = block_sum(bad, red);
  amax = block_max(amax, red);  // (the barriers publish w)
  if (bad > 0.0 || amax < 1e-10) {
    if (t < 5) o[10 + t] = t == 0 && bad > 0.0 ? -2.0 : 0.0;
    return;
  }
  double acc[kHarmonicLpcOrder + 1];
#pragma unroll
  for (int k = 0; k <= kHarmonicLpcOrder; ++k) acc[k] = 0.0;
  for (int i = t; i < m; i += kHT) {
    const double wi = w[i];
#pragma unroll
    for (int k = 0; k <= kHarmonicLpcOrder; ++k) acc[k] += i + k < m ? wi * w[i + k] : 0.0;
  }
#pragma unroll
  for (int k = 0; k <= kHarmonicLpcOrder; ++k) {
    const double r = block_sum(acc[k], red);
    if (t == 0) rr[k] = r;
  }
  __syncthreads();
  if (fabs(rr[0]) < 1e-10) {
    if (t < 5) o[10 + t] = 0.0;
    return;
  }
  if (t == 0) {
    // :168-196 as written: a[0] = 1; k_m = -(sum_j a[j] r[m - j]) / r[0]; a[i] += k_m a[m + 1 - i]
    for (int i = 0; i < 16; ++i) ca[i] = i == 0 ? 1.0 : 0.0;
    for (int mm = 0; mm < kHarmonicLpcOrder; ++mm) {
      double s = 0.0;
      for (int j = 0; j <= mm; ++j) s += ca[j] * rr[mm + (mm ? 0 : 1) - j];
      const double km = -s / rr[0];  // (m = 0: -r[1] / r[0], a[0] = 1)
      for (int i = 1; i <= mm + 1; ++i) cn[i] = ca[i] + km * ca[mm + 1 - i];
      for (int i = 1; i <= mm + 1; ++i) ca[i] = cn[i];
    }
    for (int k = 0; k < 4; ++k) fmt[k] = 0.0;
  }
  __syncthreads();
  if (t >= 64) return;
  // the roots of z^14 + ca[1] z^13 + ... + ca[14]: Aberth-Ehrlich on lanes 0..13 of wave 0
  const bool lane_on = t < kHarmonicLpcOrder;
  double rad = pow(fabs(ca[kHarmonicLpcOrder]), 1.0 / kHarmonicLpcOrder);  // the roots' geometric mean modulus
  if (!(rad >= 0.5)) rad = 0.5;
  if (rad > 2.0) rad = 2.0;
  const double ang0 = kHmTwoPi * (lane_on ? t : 0) / kHarmonicLpcOrder + 0.7;  // (off the real axis' symmetry)
  double2 z{rad * cos(ang0), rad * sin(ang0)};
  int done = 0, extra = 0;
#pragma unroll 1
  for (int it = 0; it < kHmMaxIter; ++it) {
    double2 pv{1.0, 0.0}, dp{0.0, 0.0};
#pragma unroll 1
    for (int k = 1; k <= kHarmonicLpcOrder; ++k) {
      dp = zmul(dp, z);
      dp.x += pv.x, dp.y += pv.y;
      pv = zmul(pv, z);
      pv.x += ca[k];
    }
    double2 S{0.0, 0.0};
#pragma unroll 1
    for (int k = 0; k < kHarmonicLpcOrder; ++k) {
      const double2 zk{__shfl(z.x, k, 64), __shfl(z.y, k, 64)};
      if (k != t) {
        const double2 q = hm_zdiv(double2{1.0, 0.0}, double2{z.x - zk.x, z.y - zk.y});
        S.x += q.x, S.y += q.y;
      }
    }
    const double2 nt = hm_zdiv(pv, dp);
    const double2 ns = zmul(nt, S);
    const double2 wv = hm_zdiv(nt, double2{1.0 - ns.x, -ns.y});
    double upd = 0.0;
    if (lane_on) {
      z.x -= wv.x, z.y -= wv.y;
      upd = sqrt(wv.x * wv.x + wv.y * wv.y) / fmax(1.0, sqrt(z.x * z.x + z.y * z.y));
      if (!(upd == upd)) upd = INFINITY;  // (NaN)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) upd = fmax(upd, __shfl_xor(upd, off, 64));
    if (upd <= kHmRootTol) done = 1;  // (wave-uniform)
    if (done && ++extra == 3) break;
  }
  const double zabs = sqrt(z.x * z.x + z.y * z.y);
  double fq = INFINITY;
  if (lane_on && done && z.y > kHmRealTol * fmax(1.0, zabs)) {
    const double v = atan2(z.y, z.x) * p.fs / kHmTwoPi;
    if (v > 50.0 && v < p.nyquist) fq = v;
  }
  int rank = 0;
#pragma unroll 1
  for (int k = 0; k < kHarmonicLpcOrder; ++k) {
    const double fk = __shfl(fq, k, 64);
    rank += fk < fq || (fk == fq && k < t);
  }
  const bool valid = fq < INFINITY;
  const int nvalid = __popcll(__ballot(valid));
  if (valid && rank < 4) fmt[rank] = fq;
  __builtin_amdgcn_wave_barrier();
  if (t == 0) o[10] = done ? (double)min(nvalid, 4) : -1.0;
  else if (t < 5) o[10 + t] = fmt[t - 1];
}

// :258-259: the formants only when a series was found; role 1's status becomes a flag
__global__ __launch_bounds__(kHT) void harmonic_combine_kernel(HarmonicParams p) {
  const int64_t f = (int64_t)blockIdx.x * kHT + threadIdx.x;
  if (f >= p.n_frames) return;
  double* o = p.out + f * kHarmonicCols;
  double flags = o[15], nf = o[10];
  if (nf < 0.0) {
    flags += nf == -1.0 ? 1.0 : (flags >= 2.0 ? 0.0 : 2.0);
    nf = 0.0;
  }
  if (o[0] < 1.0 && !p.ungated) nf = 0.0;
  o[10] = nf;
  for (int k = 0; k < 4; ++k)
    if (k >= (int)nf) o[11 + k] = 0.0;
  o[15] = flags;
}

size_t harmonic_lds_bytes(int n_bins, int m) {
  const size_t Kp = ((size_t)n_bins + 15) & ~(size_t)15;
  const size_t a = Kp * 6 + (size_t)kHmMaxPeaks * 12, b = (size_t)m * 8;
  return ((a > b ? a : b) + 15) & ~(size_t)15;
}

hipError_t launch_harmonic(const HarmonicParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const size_t lds = harmonic_lds_bytes(p.n_bins, p.audio.base ? p.m : 0);
  if (lds + 8 * 1024 > 64 * 1024) {  // (the kernel's static arrays take under 8 KiB)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&harmonic_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(harmonic_kernel, dim3((unsigned)(2 * p.n_frames)), dim3(kHT), lds, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(harmonic_combine_kernel, dim3((unsigned)((p.n_frames + kHT - 1) / kHT)), dim3(kHT), 0, s, p);
  return hipGetLastError();
}

}  // namespace omega
