// GenreClassifier.extract_features (omega4/panels/genre_classification.py:175-254) with the compute_* /
// estimate_* helpers it calls (:256-422, :600-783) for a batch of frames of one stream: genre_kernel runs
// two 256-thread workgroups per frame, one per role, and genre_combine_kernel (same stream, one thread
// per frame) turns a role's "non-finite input" mark into the flagged zero row. No workgroup waits for
// another: stream order is the only dependency. Every loop has a fixed bound.
//
//   role 0, the spectrum side (magnitude = |spectrum|, n_bins float32 in LDS; freqs a float64 table)
//     :600-626  centroid and bandwidth: float64 sums divided by np.sum(magnitude), the float32 pairwise sum
//     :606-614  rolloff: np.cumsum(magnitude) is a SEQUENTIAL float32 sum. Lane 0 of wave 0 walks the LDS
//               copy (eight loads per step, which do not depend on the add chain) and writes the running
//               sums to LDS while waves 1..3 do the barrier-free work below; then all lanes compare with
//               float32(0.85) * cumsum[-1] and a min-reduction gives the first index
//     band energies (:319-349, :406-422, :709-783): every mask over the increasing table is a contiguous
//               bin range found by the host; np.sum(magnitude[mask] ** 2) is numpy's float32 pairwise sum of
//               the float32 squares over the slice (numpy_emul.hpp's slice form: the leaves of all twelve
//               sums are listed by twelve lanes, summed by waves 1..3, combined by twelve lanes); the
//               ratios follow in float32, operation for operation (contraction is off in this file)
//     :382-404  flatness over 100..4000 Hz in float64 from the float32 bins above float32(1e-10)
//     :256-276  flux against the previous magnitude: float32 pairwise sum of max(0, magnitude - prev)
//     :278-317  distortion: strict local maxima above float32(np.mean(magnitude) * 2), the five largest
//               (ties to the lower bin) by five max-reductions of (magnitude bits, ~bin), one lane per peak
//               for the harmonics 2..5
//   role 1, the audio side (|x| in LDS as bit patterns, float32 or float64 like the input)
//     :616-619  sign changes, sign(0) = 0
//     :628-636  np.percentile(|x|, 95) and (|x|, 20): the order statistics at floor(q (m - 1)) and the next
//               by a radix select (8 bits per pass, most significant first; non-negative floats order as
//               unsigned integers), interpolated as numpy's _lerp does in the input's precision
//     :852      rms: float32 input np.sqrt(np.mean(x ** 2)) bit for bit, float64 input in float64
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)  // (above the project headers: numpy_emul.hpp and wg64.hpp take this state)

#include "numpy_emul.hpp"
#include "params.hpp"
#include "wg64.hpp"

namespace omega {

namespace {

constexpr int kGT = kGenreThreads;
constexpr int kGnSums = 12;        // np.sum(mag), the flux sum, np.sum(mag ** 2), nine band energies
constexpr int kGnWork = kGT - 64;  // the lanes of waves 1..3

__device__ __forceinline__ unsigned long long gn_max_u64(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const unsigned long long a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
  return a > b ? a : b;
}
// inclusive prefix sum over the workgroup
__device__ __forceinline__ int gn_scan(int v, int* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  __syncthreads();
  if (lane == 63) sh[w] = v;
  __syncthreads();
  for (int j = 0; j < w; ++j) v += sh[j];
  return v;
}

// the key of rank `rank` (0-based, ascending) among keys[0 .. m): 8 bits per pass from the top
template <class U>
__device__ __forceinline__ U gn_select(const U* keys, int m, int rank, int* hist, int* sh, int* pick) {
  const int t = threadIdx.x;
  U prefix = 0, mask = 0;
  int r = rank;
#pragma unroll 1
  for (int shift = (int)sizeof(U) * 8 - 8; shift >= 0; shift -= 8) {
    hist[t] = 0;
    __syncthreads();
    for (int i = t; i < m; i += kGT) {
      const U k = keys[i];
      if ((k & mask) == prefix) atomicAdd(&hist[(int)((k >> shift) & (U)255)], 1);
    }
    __syncthreads();
    const int c = hist[t];
    const int incl = gn_scan(c, sh), excl = incl - c;
    if (excl <= r && r < incl) pick[0] = t, pick[1] = r - excl;
    __syncthreads();
    prefix |= (U)pick[0] << shift;
    mask |= (U)255 << shift;
    r = pick[1];
  }
  return prefix;
}

__device__ __forceinline__ float gn_from_bits(unsigned k) { return __uint_as_float(k); }
__device__ __forceinline__ double gn_from_bits(unsigned long long k) { return __longlong_as_double((long long)k); }
__device__ __forceinline__ unsigned gn_bits(float v) { return __float_as_uint(v); }
__device__ __forceinline__ unsigned long long gn_bits(double v) { return (unsigned long long)__double_as_longlong(v); }

// numpy's _lerp(a, b, t): a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5
template <class T>
__device__ __forceinline__ T gn_lerp(T a, T b, T t) {
  const T d = b - a;
  T r = a + d * t;
  if (t >= (T)0.5) r = b - d * ((T)1 - t);
  return r;
}

// role 1 for audio of type T (float / double), U its bit pattern
template <class T, class U>
__device__ __forceinline__ void gn_audio(const GenreParams& p, int64_t f, double* o, unsigned char* smem, double* red,
                                         int* hist, int* sh, int* pick, unsigned* ltab, float* lsum) {
  const int t = threadIdx.x, m = p.m;
  const T* x = p.audio.row_as<T>(f);
  U* keys = reinterpret_cast<U*>(smem);
  double bad = 0.0, zc = 0.0, sq = 0.0;
  for (int i = t; i < m; i += kGT) {
    const T v = x[i];
    if (!isfinite(v)) bad = 1.0;
    keys[i] = gn_bits((T)fabs(v));
    if (i + 1 < m) {
      const T w = x[i + 1];
      const int sa = (v > (T)0) - (v < (T)0), sb = (w > (T)0) - (w < (T)0);
      zc += sa != sb;
    }
    sq += (double)v * (double)v;
  }
  bad = block_sum(bad, red);
  if (bad > 0.0) {  // (uniform) the combine kernel zeroes the row
    if (t == 0) o[3] = -1.0;
    return;
  }
  zc = block_sum(zc, red);
  sq = block_sum(sq, red);
  double rms;
  if constexpr (sizeof(T) == 4) {
    // (|x| from the keys: the squares are the same)
    rms = (double)np_rms_f32(reinterpret_cast<const float*>(keys), m, ltab, lsum, &pick[2]);
  } else {
    rms = sqrt(sq / (double)m);
  }
  const T lo95 = gn_from_bits(gn_select<U>(keys, m, p.rank95, hist, sh, pick));
  const T hi95 = gn_from_bits(gn_select<U>(keys, m, p.rank95 + 1, hist, sh, pick));
  const T lo20 = gn_from_bits(gn_select<U>(keys, m, p.rank20, hist, sh, pick));
  const T hi20 = gn_from_bits(gn_select<U>(keys, m, p.rank20 + 1, hist, sh, pick));
  if (t == 0) {
    const T loud = gn_lerp<T>(lo95, hi95, (T)p.gamma95), quiet = gn_lerp<T>(lo20, hi20, (T)p.gamma20);
    T dr = (T)0;
    if (quiet > (T)0) {
      dr = (loud - quiet) / loud;
      if (!(dr < (T)1)) dr = (T)1;  // min(1.0, dr)
    }
    o[3] = zc;
    o[5] = (double)dr;
    o[6] = (double)loud;
    o[7] = (double)quiet;
    o[8] = rms;
  }
}

}  // namespace

__global__ __launch_bounds__(kGT) void genre_kernel(GenreParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gn_smem[];
  __shared__ double red[8];
  __shared__ unsigned long long redu[4];
  __shared__ int hist[kGT];
  __shared__ int sh[4];
  __shared__ int pick[4];
  __shared__ unsigned ltab[kGnSums * kNpMaxLeaves];
  __shared__ float lsum[kGnSums * kNpMaxLeaves];
  __shared__ int nleaf[kGnSums];
  __shared__ float sres[kGnSums];
  __shared__ int pk[kGenrePeaks];
  const int t = threadIdx.x;
  const int64_t f = blockIdx.x >> 1;
  double* o = p.out + f * kGenreCols;

  if (blockIdx.x & 1) {
    if (p.audio.f64) gn_audio<double, unsigned long long>(p, f, o, gn_smem, red, hist, sh, pick, ltab, lsum);
    else gn_audio<float, unsigned>(p, f, o, gn_smem, red, hist, sh, pick, ltab, lsum);
    return;
  }

  // ---- role 0 ----
  const int K = p.n_bins;
  const int Kp = (K + 7) & ~7;
  float* mag = reinterpret_cast<float*>(gn_smem);  // [Kp], zero past K
  float* cs = mag + Kp;                             // [Kp] np.cumsum(mag)
  const double* __restrict__ fr = p.freqs;
  const float* sp = p.spec.row(f);
  const float* prev = f > 0 ? p.spec.row(f - 1) : p.prev_in;
  float* keep_out = f == p.n_frames - 1 ? p.prev_out : nullptr;  // stored whatever the frame holds
  int* pb = p.peak_bins + f * kGenrePeaks;

  double bad = 0.0;
  for (int i = t; i < Kp; i += kGT) {
    float v = 0.f;
    if (i < K) {
      v = fabsf(sp[i]);
      if (keep_out) keep_out[i] = v;
      if (!isfinite(v)) bad = 1.0;
    }
    mag[i] = v;
  }
  // the leaves of the twelve sums: 0 np.sum(mag), 1 the flux sum, 2 np.sum(mag ** 2), 3.. the bands
  if (t < kGnSums) {
    const int lo = t < 3 ? 0 : p.band_lo[t - 3], n = t < 3 ? K : p.band_n[t - 3];
    int nl = 0;
    if (n > 0) np_emit_leaves<7>(lo, n, ltab + t * kNpMaxLeaves, nl);
    nleaf[t] = nl;
  }
  bad = block_sum(bad, red);  // (the barriers publish mag, ltab and nleaf)
  if (bad > 0.0) {         // (uniform) the combine kernel zeroes the row
    if (t == 0) o[14] = -1.0;
    if (t < kGenrePeaks) pb[t] = -1;
    return;
  }

  // ---- the barrier-free stretch: the serial running sum on one lane, everything else on waves 1..3 ----
  double sfx = 0.0, slog = 0.0, sam = 0.0, cnt = 0.0, pbad = 0.0;
  if (t == 0) {
    float run = 0.f;
#pragma unroll 2
    for (int i = 0; i < Kp; i += 8) {
      const float4 a = *reinterpret_cast<const float4*>(mag + i), b = *reinterpret_cast<const float4*>(mag + i + 4);
      float4 ca, cb;
      run = __fadd_rn(run, a.x), ca.x = run;
      run = __fadd_rn(run, a.y), ca.y = run;
      run = __fadd_rn(run, a.z), ca.z = run;
      run = __fadd_rn(run, a.w), ca.w = run;
      run = __fadd_rn(run, b.x), cb.x = run;
      run = __fadd_rn(run, b.y), cb.y = run;
      run = __fadd_rn(run, b.z), cb.z = run;
      run = __fadd_rn(run, b.w), cb.w = run;
      *reinterpret_cast<float4*>(cs + i) = ca;
      *reinterpret_cast<float4*>(cs + i + 4) = cb;
    }
  } else if (t >= 64) {
    const int u = t - 64;
    for (int l = u; l < kGnSums * kNpMaxLeaves; l += kGnWork) {
      const int s = l / kNpMaxLeaves;
      if (l - s * kNpMaxLeaves >= nleaf[s]) continue;
      const int off = (int)(ltab[l] & 0xFFFFu), n = (int)(ltab[l] >> 16);
      const float* a = mag + off;
      float r;
      if (s == 0) {
        r = np_slice_leaf(n, [&](int i) { return a[i]; });
      } else if (s == 1) {
        r = 0.f;
        if (prev) {
          const float* q = prev + off;
          r = np_slice_leaf(n, [&](int i) {
            const float pv = fabsf(q[i]);
            // (a stored non-finite magnitude: its bins are left out and the frame is flagged)
            return isfinite(pv) ? fmaxf(0.f, a[i] - pv) : 0.f;
          });
        }
      } else {
        r = np_slice_leaf(n, [&](int i) { return a[i] * a[i]; });
      }
      lsum[l] = r;
    }
    const int h0 = p.band_lo[9], h1 = h0 + p.band_n[9];
    for (int i = u; i < K; i += kGnWork) {
      const float v = mag[i];
      sfx += fr[i] * (double)v;
      if (i >= h0 && i < h1 && v > 1e-10f) {
        cnt += 1.0;
        slog += log((double)v);
        sam += (double)v;
      }
      if (prev && !isfinite(prev[i])) pbad = 1.0;
    }
  }
  sfx = block_sum(sfx, red);  // (the barriers publish cs and lsum)
  slog = block_sum(slog, red);
  sam = block_sum(sam, red);
  cnt = block_sum(cnt, red);
  pbad = block_sum(pbad, red);
  if (t < kGnSums) {
    const int n = t < 3 ? K : p.band_n[t - 3];
    int idx = 0;
    sres[t] = n > 0 ? np_leaf_combine<7>(n, lsum + t * kNpMaxLeaves, idx) : 0.f;
  }
  __syncthreads();
  const float sabs = sres[0];
  const double centroid = sabs == 0.f ? 0.0 : sfx / (double)sabs;
  double var = 0.0;
  for (int i = t; i < K; i += kGT) {
    const double d = fr[i] - centroid;
    var += (d * d) * (double)mag[i];
  }
  var = block_sum(var, red);
  // rolloff: the first index with cumsum >= float32(0.85) * cumsum[-1]
  const float ctot = cs[K - 1], cthr = __fmul_rn(0.85f, ctot);
  unsigned long long first = 0;
  for (int i = t; i < K; i += kGT)
    if (cs[i] >= cthr) {
      first = ~(unsigned long long)i;  // (the max of ~i is the smallest i; this lane's first hit is its smallest)
      break;
    }
  first = gn_max_u64(first, redu);
  int ridx = first ? (int)~first : K;
  // distortion: the five largest strict local maxima above float32(np.mean(mag) * 2)
  const float thr2 = __fmul_rn((float)((double)sabs / (double)K), 2.0f);
  unsigned long long last = ~0ull;
#pragma unroll 1
  for (int r = 0; r < kGenrePeaks; ++r) {
    unsigned long long best = 0;
    for (int i = t; i < K; i += kGT) {
      if (i < 1 || i > K - 2) continue;
      const float v = mag[i];
      if (v > mag[i - 1] && v > mag[i + 1] && v > thr2) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)i);
        if (key < last && key > best) best = key;
      }
    }
    best = gn_max_u64(best, redu);
    if (t == 0) pk[r] = best ? (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)) : -1;
    last = best ? best : 0ull;  // (none left: nothing passes key < 0)
  }
  __syncthreads();
  bool qual = false;
  if (t < kGenrePeaks) {
    const int b = pk[t];
    pb[t] = b;
    if (b >= 5) {
      const float lim = __fmul_rn(mag[b], 0.1f);
      int hc = 0;
      for (int n = 2; n <= 5; ++n) {
        const int h = b * n;
        if (h < K) {
          float mx = 0.f;
          for (int j = max(0, h - 3); j < min(K, h + 4); ++j) mx = fmaxf(mx, mag[j]);
          hc += mx > lim;
        }
      }
      qual = hc >= 2;
    }
  }
  const int nqual = t < 64 ? __popcll(__ballot(qual)) : 0;
  if (t == 0) {
    const float tot = sres[2];
    // bass_emphasis (:709-739)
    float bass = 0.f;
    if (p.band_n[0] > 0 && p.band_n[1] > 0 && tot != 0.f) {
      const float be = sres[3], me = sres[4];
      const float ratio = __fdiv_rn(be, tot), b2m = __fdiv_rn(be, __fadd_rn(me, 1e-10f));
      const float e = __fmul_rn(ratio, fminf(__fdiv_rn(b2m, 2.0f), 1.0f));
      bass = fminf(e, 1.0f);
    }
    // vocal_presence (:753-783)
    float vocal = 0.f;
    if (p.band_n[2] > 0 && tot != 0.f) {
      const float ve = sres[5], ce = p.band_n[3] > 0 ? sres[6] : 0.f;
      const float vr = __fdiv_rn(ve, tot), cr = ve > 0.f ? __fdiv_rn(ce, ve) : 0.f;
      const float pr = __fmul_rn(vr, __fadd_rn(0.5f, __fmul_rn(0.5f, cr)));
      vocal = fminf(__fmul_rn(pr, 2.0f), 1.0f);
    }
    // high_freq_energy (:406-422)
    float high = 0.f;
    if (p.band_n[4] > 0 && p.band_n[5] > 0 && sres[8] > 0.f) high = __fdiv_rn(sres[7], sres[8]);
    // mid_frequency_dominance (:319-349)
    float middom = 0.f;
    if (p.band_n[7] > 0) {
      const float le = p.band_n[6] > 0 ? sres[9] : 0.f, me = sres[10], he = p.band_n[8] > 0 ? sres[11] : 0.f;
      const float te = __fadd_rn(__fadd_rn(le, me), he);
      if (te != 0.f) {
        const float mr = __fdiv_rn(me, te);
        middom = me > __fmul_rn(le, 1.2f) && me > __fmul_rn(he, 1.5f) ? fminf(__fmul_rn(mr, 1.5f), 1.0f) : mr;
      }
    }
    // spectral_flux (:256-276)
    float flux = 0.f;
    if (prev && sabs > 0.f) flux = fminf(__fdiv_rn(sres[1], sabs), 1.0f);
    // compute_spectral_complexity (:382-404)
    double cx = 0.3;
    if (p.band_n[9] > 0 && cnt > 0.0) {
      const double am = sam / cnt;
      if (am > 0.0) cx = fmin(fmax(1.0 - exp(slog / cnt) / am, 0.0), 1.0);
    }
    if (ctot == 0.f) ridx = 0;
    o[0] = centroid;
    o[1] = ctot == 0.f ? 0.0 : fr[min(ridx, K - 1)];
    o[2] = (double)ridx;
    o[4] = sabs == 0.f ? 0.0 : sqrt(var / (double)sabs);
    o[9] = cx;
    o[10] = (double)bass;
    o[11] = (double)vocal;
    o[12] = (double)high;
    o[13] = (double)flux;
    o[14] = (double)nqual;
    o[15] = (double)middom;
    o[16] = pbad > 0.0 ? 2.0 : 0.0;
  }
}

// a role that met a non-finite value left a mark (zero crossings or distortion count -1): the zero row,
// flag 2, no peaks
__global__ __launch_bounds__(kGT) void genre_combine_kernel(GenreParams p) {
  const int64_t f = (int64_t)blockIdx.x * kGT + threadIdx.x;
  if (f >= p.n_frames) return;
  double* o = p.out + f * kGenreCols;
  if (o[3] < 0.0 || o[14] < 0.0) {
    for (int k = 0; k < kGenreCols; ++k) o[k] = k == kGenreCols - 1 ? 2.0 : 0.0;
    for (int k = 0; k < kGenrePeaks; ++k) p.peak_bins[f * kGenrePeaks + k] = -1;
  }
}

size_t genre_lds_bytes(int n_bins, int m, int f64) {
  const size_t Kp = ((size_t)n_bins + 7) & ~(size_t)7;
  const size_t a = Kp * 8, b = (size_t)m * (f64 ? 8 : 4);
  return ((a > b ? a : b) + 15) & ~(size_t)15;
}

hipError_t launch_genre(const GenreParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const size_t lds = genre_lds_bytes(p.n_bins, p.m, p.audio.f64);
  if (lds + 16 * 1024 > 64 * 1024) {  // (the kernel's static arrays take under 16 KiB)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&genre_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(genre_kernel, dim3((unsigned)(2 * p.n_frames)), dim3(kGT), lds, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(genre_combine_kernel, dim3((unsigned)((p.n_frames + kGT - 1) / kGT)), dim3(kGT), 0, s, p);
  return hipGetLastError();
}

}  // namespace omega
