// HipHopDetector.analyze (omega4/panels/hip_hop_detector.py:94-154) with the helpers it calls (:156-384)
// for a batch of independent frames: hiphop_kernel runs two 256-thread workgroups per frame, one per
// role, and hiphop_combine_kernel (same stream, one thread per frame) applies the silence gate, joins the
// two roles' sub-bass terms and turns a role's "non-finite input" mark into the flagged zero row. No
// workgroup waits for another: stream order is the only dependency. Every loop has a fixed bound.
//
//   role 0, the spectrum side (magnitude = |spectrum|, n_bins float32 in LDS)
//     every mask over the increasing table is a contiguous bin range found by the host;
//     np.sum(np.abs(fft_data[mask]) ** 2) is numpy's float32 pairwise sum of the float32 squares over the
//     slice (numpy_emul.hpp's slice form), the ratios follow in float32, operation for operation
//     (contraction is off in this file)
//     :293-330  spectral tilt from the low / mid / high sums, the x 1.2 boost above low_ratio > 0.5
//     :332-384  rap vocals: find_peaks(|spectrum[vocal]|, prominence = float32(max * 0.3), distance = 20):
//               scipy's local maxima (the middle of a plateau), its distance rule in the parallel form of
//               peaks.hpp, then one lane per surviving peak walks left and right to the next higher
//               sample or the array end for the two minima; prominence and threshold compare in float64
//   role 1, the audio side (float64 like the reference's scipy path; sosfilt of float32 audio is float64)
//     :100      rms = np.sqrt(np.mean(x ** 2)) in the audio's precision (float32: bit for bit)
//     :164-165  sub-bass band-pass (four DF2T sections from the zero state), its RMS
//     :268-276  hi-hat band-pass, count of nonzero np.diff(np.sign(.)), its RMS
//     :226-236  kick band-pass, |hilbert(.)| over the frame's own length, mean + 1.5 np.std, find_peaks(height,
//               distance = int(0.1 fs)): the highest undecided peak is kept and removes those nearer than the
//               distance, until none is left (scipy's greedy order; at most kHipHopPeaks survive)
//     :238-253  np.diff of the kept peaks, regularity, median, syncopation: the factor that multiplies the
//               caller's kick magnitude (0.5 with at most one peak)
//
// LDS: the audio role holds the frame as m float64 samples and, for the envelope, a second buffer of m / 2
// complex values: the Hilbert transform is the packed real FFT pair of transient.hip run in place
// (decimation in frequency to bit-reversed order, decimation in time back: wg64.hpp's pair), so filters
// and envelope are ONE kernel of 16 m bytes (plus 4 KiB of carries and 11.6 KiB static): 143 KiB at m = 8192
// (one workgroup per CU), 47 KiB at m = 2048 (three per CU). The peak flags reuse the transform buffer.
//
// Each cascade section is wg64.hpp's chunked scan (sos_section_scan). At m = 64 and 128 the chunk is one
// sample and only the first m threads own one; the others carry a zero state that no owning thread
// reads. A zero input prefix gives exact zeros either way (0 * c + 0).
//
// Reductions: the float64 sums (filtered RMS, envelope mean and np.std) are lane-strided block sums, not
// numpy's pairwise order; they agree with it to a few 1e-16 relative, far inside the 1e-9 the filters set.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)  // (above the project headers: numpy_emul.hpp, peaks.hpp and wg64.hpp take this state)

#include "numpy_emul.hpp"
#include "params.hpp"
#include "peaks.hpp"
#include "wg64.hpp"

namespace omega {

namespace {

constexpr int kHT = kHipHopThreads;
constexpr int kHhVocalDistance = 20;  // find_peaks(distance=20): a kept peak removes those < 20 bins away

// ---- role 1: the audio side ----
__device__ __forceinline__ void hh_audio(const HipHopParams& p, int64_t f, double* o, unsigned char* smem) {
  __shared__ double red[4];
  __shared__ unsigned ltab[72];
  __shared__ float lsum[72];
  __shared__ int nl_s;
  __shared__ int kept[kHipHopPeaks];
  __shared__ int pos[kHipHopPeaks];
  __shared__ double sp[kHipHopPeaks];
  __shared__ double cf[3][4][5];  // the sections' b0 b1 b2 a1 a2 (constant indices into the kernel argument)
  const int t = threadIdx.x, m = p.m, K = m / 2;
  double* S = reinterpret_cast<double*>(smem);                          // [m] the filtered signal, the envelope
  double2* Z = reinterpret_cast<double2*>(smem + (size_t)m * 8);        // [m / 2] the transform; then the flags
  double2* sc = reinterpret_cast<double2*>(smem + (size_t)m * 16);      // [kHT]
  const Row x = p.audio.row(f);
  auto load = [&]() {
    for (int i = t; i < m; i += kHT) S[i] = x[i];
    __syncthreads();
  };
  auto filter = [&](int which) {
    for (int s = 0; s < 4; ++s) {
      const double* c = cf[which][s];
      sos_section_scan<kHT>(S, m, c[0], c[1], c[2], c[3], c[4], sc);
    }
  };
  if (t == 0) {
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const W64Stage& q = p.sos[w][s];
        cf[w][s][0] = q.b0, cf[w][s][1] = q.b1, cf[w][s][2] = q.b2, cf[w][s][3] = q.a1, cf[w][s][4] = q.a2;
      }
  }
  int* kp = p.kick_peaks ? p.kick_peaks + f * kHipHopPeaks : nullptr;
  if (kp && t < kHipHopPeaks) kp[t] = -1;

  load();
  double bad = 0.0, sq = 0.0;
  for (int i = t; i < m; i += kHT) {
    const double v = S[i];
    if (!isfinite(v)) bad = 1.0;
    sq += v * v;
  }
  bad = block_sum(bad, red);
  if (bad > 0.0) {  // (uniform) the combine kernel zeroes the row
    if (t == 0) o[4] = -1.0;
    return;
  }
  sq = block_sum(sq, red);
  double rms;
  if (!p.audio.f64) {
    rms = (double)np_rms_f32(p.audio.row_as<float>(f), m, ltab, lsum, &nl_s);
  } else {
    rms = sqrt(sq / (double)m);
  }
  if (t == 0) o[0] = rms;
  if (rms < 0.001) {  // (uniform) :101, the silence gate: nothing else is computed
    if (t == 0) o[4] = -2.0;
    return;
  }

  // sub-bass (:164-165)
  filter(0);
  double s2 = 0.0;
  for (int i = t; i < m; i += kHT) s2 += S[i] * S[i];
  const double sub_rms = sqrt(block_sum(s2, red) / (double)m);
  // hi-hat (:268-276)
  load();
  filter(2);
  double zc = 0.0;
  s2 = 0.0;
  for (int i = t; i < m; i += kHT) {
    const double v = S[i];
    s2 += v * v;
    if (i + 1 < m) {
      const double w = S[i + 1];
      const int sa = (v > 0.0) - (v < 0.0), sb = (w > 0.0) - (w < 0.0);
      zc += sa != sb;
    }
  }
  const double hat_rms = sqrt(block_sum(s2, red) / (double)m);
  zc = block_sum(zc, red);
  // kick (:226-229): H(x) = irfft(-i X), X = rfft(x) with DC and Nyquist zeroed, as two K-point complex
  // transforms of z[n] = x[2n] + i x[2n+1]
  load();
  filter(1);
  for (int k = t; k < K; k += kHT) Z[k] = make_double2(S[2 * k], S[2 * k + 1]);
  __syncthreads();
  int bits = 0;
  while ((1 << bits) < K) ++bits;
  fft_dif<kHT>(Z, K, p.tw, 2);
  // X_q = (Z_q + conj Z_{K-q}) / 2 + e^{-2 pi i q / m} (Z_q - conj Z_{K-q}) / 2i, Y_q = -i X_q; the packed
  // inverse spectrum Z'_k = (Y_k + conj Y_{K-k}) + i e^{2 pi i k / m} (Y_k - conj Y_{K-k}), stored conjugated
  // so that the forward transform returns conj(K ifft). Bins k and K - k read and write the same two
  // slots, so one thread does the pair.
  for (int k = t; k <= K / 2; k += kHT) {
    const int mk = (K - k) & (K - 1);
    const int pk = brev(k, bits), pm = brev(mk, bits);
    const double2 zk = Z[pk], zm = Z[pm];
    auto Y = [&](double2 za, double2 zb, int q) {  // -i X_q, za = Z_q, zb = Z_{K-q}
      const double2 e = make_double2(0.5 * (za.x + zb.x), 0.5 * (za.y - zb.y));
      const double2 od = make_double2(0.5 * (za.y + zb.y), -0.5 * (za.x - zb.x));
      const double2 ow = zmul(od, p.tw[q]);
      return make_double2(e.y + ow.y, -(e.x + ow.x));
    };
    const double2 zero = make_double2(0.0, 0.0);
    const double2 yk = k == 0 ? zero : Y(zk, zm, k);
    const double2 ym = k == 0 ? zero : Y(zm, zk, K - k);  // (k = 0: Y_0 = Y_K = 0)
    auto pack = [&](double2 ya, double2 yb, int q) {     // conj Z'_q, ya = Y_q, yb = Y_{K-q}
      const double2 s = make_double2(ya.x + yb.x, ya.y - yb.y);
      const double2 d = make_double2(ya.x - yb.x, ya.y + yb.y);
      const double2 w = p.tw[q];
      const double2 id = zmul(make_double2(-d.y, d.x), make_double2(w.x, -w.y));
      return make_double2(s.x + id.x, -(s.y + id.y));
    };
    Z[pk] = pack(yk, ym, k);
    if (mk != k) Z[pm] = pack(ym, yk, K - k);
  }
  __syncthreads();
  fft_dit<kHT>(Z, K, p.tw, 2);
  // envelope: H(x)[2n] = Re(ifft) / 2, H(x)[2n + 1] = Im(ifft) / 2, ifft = conj(FFT(conj)) / K
  const double scl = 0.5 / K;
  double s1 = 0.0;
  for (int k = t; k < K; k += kHT) {
    const double h0 = Z[k].x * scl, h1 = -Z[k].y * scl;
    const double x0 = S[2 * k], x1 = S[2 * k + 1];
    const double e0 = sqrt(x0 * x0 + h0 * h0), e1 = sqrt(x1 * x1 + h1 * h1);
    S[2 * k] = e0;
    S[2 * k + 1] = e1;
    s1 += e0 + e1;
  }
  const double mean = block_sum(s1, red) / (double)m;  // (the barriers publish the envelope; Z is free)
  s2 = 0.0;
  for (int i = t; i < m; i += kHT) {
    const double d = S[i] - mean;
    s2 += d * d;
  }
  const double thr = mean + 1.5 * sqrt(block_sum(s2, red) / (double)m);
  // find_peaks(envelope, height = thr, distance): candidates, then scipy's greedy distance rule
  int* cand = reinterpret_cast<int*>(Z);  // [m]
  for (int i = t; i < m; i += kHT) cand[i] = 0;
  __syncthreads();
  for (int i = 1 + t; i < m - 1; i += kHT) {
    const int pkx = local_max_at(S, m, i);
    if (pkx >= 0 && S[pkx] >= thr) cand[pkx] = 1;
  }
  __syncthreads();
  int nk = 0;
#pragma unroll 1
  for (int r = 0; r < kHipHopPeaks; ++r) {
    double best = -1.0;
    for (int i = t; i < m; i += kHT)
      if (cand[i]) best = fmax(best, S[i]);
    best = block_max(best, red);
    if (best < 0.0) break;  // (uniform) none left
    int at = -1;
    for (int i = t; i < m; i += kHT)
      if (cand[i] && S[i] == best) at = max(at, i);
    at = (int)block_max((double)at, red);
    if (t == 0) kept[nk] = at;
    ++nk;
    for (int i = t; i < m; i += kHT)
      if (cand[i] && abs(i - at) < p.distance) cand[i] = 0;
    __syncthreads();
  }
  if (t == 0) {
    // the kept peaks in index order, the spacing statistics (:238-253)
    for (int i = 0; i < nk; ++i) {
      int j = i;
      const int v = kept[i];
      for (; j > 0 && pos[j - 1] > v; --j) pos[j] = pos[j - 1];
      pos[j] = v;
    }
    double factor = 0.5;
    if (nk > 1) {
      const int ns = nk - 1;
      double sum = 0.0;
      for (int i = 0; i < ns; ++i) {
        const double v = (double)(pos[i + 1] - pos[i]);
        int j = i;
        for (; j > 0 && sp[j - 1] > v; --j) sp[j] = sp[j - 1];
        sp[j] = v;  // (sorted: the statistics below do not depend on the order)
        sum += v;
      }
      const double mu = sum / ns;
      double var = 0.0;
      for (int i = 0; i < ns; ++i) var += (sp[i] - mu) * (sp[i] - mu);
      double reg = 1.0 - sqrt(var / ns) / (mu + 1e-10);
      reg = fmax(0.0, fmin(reg, 1.0));
      const double med = ns & 1 ? sp[ns / 2] : (sp[ns / 2 - 1] + sp[ns / 2]) / 2.0;
      int off = 0;
      for (int i = 0; i < ns; ++i) off += fabs(sp[i] - med) > med * 0.2;
      const double sync = (double)off / ns;
      factor = 0.6 * reg + 0.4 * (1.0 - sync);
    }
    if (kp)
      for (int i = 0; i < nk; ++i) kp[i] = pos[i];
    o[2] = (double)nk;
    o[3] = factor;
    o[4] = zc;
    o[10] = sub_rms;
    o[11] = hat_rms;
    o[12] = thr;
  }
}

// ---- role 0: the spectrum side ----
__device__ __forceinline__ void hh_spectrum(const HipHopParams& p, int64_t f, double* o, unsigned char* smem) {
  __shared__ double red[4];
  __shared__ unsigned ltab[kHipHopBands * kNpMaxLeaves];
  __shared__ float lsum[kHipHopBands * kNpMaxLeaves];
  __shared__ int nleaf[kHipHopBands];
  __shared__ float sres[kHipHopBands];
  __shared__ int blo[kHipHopBands], bn[kHipHopBands];  // (constant indices into the kernel argument)
  const int t = threadIdx.x, K = p.n_bins;
  if (t == 0) {
#pragma unroll
    for (int b = 0; b < kHipHopBands; ++b) blo[b] = p.band_lo[b], bn[b] = p.band_n[b];
  }
  __syncthreads();
  const int Kp = (K + 7) & ~7;
  float* mag = reinterpret_cast<float*>(smem);             // [Kp], zero past K
  unsigned char* und = smem + (size_t)Kp * 4;              // [Kp] 1: a peak the distance rule has not decided
  unsigned char* keep = und + Kp;                          // [Kp] 1: a peak the distance rule keeps
  const float* sp = p.spec.row(f);
  double bad = 0.0;
  for (int i = t; i < Kp; i += kHT) {
    float v = 0.f;
    if (i < K) {
      v = fabsf(sp[i]);
      if (!isfinite(v)) bad = 1.0;
    }
    mag[i] = v;
    und[i] = 0;
    keep[i] = 0;
  }
  if (t < kHipHopBands) {
    int nl = 0;
    if (bn[t] > 0) np_emit_leaves<7>(blo[t], bn[t], ltab + t * kNpMaxLeaves, nl);
    nleaf[t] = nl;
  }
  bad = block_sum(bad, red);  // (the barriers publish mag, ltab and nleaf)
  if (bad > 0.0) {         // (uniform) the combine kernel zeroes the row
    if (t == 0) o[7] = -1.0;
    return;
  }
  for (int l = t; l < kHipHopBands * kNpMaxLeaves; l += kHT) {
    const int s = l / kNpMaxLeaves;
    if (l - s * kNpMaxLeaves >= nleaf[s]) continue;
    const float* a = mag + (ltab[l] & 0xFFFFu);
    lsum[l] = np_slice_leaf((int)(ltab[l] >> 16), [&](int i) { return a[i] * a[i]; });
  }
  __syncthreads();
  if (t < kHipHopBands) {
    int idx = 0;
    sres[t] = bn[t] > 0 ? np_leaf_combine<7>(bn[t], lsum + t * kNpMaxLeaves, idx) : 0.f;
  }
  __syncthreads();

  // :359-367 find_peaks over the vocal range (more than 10 bins)
  const int n = p.band_n[6];
  const float* v = mag + p.band_lo[6];
  double npk = 0.0;
  if (n > 10) {  // (uniform)
    double vm = 0.0;
    for (int i = t; i < n; i += kHT) vm = fmax(vm, (double)v[i]);
    const float vmax = (float)block_max(vm, red);
    const double pmin = (double)__fmul_rn(vmax, 0.3f);  // np.max(.) * 0.3 is a float32, widened for the comparison
    int any = 0;
    for (int i = 1 + t; i < n - 1; i += kHT) {
      const int pkx = local_max_at(v, n, i);
      if (pkx >= 0) und[pkx] = 1, any = 1;
    }
    select_by_distance<kHT>(v, und, keep, 0, n, kHhVocalDistance, any);
    // one lane per surviving peak: its prominence against the threshold, in float64
    for (int i = t; i < n; i += kHT)
      if (keep[i] && pmin <= prominence(v, n, i)) npk += 1.0;
    npk = block_sum(npk, red);
  }
  if (t == 0) {
    // :293-330
    float tilt = 0.f;
    int tbr = 0;
    if (p.band_n[3] > 0 && p.band_n[4] > 0 && p.band_n[5] > 0) {
      const float le = sres[3], me = sres[4], he = sres[5];
      const float te = __fadd_rn(__fadd_rn(le, me), he);
      if (!(te == 0.f)) {
        const float lr = __fdiv_rn(le, te), hr = __fdiv_rn(he, te);
        tilt = __fdiv_rn(__fadd_rn(__fsub_rn(lr, hr), 1.0f), 2.0f);
        tbr = 1;
        if (lr > 0.5f) {
          const float b = __fmul_rn(tilt, 1.2f);
          if (1.0f < b) tilt = 1.0f, tbr = 3;  // min(tilt * 1.2, 1.0) gives the Python float
          else tilt = b, tbr = 2;
        }
      }
    }
    // :332-384
    float vocal = 0.f;
    int vbr = 0;
    const float ve = sres[6], ce = sres[7], tot = sres[8];
    if (n > 0 && !(tot == 0.f || ve == 0.f) && n > 10) {
      const double density = npk / (double)n;
      const float vr = __fdiv_rn(ve, tot), cc = __fdiv_rn(ce, ve);
      const float pr = __fadd_rn(__fadd_rn(__fmul_rn(0.4f, vr), __fmul_rn(0.3f, cc)), (float)(0.3 * density));
      const float b = __fmul_rn(pr, 2.5f);
      if (1.0f < b) vocal = 1.0f, vbr = 2;
      else vocal = b, vbr = 1;
    }
    o[6] = (double)tilt;
    o[7] = npk;
    o[8] = (double)vocal;
    for (int b = 0; b < kHipHopBands; ++b) o[13 + b] = (double)sres[b];
    o[22] = (double)tbr;
    o[23] = (double)vbr;
  }
}

}  // namespace

__global__ __launch_bounds__(kHT) void hiphop_kernel(HipHopParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hh_smem[];
  const int64_t f = blockIdx.x >> 1;
  double* o = p.out + f * kHipHopCols;
  if (blockIdx.x & 1) hh_audio(p, f, o, hh_smem);
  else hh_spectrum(p, f, o, hh_smem);
}

// the silence gate (:100-110), _detect_sub_bass' combination (:168-213) and the hi-hat density (:278-285)
// in the reference's operation order; a role that met a non-finite value left a mark (crossings or vocal
// peak count -1): the zero row, flag 2, no peaks
__global__ __launch_bounds__(kHT) void hiphop_combine_kernel(HipHopParams p) {
  const int64_t f = (int64_t)blockIdx.x * kHT + threadIdx.x;
  if (f >= p.n_frames) return;
  double* o = p.out + f * kHipHopCols;
  const bool bad = o[4] == -1.0 || o[7] == -1.0, silent = o[4] == -2.0;
  if (bad || silent) {
    const double rms = bad ? 0.0 : o[0];
    for (int k = 0; k < kHipHopCols; ++k) o[k] = 0.0;
    o[0] = rms;
    o[9] = (bad ? 2.0 : 0.0) + (silent ? 1.0 : 0.0);
    if (p.kick_peaks)
      for (int k = 0; k < kHipHopPeaks; ++k) p.kick_peaks[f * kHipHopPeaks + k] = -1;
    return;
  }
  const double rms = o[0];
  const double tdr = o[10] / rms;
  double fterm = 0.0, sterm = 0.0;
  const float sub = (float)o[13], bass = (float)o[14], tp = (float)o[15];
  if (p.band_n[0] > 0 && tp > 0.f) {
    const float fdr = __fdiv_rn(sub, tp), sbr = __fdiv_rn(sub, __fadd_rn(bass, 1e-10f));
    fterm = (double)__fmul_rn(0.5f, fdr);
    sterm = 1.0f < sbr ? 0.2 * 1.0 : (double)__fmul_rn(0.2f, sbr);  // 0.2 * min(ratio, 1.0): float32 unless clipped
  }
  const double presence = 0.3 * tdr + fterm + sterm;
  o[1] = fmin(presence * 3.0, 1.0);
  const double zcr = o[4] / (double)p.m, er = o[11] / rms;
  o[5] = fmin(zcr * 10.0, 1.0) * fmin(er * 5.0, 1.0);
  o[9] = 0.0;
}

size_t hiphop_lds_bytes(int n_bins, int m) {
  const size_t Kp = ((size_t)n_bins + 7) & ~(size_t)7;
  const size_t a = Kp * 6, b = (size_t)m * 16 + kHT * sizeof(double2);
  return ((a > b ? a : b) + 15) & ~(size_t)15;
}

hipError_t launch_hiphop(const HipHopParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const size_t lds = hiphop_lds_bytes(p.n_bins, p.m);
  if (lds + 16 * 1024 > 64 * 1024) {  // (the kernel's static arrays take under 16 KiB)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&hiphop_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(hiphop_kernel, dim3((unsigned)(2 * p.n_frames)), dim3(kHT), lds, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hiphop_combine_kernel, dim3((unsigned)((p.n_frames + kHT - 1) / kHT)), dim3(kHT), 0, s, p);
  return hipGetLastError();
}

}  // namespace omega
