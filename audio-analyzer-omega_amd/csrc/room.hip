// RoomModeAnalyzer (omega4/analyzers/room_modes.py) on the device, everything in float64 (float32 input is
// widened on load). Contraction is off in this file: frequency, magnitude, prominence, q_factor and bandwidth
// are the reference's plain IEEE + - * / in its operation order, bit for bit.
//
// room_modes_kernel -- detect_room_modes :71-141 for a batch of spectra, one 256-thread workgroup per frame
// over the K <= 4096 in-range bins [first, last) of the caller's frequency table:
//   :86-92    np.mean, then np.std as sqrt(mean((x - mean)^2)) in a second pass (lane-strided block sums,
//             not numpy's pairwise order: 1e-15 relative); mean or std 0: no modes (flag bit 1)
//   :96-100   scipy's find_peaks(x, height=, prominence=): _local_maxima_1d (strict rise on the left, strict
//             fall on the right, a plateau gives (left + right) // 2, never the first or last bin) evaluated at
//             every rising edge at once; x[p] >= height; _peak_prominences with wlen=None. The surviving
//             peaks are compacted with an LDS counter so that each lane walks one peak.
//   :143-189  estimate_q_factor, :119-122 the severity, :191-239 classify_room_mode (the host passes the six
//             expected frequencies of the dimension hints), per peak on its lane
//   :136      sorted(..., reverse=True) is stable: a mode's rank is the number of modes with greater severity
//             plus those of equal severity at a lower bin, so the compaction order does not matter
// LDS: K doubles for the bins, and per possible peak (at most K / 2) its bin, severity, Q and prominence:
// 22 bytes per in-range bin, 88 KiB at the cap, 2 KiB at the app's sizes.
//
// room_rt60_kernel -- _calculate_rt60_schroeder :356-420 and _calculate_rt60_edt :422-458 for a batch of
// sample histories, one 1024-thread workgroup per stream of 2 <= L <= 2^20 samples. Thread t owns the
// contiguous chunk [t c, (t + 1) c), c = ceil(L / 1024). The backward inclusive sum of x^2 is blocked: chunk
// sums, a workgroup suffix scan of them, then sweeps that rebuild curve[i] = (sum behind the chunk) + (running
// sum inside it) sample by sample; the curve is never stored. The curve does not increase, so the first index
// with db <= T is the number of samples with db > T: a reduction. The line through [idx5, idx35) is fitted in
// centred form (the means, the centred sums, then the residuals): five sweeps in all, each re-reading the
// stream from cache.
#include <hip/hip_runtime.h>

#include <algorithm>

#pragma clang fp contract(off)  // (above the project headers: peaks.hpp and wg64.hpp take this state)

#include "params.hpp"
#include "peaks.hpp"
#include "wg64.hpp"

namespace omega {

namespace {

constexpr int kRT = kRoomThreads, kTT = kRt60Threads;

// :191-239 as base + 8 harmonic (base: 0 axial_length, 1 axial_width, 2 axial_height, 3 tangential, 4 oblique)
__device__ __forceinline__ int rm_type(double f, const double (&h)[6]) {
  if (h[0] > 0.0) {
    for (int k = 1; k <= 3; ++k)
      for (int d = 0; d < 3; ++d)
        if (fabs(f - h[d] * (double)k) < 5.0) return d + 8 * k;
    for (int d = 3; d < 6; ++d)
      if (fabs(f - h[d]) < 10.0) return 3;
  }
  if (30.0 <= f && f <= 80.0) return 0;
  if (80.0 <= f && f <= 120.0) return 1;
  if (120.0 <= f && f <= 200.0) return 2;
  if (200.0 <= f && f <= 300.0) return 3;
  return 4;
}

}  // namespace

__global__ __launch_bounds__(kRT) void room_modes_kernel(RoomModesParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rm_smem[];
  __shared__ double red[4 * 2];
  __shared__ int npk;
  const int t = threadIdx.x, K = p.last - p.first, P = max(K / 2, 1);
  const int64_t f = blockIdx.x;
  double* x = reinterpret_cast<double*>(rm_smem);  // [K] the in-range bins
  double* msev = x + K;                            // [P] per peak: severity (-1: not a mode), Q, prominence
  double* mq = msev + P;
  double* mprom = mq + P;
  int* pk = reinterpret_cast<int*>(mprom + P);     // [P] per peak: its in-range bin
  const Row sp = p.spec.row(f);
  const double* fr = p.freqs + p.first;
  double* o = p.out + f * (kRoomRows * kRoomCols);
  if (t == 0) npk = 0;

  // :52 over the whole spectrum; the in-range bins and their sum
  double a[2] = {0.0, 0.0};
  for (int i = t; i < p.n_bins; i += kRT) {
    const double v = sp[i];
    if (!isfinite(v)) a[0] = 1.0;
    if (i >= p.first && i < p.last) {
      x[i - p.first] = v;
      a[1] += v;
    }
  }
  block_sums<2, 4>(a, red);  // (the barriers publish x and npk)
  const bool bad = a[0] > 0.0 || p.freqs_bad;
  const double mean = (bad || K == 0) ? 0.0 : a[1] / (double)K;
  double c[1] = {0.0};
  for (int i = t; i < K; i += kRT) {
    const double d = x[i] - mean;
    c[0] += d * d;
  }
  block_sums<1, 4>(c, red);
  const double sd = (bad || K == 0) ? 0.0 : sqrt(c[0] / (double)K);
  if (bad || mean == 0.0 || sd == 0.0) {  // (uniform) no modes: the header alone
    for (int i = t; i < kRoomRows * kRoomCols; i += kRT)
      o[i] = i == 1 ? (bad ? 1.0 : 2.0) : (i == 2 ? mean : (i == 3 ? sd : 0.0));
    return;
  }
  const double height = mean * p.height_mult, pmin = sd * p.prom_std;

  // _local_maxima_1d from every rising edge, then the height condition
  for (int i = t + 1; i < K - 1; i += kRT) {
    // (peaks.hpp's local_max_at written out: through its -1 return the compiler lays this loop out with 28
    // more instructions, 25.3 us against 25.0 us per call of 512 frames at K = 92)
    const double xi = x[i];
    if (!(x[i - 1] < xi)) continue;
    int ahead = i + 1;
    while (ahead < K - 1 && x[ahead] == xi) ++ahead;
    if (x[ahead] < xi && xi >= height) {
      const int s = atomicAdd(&npk, 1);
      if (s < P) pk[s] = (i + ahead - 1) / 2;  // (at most (K - 1) / 2 peaks: each needs a lower bin after it)
    }
  }
  __syncthreads();
  const int n = min(npk, P);

  // one peak per lane: prominence, Q, severity
  for (int j = t; j < n; j += kRT) {
    const int pi = pk[j];
    const double xp = x[pi];
    const double prom = prominence(x, K, pi);
    double sev = -1.0, q = 0.0;
    if (prom >= pmin) {
      const double half = xp / 1.4142135623730951;  // np.sqrt(2)
      const double cf = fr[pi];
      double lf = cf, rf = cf;
      for (int i = pi - 1; i >= 0; --i)
        if (x[i] <= half) {
          const double y1 = x[i], y2 = x[i + 1], f1 = fr[i], f2 = fr[i + 1];
          lf = f1 + (half - y1) * (f2 - f1) / (y2 - y1);
          break;
        }
      for (int i = pi + 1; i < K; ++i)
        if (x[i] <= half) {
          const double y1 = x[i - 1], y2 = x[i], f1 = fr[i - 1], f2 = fr[i];
          rf = f1 + (half - y1) * (f2 - f1) / (y2 - y1);
          break;
        }
      const double bw = rf - lf;
      q = bw > 0.0 ? cf / bw : 50.0;
      q = q > p.min_q ? q : p.min_q;  // Python's max(min_q, q), then min(max_q, .)
      q = q < p.max_q ? q : p.max_q;
      const double rel = xp / mean, q10 = q / 10.0, nq = 1.0 < q10 ? 1.0 : q10;
      const double s = rel * nq * 0.5;
      const double s1 = s < 1.0 ? s : 1.0;
      if (s1 > p.min_sev) sev = s1;
    }
    msev[j] = sev;
    mq[j] = q;
    mprom[j] = prom;
  }
  double m[1] = {0.0};
  for (int j = t; j < n; j += kRT) m[0] += msev[j] >= 0.0 ? 1.0 : 0.0;  // (own entries)
  block_sums<1, 4>(m, red);  // (the barriers publish the per-peak arrays)
  const int count = (int)m[0];

  for (int j = t; j < n; j += kRT) {
    const double s = msev[j];
    if (!(s >= 0.0)) continue;
    const int pi = pk[j];
    int rank = 0;
    for (int k = 0; k < n; ++k) {
      const double sk = msev[k];
      rank += (sk > s || (sk == s && pk[k] < pi)) ? 1 : 0;
    }
    if (rank >= kRoomMaxModes) continue;
    double* r = o + (1 + rank) * kRoomCols;
    const double cf = fr[pi], q = mq[j];
    r[0] = cf;
    r[1] = x[pi];
    r[2] = q;
    r[3] = s;
    r[4] = (double)rm_type(cf, p.hints);
    r[5] = mprom[j];
    r[6] = q > 0.0 ? cf / q : 0.0;
    r[7] = (double)(p.first + pi);
  }
  // the rows past the modes, and the header
  for (int i = (1 + min(count, kRoomMaxModes)) * kRoomCols + t; i < kRoomRows * kRoomCols; i += kRT) o[i] = 0.0;
  if (t < kRoomCols)
    o[t] = t == 0 ? (double)count : (t == 1 ? (count > kRoomMaxModes ? 4.0 : 0.0) : (t == 2 ? mean : (t == 3 ? sd : 0.0)));
}

namespace {

// the samples of [lo, hi) from the back, with curve[i] = behind + (running sum of squares inside the chunk);
// stops below `stop`
template <class F>
__device__ __forceinline__ void rt_sweep(Row a, int lo, int hi, int stop, double behind, F body) {
  double run = 0.0;
  for (int i = hi - 1; i >= lo && i >= stop; --i) {
    const double v = a[i];
    run += v * v;
    body(i, behind + run);
  }
}

}  // namespace

__global__ __launch_bounds__(kTT) void room_rt60_kernel(RoomRt60Params p) {
  constexpr int NW = kTT / 64;
  __shared__ double red[NW * 3];
  __shared__ double wtot[NW];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, L = p.L;
  const int64_t s = blockIdx.x;
  const Row a = p.audio.row(s);
  double* o = p.out + s * kRt60Cols;
  const int chunk = (L + kTT - 1) / kTT, lo = min(t * chunk, L), hi = min(lo + chunk, L);

  // :463 the frames' sums of squares (for the facade's `simple` method)
  if (p.energies && p.W > 0) {
    const int nf = L / p.W;
    for (int k = w; k < nf; k += NW) {
      double e = 0.0;
      for (int i = lane; i < p.W; i += 64) {
        const int64_t at = (int64_t)k * p.W + i;
        const double v = a[at];
        e += v * v;
      }
#pragma unroll
      for (int q = 32; q > 0; q >>= 1) e += __shfl_xor(e, q, 64);
      if (lane == 0) p.energies[s * nf + k] = e;
    }
  }

  // the chunk sums and their suffix scan
  double cs = 0.0, nf1[1] = {0.0};
  rt_sweep(a, lo, hi, 0, 0.0, [&](int, double cv) { cs = cv; });
  if (!isfinite(cs)) nf1[0] = 1.0;  // (a non-finite sample or square makes its chunk's sum non-finite)
  double inc = cs;  // sum over the lanes >= this one of the wave
#pragma unroll
  for (int q = 1; q < 64; q <<= 1) {
    const double u = __shfl_down(inc, q, 64);
    if (lane + q < 64) inc += u;
  }
  const double next = __shfl_down(inc, 1, 64);
  if (lane == 0) wtot[w] = inc;
  block_sums<1, NW>(nf1, red);  // (the barriers publish wtot)
  double behind = lane < 63 ? next : 0.0;
  for (int k = NW - 1; k > w; --k) behind += wtot[k];
  if (t == 0) wtot[0] = behind + cs;  // curve[0]: what thread 0's own sweeps end on
  __syncthreads();
  const double total = wtot[0];
  if (nf1[0] > 0.0) {  // (uniform)
    if (t < kRt60Cols) o[t] = t == 7 ? 1.0 : 0.0;
    return;
  }
  const double den = fmax(total, 1e-10);

  // :371-382, :436 the crossings as counts
  double cnt[3] = {0.0, 0.0, 0.0};
  rt_sweep(a, lo, hi, 0, behind, [&](int, double cv) {
    const double db = 10.0 * log10(fmax(cv, 1e-10) / den);
    cnt[0] += db > -5.0 ? 1.0 : 0.0;
    cnt[1] += db > -10.0 ? 1.0 : 0.0;
    cnt[2] += db > -35.0 ? 1.0 : 0.0;
  });
  block_sums<3, NW>(cnt, red);
  const int i5 = (int)cnt[0], i10 = (int)cnt[1], i35 = (int)cnt[2], n = i35 - i5;
  int flags = 0;
  if (i5 >= L || i35 >= L || i35 <= i5)
    flags = 2;
  else if (n < 3)
    flags = 4;
  if (flags) {  // (uniform)
    if (t == 0) {
      o[0] = total, o[1] = (double)i5, o[2] = (double)i10, o[3] = (double)i35;
      o[4] = 0.0, o[5] = 0.0, o[6] = 0.0, o[7] = (double)flags;
    }
    return;
  }

  // :388-406 the line of db on t = i / fs over [i5, i35), centred
  const int b1 = min(hi, i35);  // (the sweeps stop below i5 and skip i >= i35 in their bodies)
  double mu[2] = {0.0, 0.0};
  rt_sweep(a, lo, hi, i5, behind, [&](int i, double cv) {
    if (i >= b1) return;
    mu[0] += (double)i / p.fs;
    mu[1] += 10.0 * log10(fmax(cv, 1e-10) / den);
  });
  block_sums<2, NW>(mu, red);
  const double mt = mu[0] / (double)n, md = mu[1] / (double)n;
  double cen[3] = {0.0, 0.0, 0.0};
  rt_sweep(a, lo, hi, i5, behind, [&](int i, double cv) {
    if (i >= b1) return;
    const double dt = (double)i / p.fs - mt, dd = 10.0 * log10(fmax(cv, 1e-10) / den) - md;
    cen[0] += dt * dt;
    cen[1] += dt * dd;
    cen[2] += dd * dd;
  });
  block_sums<3, NW>(cen, red);
  const double slope = cen[1] / cen[0], icpt = md - slope * mt;
  double ssr[1] = {0.0};
  rt_sweep(a, lo, hi, i5, behind, [&](int i, double cv) {
    if (i >= b1) return;
    const double r = 10.0 * log10(fmax(cv, 1e-10) / den) - (slope * ((double)i / p.fs) + icpt);
    ssr[0] += r * r;
  });
  block_sums<1, NW>(ssr, red);
  if (t == 0) {
    o[0] = total, o[1] = (double)i5, o[2] = (double)i10, o[3] = (double)i35;
    o[4] = slope, o[5] = icpt, o[6] = 1.0 - ssr[0] / cen[2], o[7] = slope >= 0.0 ? 8.0 : 0.0;
  }
}

size_t room_modes_lds_bytes(int K) {
  const size_t P = (size_t)std::max(K / 2, 1);
  return (size_t)K * sizeof(double) + P * (3 * sizeof(double) + sizeof(int));
}

hipError_t launch_room_modes(const RoomModesParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const size_t lds = room_modes_lds_bytes(p.last - p.first);
  if (lds + 1024 > 64 * 1024) {  // (the kernel's static arrays take under 1 KiB)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&room_modes_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(room_modes_kernel, dim3((unsigned)p.n_frames), dim3(kRT), lds, s, p);
  return hipGetLastError();
}

hipError_t launch_room_rt60(const RoomRt60Params& p, hipStream_t s) {
  if (p.n_streams <= 0) return hipSuccess;
  hipLaunchKernelGGL(room_rt60_kernel, dim3((unsigned)p.n_streams), dim3(kTT), 0, s, p);
  return hipGetLastError();
}

}  // namespace omega
