// TransientDetectionPanel (omega4/panels/transient_detection.py) on the device, in float64 like the reference's
// numpy / scipy path (float32 frames are widened exactly on load). tdetect_kernel holds every frame-local
// quantity, 256 threads per workgroup, the role by blockIdx as in voice_kernel; no role waits on another, and
// each scans the frame's samples and bins for non-finite values so that all know the frame's flag:
//
//   envelope  :120-131  mean(savgol_filter(|hilbert(x)|, 11, 3)): the m-point transform of hilbert64.hpp, every
//                       smoothed value as the dot product of the host-designed weights of its window position
//   flux      :152-166  abs(rfft(x[:512] * hanning(512)))[:128] (zero-padded at m = 256) and its sum, to the
//                       frame's workspace row
//   novelty   :319-332  x[n] - 0.97 x[n-1] (the first sample kept), its last 1024 samples times hanning(1024),
//                       rfft: 513 phases and magnitudes to the workspace row. DC and Nyquist have the imaginary
//                       part +0.0 that pocketfft gives them: their phase is 0 or +pi
//   hf        :191-200  filtfilt(butter(4, 5000 / (fs / 2), 'high'), x) in ba form: odd extension of 15, one
//                       order-4 DF2T recurrence per pass (forward from zi ext[0], backward from zi y[-1]) as a
//                       chunked scan -- weight64.hip's scheme with 4-state carries: every thread runs its chunk
//                       from the zero state, the carries are combined with the host's powers of P = A^L (in a
//                       wave by shuffles, across the four waves through LDS), and every thread re-runs its chunk
//                       from its true incoming state. The outputs come from the plain recurrence in scipy's
//                       coefficient order; only the incoming states' rounding differs from scipy
//   scalar    :93-94, :136, :237, :285-313 sum x^2, max |x|, sum |diff(sign x)|, the first argmax |x| and the
//                       nearest samples below a tenth of the peak on either side (integer LDS atomics);
//             :231-255  sum s, sum f s, the float64 prefix sum's first bin at 0.85 of the total (thread chunks,
//                       their sums scanned in a fixed order) and the four band sums
//
// tdetect_cross_kernel, behind it on the same stream: frame f's spectral flux (:173) from the workspace rows of f
// and its predecessor, its novelty (:343-348) from f's row and its two predecessors' phases; a stream's first
// rows take them from the carried state, and workgroup n_frames writes the outgoing state. Frames with a
// non-finite input are passed over as predecessors. Every sum has a fixed order that does not depend on the
// number of frames in the call: F frames in one call equal F chained calls bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hilbert64.hpp"
#include "params.hpp"

namespace omega {

namespace {

constexpr int kT = kTdThreads;
static_assert(kTdThreads == kTrThreads, "hilbert64.hpp's loops stride by kTrThreads");
constexpr double kTdPi = 3.14159265358979323846;

// > 0 where frame f holds a non-finite sample or bin (every thread gets the answer)
__device__ __forceinline__ bool td_bad(const TdetectParams& p, int64_t f, double* red) {
  double bad = 0.0;
  for (int i = threadIdx.x; i < p.m; i += kT)
    if (!isfinite(p.audio.at(f, i))) bad = 1.0;
  const float* g = p.spec.row(f);
  for (int i = threadIdx.x; i < p.n_bins; i += kT)
    if (!isfinite(g[i])) bad = 1.0;
  return block_sum(bad, red) > 0.0;
}

__device__ __forceinline__ void td_envelope(const TdetectParams& p, int64_t f, double2* smem, double* red) {
  const int m = p.m;
  double* o = p.out + f * kTdCols;
  if (td_bad(p, f, red)) {  // (uniform)
    if (threadIdx.x == 0) o[1] = 0.0;
    return;
  }
  auto xin = [&](int i) { return p.audio.at(f, i); };
  double2* spare = nullptr;
  const double* env = tr_hilbert_env(xin, m, smem, smem + m / 2, p.tw_m, p.tw2_m, &spare);
  double s = 0.0;
  for (int n = threadIdx.x; n < m; n += kT) {
    const int w0 = n < 5 ? 0 : (n >= m - 5 ? m - 11 : n - 5);
    const double* wt = p.sg + 11 * (n - w0);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 11; ++j) acc = fma(wt[j], env[w0 + j], acc);
    s += acc;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) o[1] = s / m;
}

__device__ __forceinline__ void td_flux(const TdetectParams& p, int64_t f, double2* smem, double* red) {
  constexpr int K = kTdFluxLen / 2;
  const int t = threadIdx.x;
  double* o = p.out + f * kTdCols;
  double* w = p.ws + f * kTdWsStride;
  const bool bad = td_bad(p, f, red);
  if (t == 0) w[0] = bad ? 1.0 : 0.0;
  if (bad) {  // (uniform; the cross kernel never reads a flagged row's spectra)
    if (t == 0) o[4] = 0.0;
    return;
  }
  double2* A = smem;
  double2* B = smem + K;
  for (int k = t; k < K; k += kT) {
    const int i0 = 2 * k, i1 = 2 * k + 1;
    A[k] = make_double2(i0 < p.m ? p.audio.at(f, i0) * p.han_f[i0] : 0.0, i1 < p.m ? p.audio.at(f, i1) * p.han_f[i1] : 0.0);
  }
  __syncthreads();
  const double2* Z = tr_fft(A, B, K, p.tw_f);
  double s = 0.0;
  for (int q = t; q < kTdFluxBins; q += kT) {
    double mag;
    if (q == 0) {
      mag = fabs(Z[0].x + Z[0].y);
    } else {
      const double2 X = tr_rfft_bin(Z, K, q, p.tw2_f);
      mag = hypot(X.x, X.y);
    }
    w[2 + q] = mag;
    s += mag;
  }
  s = block_sum(s, red);
  if (t == 0) {
    w[1] = s;
    o[4] = s;
  }
}

__device__ __forceinline__ void td_novelty(const TdetectParams& p, int64_t f, double2* smem, double* red) {
  constexpr int K = kTdNovLen / 2;
  const int t = threadIdx.x;
  double* o = p.out + f * kTdCols;
  double* w = p.ws + f * kTdWsStride + 2 + kTdFluxBins;
  if (td_bad(p, f, red)) {  // (uniform)
    if (t == 0) o[7] = 0.0;
    return;
  }
  const int base = p.m - kTdNovLen;  // (>= 0: the role runs from m = 1024 on)
  auto pe = [&](int i) {
    const int j = base + i;
    const double v = p.audio.at(f, j);
    return (j == 0 ? v : v - 0.97 * p.audio.at(f, j - 1)) * p.han_n[i];
  };
  double2* A = smem;
  double2* B = smem + K;
  for (int k = t; k < K; k += kT) A[k] = make_double2(pe(2 * k), pe(2 * k + 1));
  __syncthreads();
  const double2* Z = tr_fft(A, B, K, p.tw_n);
  double s = 0.0;
  for (int q = t; q < kTdNovBins; q += kT) {
    double2 X;
    if (q == 0)
      X = make_double2(Z[0].x + Z[0].y, 0.0);
    else if (q == K)
      X = make_double2(Z[0].x - Z[0].y, 0.0);
    else
      X = tr_rfft_bin(Z, K, q, p.tw2_n);
    const double mag = hypot(X.x, X.y);
    w[q] = atan2(X.y, X.x);
    w[kTdNovBins + q] = mag;
    s += mag;
  }
  s = block_sum(s, red);
  if (t == 0) o[7] = s;
}

struct V4 {
  double a, b, c, d;
};
__device__ __forceinline__ V4 mv4(const double* __restrict__ M, const V4& v) {
  return {M[0] * v.a + M[1] * v.b + M[2] * v.c + M[3] * v.d, M[4] * v.a + M[5] * v.b + M[6] * v.c + M[7] * v.d,
          M[8] * v.a + M[9] * v.b + M[10] * v.c + M[11] * v.d, M[12] * v.a + M[13] * v.b + M[14] * v.c + M[15] * v.d};
}
__device__ __forceinline__ V4 add4(const V4& x, const V4& y) { return {x.a + y.a, x.b + y.b, x.c + y.c, x.d + y.d}; }
__device__ __forceinline__ V4 shfl_up4(const V4& v, int d) {
  return {__shfl_up(v.a, d, 64), __shfl_up(v.b, d, 64), __shfl_up(v.c, d, 64), __shfl_up(v.d, d, 64)};
}

// One order-4 lfilter pass over v[0..n) in place (rev: over v[n-1..0]), from the state s0
__device__ __forceinline__ void td_lfilter(double* v, int n, bool rev, const TdetectParams& p, V4 s0, V4* sc) {
  const int t = threadIdx.x;
  const int L = (n + kT - 1) / kT;
  const int lo = min(t * L, n), hi = min(lo + L, n);
  const TdScan& S = *p.scan;
  auto at = [&](int k) -> double& { return v[rev ? n - 1 - k : k]; };
  V4 z{0.0, 0.0, 0.0, 0.0};
  auto step = [&](double u) {
    const double y = p.b[0] * u + z.a;
    z.a = (z.b + p.b[1] * u) - p.a[1] * y;
    z.b = (z.c + p.b[2] * u) - p.a[2] * y;
    z.c = (z.d + p.b[3] * u) - p.a[3] * y;
    z.d = p.b[4] * u - p.a[4] * y;
    return y;
  };
  // 1) the chunk's end state from the zero state
  for (int k = lo; k < hi; ++k) step(at(k));
  V4 c = z;
  if (t == 0) c = add4(c, mv4(S.Pd[0], s0));
  // 2) inclusive scan of the carries, c_t = sum_j P^(t-j) e_j (the initial state folded into e_0)
  const int lane = t & 63, wv = t >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int d = 1 << k;
    const V4 o = shfl_up4(c, d);
    if (lane >= d) c = add4(c, mv4(S.Pd[k], o));
  }
  if (lane == 63) sc[wv] = c;  // wave totals
  __syncthreads();
  V4 X{0.0, 0.0, 0.0, 0.0};  // carry into this wave: X_w = P^64 X_{w-1} + S_{w-1}
  for (int j = 0; j < wv; ++j) X = add4(mv4(S.P64, X), sc[j]);
  c = add4(c, mv4(S.Pl[lane], X));
  // the incoming state of this thread's chunk: the prefix of the thread before it
  V4 s = shfl_up4(c, 1);
  if (lane == 0) s = wv == 0 ? s0 : X;
  // 3) the chunk from its incoming state, outputs in place
  z = s;
  for (int k = lo; k < hi; ++k) {
    double& r = at(k);
    r = step(r);
  }
  __syncthreads();  // (sc is next written by the following pass)
}

__device__ __forceinline__ void td_hf(const TdetectParams& p, int64_t f, double2* smem, double* red, V4* sc) {
  constexpr int E = kTdPad;
  const int t = threadIdx.x, m = p.m, n = m + 2 * E;
  double* o = p.out + f * kTdCols;
  double* ext = reinterpret_cast<double*>(smem);  // [m + 2 E] <= 2 m doubles (m >= 256)
  if (td_bad(p, f, red)) {  // (uniform)
    if (t == 0) o[8] = 0.0;
    return;
  }
  const double x0 = p.audio.at(f, 0), xl = p.audio.at(f, m - 1);
  for (int j = t; j < n; j += kT) {
    double v;
    if (j >= E && j < E + m)
      v = p.audio.at(f, j - E);
    else if (j < E)
      v = 2.0 * x0 - p.audio.at(f, E - j);  // odd_ext
    else
      v = 2.0 * xl - p.audio.at(f, m - 2 - (j - E - m));
    ext[j] = v;
  }
  __syncthreads();
  const double e0 = ext[0];
  td_lfilter(ext, n, false, p, V4{p.zi[0] * e0, p.zi[1] * e0, p.zi[2] * e0, p.zi[3] * e0}, sc);
  const double e1 = ext[n - 1];  // (rewritten only behind the backward pass's first barrier)
  td_lfilter(ext, n, true, p, V4{p.zi[0] * e1, p.zi[1] * e1, p.zi[2] * e1, p.zi[3] * e1}, sc);
  double s = 0.0;
  for (int k = t; k < m; k += kT) s = fma(ext[E + k], ext[E + k], s);
  s = block_sum(s, red);
  if (t == 0) o[8] = s;
}

__device__ __forceinline__ void td_scalar(const TdetectParams& p, int64_t f, double2* smem, double* red, int* ii,
                                          double* chunk) {
  const int t = threadIdx.x, m = p.m, K = p.n_bins;
  double* o = p.out + f * kTdCols;
  double* x = reinterpret_cast<double*>(smem);  // [m]
  const float* g = p.spec.row(f);
  if (t == 0) {
    ii[0] = m;      // the first argmax
    ii[1] = 0;      // start: the last i < peak below a tenth of the peak
    ii[2] = m - 1;  // end: the first i > peak below it
    ii[3] = K;      // the rolloff bin
  }
  double bad = 0.0;
  for (int i = t; i < m; i += kT) {
    const double v = p.audio.at(f, i);
    if (!isfinite(v)) bad = 1.0;
    x[i] = v;
  }
  for (int i = t; i < K; i += kT)
    if (!isfinite(g[i])) bad = 1.0;
  bad = block_sum(bad, red);  // (the barriers publish x and ii)
  if (bad > 0.0) {              // (uniform)
    if (t < kTdCols && (t == 2 || t == 3 || t >= 9 || (t == 7 && !p.nov) || (t == 8 && !p.hf))) o[t] = 0.0;
    return;
  }
  // the time domain
  double ssq = 0.0, mx = 0.0, sgn = 0.0;
  for (int i = t; i < m; i += kT) {
    const double v = x[i];
    ssq = fma(v, v, ssq);
    mx = fmax(mx, fabs(v));
    if (i + 1 < m) {
      const double u = x[i + 1];
      sgn += fabs((double)((u > 0.0) - (u < 0.0)) - (double)((v > 0.0) - (v < 0.0)));
    }
  }
  ssq = block_sum(ssq, red);
  sgn = block_sum(sgn, red);
  const double peak = block_max(mx, red);
  for (int i = t; i < m; i += kT)
    if (fabs(x[i]) == peak) {
      atomicMin(&ii[0], i);
      break;  // (ascending on a thread)
    }
  __syncthreads();
  const int pk = ii[0];
  const double tenth = 0.1 * peak;
  for (int i = t; i < m; i += kT)
    if (fabs(x[i]) < tenth) {
      if (i < pk) atomicMax(&ii[1], i);
      if (i > pk) atomicMin(&ii[2], i);
    }
  // the spectrum: thread t owns the bins [lo, hi)
  const int C = (K + kT - 1) / kT, lo = min(t * C, K), hi = min(lo + C, K);
  double cs = 0.0, fsum = 0.0, band[4] = {0.0, 0.0, 0.0, 0.0};
  int guard = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (p.band_idx[b] < K && p.band_idx[b + 1] < K) guard |= 1 << b;
  for (int i = lo; i < hi; ++i) {
    const double s = (double)g[i];
    cs += s;
    fsum = fma((double)i * p.bin_hz, s, fsum);
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (((guard >> b) & 1) && i >= p.band_idx[b] && i < p.band_idx[b + 1]) band[b] += s;
  }
  chunk[t] = cs;
  __syncthreads();  // (publishes chunk, and the index atomics above)
  double run = 0.0, off = 0.0;
  for (int j = 0; j < kT; ++j) {
    if (j == t) off = run;
    run += chunk[j];
  }
  const double total = run, thr = 0.85 * total;
  if (total > 0.0) {
    double cum = off;
    for (int i = lo; i < hi; ++i) {
      cum += (double)g[i];
      if (cum >= thr) {
        atomicMin(&ii[3], i);
        break;
      }
    }
  }
  fsum = block_sum(fsum, red);
#pragma unroll
  for (int b = 0; b < 4; ++b) band[b] = block_sum(band[b], red);  // (the barriers publish ii[3])
  if (t == 0) {
    o[2] = peak;
    o[3] = ssq;
    if (!p.nov) o[7] = 0.0;
    if (!p.hf) o[8] = 0.0;
    o[9] = sgn;
    o[10] = (double)pk;
    o[11] = (double)ii[1];
    o[12] = (double)ii[2];
    o[13] = total;
    o[14] = fsum;
    o[15] = total > 0.0 ? (double)min(ii[3], K - 1) : 0.0;
    for (int b = 0; b < 4; ++b) o[16 + b] = band[b];
    o[20] = (double)guard;
  }
}

}  // namespace

__global__ __launch_bounds__(kT) void tdetect_kernel(TdetectParams p) {
  extern __shared__ __attribute__((aligned(16))) double2 td_smem[];
  __shared__ double red[4];
  __shared__ V4 sc[kT / 64];
  __shared__ int ii[4];
  __shared__ double chunk[kT];
  const int64_t b = blockIdx.x, f = b % p.n_frames;
  switch (p.roles[b / p.n_frames]) {
    case kTdEnvelope: td_envelope(p, f, td_smem, red); break;
    case kTdFlux: td_flux(p, f, td_smem, red); break;
    case kTdNovelty: td_novelty(p, f, td_smem, red); break;
    case kTdHf: td_hf(p, f, td_smem, red, sc); break;
    default: td_scalar(p, f, td_smem, red, ii, chunk); break;
  }
}

// Workgroup f < n_frames: frame f's flags, flux and novelty. Workgroup n_frames: the outgoing state.
__global__ __launch_bounds__(kT) void tdetect_cross_kernel(TdetectParams p) {
  __shared__ double red[4];
  __shared__ int prev[2];
  const int t = threadIdx.x;
  const int64_t f = blockIdx.x, F = p.n_frames;
  const double* sin = p.state_in;
  if (t == 0) {  // the nearest two frames before f without a non-finite input
    int n = 0;
    prev[0] = prev[1] = -1;
    for (int64_t g = f - 1; g >= 0 && n < 2; --g)
      if (p.ws[g * kTdWsStride] == 0.0) prev[n++] = (int)g;
  }
  __syncthreads();
  const bool has_spec = sin && sin[0] != 0.0, has_phase = p.nov && sin && sin[1] != 0.0;
  const double* sp = prev[0] >= 0 ? p.ws + (int64_t)prev[0] * kTdWsStride + 2 : (has_spec ? sin + 4 : nullptr);
  const double *p1 = nullptr, *p2 = nullptr;  // prev_phase, prev_prev_phase
  if (p.nov) {
    const double* s1 = has_phase ? sin + 4 + kTdFluxBins : nullptr;
    if (prev[0] >= 0) {
      p1 = p.ws + (int64_t)prev[0] * kTdWsStride + 2 + kTdFluxBins;
      // :364 a stream's second frame: prev_prev_phase is the first frame's phase too
      p2 = prev[1] >= 0 ? p.ws + (int64_t)prev[1] * kTdWsStride + 2 + kTdFluxBins : (has_phase ? s1 : p1);
    } else if (has_phase) {
      p1 = s1;
      p2 = s1 + kTdNovBins;
    }
  }
  if (f == F) {
    double* so = p.state_out;
    if (!so) return;
    if (t < 4) so[t] = t == 0 ? (sp ? 1.0 : 0.0) : (t == 1 ? (p1 ? 1.0 : 0.0) : 0.0);
    for (int i = t; i < kTdFluxBins; i += kT) so[4 + i] = sp ? sp[i] : 0.0;
    for (int i = t; i < kTdNovBins; i += kT) {
      so[4 + kTdFluxBins + i] = p1 ? p1[i] : 0.0;
      so[4 + kTdFluxBins + kTdNovBins + i] = p2 ? p2[i] : 0.0;
    }
    return;
  }
  double* o = p.out + f * kTdCols;
  const double* w = p.ws + f * kTdWsStride;
  const int shape = (p.hf ? 0 : 2) | (p.nov ? 0 : 4);
  if (w[0] != 0.0) {  // (uniform) a non-finite input: the flag alone
    if (t == 0) {
      o[0] = 1.0;
      o[5] = 0.0;
      o[6] = 0.0;
    }
    return;
  }
  double flux = 0.0, nov = 0.0;
  if (sp)
    for (int i = t; i < kTdFluxBins; i += kT) flux += fmax(0.0, w[2 + i] - sp[i]);
  if (p1) {
    const double* ph = w + 2 + kTdFluxBins;
    for (int i = t; i < kTdNovBins; i += kT) {
      const double target = 2.0 * p1[i] - p2[i];
      nov += ph[kTdNovBins + i] * fmin(fabs(ph[i] - target), kTdPi);
    }
  }
  flux = block_sum(flux, red);
  nov = block_sum(nov, red);
  if (t == 0) {
    o[0] = (double)(shape | (sp ? 0 : 8) | (p1 ? 0 : 16));
    o[5] = flux;
    o[6] = nov;
  }
}

size_t tdetect_lds_bytes(int m) { return std::max<size_t>((size_t)m * sizeof(double2), kTdFluxLen * sizeof(double2)); }

hipError_t launch_tdetect(const TdetectParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const size_t lds = tdetect_lds_bytes(p.m);
  if (lds + 4 * 1024 > 64 * 1024) {  // (the kernel's static arrays take under 4 KiB)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&tdetect_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(tdetect_kernel, dim3((unsigned)(p.n_frames * p.n_roles)), dim3(kT), lds, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tdetect_cross_kernel, dim3((unsigned)(p.n_frames + 1)), dim3(kT), 0, s, p);
  return hipGetLastError();
}

}  // namespace omega
