// SpectrogramWaterfall / SpectrogramWaterfallPanel (omega4/panels/spectrogram_waterfall.py) on the device: the dB
// row, the auto-range over the last 20 frames, the normalised row and its colours, in the input's precision as
// numpy 2.x runs the reference (T = float for float32 spectra, double for float64), 256 threads per workgroup.
//
//   waterfall_scan_kernel<T>, one workgroup per frame (:85-91, :302-305): the whole spectrum is scanned for
//     non-finite values and for np.argmax (first occurrence), the n_cells bins of the slice become
//     dB = 20 log10(max(x, 1e-10)) -- log10 in float64 of the exactly widened value, for float32 rounded to float32
//     and then multiplied by 20 in float32 -- and their maximum and minimum are reduced. The stats row gets the
//     flag, (max, min) and the argmax; the dB row is kept in the frame's `rows` output for the second launch (see
//     DESIGN.md for the measurement against recomputing it; OMEGA_WF_RECOMPUTE builds the other variant).
//   waterfall_rows_kernel<T>, behind it on the same stream, one workgroup per frame (:93-121): wave 0 gathers the
//     newest 20 (max, min) pairs -- this frame's, its live predecessors' in this launch (flagged frames passed over,
//     found 64 at a time with a ballot), then the carried state's -- the workgroup rank-sorts both lists, and
//     np.percentile(., 95) and (., 5), numpy's `linear` method with its _lerp, run in T. Every thread then normalises
//     clip((dB + gain - floor) / (peak - floor), 0, 1) and, where asked, maps the cell to RGB (:142-205). Workgroup
//     n_frames gathers the same way over all the launch's frames and writes the outgoing state.
//   waterfall_colors_kernel<T>, one workgroup per row: the colour map alone.
//
// Every thread produces whole pixels. A row's bytes start at any address; the cells in front of the first 4-byte
// boundary and behind the last are stored byte by byte, the rest as four pixels = three 32-bit words per thread.
// Nothing depends on the number of frames in the call: F frames in one call equal F chained calls bit for bit.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)  // (above the project headers: wg64.hpp takes this state)

#include "params.hpp"
#include "wg64.hpp"

namespace omega {

namespace {

constexpr int kT = kWfThreads;
constexpr int kW = kT / 64;

// block maxima of N values at once (red: kW N doubles); every thread gets every maximum
template <int N>
__device__ __forceinline__ void wf_block_maxes(double (&v)[N], double* red) {
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[n] = fmax(v[n], __shfl_xor(v[n], o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) red[(threadIdx.x >> 6) * N + n] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) {
    double m = red[n];
#pragma unroll
    for (int w = 1; w < kW; ++w) m = fmax(m, red[w * N + n]);
    v[n] = m;
  }
}

// 20 * np.log10(np.maximum(x, 1e-10)) in T, as a double (:85)
template <class T>
__device__ __forceinline__ double wf_db(double x) {
  const double l = log10(fmax(x, (double)(T)1e-10));
  return (double)((T)20 * (T)l);
}

// numpy's _lerp
template <class T>
__device__ __forceinline__ T wf_lerp(T a, T b, T t) {
  const T d = b - a;
  T r = a + d * t;
  if (t >= (T)0.5) r = b - d * ((T)1 - t);
  return r;
}

// np.percentile(s, q100) of the n sorted values s, method 'linear', every step in T as numpy takes it on T data:
// q = q100 / T(100), the virtual index (n - 1) q, gamma its fraction
template <class T>
__device__ __forceinline__ T wf_percentile(const double* s, int n, T q100) {
  if (n == 1) return (T)s[0];
  const T vi = (T)(n - 1) * (q100 / (T)100);
  const T lo = floor(vi);
  const int i = (int)lo;
  return wf_lerp<T>((T)s[i], (T)s[i + 1], vi - lo);
}

// _spectrum_to_color (:142-205) of one cell in T: int(255 * ...) truncations of IEEE expressions
template <class T>
__device__ __forceinline__ void wf_color(T x, int scheme, unsigned char* c) {
  x = x < (T)1 ? x : (T)1;  // max(0.0, min(1.0, intensity)); a NaN becomes 1 as Python's min leaves it
  x = x > (T)0 ? x : (T)0;
  int r, g, b;
  if (scheme == 0) {
    if (x < (T)0.25) {
      r = 0, g = (int)((T)255 * (x / (T)0.25)), b = 255;
    } else if (x < (T)0.5) {
      r = 0, g = 255, b = (int)((T)255 * ((T)1 - (x - (T)0.25) / (T)0.25));
    } else if (x < (T)0.75) {
      r = (int)((T)255 * ((x - (T)0.5) / (T)0.25)), g = 255, b = 0;
    } else {
      r = 255, g = (int)((T)255 * ((T)1 - (x - (T)0.75) / (T)0.25)), b = 0;
    }
  } else if (scheme == 1) {
    if (x < (T)0.33) {
      r = (int)((T)255 * (x / (T)0.33)), g = 0, b = 0;
    } else if (x < (T)0.66) {
      r = 255, g = (int)((T)255 * ((x - (T)0.33) / (T)0.33)), b = 0;
    } else {
      r = 255, g = 255, b = (int)((T)255 * ((x - (T)0.66) / (T)0.34));
    }
  } else if (scheme == 2) {
    r = (int)((T)255 * x), g = (int)((T)255 * ((T)1 - x)), b = 255;
  } else if (scheme == 3) {
    // colorsys.hsv_to_rgb(h, 0.9, v); 1.0 - s is Python's float64 difference, then rounded to T
    const T h = (T)0.8 - (T)0.8 * x, v = (T)0.2 + (T)0.8 * x, s = (T)0.9;
    const T h6 = h * (T)6;
    const int i = (int)h6;
    const T f = h6 - (T)i;
    const T p = v * (T)(1.0 - 0.9);
    const T q = v * ((T)1 - s * f);
    const T t = v * ((T)1 - s * ((T)1 - f));
    T cr, cg, cb;
    switch (i % 6) {
      case 0: cr = v, cg = t, cb = p; break;
      case 1: cr = q, cg = v, cb = p; break;
      case 2: cr = p, cg = v, cb = t; break;
      case 3: cr = p, cg = q, cb = v; break;
      case 4: cr = t, cg = p, cb = v; break;
      default: cr = v, cg = p, cb = q; break;
    }
    r = (int)(cr * (T)255), g = (int)(cg * (T)255), b = (int)(cb * (T)255);
  } else {
    r = g = b = (int)((T)255 * x);
  }
  c[0] = (unsigned char)r;
  c[1] = (unsigned char)g;
  c[2] = (unsigned char)b;
}

// One row of n cells through cell(i, c): cell i's work, its colour into c[0..2] where `dst` is wanted. With dst the
// workgroup's threads take the cells in front of dst's first 4-byte boundary and behind the last full group one by
// one and the rest four at a time: pixel s + 4 g starts at a 4-byte boundary when s = address mod 4 (3 s = -s mod 4).
template <class Cell>
__device__ __forceinline__ void wf_row(unsigned char* dst, int n, Cell cell) {
  const int t = threadIdx.x;
  if (!dst) {
    unsigned char none[3];
    for (int i = t; i < n; i += kT) cell(i, none);
    return;
  }
  const int head = min((int)(reinterpret_cast<uintptr_t>(dst) & 3), n);
  const int groups = (n - head) / 4, tail = head + 4 * groups;
  for (int i = t; i < head + (n - tail); i += kT) {
    const int k = i < head ? i : tail + (i - head);
    unsigned char c[3];
    cell(k, c);
    dst[3 * k] = c[0];
    dst[3 * k + 1] = c[1];
    dst[3 * k + 2] = c[2];
  }
  for (int g = t; g < groups; g += kT) {
    const int k = head + 4 * g;
    unsigned char c[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) cell(k + j, c + 3 * j);
    uint32_t* w = reinterpret_cast<uint32_t*>(dst + 3 * k);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      w[j] = (uint32_t)c[4 * j] | (uint32_t)c[4 * j + 1] << 8 | (uint32_t)c[4 * j + 2] << 16 | (uint32_t)c[4 * j + 3] << 24;
  }
}

// Wave 0: the newest kWfHist (max, min) pairs of the live frames [0, upto] of this launch and then of the carried
// state, newest first, into hmax / hmin; returns their number (wave-uniform)
__device__ __forceinline__ int wf_gather(const WaterfallParams& p, int64_t upto, bool has_state, double* hmax, double* hmin) {
  const int lane = threadIdx.x;
  int have = 0;
  for (int64_t base = upto; base >= 0 && have < kWfHist; base -= 64) {
    const int64_t g = base - lane;
    const bool live = g >= 0 && p.stats[g * kWfCols] == 0.0;
    const unsigned long long mask = __ballot(live);
    const int slot = have + __popcll(mask & ((1ull << lane) - 1ull));
    if (live && slot < kWfHist) {
      hmax[slot] = p.stats[g * kWfCols + 1];
      hmin[slot] = p.stats[g * kWfCols + 2];
    }
    have += __popcll(mask);
  }
  have = min(have, kWfHist);
  if (has_state && have < kWfHist) {
    const int cnt = min(max((int)p.state_in[2], 0), kWfHist), take = min(kWfHist - have, cnt);
    if (lane < take) {
      hmax[have + lane] = p.state_in[kWfStateMax + cnt - 1 - lane];
      hmin[have + lane] = p.state_in[kWfStateMin + cnt - 1 - lane];
    }
    have += take;
  }
  return have;
}

}  // namespace

template <class T>
__global__ __launch_bounds__(kT) void waterfall_scan_kernel(WaterfallParams p) {
  __shared__ double red[4 * kW];
  const int t = threadIdx.x, K = p.n_cells, lo = p.first_bin;
  const int64_t f = blockIdx.x;
  const T* x = p.spec.row_as<T>(f);
  T* row = static_cast<T*>(p.rows) + f * K;
  double v[4] = {0.0, -INFINITY, -INFINITY, -INFINITY};  // non-finite, the largest bin, dB max, -(dB min)
  int at = INT32_MAX;
  for (int i = t; i < p.n_bins; i += kT) {
    const double s = (double)x[i];
    if (!isfinite(s)) v[0] = 1.0;
    if (s > v[1]) {  // (i ascends: a thread keeps the first of its equal bins)
      v[1] = s;
      at = i;
    }
    if (i >= lo && i < lo + K) {
      const double d = wf_db<T>(s);
#ifndef OMEGA_WF_RECOMPUTE
      row[i - lo] = (T)d;
#endif
      v[2] = fmax(v[2], d);
      v[3] = fmax(v[3], -d);
    }
  }
  const double mine = v[1];
  wf_block_maxes<4>(v, red);
  const bool bad = v[0] > 0.0;
  double first[1] = {mine == v[1] ? -(double)at : -(double)INT32_MAX};  // np.argmax: the first of the largest
  wf_block_maxes<1>(first, red);  // (its first barrier stands between the reads of red above and its writes)
  double* o = p.stats + f * kWfCols;
  if (bad) {  // (uniform) the flag alone, and a zero row
    if (t < kWfCols) o[t] = t == 0 ? (double)kWfNonFinite : 0.0;
    for (int i = t; i < K; i += kT) row[i] = (T)0;
    return;
  }
  if (t == 0) {
    o[0] = 0.0;
    o[1] = v[2];
    o[2] = -v[3];
    o[3] = o[4] = 0.0;
    o[5] = -first[0];
    o[6] = v[1];
  }
}

// Workgroup f < n_frames: frame f's range, row and colours. Workgroup n_frames: the outgoing state.
template <class T>
__global__ __launch_bounds__(kT) void waterfall_rows_kernel(WaterfallParams p) {
  __shared__ double hmax[kWfHist], hmin[kWfHist], smax[kWfHist], smin[kWfHist];
  __shared__ double range[2];
  __shared__ int count;
  const int t = threadIdx.x, K = p.n_cells;
  const int64_t f = blockIdx.x, F = p.n_frames;
  const bool writer = f == F;
  if (writer && !p.state_out) return;
  const double* sin = p.state_in;
  const bool has_state = sin && sin[0] != 0.0;
  unsigned char* rgb = !writer && p.rgb ? p.rgb + (size_t)f * K * 3 : nullptr;
  T* row = static_cast<T*>(p.rows) + f * K;
  if (!writer && p.stats[f * kWfCols] != 0.0) {  // (uniform) a flagged frame: the zero row's colours
    const int scheme = p.scheme;
    if (rgb) wf_row(rgb, K, [&](int, unsigned char* c) { wf_color<T>((T)0, scheme, c); });
    return;
  }
  if (t < 64) {
    const int n = wf_gather(p, writer ? F - 1 : f, has_state, hmax, hmin);
    if (t == 0) count = n;
  }
  __syncthreads();
  const int n = count;
  if (t < n) {
    const double a = hmax[t], b = hmin[t];
    int ra = 0, rb = 0;
    for (int j = 0; j < n; ++j) {
      ra += hmax[j] < a || (hmax[j] == a && j < t);
      rb += hmin[j] < b || (hmin[j] == b && j < t);
    }
    smax[ra] = a;
    smin[rb] = b;
  }
  __syncthreads();
  if (t == 0) {
    double peak = has_state ? sin[kWfStatePeak] : 0.0, floor_ = has_state ? sin[kWfStatePeak + 1] : -80.0;  // :39-40
    if (p.auto_gain && n > 0) {
      peak = (double)wf_percentile<T>(smax, n, (T)95);
      floor_ = (double)wf_percentile<T>(smin, n, (T)5);
    }
    range[0] = peak;
    range[1] = floor_;
    if (!writer) {
      p.stats[f * kWfCols + 3] = peak;
      p.stats[f * kWfCols + 4] = floor_;
    }
  }
  __syncthreads();
  if (writer) {
    double* so = p.state_out;
    const bool valid = n > 0 || has_state;  // (no live frame yet: the zeros of a blob that was never written)
    if (t < kWfHist) {  // oldest first
      so[kWfStateMax + t] = t < n ? hmax[n - 1 - t] : 0.0;
      so[kWfStateMin + t] = t < n ? hmin[n - 1 - t] : 0.0;
    }
    if (t == 0) {
      so[0] = valid ? 1.0 : 0.0;
      so[1] = valid ? (double)p.spec.f64 : 0.0;
      so[2] = (double)n;
      so[kWfStatePeak] = valid ? range[0] : 0.0;
      so[kWfStatePeak + 1] = valid ? range[1] : 0.0;
    }
    return;
  }
  const T peak = (T)range[0], floor_ = (T)range[1], gain = (T)p.gain_db;
  const T span = peak - floor_;
  const int scheme = p.scheme;
#ifdef OMEGA_WF_RECOMPUTE
  const T* x = p.spec.row_as<T>(f) + p.first_bin;
#endif
  wf_row(rgb, K, [&](int i, unsigned char* c) {
#ifdef OMEGA_WF_RECOMPUTE
    const T db = (T)wf_db<T>((double)x[i]);
#else
    const T db = row[i];
#endif
    T v = (T)0;
    if (span > (T)0) {  // :114-121
      v = (db + gain - floor_) / span;
      v = v > (T)0 ? v : (T)0;
      v = v < (T)1 ? v : (T)1;
    }
    row[i] = v;
    if (rgb) wf_color<T>(v, scheme, c);
  });
}

template <class T>
__global__ __launch_bounds__(kT) void waterfall_colors_kernel(WaterfallColorParams p) {
  const int64_t r = blockIdx.x;
  const T* x = p.in.row_as<T>(r);
  const int scheme = p.scheme;
  wf_row(p.rgb + (size_t)r * p.n_cells * 3, p.n_cells, [&](int i, unsigned char* c) { wf_color<T>(x[i], scheme, c); });
}

hipError_t launch_waterfall(const WaterfallParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const dim3 scan((unsigned)p.n_frames), rows((unsigned)(p.n_frames + 1));
  if (p.spec.f64)
    hipLaunchKernelGGL(waterfall_scan_kernel<double>, scan, dim3(kT), 0, s, p);
  else
    hipLaunchKernelGGL(waterfall_scan_kernel<float>, scan, dim3(kT), 0, s, p);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (p.spec.f64)
    hipLaunchKernelGGL(waterfall_rows_kernel<double>, rows, dim3(kT), 0, s, p);
  else
    hipLaunchKernelGGL(waterfall_rows_kernel<float>, rows, dim3(kT), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_waterfall_colors(const WaterfallColorParams& p, hipStream_t s) {
  if (p.n_rows <= 0) return hipSuccess;
  if (p.in.f64)
    hipLaunchKernelGGL(waterfall_colors_kernel<double>, dim3((unsigned)p.n_rows), dim3(kT), 0, s, p);
  else
    hipLaunchKernelGGL(waterfall_colors_kernel<float>, dim3((unsigned)p.n_rows), dim3(kT), 0, s, p);
  return hipGetLastError();
}

}  // namespace omega
