// The float64 workgroup primitives of the feature kernels (pitch, harmonic, genre, hip-hop, phase, room,
// voice, transients, transient detection, bass zoom): complex multiply, bit reversal, wave and block
// reductions, the in-place radix-2 transform pair in LDS, and the chunked scan of one biquad section.
//
// CONTRACTION. These functions take the floating-point contraction state of the including file at the
// point of inclusion: a function is compiled under the state in force where its text is parsed. A file
// that sets `#pragma clang fp contract(off)` at file scope includes this header AFTER the pragma (hiphop,
// harmonic, genre, phase, room, voice: their a * b + c stays two roundings, here as in their own code);
// a file without the pragma gets the compiler's default, fused multiply-adds (pitch, transient, tdetect,
// basszoom). Which side a kernel is on is part of its result bits. No file-scope pragma belongs in this
// or any other header: it would leak into the rest of the including file.
//
// WAVES. block_sum, block_max, block_min_i and block_sums reduce over W waves and read W slots per value:
// W is blockDim.x / 64 of the calling kernel, and the default of 4 is for 256-thread workgroups only.
//
// Deliberately NOT here, because each differs in more than a name:
//   - w64_lfilter (weight64.hip): precomputed powers, a shuffle scan, a reverse pass, an initial state,
//     1024 threads
//   - td_lfilter (tdetect.hip): order 4 with a 4-state carry
//   - tr_fft (hilbert64.hpp): the out-of-place Stockham transform with its ping-pong; the in-place pair
//     below runs the butterflies in another order and so gives other result bits
//   - the packing loops around the transforms (pitch's real-even round trip, hip-hop's in-place Hilbert
//     pack, phase's L/R split): each packs differently
//   - gn_max_u64, gn_scan, gn_select (genre.hip): a single user
#pragma once

#include <hip/hip_runtime.h>

namespace omega {

__device__ __forceinline__ double2 zmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

__device__ __forceinline__ int brev(int i, int bits) { return (int)(__brev((unsigned)i) >> (32 - bits)); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block sum over W waves (red: W doubles); every thread gets the sum, the waves added in index order
// (the shuffle loop is written out here and in block_sums: through wave_sum the compiler schedules the
// kernels' code differently from the copies these replaced)
template <int W = 4>
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < W; ++w) s += red[w];
  return s;
}

// block maximum over W waves (W a power of two; red: W doubles), and the minimum of an int on top of it
template <int W = 4>
__device__ __forceinline__ double block_max(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double m[W];
#pragma unroll
  for (int w = 0; w < W; ++w) m[w] = red[w];
#pragma unroll
  for (int s = 1; s < W; s <<= 1)
#pragma unroll
    for (int w = 0; w < W; w += 2 * s) m[w] = fmax(m[w], m[w + s]);
  return m[0];
}
template <int W = 4>
__device__ __forceinline__ int block_min_i(int v, double* red) {
  return (int)-block_max<W>(-(double)v, red);
}

// block sums of N values at once over W waves (red: W N doubles); every thread gets every sum, the waves
// added in index order
template <int N, int W>
__device__ __forceinline__ void block_sums(double (&v)[N], double* red) {
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[n] += __shfl_xor(v[n], o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) red[(threadIdx.x >> 6) * N + n] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) {
    double s = red[n];
#pragma unroll
    for (int w = 1; w < W; ++w) s += red[w * N + n];
    v[n] = s;
  }
}

// K-point complex FFT in place in LDS by T threads, decimation in frequency: natural order in, X[q] at
// brev(q) out. tw[q * tw_stride] = e^{-2 pi i q / K}; slot maps a logical index to its LDS index.
struct SlotIdentity {
  __device__ __forceinline__ int operator()(int i) const { return i; }
};
template <int T, class Slot = SlotIdentity>
__device__ inline void fft_dif(double2* a, int K, const double2* __restrict__ tw, int tw_stride, Slot slot = Slot{}) {
  for (int half = K / 2; half >= 1; half >>= 1) {
    const int step = K / (2 * half);
    for (int j = threadIdx.x; j < K / 2; j += T) {
      const int k = j & (half - 1), i0 = slot((j - k) * 2 + k), i1 = slot((j - k) * 2 + k + half);
      const double2 u = a[i0], v = a[i1];
      a[i0] = make_double2(u.x + v.x, u.y + v.y);
      a[i1] = zmul(make_double2(u.x - v.x, u.y - v.y), tw[k * step * tw_stride]);
    }
    __syncthreads();
  }
}
// the same transform, decimation in time: element q at brev(q) in, natural order out
template <int T, class Slot = SlotIdentity>
__device__ inline void fft_dit(double2* a, int K, const double2* __restrict__ tw, int tw_stride, Slot slot = Slot{}) {
  for (int half = 1; half < K; half <<= 1) {
    const int step = K / (2 * half);
    for (int j = threadIdx.x; j < K / 2; j += T) {
      const int k = j & (half - 1), i0 = slot((j - k) * 2 + k), i1 = slot((j - k) * 2 + k + half);
      const double2 u = a[i0], v = zmul(a[i1], tw[k * step * tw_stride]);
      a[i0] = make_double2(u.x + v.x, u.y + v.y);
      a[i1] = make_double2(u.x - v.x, u.y - v.y);
    }
    __syncthreads();
  }
}

struct M2 {
  double a, b, c, d;
};
__device__ __forceinline__ M2 mmul(const M2& x, const M2& y) {
  return {x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}

// scipy.signal.sosfilt's section (DF2T, zero initial state) over v[0..n) in place by T threads, as a
// chunked scan (sc: [T]): every thread runs its chunk of ceil(n / T) samples from the zero state, the
// chunk end states are combined over the workgroup with the powers of P = A^chunk, and every thread
// re-runs its chunk from its true incoming state. With n < T the chunk is one sample and only the first n
// threads own one: a thread without samples has end state 0 and lies past every thread that owns some,
// so its carry is not read.
template <int T>
__device__ inline void sos_section_scan(double* v, int n, double b0, double b1, double b2, double a1, double a2,
                                        double2* sc) {
  const int t = threadIdx.x;
  const int L = (n + T - 1) / T;
  const int lo = min(t * L, n), hi = min(lo + L, n);
  double z0 = 0.0, z1 = 0.0;
  auto step = [&](double u) {
    const double y = b0 * u + z0;
    z0 = b1 * u + z1 - a1 * y;
    z1 = b2 * u - a2 * y;
    return y;
  };
  for (int k = lo; k < hi; ++k) step(v[k]);
  // inclusive scan of the chunk end states, c_t = sum_j P^(t-j) e_j with P = A^L, A = [[-a1, 1], [-a2, 0]]
  M2 P{1.0, 0.0, 0.0, 1.0}, Ak{-a1, 1.0, -a2, 0.0};
  for (int e = L; e; e >>= 1) {
    if (e & 1) P = mmul(P, Ak);
    Ak = mmul(Ak, Ak);
  }
  double2 c = make_double2(z0, z1);
  for (int d = 1; d < T; d <<= 1) {
    sc[t] = c;
    __syncthreads();
    if (t >= d) {
      const double2 o = sc[t - d];
      c = make_double2(c.x + (P.a * o.x + P.b * o.y), c.y + (P.c * o.x + P.d * o.y));
    }
    __syncthreads();
    P = mmul(P, P);
  }
  sc[t] = c;
  __syncthreads();
  const double2 s = t > 0 ? sc[t - 1] : make_double2(0.0, 0.0);
  z0 = s.x;
  z1 = s.y;
  for (int k = lo; k < hi; ++k) v[k] = step(v[k]);
  __syncthreads();
}

}  // namespace omega
