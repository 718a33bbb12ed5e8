// The float64 transform shared by transient.hip and tdetect.hip, for 256-thread workgroups: the radix-2
// Stockham FFT in LDS with a float64 twiddle table, the real-signal (un)packing around it and |hilbert(x)|
// of a power-of-two frame. Like wg64.hpp, whose primitives it uses, it takes the including file's
// floating-point contraction state.
#pragma once

#include <hip/hip_runtime.h>

#include "wg64.hpp"

namespace omega {

constexpr int kTrThreads = 256;

// Stockham radix-2 forward FFT of K points: a -> (a, b ping-pong); returns the buffer holding X
// (tw: [K / 2] e^{-2 pi i m / K})
__device__ inline double2* tr_fft(double2* a, double2* b, int K, const double2* __restrict__ tw) {
  for (int ns = 1; ns < K; ns <<= 1) {
    const int step = K / (2 * ns);
    for (int j = threadIdx.x; j < K / 2; j += kTrThreads) {
      const int k = j & (ns - 1);
      const double2 u = a[j], v = zmul(a[j + K / 2], tw[k * step]);
      const int o = (j / ns) * 2 * ns + k;
      b[o] = make_double2(u.x + v.x, u.y + v.y);
      b[o + ns] = make_double2(u.x - v.x, u.y - v.y);
    }
    __syncthreads();
    double2* t = a;
    a = b;
    b = t;
  }
  return a;
}

// rfft bin q in 0..K of the real signal packed as z[n] = x[2n] + i x[2n+1], from Z = FFT_K(z)
// (tw2: [K + 1] e^{-2 pi i q / (2 K)})
__device__ __forceinline__ double2 tr_rfft_bin(const double2* Z, int K, int q, const double2* __restrict__ tw2) {
  const double2 a = Z[q % K], b = Z[(K - q) % K];
  const double2 e = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));   // (Z_q + conj Z_{K-q}) / 2
  const double2 o = make_double2(0.5 * (a.y + b.y), -0.5 * (a.x - b.x));  // (Z_q - conj Z_{K-q}) / 2i
  const double2 w = tw2[q];                                               // e^{-2 pi i q / N}
  const double2 ow = zmul(o, w);
  return make_double2(e.x + ow.x, e.y + ow.y);
}

// |hilbert(x)| = sqrt(x^2 + H(x)^2) of the N = 2 K samples xin(0..N), H(x) = irfft(-i X) with X = rfft(x) (DC and
// Nyquist zeroed: scipy's h = [1, 2, ..., 2, 1, 0, ...]) -- two K-point complex FFTs over the LDS buffers A and B
// (K double2 each). Returns the envelope's N doubles (in A or B) and in *spare the other buffer.
template <class XIn>
__device__ __forceinline__ double* tr_hilbert_env(XIn xin, int N, double2* A, double2* B, const double2* __restrict__ tw,
                                                  const double2* __restrict__ tw2, double2** spare) {
  const int K = N / 2;
  // 1) rfft of x as a K-point complex FFT of z[n] = x[2n] + i x[2n+1]
  for (int k = threadIdx.x; k < K; k += kTrThreads) A[k] = make_double2(xin(2 * k), xin(2 * k + 1));
  __syncthreads();
  double2* Z = tr_fft(A, B, K, tw);
  double2* Y = Z == A ? B : A;
  // 2) X_k (k = 0..K) and Y_k = -i X_k, DC and Nyquist zeroed; then the packed inverse spectrum
  //    Z'_k = (Y_k + conj Y_{K-k}) + i e^{2 pi i k / N} (Y_k - conj Y_{K-k}), stored conjugated so that
  //    the forward FFT gives conj(K * ifft)
  for (int k = threadIdx.x; k < K; k += kTrThreads) {
    auto Yq = [&](int q) {
      if (q == 0 || q == K) return make_double2(0.0, 0.0);
      const double2 x = tr_rfft_bin(Z, K, q, tw2);
      return make_double2(x.y, -x.x);  // -i X
    };
    const double2 yk = Yq(k), ym = Yq(K - k);
    const double2 s = make_double2(yk.x + ym.x, yk.y - ym.y);  // Y_k + conj Y_{K-k}
    const double2 d = make_double2(yk.x - ym.x, yk.y + ym.y);  // Y_k - conj Y_{K-k}
    const double2 w = tw2[k];                                   // conj e^{2 pi i k / N}
    const double2 id = zmul(make_double2(-d.y, d.x), make_double2(w.x, -w.y));
    Y[k] = make_double2(s.x + id.x, -(s.y + id.y));
  }
  __syncthreads();
  double2* Bf = Y == A ? B : A;
  double2* Hz = tr_fft(Y, Bf, K, tw);
  // 3) envelope: H(x)[2n] = Re(ifft) / 2, H(x)[2n + 1] = Im(ifft) / 2, ifft = conj(FFT(conj)) / K
  double* env = reinterpret_cast<double*>(Hz == A ? B : A);
  const double sc = 0.5 / K;
  for (int k = threadIdx.x; k < K; k += kTrThreads) {
    const double h0 = Hz[k].x * sc, h1 = -Hz[k].y * sc;
    const double x0 = xin(2 * k), x1 = xin(2 * k + 1);
    env[2 * k] = sqrt(x0 * x0 + h0 * h0);
    env[2 * k + 1] = sqrt(x1 * x1 + h1 * h1);
  }
  __syncthreads();
  *spare = Hz;
  return env;
}

}  // namespace omega
