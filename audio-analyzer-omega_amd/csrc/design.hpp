// Pure host maths of the C API's tables (no HIP call): numpy's windows, float64 twiddles, np.fft.rfftfreq, np.linspace,
// scipy's Butterworth designs and their state-space tables, Savitzky-Golay weights, numpy's pairwise-sum leaves.
// Private to libomega.so: everything here is hidden from the dynamic symbol table.
#pragma once

#include <vector>

#include "params.hpp"

namespace omega_host __attribute__((visibility("hidden"))) {

constexpr double kPi = 3.14159265358979323846;

inline bool is_pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }

// Point i of np.blackman / np.hanning / np.hamming (M) in float64 (kind: OMEGA_WIN_*, any other 1.0);
// M >= 2 (numpy returns ones(1) for M = 1: make_window's case)
double np_window(int kind, int M, int i);
std::vector<float> make_window(int M, int kind);
// np.blackman / np.hanning / np.hamming (M) whole, in float64: np_window per point, [1.0] for M = 1
std::vector<double> np_window64(int kind, int M);
// e^{-2 pi i q / period} for q < count in float64: (cos(2 * M_PI * q / period), -sin(2 * M_PI * q / period)),
// these operations in this order
std::vector<double2> twiddles64(int period, int count);

double rfreq(int k, int N, double fs);
// np.fft.rfftfreq(n, 1 / fs) as numpy evaluates it: val = 1.0 / (n * d), results = arange * val. Not rfreq: the
// rounding differs, and the features' golden files pin this one.
inline double np_rfftfreq_step(int n, double fs) {
  const double d = 1.0 / fs;
  return 1.0 / ((double)n * d);
}
// np.searchsorted(arange(n_bins) * step, v) (side 'left')
inline int searchsorted_left_uniform(double step, int n_bins, double v) {
  int k = 0;
  while (k < n_bins && (double)k * step < v) ++k;
  return k;
}

// np.linspace(0, stop, num)[k] as numpy evaluates it (num >= 2, stop != 0): step = stop / (num - 1), arange * step,
// and the last point is stop itself
inline double np_linspace0(int k, int num, double stop) {
  return k == num - 1 ? stop : (double)k * (stop / (double)(num - 1));
}
// np.linspace(start, stop, num)[k] as numpy evaluates it (num >= 2, stop != start): step = (stop - start) / (num - 1),
// arange * step rounded, + start rounded (two roundings, never one fused), and the last point is stop itself
inline double np_linspace(int k, int num, double start, double stop) {
#pragma clang fp contract(off)
  if (k == num - 1) return stop;
  const double step = (stop - start) / (double)(num - 1);
  const double prod = (double)k * step;
  return prod + start;
}
// np.argmax(np.linspace(0, stop, num) >= v): the first such index, 0 where there is none
inline int linspace0_argmax_ge(int num, double stop, double v) {
  for (int k = 0; k < num; ++k)
    if (np_linspace0(k, num, stop) >= v) return k;
  return 0;
}

struct BiquadCoef {
  double b[3], a[3];
};
BiquadCoef butter2(double fc, double fs, bool high);
BiquadCoef butter1(double fc, double fs, bool high);
void butter4_highpass_sos(double fc, double fs, BiquadCoef out[2]);
void butter4_bandpass_sos(double lo, double hi, double fs, double out[4][6]);
// scipy.signal.butter(4, fc / (fs / 2), 'high') in ba form, its lfilter_zi, and the carry-scan powers of the
// order-4 DF2T recurrence's state matrix for chunks of L samples (tdetect.hip)
void butter4_highpass_ba(double fc, double fs, double b[5], double a[5]);
void lfilter_zi4(const double b[5], const double a[5], double zi[4]);
void lfilter4_scan(const double a[5], int L, omega::TdScan* out);

void mat2_mul(const double* A, const double* B, double* C);
omega::BiquadTab make_biquad_tab(const BiquadCoef& c, int L);

// the mixed-radix transforms' stages for length n: 4s, then 2, 3, 5, 7, then the remaining primes
std::vector<int> fft_radices(int n);
// Savitzky-Golay cubic weights for any odd window w >= 5: W[p * w + t], p the output's position in the window
void savgol_cubic(int w, double* W);
void np_leaves(int off, int n, int depth, std::vector<unsigned>& out);

// ChromagramAnalyzer's genre settings (chromagram.py:37-68, :226-234; genre: omega_tonal_genre, `other` reads pop's
// weights and tolerance as genre_profiles.get(..., pop) does): the blend factor, chromatic_tolerance, and the table
// tonal.hip reads (params.hpp kTnTab*) -- per key 2 root + minor the rotated weighted profile / (its sum + 1e-10)
// (:279-288), the key factors (:305-328), Mw + mw (:272), the plain rotated Krumhansl profiles (:403-404)
double tonal_blend(int genre);
double tonal_tolerance(int genre);
std::vector<double> tonal_table(int genre);

}  // namespace omega_host
