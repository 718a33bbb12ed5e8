// The pure host maths declared in design.hpp, each in float64 with the operations of the numpy / scipy
// routine it reproduces.
#include "design.hpp"

#include <cmath>
#include <complex>
#include <cstring>

#include "../../include/omega.h"

using namespace omega;

namespace omega_host __attribute__((visibility("hidden"))) {

// numpy window formulas (numpy 2.x): n = arange(1-M, M, 2)
double np_window(int kind, int M, int i) {
  const double n = (double)(1 - M + 2 * i);
  switch (kind) {
    case OMEGA_WIN_BLACKMAN: return 0.42 + 0.5 * std::cos(kPi * n / (M - 1)) + 0.08 * std::cos(2.0 * kPi * n / (M - 1));
    case OMEGA_WIN_HANN: return 0.5 + 0.5 * std::cos(kPi * n / (M - 1));
    case OMEGA_WIN_HAMMING: return 0.54 + 0.46 * std::cos(kPi * n / (M - 1));
    default: return 1.0;
  }
}

std::vector<float> make_window(int M, int kind) {
  std::vector<float> w(M);
  for (int i = 0; i < M; ++i) w[i] = M == 1 ? 1.0f : (float)np_window(kind, M, i);
  return w;
}

std::vector<double> np_window64(int kind, int M) {
  std::vector<double> w(M);
  for (int i = 0; i < M; ++i) w[i] = M == 1 ? 1.0 : np_window(kind, M, i);
  return w;
}

std::vector<double2> twiddles64(int period, int count) {
  std::vector<double2> t(count);
  for (int q = 0; q < count; ++q) t[q] = make_double2(std::cos(2 * M_PI * q / period), -std::sin(2 * M_PI * q / period));
  return t;
}

// np.fft.rfftfreq(N, 1/fs)
double rfreq(int k, int N, double fs) {
  const double d = 1.0 / fs;
  const double val = 1.0 / (N * d);
  return k * val;
}

// scipy.signal.butter(2, fc/(fs/2), 'low' / 'high') and butter(1, ..., 'high' / 'low') (bilinear transform,
// prewarped); first-order sections as biquads with b2 = a2 = 0
BiquadCoef butter2(double fc, double fs, bool high) {
  const double K = std::tan(kPi * fc / fs);
  const double n = 1.0 + std::sqrt(2.0) * K + K * K;
  BiquadCoef c;
  c.b[0] = high ? 1.0 / n : K * K / n;
  c.b[1] = high ? -2.0 / n : 2.0 * K * K / n;
  c.b[2] = high ? 1.0 / n : K * K / n;
  c.a[0] = 1.0;
  c.a[1] = 2.0 * (K * K - 1.0) / n;
  c.a[2] = (1.0 - std::sqrt(2.0) * K + K * K) / n;
  return c;
}
BiquadCoef butter1(double fc, double fs, bool high) {
  const double K = std::tan(kPi * fc / fs);
  BiquadCoef c;
  c.b[0] = high ? 1.0 / (1.0 + K) : K / (1.0 + K);
  c.b[1] = high ? -1.0 / (1.0 + K) : K / (1.0 + K);
  c.b[2] = 0.0;
  c.a[0] = 1.0;
  c.a[1] = (K - 1.0) / (K + 1.0);
  c.a[2] = 0.0;
  return c;
}

// scipy.signal.butter(4, fc/(fs/2), 'high', output='sos'): the analog prototype's pole pairs at angles
// pi/8 and 3 pi/8 from the negative real axis (Q = 1 / (2 cos)), each through lp2hp and the prewarped
// bilinear transform: b = (1, -2, 1) / n, a = (1, 2 (K^2 - 1) / n, (1 - K / Q + K^2) / n), n = 1 + K / Q + K^2.
// zpk2sos orders the sections by pole radius (the pair nearest the unit circle, 3 pi/8, last) and
// puts the whole gain on the first.
void butter4_highpass_sos(double fc, double fs, BiquadCoef out[2]) {
  const double K = std::tan(kPi * fc / fs);
  double gain = 1.0;
  for (int s = 0; s < 2; ++s) {
    const double iq = 2.0 * std::cos(kPi * (s == 0 ? 1.0 : 3.0) / 8.0);  // 1 / Q
    const double n = 1.0 + K * iq + K * K;
    gain /= n;
    BiquadCoef& c = out[s];
    c.b[0] = 1.0;
    c.b[1] = -2.0;
    c.b[2] = 1.0;
    c.a[0] = 1.0;
    c.a[1] = 2.0 * (K * K - 1.0) / n;
    c.a[2] = (1.0 - K * iq + K * K) / n;
  }
  for (double& b : out[0].b) b *= gain;
}

// scipy.signal.butter(4, [lo, hi], 'bandpass', fs=fs, output='sos') as scipy builds it: buttap's four
// poles, lp2bp_zpk around wo = sqrt(w1 w2) with bw = w2 - w1 (w = 4 tan(pi f / fs): the prewarped edges
// at scipy's internal rate 2), bilinear_zpk (four zeros at +1 from the origin, four at -1 from infinity),
// then zpk2sos with pairing 'nearest': the pole pair nearest the unit circle is taken first and goes LAST,
// each with the two remaining zeros nearest to it, the whole gain on the first section. Poles come in
// exact conjugate pairs, so a = (1, -2 Re p, |p|^2). out[s] = b0 b1 b2 a0 a1 a2.
void butter4_bandpass_sos(double lo, double hi, double fs, double out[4][6]) {
  using cd = std::complex<double>;
  const double w1 = 4.0 * std::tan(kPi * (2.0 * lo / fs) / 2.0), w2 = 4.0 * std::tan(kPi * (2.0 * hi / fs) / 2.0);
  const double bw = w2 - w1, wo = std::sqrt(w1 * w2);
  cd p[8];
  for (int i = 0; i < 4; ++i) {
    const int m = -3 + 2 * i;
    const cd lp = -std::exp(cd(0.0, kPi * m / 8.0)) * bw / 2.0;
    const cd r = std::sqrt(lp * lp - wo * wo);
    p[i] = lp + r;
    p[4 + i] = lp - r;
  }
  cd den(1.0, 0.0);
  for (int i = 0; i < 8; ++i) den *= 4.0 - p[i];
  const double gain = bw * bw * bw * bw * (cd(256.0, 0.0) / den).real();
  std::vector<cd> pz;  // one pole of each conjugate pair
  for (int i = 0; i < 8; ++i) {
    const cd z = (4.0 + p[i]) / (4.0 - p[i]);
    if (z.imag() > 0.0) pz.push_back(z);
  }
  int n_minus = 4, n_plus = 4;  // zeros left at -1 and at +1
  for (int si = 0; si < 4 && !pz.empty(); ++si) {
    size_t best = 0;
    for (size_t i = 1; i < pz.size(); ++i)
      if (std::abs(1.0 - std::abs(pz[i])) < std::abs(1.0 - std::abs(pz[best]))) best = i;
    const cd p1 = pz[best];
    pz.erase(pz.begin() + (long)best);
    double z[2];
    for (double& zz : z) {
      const bool minus = n_minus > 0 && (n_plus == 0 || std::abs(p1 + 1.0) <= std::abs(p1 - 1.0));
      zz = minus ? -1.0 : 1.0;
      --(minus ? n_minus : n_plus);
    }
    double* o = out[3 - si];
    o[0] = 1.0;
    o[1] = -(z[0] + z[1]);
    o[2] = z[0] * z[1];
    o[3] = 1.0;
    o[4] = -2.0 * p1.real();
    o[5] = p1.real() * p1.real() + p1.imag() * p1.imag();
  }
  for (int k = 0; k < 3; ++k) out[0][k] *= gain;
}

// scipy.signal.butter(4, fc / (fs / 2), 'high'): zpk2tf's b = k poly([1, 1, 1, 1]) = k (1, -4, 6, -4, 1) and
// a = poly(p), here the product of the two sections' quadratics (the pole pairs are exact conjugates).
void butter4_highpass_ba(double fc, double fs, double b[5], double a[5]) {
  BiquadCoef s[2];
  butter4_highpass_sos(fc, fs, s);
  const double k = s[0].b[0];
  const double pb[5] = {1.0, -4.0, 6.0, -4.0, 1.0};
  for (int i = 0; i < 5; ++i) {
    b[i] = k * pb[i];
    a[i] = 0.0;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) a[i + j] += s[0].a[i] * s[1].a[j];
}

// scipy.signal.lfilter_zi: (I - companion(a).T) zi = b[1:] - a[1:] b[0]. The rows add up to
// zi[0] sum(a) = sum(B); each following row then gives the next state.
void lfilter_zi4(const double b[5], const double a[5], double zi[4]) {
  double B[4], sb = 0.0, sa = a[0];
  for (int i = 0; i < 4; ++i) {
    B[i] = b[i + 1] - a[i + 1] * b[0];
    sb += B[i];
    sa += a[i + 1];
  }
  zi[0] = sb / sa;
  zi[1] = (1.0 + a[1]) * zi[0] - B[0];
  zi[2] = a[2] * zi[0] + zi[1] - B[1];
  zi[3] = a[3] * zi[0] + zi[2] - B[2];
}

static void mat4_mul(const double* A, const double* B, double* C) {
  double t[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += A[i * 4 + k] * B[k * 4 + j];
      t[i * 4 + j] = s;
    }
  std::memcpy(C, t, sizeof t);
}

// z' = A z + B u with A = companion(a).T: P = A^L carries a state over a chunk of L samples
void lfilter4_scan(const double a[5], int L, TdScan* out) {
  const double A[16] = {-a[1], 1, 0, 0, -a[2], 0, 1, 0, -a[3], 0, 0, 1, -a[4], 0, 0, 0};
  double P[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (int i = 0; i < L; ++i) mat4_mul(A, P, P);
  std::memcpy(out->Pd[0], P, sizeof P);
  for (int k = 1; k < 6; ++k) mat4_mul(out->Pd[k - 1], out->Pd[k - 1], out->Pd[k]);
  mat4_mul(out->Pd[5], out->Pd[5], out->P64);
  std::memcpy(out->Pl[0], P, sizeof P);
  for (int l = 1; l < 64; ++l) mat4_mul(P, out->Pl[l - 1], out->Pl[l]);
}

void mat2_mul(const double* A, const double* B, double* C) {
  double t[4] = {A[0] * B[0] + A[1] * B[2], A[0] * B[1] + A[1] * B[3], A[2] * B[0] + A[3] * B[2],
                 A[2] * B[1] + A[3] * B[3]};
  std::memcpy(C, t, sizeof t);
}

BiquadTab make_biquad_tab(const BiquadCoef& c, int L) {
  BiquadTab t{};
  const double b0 = c.b[0], a1 = c.a[1], a2 = c.a[2];
  const double B0 = c.b[1] - a1 * b0, B1 = c.b[2] - a2 * b0;
  t.b0 = (float)b0;
  t.a1 = (float)a1;
  t.a2 = (float)a2;
  t.B0 = (float)B0;
  t.B1 = (float)B1;
  // scipy.signal.lfilter_zi: solve (I - companion(a).T) zi = B
  const double z0 = (B0 + B1) / (1.0 + a1 + a2);
  t.zi0 = (float)z0;
  t.zi1 = (float)(B1 - a2 * z0);
  const double A[4] = {-a1, 1.0, -a2, 0.0};
  double An[4] = {1, 0, 0, 1};
  for (int n = 0; n < 64; ++n) {
    if (n < L) {
      t.h0[n] = (float)An[0];
      t.h1[n] = (float)An[1];
    }
    if (n + 1 <= L) mat2_mul(A, An, An);
  }
  // A^j B, j < L
  {
    double g[2] = {B0, B1};
    for (int j = 0; j < L && j < 64; ++j) {
      t.g0[j] = (float)g[0];
      t.g1[j] = (float)g[1];
      const double n0 = A[0] * g[0] + A[1] * g[1], n1 = A[2] * g[0] + A[3] * g[1];
      g[0] = n0;
      g[1] = n1;
    }
  }
  // An = A^L now (L <= 64)
  double P[4];
  std::memcpy(P, An, sizeof P);
  double Pk[4] = {P[0], P[1], P[2], P[3]};
  for (int l = 0; l < 64; ++l) {
    for (int q = 0; q < 4; ++q) t.pw[l][q] = (float)Pk[q];
    mat2_mul(P, Pk, Pk);
  }
  return t;
}

std::vector<int> fft_radices(int n) {
  std::vector<int> rad;
  int r = n;
  while (r % 4 == 0) rad.push_back(4), r /= 4;
  for (int f : {2, 3, 5, 7})
    while (r % f == 0) rad.push_back(f), r /= f;
  for (int f = 11; (int64_t)f * f <= r; f += 2)
    while (r % f == 0) rad.push_back(f), r /= f;
  if (r > 1) rad.push_back(r);
  return rad;
}

// Savitzky-Golay cubic weights of scipy.signal.savgol_filter's 'interp' mode for any odd window w >= 5:
// W[p * w + t] is the weight of window sample t in the least-squares cubic's value at window position p
// (p = w / 2: the interior correlation; the other rows: the first / last w / 2 outputs of a frame), in the
// centred, scaled coordinate u = (t - h) / h, h = w / 2, so that the 4 x 4 normal equations stay well
// conditioned.
void savgol_cubic(int w, double* W) {
  const int h = w / 2;
  std::vector<double> A((size_t)w * 4);
  double G[4][4] = {};
  for (int t = 0; t < w; ++t)
    for (int j = 0; j < 4; ++j) A[(size_t)t * 4 + j] = std::pow((t - h) / (double)h, j);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      for (int t = 0; t < w; ++t) G[i][j] += A[(size_t)t * 4 + i] * A[(size_t)t * 4 + j];
  double M[4][8];  // Gauss-Jordan inverse of the normal matrix
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 8; ++j) M[i][j] = j < 4 ? G[i][j] : (j - 4 == i ? 1.0 : 0.0);
  for (int c = 0; c < 4; ++c) {
    int pv = c;
    for (int r = c + 1; r < 4; ++r)
      if (std::fabs(M[r][c]) > std::fabs(M[pv][c])) pv = r;
    for (int j = 0; j < 8; ++j) std::swap(M[c][j], M[pv][j]);
    const double d = M[c][c];
    for (int j = 0; j < 8; ++j) M[c][j] /= d;
    for (int r = 0; r < 4; ++r)
      if (r != c) {
        const double f = M[r][c];
        for (int j = 0; j < 8; ++j) M[r][j] -= f * M[c][j];
      }
  }
  for (int p = 0; p < w; ++p) {
    double v[4], q[4] = {};
    for (int j = 0; j < 4; ++j) v[j] = std::pow((p - h) / (double)h, j);
    for (int j = 0; j < 4; ++j)
      for (int i = 0; i < 4; ++i) q[j] += v[i] * M[i][j + 4];
    for (int t = 0; t < w; ++t) {
      double s = 0.0;
      for (int j = 0; j < 4; ++j) s += q[j] * A[(size_t)t * 4 + j];
      W[(size_t)p * w + t] = s;
    }
  }
}

// The leaves of numpy's pairwise float32 sum over n elements (numpy/_core/src/umath/loops_utils.h.src:
// up to 128 elements a leaf, above that halves split at a multiple of 8 below n / 2), in the
// recursion's depth-first order, as offset | length << 16 -- the table post_frame_kernel's range means
// read instead of walking the recursion per lane (numpy_emul.hpp np_leaf_sums_tab)
void np_leaves(int off, int n, int depth, std::vector<unsigned>& out) {
  if (depth == 0 || n <= 128) {
    out.push_back((unsigned)off | (unsigned)n << 16);
    return;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  np_leaves(off, n2, depth - 1, out);
  np_leaves(off + n2, n - n2, depth - 1, out);
}

// ---- ChromagramAnalyzer's genre tables (chromagram.py:31-68) ----
namespace {
const double kKrumhansl[2][12] = {{6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88},
                                  {6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17}};
// major_weights, minor_weights per profile: pop, jazz, classical, metal, rock
const double kGenreWeights[5][2][12] = {
    {{1.5, 0.5, 1.0, 0.5, 1.2, 1.0, 0.5, 1.2, 0.5, 1.0, 0.5, 0.8}, {1.5, 0.6, 1.0, 1.2, 0.6, 1.0, 0.6, 1.2, 1.0, 0.6, 1.0, 0.8}},
    {{1.0, 0.8, 1.0, 0.9, 1.0, 1.0, 0.9, 1.0, 0.8, 1.0, 0.8, 1.0}, {1.0, 0.8, 1.0, 1.0, 0.9, 1.0, 0.8, 1.0, 1.0, 0.9, 1.0, 0.9}},
    {{1.2, 0.7, 1.0, 0.7, 1.1, 1.0, 0.7, 1.1, 0.7, 1.0, 0.7, 0.9}, {1.2, 0.8, 1.0, 1.1, 0.8, 1.0, 0.8, 1.1, 1.0, 0.8, 1.0, 0.9}},
    {{1.8, 0.4, 1.2, 0.4, 1.0, 1.2, 0.6, 1.4, 0.4, 1.0, 0.4, 0.6}, {1.8, 0.6, 1.2, 1.4, 0.5, 1.2, 0.5, 1.4, 1.2, 0.5, 1.2, 0.7}},
    {{1.6, 0.5, 1.1, 0.5, 1.1, 1.1, 0.6, 1.3, 0.5, 1.0, 0.5, 0.7}, {1.6, 0.6, 1.1, 1.3, 0.6, 1.1, 0.6, 1.3, 1.1, 0.6, 1.1, 0.8}}};
const double kGenreTolerance[5] = {0.2, 0.8, 0.3, 0.6, 0.4};
int genre_profile(int genre) { return genre >= 0 && genre < 5 ? genre : 0; }
// np.add.reduce over 12 contiguous float64 values
double np_sum12(const double* a) {
  double r = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  for (int i = 8; i < 12; ++i) r += a[i];
  return r;
}
}  // namespace

double tonal_blend(int genre) {
  return genre == OMEGA_TONAL_METAL || genre == OMEGA_TONAL_ROCK ? 0.7 : (genre == OMEGA_TONAL_JAZZ ? 0.5 : 0.3);
}
double tonal_tolerance(int genre) { return kGenreTolerance[genre_profile(genre)]; }

std::vector<double> tonal_table(int genre) {
  const double(&W)[2][12] = kGenreWeights[genre_profile(genre)];
  std::vector<double> t(kTnTabLen, 0.0);
  for (int root = 0; root < 12; ++root)
    for (int minor = 0; minor < 2; ++minor) {
      const int k = 2 * root + minor;
      double* key = &t[kTnTabKey + k * 12];
      double* alt = &t[kTnTabAlt + k * 12];
      for (int j = 0; j < 12; ++j) {  // np.roll(v, root)[j] = v[(j - root) mod 12]
        const int src = (j - root + 12) % 12;
        alt[j] = kKrumhansl[minor][src];
        key[j] = kKrumhansl[minor][src] * W[minor][src];
      }
      const double den = np_sum12(key) + 1e-10;
      for (int j = 0; j < 12; ++j) key[j] = key[j] / den;
      // note_names holds sharps: of jazz's ['F', 'Bb', 'Eb', 'Ab'] only F ever matches (:307)
      double fac = 1.0;
      if (genre == OMEGA_TONAL_JAZZ && root == 5) fac = 1.1;
      if (genre == OMEGA_TONAL_CLASSICAL && !minor && (root == 0 || root == 7 || root == 2 || root == 9 || root == 5)) fac = 1.05;
      if (genre == OMEGA_TONAL_ROCK && (root == 4 || root == 9 || root == 2 || root == 7)) fac = 1.05;
      t[kTnTabFac + k] = fac;
    }
  for (int j = 0; j < 12; ++j) t[kTnTabW + j] = W[0][j] + W[1][j];
  return t;
}

}  // namespace omega_host
