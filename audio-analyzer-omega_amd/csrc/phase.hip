// PhaseCorrelationPanel's analysis (omega4/panels/phase_correlation.py:124-220) for a batch of independent
// stereo frames, on the real left and right channels (the reference's update() fabricates the right one):
// one 256-thread workgroup per frame, everything in float64 (float32 samples are widened on load). Every
// loop has a fixed bound and no workgroup waits for another.
//
//   :147-164  _calculate_correlation: the means, then the centred sums of a second pass over the frame
//             (two-pass like the reference, never raw moments), mean(ln rn) / (std_l std_r) clipped to
//             [-1, 1], 0.0 when a std is 0
//   :128-136  stereo_width = 1 - |correlation|; rms of both channels, balance = (r - l) / (r + l)
//   :166-177  the goniometer points of every step-th sample, in the reference's operation order (contraction
//             is off in this file; the division by sqrt(2) is IEEE's)
//   :193-220  |rfft(l hanning)| and |rfft(r hanning)| as ONE m-point complex transform of z = l w + i r w:
//             L_k = (Z_k + conj Z_{m-k}) / 2, R_k = (Z_k - conj Z_{m-k}) / 2i; per band the same clipped
//             correlation of the two magnitude segments, again two-pass. The split leaves in each channel's
//             bins about 1e-16 of the other channel's magnitudes: a channel whose sum of squares is exactly
//             0 is therefore given its exact all-zero spectrum (every band 0.0), and a channel more than
//             about 200 dB below the other has band correlations of rounding residue
//
// LDS: the frame as m double2 (l, r), windowed in place, transformed in place, the magnitude pairs written
// over the transform: 16 bytes per sample, 128.25 KiB at m = 8192 (one workgroup per CU), 32.25 KiB at 2048
// (four per CU). The transform is radix-2 decimation in frequency, natural order in, X[q] at slot brev(q)
// out. In a pass consecutive lanes own consecutive butterflies, so each 16-lane group of a 16-byte LDS read
// covers the 16 slots of one 256-byte bank row down to half = 16; the last four passes (half 8..1) are
// two-way conflicted, and the 16-byte stores stay inside their own transfer time. What comes after the
// transform reads bins in natural order, i.e. slots brev(k): 16 consecutive bins lie m / 16 slots apart, on
// ONE bank slot. The buffer is therefore skewed by one slot per m / 16 slots, slot(i) = i + (i >> (bits - 4)):
// 16 slots more in all, consecutive slots stay consecutive inside a block of m / 16 (the passes keep their
// pattern) and 16 consecutive bins fall on 16 different bank slots.
//
// Reductions are lane-strided block sums, not numpy's pairwise order: they agree with it to a few 1e-16
// relative; the bar on what they feed is 1e-9 (include/omega.h).
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)  // (above the project headers: wg64.hpp takes this state)

#include "params.hpp"
#include "wg64.hpp"

namespace omega {

namespace {

constexpr int kPT = kPhaseThreads;

// :152-164 from the centred sums over n values; *flat: a std (or their product) was 0, the 0.0 fallback
__device__ __forceinline__ double ph_corr(double cll, double crr, double clr, double n, bool* flat) {
  const double sl = sqrt(cll / n), sr = sqrt(crr / n), den = sl * sr;
  *flat = !(sl > 0.0 && sr > 0.0 && den > 0.0);
  if (*flat) return 0.0;
  const double c = (clr / n) / den;
  return fmax(-1.0, fmin(c, 1.0));
}

}  // namespace

__global__ __launch_bounds__(kPT) void phase_kernel(PhaseParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ph_smem[];
  __shared__ double red[4 * 5];
  __shared__ double bsum[kPhaseBands][4][2];
  __shared__ double bcen[kPhaseBands][4][3];
  __shared__ int blo[kPhaseBands], bhi[kPhaseBands];  // (constant indices into the kernel argument)
  const int t = threadIdx.x, m = p.m, bits = p.bits, sk = bits - 4;
  const int64_t f = blockIdx.x;
  double2* Z = reinterpret_cast<double2*>(ph_smem);  // [m + 16], slot(i) = i + (i >> sk)
  auto slot = [sk](int i) { return i + (i >> sk); };
  const Row xl = p.left.row(f), xr = p.right.row(f);
  double* o = p.out + f * kPhaseCols;
  double* pts = p.points ? p.points + f * (kPhasePoints * 2) : nullptr;
  if (t == 0) {
#pragma unroll
    for (int b = 0; b < kPhaseBands; ++b) blo[b] = p.first[b], bhi[b] = p.last[b];
  }

  // the frame, the means (:153-154)
  double a[3] = {0.0, 0.0, 0.0};
  for (int i = t; i < m; i += kPT) {
    const double l = xl[i], r = xr[i];
    Z[slot(i)] = make_double2(l, r);
    if (!isfinite(l) || !isfinite(r)) a[0] = 1.0;
    a[1] += l;
    a[2] += r;
  }
  block_sums<3, 4>(a, red);  // (the barriers publish blo and bhi)
  if (a[0] > 0.0) {  // (uniform) a non-finite sample: the zero row, flag bit 0, no points
    if (t < kPhaseCols) o[t] = t == 5 ? 1.0 : 0.0;
    if (pts) pts[t] = 0.0;  // (kPT = 2 kPhasePoints)
    return;
  }
  const double dm = (double)m, ml = a[1] / dm, mr = a[2] / dm;

  // the centred sums and the squares; each thread windows its own samples in place
  double c[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = t; i < m; i += kPT) {
    const double2 v = Z[slot(i)];
    const double dl = v.x - ml, dr = v.y - mr, w = p.hann[i];
    c[0] += dl * dl;
    c[1] += dr * dr;
    c[2] += dl * dr;
    c[3] += v.x * v.x;
    c[4] += v.y * v.y;
    Z[slot(i)] = make_double2(v.x * w, v.y * w);
  }
  block_sums<5, 4>(c, red);  // (the barriers publish the windowed frame)

  // :169-177 every step-th sample, straight from the input
  if (pts && t < kPhasePoints) {
    const int step = max(1, m / 100), i = t * step;
    double x = 0.0, y = 0.0;
    if (i < m) {
      const double l = xl[i], r = xr[i];
      const double mid = (l + r) / 2.0, side = (l - r) / 2.0, rt2 = 1.4142135623730951;  // math.sqrt(2)
      x = (mid - side) / rt2 * 0.5;
      y = (mid + side) / rt2 * 0.5;
    }
    pts[2 * t] = x;
    pts[2 * t + 1] = y;
  }

  // the m-point transform in place, decimation in frequency
  fft_dif<kPT>(Z, m, p.tw, 1, slot);
  // bins k and m - k give |L_k| and |R_k|, stored over Z_k: no other thread touches either slot
  for (int k = t; k <= m / 2; k += kPT) {
    const int pk = slot(brev(k, bits)), pm = slot(brev((m - k) & (m - 1), bits));
    const double2 zk = Z[pk], zm = Z[pm];
    const double lx = 0.5 * (zk.x + zm.x), ly = 0.5 * (zk.y - zm.y);
    const double rx = 0.5 * (zk.y + zm.y), ry = -0.5 * (zk.x - zm.x);
    Z[pk] = make_double2(sqrt(lx * lx + ly * ly), sqrt(rx * rx + ry * ry));
  }
  __syncthreads();

  // :202-220 per band: the means, then the centred sums; each wave leaves its partial sums
#pragma unroll 1
  for (int b = 0; b < kPhaseBands; ++b) {
    double s0 = 0.0, s1 = 0.0;
    for (int k = blo[b] + t; k < bhi[b]; k += kPT) {
      const double2 g = Z[slot(brev(k, bits))];
      s0 += g.x;
      s1 += g.y;
    }
    s0 = wave_sum(s0), s1 = wave_sum(s1);
    if ((t & 63) == 0) bsum[b][t >> 6][0] = s0, bsum[b][t >> 6][1] = s1;
  }
  __syncthreads();
#pragma unroll 1
  for (int b = 0; b < kPhaseBands; ++b) {
    const int n = bhi[b] - blo[b];
    if (n <= 0) continue;  // (uniform)
    const double gl = (bsum[b][0][0] + bsum[b][1][0] + bsum[b][2][0] + bsum[b][3][0]) / (double)n;
    const double gr = (bsum[b][0][1] + bsum[b][1][1] + bsum[b][2][1] + bsum[b][3][1]) / (double)n;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k = blo[b] + t; k < bhi[b]; k += kPT) {
      const double2 g = Z[slot(brev(k, bits))];
      const double dl = g.x - gl, dr = g.y - gr;
      s0 += dl * dl;
      s1 += dr * dr;
      s2 += dl * dr;
    }
    s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
    if ((t & 63) == 0) bcen[b][t >> 6][0] = s0, bcen[b][t >> 6][1] = s1, bcen[b][t >> 6][2] = s2;
  }
  __syncthreads();

  if (t < kPhaseBands) {
    const int n = bhi[t] - blo[t];
    double v = 0.0;
    // (an all-zero channel has an all-zero spectrum, std 0, the 0.0 fallback; in the shared transform its
    // bins would hold the other channel's rounding residue instead)
    if (n > 0 && c[3] > 0.0 && c[4] > 0.0) {
      bool flat;
      v = ph_corr(bcen[t][0][0] + bcen[t][1][0] + bcen[t][2][0] + bcen[t][3][0],
                  bcen[t][0][1] + bcen[t][1][1] + bcen[t][2][1] + bcen[t][3][1],
                  bcen[t][0][2] + bcen[t][1][2] + bcen[t][2][2] + bcen[t][3][2], (double)n, &flat);
    }
    o[7 + t] = v;
  }
  if (t == 0) {
    bool flat;
    const double corr = ph_corr(c[0], c[1], c[2], dm, &flat);
    const double rl = sqrt(c[3] / dm), rr = sqrt(c[4] / dm), tot = rl + rr;
    int mask = 0;
    for (int b = 0; b < kPhaseBands; ++b) mask |= (bhi[b] > blo[b]) << b;
    o[0] = corr;
    o[1] = 1.0 - fabs(corr);
    o[2] = tot > 0.0 ? (rr - rl) / tot : 0.0;
    o[3] = rl;
    o[4] = rr;
    o[5] = (tot > 0.0 ? 0.0 : 2.0) + (flat ? 4.0 : 0.0);
    o[6] = (double)mask;
  }
}

size_t phase_lds_bytes(int m) { return ((size_t)m + 16) * sizeof(double2); }

hipError_t launch_phase(const PhaseParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const size_t lds = phase_lds_bytes(p.m);
  if (lds + 4 * 1024 > 64 * 1024) {  // (the kernel's static arrays take under 1 KiB)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&phase_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(phase_kernel, dim3((unsigned)p.n_frames), dim3(kPT), lds, s, p);
  return hipGetLastError();
}

}  // namespace omega
