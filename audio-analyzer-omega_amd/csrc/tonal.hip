// ChromagramAnalyzer's key, alternative-key and chord scores and MusicTheory.analyze_mode for every root
// (omega4/panels/chromagram.py:215-339, :396-418, :670-812; omega4/panels/music_theory.py:175-200) on the device,
// float64, contraction off. G lanes work on one frame, 256 / G frames share a workgroup; G = 16 (sixteen frames per
// workgroup) is the product, G = 64 (one wave per frame) the measured alternative.
//
//   1. lanes 0..11 roll the frame's raw row and its predecessor's (the previous row of the launch, or the carried
//      state for the launch's first frame) and blend prev * (1 - a) + cur * a (:215-237); a frame marked `first`,
//      or without a carry, stays unblended. The launch's last frame writes the outgoing state.
//   2. every lane derives the scalars all scores share from the 12 values: numpy's pairwise sum, the variance, the
//      centred row, the sqrt-compressed weighted row of detect_key and its centred form.
//   3. the 24 + 24 correlations, the 84 mode correlations and the 2 x 156 chord cells are dealt to the lanes and
//      land in LDS; np.corrcoef as numpy evaluates it (centre, dot, * 1/11, / sqrt(cxx), / sqrt(cyy), clip).
//   4. sixteen lanes take the decisions, each by a serial scan in the reference's order (Python's max, a stable
//      descending sort, `score > best`), and every lane copies the detail matrices out.
//
// A frame with a non-finite value keeps its blended row, is flagged, and is scored as the all-zero row. Nothing
// depends on the number of frames in the call: F frames in one call equal F chained calls bit for bit.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#include "params.hpp"

namespace omega {

namespace {

// chord_types in dict order (chromagram.py:79-93) and MusicTheory.MODES as pitch-class masks (music_theory.py:22-30)
__device__ constexpr int kChordSize[kTnTypes] = {3, 3, 3, 3, 4, 4, 4, 5, 5, 7, 2, 3, 3};
__device__ constexpr int kChord[kTnTypes][7] = {{0, 4, 7},        {0, 3, 7},        {0, 3, 6},     {0, 4, 8},
                                                {0, 4, 7, 11},    {0, 3, 7, 10},    {0, 4, 7, 10}, {0, 4, 7, 11, 2},
                                                {0, 3, 7, 10, 2}, {0, 4, 7, 10, 2, 5, 9}, {0, 7},  {0, 2, 7},
                                                {0, 5, 7}};
__device__ constexpr unsigned kModeMask[kTnModes] = {0xAB5, 0x6AD, 0x5AB, 0xAD5, 0x6B5, 0x5AD, 0x56B};

// LDS layout of one frame (doubles)
constexpr int kX = 0, kKey = 12, kAlt = kKey + kTnKeys, kMode = kAlt + kTnKeys, kCh = kMode + 12 * kTnModes,
              kLds = kCh + 2 * kTnCells;

// np.add.reduce over 12 contiguous float64 values: eight accumulators, their tree, then the tail
__device__ __forceinline__ double sum12(const double (&a)[12]) {
  double r = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  r += a[8];
  r += a[9];
  r += a[10];
  r += a[11];
  return r;
}

// a - np.mean(a), and np.var(a) (the mean of the squares of the centred values)
__device__ __forceinline__ double centre12(const double (&a)[12], double (&c)[12]) {
  const double mean = sum12(a) / 12.0;
  double sq[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    c[j] = a[j] - mean;
    sq[j] = c[j] * c[j];
  }
  return sum12(sq) / 12.0;
}

// np.corrcoef(x, y)[0, 1] from the centred x and the raw y
__device__ __forceinline__ double corr12(const double (&xm)[12], const double (&y)[12]) {
  double ym[12];
  centre12(y, ym);
  const double fact = 1.0 / 11.0;
  double cxx = 0.0, cxy = 0.0, cyy = 0.0;
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    cxx += xm[j] * xm[j];
    cxy += xm[j] * ym[j];
    cyy += ym[j] * ym[j];
  }
  cxx *= fact;
  cxy *= fact;
  cyy *= fact;
  double r = cxy / sqrt(cxx);
  r = r / sqrt(cyy);
  return fmin(fmax(r, -1.0), 1.0);
}

__device__ __forceinline__ bool metal_or_rock(int genre) { return genre == kTnMetal || genre == kTnRock; }

// one cell of detect_chord's score matrix (:691-752), v = 1 the anti-stick variant (:781-812); NaN: not tested
__device__ double chord_cell(const double* x, int v, int r, int t, int genre, double tol) {
  const bool metal = metal_or_rock(genre);
  const unsigned tested = genre == kTnJazz ? kTnTypesAll : (metal ? kTnTypesMetal : kTnTypesBasic);
  if ((v && !metal) || !(tested >> t & 1u)) return __builtin_nan("");
  double thr = metal ? 0.02 : 0.03;
  if (!v && metal && r == 2) thr = 0.15;
  if (x[r] < thr) return __builtin_nan("");
  const int size = kChordSize[t];
  unsigned in = 0;
  double score = 0.0;
  for (int i = 0; i < size; ++i) {
    const int pitch = (r + kChord[t][i]) % 12;
    in |= 1u << pitch;
    score += x[pitch] * (i == 0 ? 2.0 : (i == 1 && t == kTnPower ? 1.8 : 1.0));
  }
  const double pen = t == kTnPower ? tol * 0.5 : tol;
  for (int pitch = 0; pitch < 12; ++pitch)
    if (!(in >> pitch & 1u)) score -= x[pitch] * pen;
  score /= (double)size;
  const bool minor_sus = t == 1 || t == 11 || t == 12;
  if (v) {
    if (t == kTnPower) score *= 1.5;
    else if (minor_sus) score *= 1.2;
    return score;
  }
  if (genre == kTnJazz) {
    if (t == 4 || t == 5 || t == 6 || t == 9) score *= 1.2;
  } else if (metal) {
    if (t == kTnPower) {
      score *= 1.5;
      if (r == 2 && x[2] > 0.15) score *= x[9] > 0.05 ? 2.0 : 1.5;
    } else if (minor_sus) {
      score *= 1.2;
    }
  } else if (genre == kTnPop) {
    if (t <= 1) score *= 1.1;
  } else if (genre == kTnClassical) {
    if (t <= 2) score *= 1.1;
  }
  return score;
}

// the first maximum of v[0..n) not at `skip0` / `skip1`, NaN cells passed over: its index, or -1
__device__ int first_max(const double* v, int n, int skip0, int skip1) {
  int best = -1;
  double bv = 0.0;
  for (int i = 0; i < n; ++i) {
    const double c = v[i];
    if (i == skip0 || i == skip1 || c != c) continue;
    if (best < 0 || c > bv) {
      best = i;
      bv = c;
    }
  }
  return best;
}

template <int G>
__global__ __launch_bounds__(kTnThreads) void tonal_kernel(TonalParams p) {
  constexpr int FPW = kTnThreads / G;
  __shared__ double sh[FPW * kLds];
  const int g = threadIdx.x / G, l = threadIdx.x % G;
  const int64_t f = (int64_t)blockIdx.x * FPW + g;
  const bool live = f < p.n_frames;
  double* s = sh + g * kLds;

  // 1. roll and blend
  double mine = 0.0;
  if (live && l < 12) {
    const int off = p.roll ? p.roll[f] : 0;
    const double cur = p.raw[f * 12 + (l - off + 12) % 12];
    if (f == p.n_frames - 1 && p.state_out) {
      p.state_out[1 + l] = cur;
      if (l == 0) p.state_out[0] = 1.0;
    }
    const bool first = p.first && p.first[f];
    bool has = false;
    double prev = 0.0;
    if (!first) {
      if (f > 0) {
        const int po = p.roll ? p.roll[f - 1] : 0;
        prev = p.raw[(f - 1) * 12 + (l - po + 12) % 12];
        has = true;
      } else if (p.state_in && p.state_in[0] != 0.0) {
        prev = p.state_in[1 + l];
        has = true;
      }
    }
    mine = has ? prev * (1.0 - p.blend) + cur * p.blend : cur;
    s[kX + l] = mine;
  }
  __syncthreads();
  bool finite = true;
  for (int j = 0; j < 12; ++j) finite = finite && isfinite(live ? s[kX + j] : 0.0);
  __syncthreads();
  if (live && l < 12 && !finite) s[kX + l] = 0.0;
  __syncthreads();

  // 2. what every score shares
  double x[12], xm[12], w[12], wm[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) x[j] = live ? s[kX + j] : 0.0;
  const double total = sum12(x);
  const double var = centre12(x, xm);
  {
    double sq[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) sq[j] = sqrt(x[j]);
    const double den = sum12(sq) + 1e-10;
#pragma unroll
    for (int j = 0; j < 12; ++j) w[j] = ((sq[j] / den) * p.tab[kTnTabW + j]) / 2.0;
  }
  const double wvar = centre12(w, wm);

  // 3. the scores
  if (live) {
    for (int i = l; i < 2 * kTnKeys; i += G) {
      const bool alt = i >= kTnKeys;
      const int k = alt ? i - kTnKeys : i;
      const double* prof = p.tab + (alt ? kTnTabAlt : kTnTabKey) + k * 12;
      double y[12], a[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        y[j] = prof[j];
        a[j] = alt ? xm[j] : wm[j];
      }
      double r = 0.0;
      if ((alt ? var : wvar) > 0.0) r = corr12(a, y);
      if (!alt) r *= p.tab[kTnTabFac + k];
      s[kKey + i] = r;  // (kAlt follows kKey)
    }
    for (int i = l; i < 12 * kTnModes; i += G) {
      const int root = i / kTnModes, m = i % kTnModes;
      double rx[12], rm[12], y[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        rx[j] = s[kX + (j + root) % 12];
        y[j] = (kModeMask[m] >> j & 1u) ? 1.0 / 7.0 : 0.0;
      }
      const double rv = centre12(rx, rm);
      s[kMode + i] = rv > 0.0 ? corr12(rm, y) : 0.0;
    }
    for (int i = l; i < 2 * kTnCells; i += G) {
      const int v = i / kTnCells, c = i % kTnCells;
      s[kCh + i] = chord_cell(s + kX, v, c / kTnTypes, c % kTnTypes, p.genre, p.tolerance);
    }
  }
  __syncthreads();
  if (!live) return;

  // 4. decisions and outputs
  double* row = p.rows + f * kTnCols;
  if (l < 12) row[l] = mine;
  if (l == 12) {
    row[12] = (double)((finite ? 0 : kTnNonFinite) | (total == 0.0 ? kTnZeroSum : 0) | (var < 0.001 ? kTnFlat : 0));
    row[13] = var;
  }
  if (l == 0) {
    const int k = first_max(s + kKey, kTnKeys, -1, -1);
    row[14] = (double)k;
    row[15] = k < 0 ? 0.0 : s[kKey + k];
  } else if (l == 1) {
    const int a0 = first_max(s + kAlt, kTnKeys, -1, -1);
    const int a1 = first_max(s + kAlt, kTnKeys, a0, -1);
    const int a2 = first_max(s + kAlt, kTnKeys, a0, a1);
    const int a[3] = {a0, a1, a2};
    for (int q = 0; q < 3; ++q) {
      row[16 + q] = (double)a[q];
      row[19 + q] = a[q] < 0 ? 0.0 : s[kAlt + a[q]];
    }
  } else if (l == 2) {
    int best = -1;
    double bv = 0.0;
    for (int i = 0; i < kTnCells; ++i)
      if (s[kCh + i] > bv) {
        bv = s[kCh + i];
        best = i;
      }
    row[22] = (double)best;
    row[23] = bv;
  } else if (l == 3) {
    const double* a = s + kCh + kTnCells;
    const int a0 = first_max(a, kTnCells, -1, -1);
    const int a1 = a0 < 0 ? -1 : first_max(a, kTnCells, a0, -1);
    row[24] = (double)a0;
    row[25] = a0 < 0 ? 0.0 : a[a0];
    row[26] = (double)a1;
    row[27] = a1 < 0 ? 0.0 : a[a1];
  } else if (l < 16) {
    const int root = l - 4;
    int best = 0;
    double bv = 0.0;
    for (int m = 0; m < kTnModes; ++m)
      if (s[kMode + root * kTnModes + m] > bv) {
        bv = s[kMode + root * kTnModes + m];
        best = m;
      }
    row[28 + root] = (double)best;
    row[40 + root] = bv;
  }
  if (p.key_corr)
    for (int i = l; i < kTnKeys; i += G) p.key_corr[f * kTnKeys + i] = s[kKey + i];
  if (p.alt_corr)
    for (int i = l; i < kTnKeys; i += G) p.alt_corr[f * kTnKeys + i] = s[kAlt + i];
  if (p.mode)
    for (int i = l; i < 12 * kTnModes; i += G) p.mode[f * 12 * kTnModes + i] = s[kMode + i];
  if (p.chord)
    for (int i = l; i < 2 * kTnCells; i += G) p.chord[f * 2 * kTnCells + i] = s[kCh + i];
}

}  // namespace

hipError_t launch_tonal(const TonalParams& p, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  constexpr int FPW = kTnThreads / kTnLanes;
  hipLaunchKernelGGL(tonal_kernel<kTnLanes>, dim3((unsigned)((p.n_frames + FPW - 1) / FPW)), dim3(kTnThreads), 0, s, p);
  return hipGetLastError();
}

}  // namespace omega
