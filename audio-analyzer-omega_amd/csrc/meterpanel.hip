// ProfessionalMetersPanel.update's own work on the device (omega4/panels/professional_meters.py:348-397, :568-579):
// what the panel does with a frame and with the dict calculate_lufs returned for it.
//
// meterpanel_frame_kernel, the per-sample work, in the frame's dtype (:376-397): d = diff(|x|) and the count and the
// first index of d > 0.1 (float32: fabsf, the float32 subtraction, the compare against float32(0.1)), max |x| with
// np.max's NaN propagation, sqrt(mean(x ** 2)) with numpy's pairwise sum (np_rms_f32's steps from numpy_emul.hpp --
// the leaf table, one leaf per thread, the combine in the recursion's order, np_sqrt_f32 -- in the frame's precision
// and one recursion level deeper, which lengths such as 16383 need), and a flag for a non-finite sample. One record of
// kMpWsCols float64 per frame. Two mappings of frames to workgroups, picked by the frame length (kMpWaveMax, DESIGN.md
// has the measurements): 256 threads per frame, or one wave per frame and four frames per workgroup. Both run the same
// leaf and combine code, so a frame's record does not depend on the mapping. Every wave of a workgroup passes every
// barrier: a wave without a frame works on the call's last one and writes nothing.
//
// meterpanel_hist_kernel + meterpanel_track_kernel<false> are the product's cross-frame path (the histogram by per-bin
// prefix counts over workgroups in parallel, the machines by one wave); meterpanel_track_kernel<true> is the measured
// alternative, built with -DOMEGA_MP_TRACK_WALK (DESIGN.md has both times).
//
// meterpanel_track_kernel<true>, behind the frame kernel on the same stream, one wave for the whole call (:353-373, :384-397, :568-579):
// frames are taken 64 at a time -- lane l loads frame f0 + l's meters and record, finds the momentary's bin by a
// binary search over the uploaded edges and computes the punch factor -- and then walked in order: lane b < n_bins
// adds the entering frame's bin and removes the one that leaves the level window (one int per lane, the row of counts
// is stored coalesced), lane 62 stores the hold machine's pair and lane 63 the carried transient values (the machines
// themselves run on every lane: their state is wave-uniform). The bin of a value that leaves the window comes from a
// ring of bin indices in LDS beside the state's ring of values; within a chunk it comes from a lane. The three rings
// are written once, behind the walk, each slot by the lane that read it, so state_out may be state_in.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "params.hpp"

#pragma clang fp contract(off)
#include "numpy_emul.hpp"

namespace omega {

namespace {

constexpr int kT = kMpThreads;
constexpr unsigned char kNoBin = 255;

// np_slice_leaf in either precision
template <class T, class Term>
__device__ __forceinline__ T mp_leaf(int n, Term term) {
  if (n < 8) {
    T r = 0;
    for (int i = 0; i < n; ++i) r += term(i);
    return r;
  }
  T r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = term(j);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += term(i + j);
  }
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += term(i);
  return res;
}

// np_leaf_combine in either precision
template <class T, int D>
__device__ __forceinline__ T mp_combine(int n, const T* ls, int& idx) {
  if constexpr (D == 0) {
    return ls[idx++];
  } else {
    if (n <= 128) return ls[idx++];
    int n2 = n / 2;
    n2 -= n2 % 8;
    const T a = mp_combine<T, D - 1>(n2, ls, idx);
    const T b = mp_combine<T, D - 1>(n - n2, ls, idx);
    return a + b;
  }
}

template <class T>
__device__ __forceinline__ T mp_abs(T v) {
  if constexpr (std::is_same<T, float>::value) {
    return fabsf(v);
  } else {
    return fabs(v);
  }
}

// G threads per frame (64: a wave; 256: the workgroup), kT / G frames per workgroup
template <class T, int G>
__global__ __launch_bounds__(kT) void meterpanel_frame_kernel(MeterPanelParams p) {
  constexpr int FP = kT / G;
  __shared__ unsigned ltab[kMpMaxLeaves];
  __shared__ T lsum[FP][kMpMaxLeaves];
  __shared__ int nl_s;
  __shared__ int red_i[3][4];
  __shared__ T red_m[4];
  const int t = threadIdx.x, u = t % G, g = t / G, lane = t & 63, wv = t >> 6;
  const int64_t f = (int64_t)blockIdx.x * FP + g;
  const bool live = f < p.n_frames;
  const int m = p.frame_len;
  const T* x = p.frames.row_as<T>(live ? f : p.n_frames - 1);
  const T thr = (T)0.1;  // float32(0.1) for a float32 frame

  int cnt = 0, first = m, bad = 0;  // bad: bit 0 a non-finite sample, bit 1 a NaN
  T mx = 0;
  for (int i = u; i < m; i += G) {
    const T v = x[i], a = mp_abs(v);
    if (!(a < (T)INFINITY)) bad |= a != a ? 3 : 1;
    mx = a > mx ? a : mx;
    if (i + 1 < m) {
      const T d = mp_abs(x[i + 1]) - a;
      if (d > thr) {
        ++cnt;
        first = min(first, i);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    first = min(first, __shfl_xor(first, o, 64));
    bad |= __shfl_xor(bad, o, 64);
    const T w = __shfl_xor(mx, o, 64);
    mx = w > mx ? w : mx;
  }
  if constexpr (G == kT) {
    if (lane == 0) {
      red_i[0][wv] = cnt;
      red_i[1][wv] = first;
      red_i[2][wv] = bad;
      red_m[wv] = mx;
    }
    __syncthreads();
    cnt = (red_i[0][0] + red_i[0][1]) + (red_i[0][2] + red_i[0][3]);
    first = min(min(red_i[1][0], red_i[1][1]), min(red_i[1][2], red_i[1][3]));
    bad = red_i[2][0] | red_i[2][1] | red_i[2][2] | red_i[2][3];
    mx = red_m[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) mx = red_m[w] > mx ? red_m[w] : mx;
  }
  if (bad & 2) mx = (T)NAN;  // np.max propagates a NaN

  // numpy's recursion reaches depth 8 below 16384 where the halves are uneven (16383 -> 8199 -> ... -> 263 -> 135 ->
  // 64 + 71), one more than np_rms_f32's tables are built for, so its pieces run here with depth 8
  if (t == 0) {
    int nl = 0;
    np_emit_leaves<8>(0, m, ltab, nl);
    nl_s = nl;
  }
  __syncthreads();
  const int nl = nl_s;
  for (int l = u; l < nl; l += G) {
    const T* a = x + (ltab[l] & 0xFFFFu);
    lsum[g][l] = mp_leaf<T>((int)(ltab[l] >> 16), [&](int i) { return a[i] * a[i]; });
  }
  __syncthreads();
  int idx = 0;
  const T s = mp_combine<T, 8>(m, lsum[g], idx);
  T rms;
  if constexpr (std::is_same<T, float>::value) {
    rms = np_sqrt_f32((float)((double)s / (double)m));  // np.mean: float32(float64(sum) / m)
  } else {
    rms = __dsqrt_rn(s / (double)m);
  }
  if (live && u == 0) {
    double* w = p.ws + f * kMpWsCols;
    w[0] = (double)cnt;
    w[1] = cnt ? (double)first : -1.0;
    w[2] = (double)mx;
    w[3] = (double)rms;
    w[4] = (bad & 1) ? 1.0 : 0.0;
  }
}

// the bin edges[b] <= v < edges[b + 1] (the last bin closed above), kNoBin for everything else, NaN included
__device__ __forceinline__ unsigned char mp_bin(const double* ed, int nb, double v) {
  if (!(v >= ed[0]) || v > ed[nb]) return kNoBin;
  if (v == ed[nb]) return (unsigned char)(nb - 1);
  int lo = 0, hi = nb;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (v >= ed[mid])
      lo = mid;
    else
      hi = mid;
  }
  return (unsigned char)lo;
}

// a fill or a position of the blob: an integer in [0, hi], else 0
__device__ __forceinline__ int64_t mp_index(double v, int hi) { return v >= 0.0 && v <= (double)hi ? (int64_t)v : 0; }

// Slot s of a ring of `len` slots after the call's F pushes of meters column `col`, the first into slot pos0: the
// last pushed frame that fell on it, or what the slot held (0 in a new panel)
__device__ __forceinline__ void mp_ring_out(const MeterPanelParams& p, int off, int len, int64_t pos0, int col) {
  const int64_t F = p.n_frames;
  for (int s = threadIdx.x; s < len; s += 64) {
    double v = p.state_in ? p.state_in[off + s] : 0.0;
    const int64_t r = (s - pos0 + len) % len;
    if (r < F) v = p.meters[(r + (F - 1 - r) / len * len) * 5 + col];
    p.state_out[off + s] = v;
  }
}

}  // namespace

// The histogram as windowed differences of per-bin prefix counts, kMpHistChunk frames per workgroup, one wave per 64 of
// them: the bins of the chunk's frames and of the level_len pushes before them (this call's frames, before those the
// blob's ring, before those nothing: kNoBin) are found in parallel into LDS; lane b counts the window in front of its
// wave's first frame and then adds the entering and subtracts the leaving bin frame by frame. Lane 63 counts every
// valid bin (the histogram's sum), lane 62 stores the fill. Reads state_in only: it runs in front of the track kernel.
__global__ __launch_bounds__(kMpHistChunk) void meterpanel_hist_kernel(MeterPanelParams p) {
  __shared__ unsigned char sb[kMpMaxHist + kMpHistChunk];
  __shared__ double ed[kMpMaxBins + 1];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, nb = p.n_bins, L = p.level_len;
  const int64_t F = p.n_frames, f0 = (int64_t)blockIdx.x * kMpHistChunk;
  const double* si = p.state_in;
  for (int i = t; i <= nb; i += kMpHistChunk) ed[i] = p.edges[i];
  const int64_t fill0 = si ? mp_index(si[kMpLevelFill], L) : 0, pos0 = si ? mp_index(si[kMpLevelPos], L - 1) : 0;
  __syncthreads();
  const int n = (int)min((int64_t)kMpHistChunk, F - f0);
  for (int i = t; i < L + n; i += kMpHistChunk) {
    const int64_t q = f0 - L + i;  // the push's index in this call; below 0: pushed before it
    unsigned char b = kNoBin;
    if (q >= 0)
      b = mp_bin(ed, nb, p.meters[q * 5]);
    else if (-q <= fill0)
      b = mp_bin(ed, nb, si[kMpHead + (int)((pos0 + q + L) % L)]);
    sb[i] = b;
  }
  __syncthreads();
  const int j0 = wv * 64, j1 = min(j0 + 64, n);
  if (j0 >= n) return;
  int cnt = 0;
  for (int i = j0; i < j0 + L; ++i) {
    const int b = sb[i];
    cnt += lane == 63 ? b != kNoBin : b == lane;
  }
  for (int j = j0; j < j1; ++j) {
    const int in = sb[j + L], out = sb[j];
    cnt += lane == 63 ? (in != kNoBin) - (out != kNoBin) : (in == lane) - (out == lane);
    const int64_t f = f0 + j;
    if (p.hist && lane < nb) p.hist[f * nb + lane] = cnt;
    if (lane == 63) p.rows[f * kMpRowCols + 7] = (double)cnt;
    if (lane == 62) p.rows[f * kMpRowCols + 6] = (double)min(fill0 + f + 1, (int64_t)L);
  }
}

// WALK: the one-wave baseline, the histogram walked with the machines. Without it the histogram, the fill and the sum
// are meterpanel_hist_kernel's and the wave runs the machines alone, a chunk's rows staged in LDS and stored together.
template <bool WALK>
__global__ __launch_bounds__(64) void meterpanel_track_kernel(MeterPanelParams p) {
  __shared__ unsigned char rb[WALK ? kMpMaxHist : 1];
  __shared__ double ed[kMpMaxBins + 1];
  __shared__ double s_tp[64], s_att[64], s_punch[64];
  __shared__ int s_cnt[64], s_nf[64];
  __shared__ double s_out[WALK ? 1 : 6][64];
  const int lane = threadIdx.x, nb = p.n_bins, L = p.level_len;
  const int64_t F = p.n_frames;
  const double* si = p.state_in;
  double hold = si ? si[kMpHold] : -100.0;
  int64_t counter = si ? (int64_t)si[kMpCounter] : 0;
  if (p.reset_hold) {
    hold = -100.0;
    counter = 0;
  }
  double attack = si ? si[kMpAttack] : 0.0, punch = si ? si[kMpPunch] : 0.0, count = si ? si[kMpCount] : 0.0;
  // (fills and positions outside their rings, which only a blob from elsewhere holds, read as 0: no index leaves a ring)
  int64_t lfill = si ? mp_index(si[kMpLevelFill], L) : 0, lpos = si ? mp_index(si[kMpLevelPos], L - 1) : 0;
  const int64_t lpos0 = lpos;
  const int64_t pfill = si ? mp_index(si[kMpPeakFill], p.peak_len) : 0, ppos = si ? mp_index(si[kMpPeakPos], p.peak_len - 1) : 0;
  const int64_t rfill = si ? mp_index(si[kMpRangeFill], p.range_len) : 0, rpos = si ? mp_index(si[kMpRangePos], p.range_len - 1) : 0;
  int cnt = 0, tot = 0;
  if constexpr (WALK) {
    for (int i = lane; i <= nb; i += 64) ed[i] = p.edges[i];
    __syncthreads();
    // the bins of the values the level ring holds (slots [0, fill) until the ring is full)
    for (int i = lane; i < L; i += 64) rb[i] = i < lfill ? mp_bin(ed, nb, si[kMpHead + i]) : kNoBin;
    __syncthreads();
    for (int i = 0; i < L; ++i) {
      const int b = rb[i];
      cnt += b == lane;
      tot += b != kNoBin;
    }
  }
  const int off_p = kMpHead + L, off_r = off_p + p.peak_len;
  for (int64_t f0 = 0; f0 < F; f0 += 64) {
    const int64_t fl = f0 + lane;
    const int n = (int)min((int64_t)64, F - f0);
    int mybin = kNoBin;
    if (lane < n) {
      const double* mt = p.meters + fl * 5;
      const double* w = p.ws + fl * kMpWsCols;
      if constexpr (WALK) mybin = mp_bin(ed, nb, mt[0]);
      s_tp[lane] = mt[4];
      s_cnt[lane] = (int)w[0];
      s_att[lane] = __dmul_rn(__ddiv_rn(w[1], p.sample_rate), 1000.0);  // (idx / sample_rate) * 1000
      const double mx = w[2], rms = w[3];
      double pf = 0.0;  // peak / rms in the frame's dtype where rms > 0 (:392-395)
      if (rms > 0.0) pf = p.frames.f64 ? __ddiv_rn(mx, rms) : (double)__fdiv_rn((float)mx, (float)rms);
      s_punch[lane] = pf;
      s_nf[lane] = w[4] != 0.0;
    }
    int oldbin = kNoBin;
    if constexpr (WALK) oldbin = rb[(int)((lpos + lane) % L)];  // what the chunk's j-th push finds in its slot, j < L
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const int64_t f = f0 + j;
      if constexpr (WALK) {
        const int nbin = __shfl(mybin, j, 64);
        const int ob = j >= L ? __shfl(mybin, j - L, 64) : __shfl(oldbin, j, 64);
        const bool evict = lfill == L;
        cnt += (nbin == lane) - (evict && ob == lane);
        tot += (nbin != kNoBin) - (evict && ob != kNoBin);
        lfill = min(lfill + 1, (int64_t)L);
      }
      const double tp = s_tp[j];
      if (tp > hold) {
        hold = tp;
        counter = p.hold_samples;
      } else {
        counter -= 1;
        if (counter <= 0) hold = tp;
      }
      const int c = s_cnt[j];
      if (c > 0) {
        attack = s_att[j];
        punch = s_punch[j];
        count = (double)c;
      }
      const double flags = (double)((c > 0 ? kMpFlagAttack : 0) | (s_nf[j] ? kMpFlagNonFinite : 0));
      if constexpr (WALK) {
        double* row = p.rows + f * kMpRowCols;
        if (lane == 62) {
          row[0] = hold;
          row[1] = (double)counter;
        } else if (lane == 63) {
          row[2] = attack;
          row[3] = punch;
          row[4] = count;
          row[5] = flags;
        } else if (lane == 0) {
          row[6] = (double)lfill;
          row[7] = (double)tot;
        }
        if (p.hist && lane < nb) p.hist[f * nb + lane] = cnt;
      } else if (lane == j) {  // (the state is wave-uniform: lane j keeps frame j's values)
        s_out[0][j] = hold;
        s_out[1][j] = (double)counter;
        s_out[2][j] = attack;
        s_out[3][j] = punch;
        s_out[4][j] = count;
        s_out[5][j] = flags;
      }
    }
    __syncthreads();
    if constexpr (WALK) {
      // the chunk's bins into the ring: of several pushes into one slot (L < n) the last
      if (lane < n && lane >= n - L) rb[(int)((lpos + lane) % L)] = (unsigned char)mybin;
      lpos = (lpos + n) % L;
    } else if (lane < n) {
#pragma unroll
      for (int k = 0; k < 6; ++k) p.rows[fl * kMpRowCols + k] = s_out[k][lane];
    }
    __syncthreads();
  }
  if constexpr (!WALK) {
    lfill = min(lfill + F, (int64_t)L);
    lpos = (lpos0 + F) % L;
  }
  if (p.state_out) {
    mp_ring_out(p, kMpHead, L, lpos0, 0);
    mp_ring_out(p, off_p, p.peak_len, ppos, 4);
    mp_ring_out(p, off_r, p.range_len, rpos, 3);
    if (lane == 0) {
      double* so = p.state_out;
      so[kMpHold] = hold;
      so[kMpCounter] = (double)counter;
      so[kMpAttack] = attack;
      so[kMpPunch] = punch;
      so[kMpCount] = count;
      so[kMpLevelFill] = (double)lfill;
      so[kMpLevelPos] = (double)lpos;
      so[kMpPeakFill] = (double)min(pfill + F, (int64_t)p.peak_len);
      so[kMpPeakPos] = (double)((ppos + F) % p.peak_len);
      so[kMpRangeFill] = (double)min(rfill + F, (int64_t)p.range_len);
      so[kMpRangePos] = (double)((rpos + F) % p.range_len);
      for (int i = kMpRangePos + 1; i < kMpHead; ++i) so[i] = 0.0;
    }
  }
}

hipError_t launch_meterpanel_frames(const MeterPanelParams& p, int wave_max, hipStream_t s) {
  if (p.n_frames <= 0) return hipSuccess;
  const bool wave = p.frame_len <= wave_max;
  const unsigned grid = (unsigned)(wave ? (p.n_frames + 3) / 4 : p.n_frames);
  if (p.frames.f64) {
    if (wave)
      hipLaunchKernelGGL((meterpanel_frame_kernel<double, 64>), dim3(grid), dim3(kT), 0, s, p);
    else
      hipLaunchKernelGGL((meterpanel_frame_kernel<double, kT>), dim3(grid), dim3(kT), 0, s, p);
  } else {
    if (wave)
      hipLaunchKernelGGL((meterpanel_frame_kernel<float, 64>), dim3(grid), dim3(kT), 0, s, p);
    else
      hipLaunchKernelGGL((meterpanel_frame_kernel<float, kT>), dim3(grid), dim3(kT), 0, s, p);
  }
  return hipGetLastError();
}

// (the histogram kernel reads state_in's ring, which the track kernel may overwrite as state_out: it goes first)
hipError_t launch_meterpanel_track(const MeterPanelParams& p, bool walk, hipStream_t s) {
  if (walk) {
    hipLaunchKernelGGL(meterpanel_track_kernel<true>, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
  }
  if (p.n_frames > 0) {
    const unsigned grid = (unsigned)((p.n_frames + kMpHistChunk - 1) / kMpHistChunk);
    hipLaunchKernelGGL(meterpanel_hist_kernel, dim3(grid), dim3(kMpHistChunk), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(meterpanel_track_kernel<false>, dim3(1), dim3(64), 0, s, p);
  return hipGetLastError();
}

}  // namespace omega
