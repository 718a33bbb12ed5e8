// Kernel parameter blocks shared by the host launcher (capi_*.cpp) and the device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frames.hpp"

namespace omega {

constexpr int kMaxRes = 4;
constexpr int kMaxLog2 = 15;  // twiddle tables for sizes 2^1 .. 2^14 (+1 spare)

// True peak in dB of a frame's float32 peak (professional_meters.py:295-299): -100 below 1e-10, else
// 20 log10(peak) rounded once to float32 (20.0f * log10f(peak) rounds twice: up to an ulp of the result
// off for an exact peak). One lane per frame runs it.
__device__ __forceinline__ float tp_db(float peak) {
  return peak < 1e-10f ? -100.0f : (float)(20.0 * log10((double)peak));
}

// One resolution of the multi-resolution FFT (FFTConfig, multi_resolution_fft.py:26-44).
// One combine entry. tm = t | op << 24 with op 0: store, 1: add (a later owner of t), 2: store 0
// (no owner). Entries of a resolution are contiguous; owners of one target run in resolution order.
struct alignas(16) CombEnt {
  int tm, j;
  float c0, c1;
};

struct ResParam {
  int n;                 // real FFT size N_r
  int offset;            // W - N_r: the resolution reads the last N_r samples of the frame
  const float* win;      // [N_r] window (np.blackman(N).astype(f32))
  const float* wgt;      // [N_r/2+1] psychoacoustic weights (ones if apply_weighting is off)
  float* mag_out;        // [n_cf, N_r/2+1] or nullptr
  int ent_begin, ent_end;  // this resolution's combine entries
  float cw;              // combine weight (config.weight)
  int low_band;          // the entries read only bins < 256 (the 16384-point register FFT then forms
                         // just the lowest and highest 256 frequencies: RegFFT::run_low)
  // combine without a magnitude output, when the entries read more bins than half their count: the
  // magnitudes of the pairs (k, K - k), pair_lo <= k < pair_hi, into the spectrum's slots first (one
  // untangle per pair), then the entries from them (two LDS reads each). pair_hi == 0: every entry
  // untangles the two bins it reads itself.
  int pair_lo, pair_hi;
};

struct SpectralParams {
  const float* x;
  int64_t frame_stride, chan_stride;
  int C;
  int64_t n_cf;
  int n_res;
  ResParam res[kMaxRes];
  // combine plan (multi_resolution_fft.py:353-395): entry e writes or adds
  // c0 * mag[j] + c1 * mag[j+1] to target t (c0, c1 fold the interpolation fraction, the
  // psychoacoustic weights of bins j, j+1, the resolution weight and 1 / the target's weight sum)
  const CombEnt* ent;
  int T;
  float* comb_out;    // [n_cf, T] or nullptr
  // true peak (professional_meters.py:283-299)
  float* tp_out;      // [n_cf] or nullptr
  const float2* rot;  // [W/2 + 1] exp(+2 pi i k / (4W))
  // true-peak phases y(n + P/4) computed besides the samples (P = 0): bit P set. 0xE = 4x
  // oversampling (the reference's default), 0x4 = 2x (n + 1/2 only), 0 = 1x (the samples)
  int tp_phases;
  const float2* tw[kMaxLog2];  // tw[l][m] = exp(-2 pi i m / 2^l)
  int rf_sizes;  // host-side launch choice: bit log2(N) set = resolution size N runs on the register-FFT kernel
  // batch_kernel's true-peak role: when set, the value is stored write-through and the workgroup adds 1
  // after it (the true-peak meter query on the side stream waits for the batch's count)
  unsigned* tp_done;
  // batch_kernel's true-peak role with meter pipelining: tp_out is the context's staging slot the
  // deferred meter segment reads, and the caller's buffer (when given) gets this copy
  float* tp_copy;
};

// One zero-phase biquad (filtfilt with scipy's defaults) in state-space form:
// s' = A s + B u, y = s0 + b0 u, A = [[-a1, 1], [-a2, 0]], B = [b1 - a1 b0, b2 - a2 b0].
struct BiquadTab {
  float b0, a1, a2, B0, B1;
  float zi0, zi1;      // scipy.signal.lfilter_zi
  float h0[64], h1[64];  // first row of A^n, n < L (zero-input response of a chunk)
  float pw[64][4];     // P^(l+1), P = A^L, row-major 2x2
  float g0[64], g1[64];  // A^j B, j < L: a sample's share of its (sub-)chunk's zero-state end state
};

// K-weighting LDS table per filter (float4 entries): [0, 64) the scan powers P^(l+1), [64, 96) the
// first row of A^i and A^i B, i < 32, as (h0, h1, g0, g1) -- read where used, not held in registers
constexpr int kPwl = 96;
// K-weighting workgroup: up to 32 samples per thread (M/32 threads, 64..512), the chunk length L of
// the scan tables (make_biquad_tab) follows from it.
constexpr int kw_threads(int M) { return M / 32 < 64 ? 64 : (M / 32 > 512 ? 512 : M / 32); }
constexpr int kw_chunk(int M) { return M / kw_threads(M); }

struct KWeightParams {
  const float* x;
  int64_t frame_stride, chan_stride;
  int C;
  int64_t n_cf;
  const BiquadTab* hp;     // 38 Hz Butterworth high-pass (professional_meters.py:52-54)
  const BiquadTab* shelf;  // 1500 Hz Butterworth high-pass "shelf" (:56-64)
  float* lufs_out;         // [n_cf] or nullptr
  float* weighted_out;     // [n_cf, M] or nullptr
  int mode;                // 0: K-weighting, 3: Z (no filter, no gate: professional_meters.py:228-229)
  // when set: LUFS_inst is stored write-through and each workgroup adds 1 after it (the meter prep
  // kernel on the side stream waits for the batch's count instead of a stream event)
  unsigned* kw_done;
  // batch_kernel with meter pipelining: lufs_out is the context's staging slot the meter prep and the
  // deferred segment read, and the caller's buffer (when given) gets this copy
  float* lufs_copy;
  // (meter pipelining) instead of the count: thread 0 also stores {mirror_gen, LUFS bits} as one 64-bit
  // word into lufs_mirror[cf] -- no drain, no count; the meter prep polls the words for the generation
  unsigned long long* lufs_mirror;
  unsigned mirror_gen;
};

// Meter aggregates (meters.hip): per-channel double-buffered state (in -> out) plus per-batch scratch.
// Meter aggregate capacities: frames per launch (the host splits longer batches), history length
// (>= integrated_len - 1) and the time-ordered sequence history ++ batch.
constexpr int kMeterChunk = 2048;
constexpr int kMeterHistCap = 4096;
constexpr int kMeterSeqCap = kMeterChunk + kMeterHistCap;

// A gated value outside the batch's common window core: value, absolute frame index, and the number
// of core values below it.
struct alignas(16) MeterExt {
  float v;
  uint32_t t;
  int rc;
  int pad;
};

// omega_meter_load_history: the meter state (parity cur) of a stream whose last n_l frames had the
// LUFS_inst values lufs[f * C + c] and whose last n_t of them the true peaks tp[f * C + c] (time order),
// the next frame at absolute index n_l -- what omega_meter_reset + omega_meter_update over those frames
// leave (true peaks of the older frames -100), without computing their aggregates.
struct MeterLoadParams {
  const float* lufs;  // [n_l, C]
  const float* tp;    // [n_t, C]
  int n_l, n_t, C, HL, HT;
  float gate;
  float* hist_l;      // [C, HL]
  float* hist_t;      // [C, HT]
  int* n_l_out;
  int* n_t_out;
  unsigned long long* skeys;  // [C, HL]
  int* n_s_out;
  uint32_t* t0_out;
};

struct MeterPrepParams {
  const float* lufs;    // [n_frames * C] batch instantaneous LUFS
  // when set (meter pipelining): the batch's values come from these {generation, value} words instead of
  // `lufs` after wait_ctr (KWeightParams::lufs_mirror): each is polled until it carries mirror_gen
  const unsigned long long* lufs_mirror;
  unsigned mirror_gen;
  const float* tp;      // [n_frames * C]
  int64_t n_frames;     // <= kMeterChunk per launch
  int C;
  const float* hist_l_in;  // [C, HL] last LUFS_inst values, time order
  const float* hist_t_in;  // [C, HT] last TP values
  const int* n_l_in;
  const int* n_t_in;
  const unsigned long long* skeys_in;  // [C, HL] gated keys of hist_l, sorted
  const int* n_s_in;
  const uint32_t* t0_in;  // absolute index of the batch's first frame
  float* hist_l_out;
  float* hist_t_out;
  int* n_l_out;
  int* n_t_out;
  unsigned long long* skeys_out;
  int* n_s_out;
  uint32_t* t0_out;
  int HL, HT;  // integrated_len - 1, peak_len - 1
  int mom_len, short_len, int_len, peak_len;
  float gate;
  // per-batch scratch written by meter_prep_kernel for meter_query_kernel
  float* core;      // [C, kMeterSeqCap] gated values in every window of the batch, ascending
  MeterExt* ext;    // [C, kMeterSeqCap] the other gated values of the batch's windows, ascending
  int* n_core;      // [C]
  int* n_ext;       // [C]
  int* gcount;      // [C, kMeterSeqCap + 1] gated-count prefix in time order
  double* gsum;     // [C, kMeterSeqCap + 1] gated-sum prefix in time order
  double* out;                     // [n_frames * C, 5]
  int parts;  // meter_query_kernel: bit 0 the LUFS meters (columns 0-3), bit 1 the true-peak meter (4)
  // meter_prep_kernel: when set, wait until (int)(*wait_ctr - wait_target) >= 0 before reading `lufs`
  // (the batch kernel's K-weighting workgroups count themselves in after storing their value)
  unsigned* wait_ctr;
  unsigned wait_target;
  // meter_query_kernel: q_done set -> every workgroup adds 1 after its outputs are out (release);
  // join_ctr set -> workgroup (0, 0) does not finish before (int)(*join_ctr - join_target) >= 0, so the
  // stream it runs on completes only after the side stream's query workgroups (no stream event)
  unsigned* q_done;
  unsigned* join_ctr;
  unsigned join_target;
  // tail layout (omega_ctx::meter_tail): meter_prep_kernel counts itself into q_done when set;
  // meter_query_kernel waits (every workgroup, bounded) until (int)(*start_ctr - start_target) >= 0
  unsigned* start_ctr;
  unsigned start_target;
  // the batch's meter segment (batch_meter_role): when seg_ctr is set every workgroup adds 1 to it
  // once its reads are done. meter_prep_kernel: before writing the per-batch scratch of its parity it
  // waits until (int)(*seg_ctr - seg_pre_target) >= 0 (the last segment that reads that scratch is
  // done), before writing the next state until (int)(*seg_ctr - seg_post_target) >= 0 (the last
  // segment that reads that state) -- with meter pipelining that segment may run in a later launch
  unsigned* seg_ctr;
  unsigned seg_pre_target, seg_post_target;
  // bounded polls: at most poll_limit iterations; on expiry the kernel stores 1 into err_word[0] (prep)
  // or err_word[1] (join) -- host-mapped memory the host checks in omega_synchronize and the next call
  // (OMEGA_EHIP instead of silently stale meters)
  int poll_limit;
  unsigned* err_word;
};

struct BandParams {
  const float* spec;
  int64_t n, spec_stride;
  int n_bins;
  int n_out;
  const int* starts;
  const int* ends;
  const float* scale;      // [n_out] per-band multiplier (MAX) or nullptr
  const float* bin_scale;  // [n_bins] per-bin multiplier (MEAN) or nullptr
  int op;                  // 0 max, 1 mean
  int n_valid;             // bands computed; the rest are 0
  float* out;              // [n, n_out]
};

struct ChromaParams {
  const float* spec;
  int64_t n;
  int n_bins;
  double df;
  const float* mat;     // [12, n_bins] projection (chromagram.py:122-146), zero outside 20..8000 Hz
  double* out;          // [n, 12] normalised smoothed chroma (before the temporal blend)
};

// combine_results_optimized over externally supplied (already weighted) magnitudes; a missing
// resolution (mag[r] == nullptr) is skipped like a key absent from the results dict.
struct CombineParams {
  const float* mag[kMaxRes];
  int nbins[kMaxRes];
  float cw[kMaxRes];
  int64_t n_cf;
  int T;
  const int* own_off;   // [T+1]
  const int* own_rj;    // (r << 24) | j
  const float* own_frac;
  float* out;           // [n_cf, T]
};

// Fused spectrum analysis (cfg3): windowed rfft magnitude (A13) -> log-band max (A10) and raw
// chromagram (A12) of each frame, one pass over the frame.
struct SpectraParams {
  const float* x;
  int64_t n, stride;       // frames of 2K samples at x + f * stride
  const float* win;        // [2K]
  float* mag_out;          // [n, K+1] or nullptr
  // A10 (MAX op): bands [0, n_valid) of n_out, band i = max(mag[starts[i]:ends[i]]) * scale[i]
  int n_out, n_valid;
  const int* starts;
  const int* ends;
  const float* scale;
  float* bands_out;        // [n, n_out] or nullptr
  // A12: bins [c_lo, c_hi): weights of the 5 pitch classes base-2..base+2 (w4 = 5th); the bins
  // grouped by base class: cperm[cgoff[b] .. cgoff[b+1]) = bin - c_lo of the bins with base class b
  int c_lo, c_hi;
  const float4* cw4;
  const float* cw1;
  const unsigned short* cperm;
  const int* cgoff;        // [13]
  // the same bins in group order as 12-byte records {a, g, bin} for the register-FFT kernel (record j
  // read directly: no dependent permutation load): with u = c - b the fraction of the bin's pitch class
  // and s its octave-band scale, a = s exp(-2 u^2) and g = exp(4 u), so the five weights
  // s exp(-2 (u - o)^2), o = -2..2, are a g^o e^{-2 o^2} (rtol 1e-5 of the chromagram: ~3e-7 here)
  const float* crec;       // [3 * cgoff[12]]
  double* chroma_out;      // [n, 12] or nullptr (smoothed, normalised; before the temporal blend)
  const float2* tw[kMaxLog2];
};

// Drum-detection spectral features (drum.hip): 7 flux bands (kick sub / body /
// click, snare fundamental / body / snap / rattle), the snare centroid range, and one stream's state
// (previous magnitude frame, 21-deep flux histories, frames seen), double-buffered (in -> out).
constexpr int kDrumBands = 7;
constexpr int kDrumHist = 21;
constexpr int kDrumCols = 14;

// App spectrum post-processing (post.hip): per-bin tables from the host.
constexpr int kPostMaxBins = 2048;
constexpr int kEmaSpareRows = 32;  // band_raw rows past the last frame (post_ema_kernel's unguarded block loads)
constexpr int kPostMaxBands = 1024;
// band EMA factor f (omega4_main.py:1044-1054: prev * f + v * (1 - f) with a Python float f): the
// float64 forms (f, 1 - f) and the float32 forms numpy's weak-scalar promotion uses on float32 scalars
struct EmaCoef {
  double f, g;    // f, 1 - f
  float f32, g32; // float32(f), float32(1 - f)
};
struct PostParams {
  const float* in;  // [n, stride] combined spectra
  int64_t n, stride;
  int T;
  const double* curve;         // [T] equal-loudness curve by position
  const unsigned char* bass;   // [T] combine frequency < 250 Hz
  const float* comp[2];        // [T] frequency compensation: [0] instrumental / bass-heavy, [1] vocal
  const float* vsup;           // [T] vocal-suppression factor (1 outside 800-4000 Hz)
  int be, vs, ve, hs;          // content ranges [0, be), [vs, ve), [hs, T)
  const unsigned* leaf_tab;    // [4][32] numpy pairwise-sum leaves of the four ranges (capi post configure)
  int p_lo, p_hi;              // 98th percentile: sorted ranks and float32 gamma
  float p_g;
  const int* bs;               // [nb] band starts / ends
  const int* bend;
  const EmaCoef* sf;           // [nb] EMA factor f in the forms the reference's numpy arithmetic uses
  int nb;
  int flags;                   // OMEGA_POST_* bits
  float bass_boost;
  float* spec_out;             // [n, T]
  double* band_out;            // [n, nb] (float32 values, or float64 on frames whose list held the int 1)
  float* band_raw;             // [n, nb] scratch: the clamped band values before the EMA
  int* frame64;                // [n] scratch: 1 where a band clamped to the Python int 1 (float64 array)
  double* ema_pre;             // [n / 64 chunks, nb] scratch: each EMA chunk's warm-up value at the frame
                               // before it (post.hip post_ema_kernel)
  double* ema_end;             // [n / 64 chunks, nb] scratch: each chunk's value at its last frame
  int* content_out;            // [n]
  // EMA state {value, float64 dtype, present} in (double-buffered: the kernels read one, write the
  // other)
  double* prev;                // [nb]
  int* has_prev;               // [2]: present, float64 dtype
  double* prev_out;            // [nb] EMA state out
  int* has_prev_out;
};

struct DrumParams {
  const float* mag;
  int64_t n, stride;
  int n_bins;
  int bs[kDrumBands], be[kDrumBands];  // band bins [bs, be)
  int cs, ce;                          // centroid bins
  double fstep;                        // rfftfreq(2 n_bins - 1) spacing: fs / (2 n_bins - 1)
  float mult[kDrumBands];              // float32(sensitivity * multiplier); 0: no threshold
  const float* prev_in;
  float* prev_out;                     // [n_bins]
  const float* hist_in;
  float* hist_out;                     // [kDrumBands][kDrumHist], oldest first
  const int* len_in;
  int* len_out;                        // [kDrumBands]
  const long long* pos_in;
  long long* pos_out;                  // frames of the stream seen before / after this call
  float* flux;                         // [n, kDrumBands] scratch
  double* out;                         // [n, kDrumCols] (oracle DRUM_COLUMNS order)
};

struct RfftParams {
  const float* x;
  int64_t n;
  const float* win;
  float* mag;    // [n, m/2+1] or nullptr
  float* cplx;   // [n, m/2+1, 2] or nullptr
  const float2* tw[kMaxLog2];
};

// VU meter ballistics (vu.hip; vu_meters.py:55-99) over n consecutive update calls of chunk samples
// per channel: update u is row u of x, channel c at c * channel_stride in it
struct VuParams {
  Rows x;
  int64_t n;
  int chunk;
  int64_t channel_stride;
  int C;
  const double* dt;        // [n] seconds since the previous update
  const double* hist_in;   // [C, Wv] the last hist_n samples before this batch, oldest first
  double* hist_out;        // [C, Wv]
  int64_t hist_n;
  int64_t Wv;              // int(0.3 fs): the deque length
  double* ms;              // [n, C] scratch: window mean squares
  const double* st_in;     // [C, 3] display, peak, peak_time
  double* st_out;
  double* out;             // [n, C, 3] vu_db (+18 offset applied), display, peak_db
};

// TransientAnalyzer.analyze_transients (transient.hip; transient.py:19-108), one frame per workgroup
constexpr int kTransientCols = 6;  // detected, attack_time_ms, punch, envelope_peak, envelope_rms, envelope_mean
constexpr int kTrMaxStages = 32;
struct TransientParams {
  Rows x;                   // the frames, n samples each
  int64_t n_frames;
  int n;                    // frame length (>= 64; powers of two up to 8192 on the packed transform)
  const double2* tw;        // [n/4] e^{-2 pi i m / (n/2)}
  const double2* tw2;       // [n/2 + 1] e^{-2 pi i q / n}
  const double* sg;         // [21, 21] Savitzky-Golay (21, 3) weights by output position in the window
  double fs;
  double* out;              // [n_frames, kTransientCols]
  // other lengths: a complex n-point mixed-radix transform (radices as anyfft.hip) with the float64
  // table e^{-2 pi i m / n}, buffers in LDS (2 n double2) or, when scratch is set, global memory
  int n_stages;
  int radix[kTrMaxStages];
  const double2* twn;       // [n] or nullptr (power-of-two path)
  double2* scratch;         // [n_frames, 2 n] or nullptr
};

// omega_weighting (weight64.hip): scipy's float64 filtfilt cascades of professional_meters.py:129-218
// for frames of any length > 9. One section: DF2T biquad (first-order sections have b2 = a2 = 0), its
// lfilter_zi and filtfilt's padlen E.
struct W64Stage {
  double b0, b1, b2, a1, a2, zi0, zi1;
  int E;
  int pad_;
};
// weighting modes (omega.h omega_weighting_mode)
enum WeightMode : int { kWeightK = 0, kWeightA = 1, kWeightC = 2, kWeightZ = 3 };
struct Weight64Params {
  const float* x;           // [n, M]
  int M;
  int mode;                 // OMEGA_WEIGHT_K / A / C / Z
  int64_t n;
  W64Stage* st;             // the mode's sections in order
  int n_st;
  double* scratch;          // [n, scratch_stride]: signal (M) + odd extension (M + 2E)
  int64_t scratch_stride;
  float* weighted_out;      // [n, M] or nullptr
  float* lufs_out;          // [n] or nullptr
};

// CepstralAnalyzer.detect_pitch_advanced (pitch.hip; omega4/panels/pitch_detection.py:21-611): three
// workgroup roles per frame (cepstrum, autocorrelation, YIN) and a per-frame combine
constexpr int kPitchCols = 10;  // pitch, confidence, cepstral / autocorrelation / YIN (pitch, confidence), rms, flags
constexpr int kPitchThreads = 256;
struct PitchParams {
  Rows x;                   // the frames, n samples each
  int64_t n_frames;
  int n;                    // 2048, 4096 or 8192
  double fs, min_pitch, max_pitch;
  int min_period, max_period;
  double yin_threshold;
  int yin_window;           // <= n
  int preprocess, compress;
  double comp_threshold, comp_ratio;
  W64Stage hp[2];           // the order-4 high-pass as two DF2T sections (b0, b1, b2, a1, a2)
  const double2* tw;        // [n + 1] e^{-2 pi i q / (2 n)}
  const double* win;        // [n] np.hanning(n)
  double* out;              // [n_frames, kPitchCols]
};

// HarmonicAnalyzer.detect_harmonic_series (harmonic.hip; omega4/panels/harmonic_analysis.py:193-333 and
// omega4/analyzers/harmonic_metrics.py): two workgroup roles per frame (spectrum side, LPC formants) and
// a per-frame combine
constexpr int kHarmonicCols = 16;     // series count, dominant fundamental, thd, thd+n, centroid, spread, flux,
                                      // rolloff, inharmonicity, hnr, formant count, F1..F4, flags
constexpr int kHarmonicThreads = 256;
constexpr int kHarmonicMaxHarm = 16;  // harmonics per series; a series row is the peak bin and these
constexpr int kHarmonicMinBins = 16, kHarmonicMaxBins = 8193;
constexpr int kHarmonicMinAudio = 15, kHarmonicMaxAudio = 8192;
constexpr int kHarmonicLpcOrder = 14;
struct HarmonicParams {
  Rows32 spec;              // n_bins float32 magnitudes per frame
  int n_bins;
  const double* freqs;      // [n_bins] strictly increasing
  Rows audio;               // m samples per frame; a null base: none
  int m;                    // audio samples per frame
  const double* ham;        // [m] np.hamming(m)
  int64_t n_frames;
  double fs, nyquist;
  int max_series;
  int ungated;              // omega_harmonic_metrics: metrics for f0 and formants whether or not a series is found
  double f0;                // the caller's fundamental when ungated (<= 0: the f0 metrics are 0)
  const float* prev_in;     // the spectrum frame 0 compares with, or nullptr (flux 0)
  float* prev_out;          // [n_bins] the last frame's spectrum, or nullptr (not this launch's last)
  double* out;              // [n_frames, kHarmonicCols]
  int* series_bins;         // [n_frames, max_series, 1 + kHarmonicMaxHarm] or nullptr
  double* series_strength;  // [n_frames, max_series] or nullptr
};

// GenreClassifier.extract_features (genre.hip; omega4/panels/genre_classification.py:175-422, :600-783):
// two workgroup roles per frame (spectrum side, audio side) and a per-frame combine
constexpr int kGenreCols = 17;  // centroid, rolloff, rolloff index, zero crossings, bandwidth, dynamic range, loud,
                                // quiet, rms, spectral complexity, bass emphasis, vocal presence, high-frequency
                                // energy, flux, distortion count, mid-frequency dominance, flags
constexpr int kGenreThreads = 256;
constexpr int kGenrePeaks = 5;   // compute_harmonic_distortion weighs the five largest peaks
// the contiguous bin ranges of the reference's masks over the increasing table: bass [20, 250], its mid
// (250, 2000], vocal [200, 4000], core vocal [300, 3000], high [4000, 10000], <= 10000, low [20, 500),
// mid [500, 2000], upper (2000, 8000], and the flatness range [100, 4000]
constexpr int kGenreBands = 10;
struct GenreParams {
  Rows32 spec;              // n_bins float32 values per frame (|.| is taken)
  int n_bins;
  const double* freqs;      // [n_bins] strictly increasing
  Rows audio;               // m samples per frame
  int m;                    // audio samples per frame
  int64_t n_frames;
  int band_lo[kGenreBands], band_n[kGenreBands];  // first bin and bin count of each range (0: no bins)
  int rank95, rank20;       // floor(q (m - 1)) for np.percentile's q = 0.95 and 0.20, in the audio's precision
  double gamma95, gamma20;  // q (m - 1) - rank
  const float* prev_in;     // the magnitude frame 0's flux compares with, or nullptr (flux 0)
  float* prev_out;          // [n_bins] the last frame's magnitude, or nullptr (not this launch's last)
  double* out;              // [n_frames, kGenreCols]
  int* peak_bins;           // [n_frames, kGenrePeaks] the largest peaks' bins, -1 past their number
};

// HipHopDetector.analyze (hiphop.hip; omega4/panels/hip_hop_detector.py:94-384): two workgroup roles per
// frame (spectrum side, audio side) and a per-frame combine
constexpr int kHipHopCols = 24;   // see include/omega.h for the columns
constexpr int kHipHopThreads = 256;
constexpr int kHipHopPeaks = 16;  // kept envelope peaks: floor((8192 - 3) / int(0.1 * 8000)) + 1 = 11 at the most
constexpr int kHipHopMinRate = 8000;
constexpr int kHipHopMinAudio = 64, kHipHopMaxAudio = 8192;
// the contiguous bin ranges of the reference's masks over the increasing table: sub-bass [20, 60], bass
// [60, 250], below Nyquist, low [20, 500], mid [500, 2000], high [2000, 8000], vocal [200, 3000], core
// vocal [300, 2000], and every bin
constexpr int kHipHopBands = 9;
struct HipHopParams {
  Rows32 spec;              // n_bins float32 values per frame (|.| is taken)
  int n_bins;
  Rows audio;               // m samples per frame
  int m;
  int64_t n_frames;
  int band_lo[kHipHopBands], band_n[kHipHopBands];  // first bin and bin count of each range (0: no bins)
  W64Stage sos[3][4];       // sub-bass, kick, hi-hat: four DF2T sections each (b0, b1, b2, a1, a2)
  int distance;             // int(0.1 * sample_rate): find_peaks' distance on the kick envelope
  const double2* tw;        // [m / 2 + 1] e^{-2 pi i q / m}
  double* out;              // [n_frames, kHipHopCols]
  int* kick_peaks;          // [n_frames, kHipHopPeaks] or nullptr
};

// PhaseCorrelationPanel's analysis (phase.hip; omega4/panels/phase_correlation.py:124-220) on real stereo
// frames: one workgroup per frame
constexpr int kPhaseCols = 17;    // see include/omega.h for the columns
constexpr int kPhaseBands = 10;
constexpr int kPhasePoints = 128;  // ceil(m / max(1, m / 100)) is 128 at m = 128 and 256, less elsewhere
constexpr int kPhaseThreads = 256;
constexpr int kPhaseMinFrame = 64, kPhaseMaxFrame = 8192;
struct PhaseParams {
  Rows left, right;         // m samples per frame each, of one stride and one precision
  int64_t n_frames;
  int m, bits;              // m = 1 << bits
  int first[kPhaseBands], last[kPhaseBands];  // the masks' bin ranges [first, last) (equal: no bins)
  const double* hann;       // [m] np.hanning(m)
  const double2* tw;        // [m / 2] e^{-2 pi i q / m}
  double* out;              // [n_frames, kPhaseCols]
  double* points;           // [n_frames, kPhasePoints, 2] or nullptr
};

// RoomModeAnalyzer (room.hip; omega4/analyzers/room_modes.py:71-239 and :356-458): the room modes of a
// batch of spectra, one workgroup per frame, and the Schroeder decay fit of a batch of sample histories, one
// workgroup per stream
constexpr int kRoomMaxModes = 64;
constexpr int kRoomCols = 8;                   // see include/omega.h for the columns
constexpr int kRoomRows = kRoomMaxModes + 1;   // the header row, then the modes
constexpr int kRoomMaxBins = 4096;             // in-range bins held in LDS
constexpr int kRoomThreads = 256;
constexpr int kRt60Threads = 1024, kRt60Cols = 8;
constexpr int kRt60MaxLen = 1 << 20;
struct RoomModesParams {
  Rows spec;                // n_bins values per frame
  int64_t n_frames;
  int n_bins;
  int first, last;          // the in-range bins [first, last) of the caller's table
  int freqs_bad;            // the table holds a non-finite entry: every frame gets flag bit 0
  const double* freqs;      // [n_bins] the caller's table
  double height_mult, prom_std, min_q, max_q, min_sev;
  double hints[6];          // axial fundamentals (length, width, height), tangential frequencies; [0] == 0: none
  double* out;              // [n_frames, kRoomRows, kRoomCols]
};
struct RoomRt60Params {
  Rows audio;               // one row of L samples per stream
  int64_t n_streams;
  int L, W;                 // W > 0: frames of W samples (W divides L), their sums of squares to `energies`
  double fs;
  double* out;              // [n_streams, kRt60Cols]
  double* energies;         // [n_streams, L / W] or nullptr
};

// VoiceDetectionPanel's per-frame analysis (voice.hip; omega4/panels/voice_detection.py:57-122 and :169-192):
// two workgroups per frame in one launch, the spectrum side (blockIdx < n_frames) and, where a pitch can be
// taken at all, the audio side
constexpr int kVoiceCols = 17;       // see include/omega.h for the columns
constexpr int kVoiceThreads = 256;
constexpr int kVoiceMaxBins = 8193;
constexpr int kVoiceMinFrame = 64, kVoiceMaxFrame = 8192;
constexpr int kVoicePitchFrame = 2048;  // :174 shorter frames give no pitch
constexpr double kVoiceMinRate = 8000.0;
constexpr int kVoiceLagBlock = 4;    // lags per thread of the autocorrelation
constexpr int kVoicePad = 8;         // zeros behind the staged audio frame (the lag block's overrun)
struct VoiceParams {
  Rows32 spec;              // n_bins float32 values per frame
  Rows audio;               // m samples per frame
  int64_t n_frames;
  int n_bins, m;
  int n_freq;               // m / 2 + 1: len(np.fft.rfftfreq(m, 1 / fs))
  double bin_hz;            // rfftfreq's factor 1.0 / (m * (1 / fs)): freq_bins[k] = k * bin_hz
  int voice_start, voice_end;  // searchsorted(freq_bins, 85), searchsorted(freq_bins, 255)
  int sg_w;                 // savgol window min(11, n_bins / 4 * 2 + 1); 0: n_bins <= 10, no smoothing
  const double* sg;         // [sg_w, sg_w] Savitzky-Golay (sg_w, 3) weights by output position in the window
  int pitch;                // m >= 2048 and int(fs / 80) < m: the audio side runs
  int lag_lo, lag_hi;       // int(fs / 400), int(fs / 80)
  double* out;              // [n_frames, kVoiceCols]
};

// TransientDetectionPanel's per-frame analysis (tdetect.hip; omega4/panels/transient_detection.py:79-365): one
// launch of n_roles workgroups per frame (the role by blockIdx), then a small launch that forms the two
// quantities that compare a frame with the ones before it (spectral flux, phase-deviation novelty)
constexpr int kTdCols = 21;          // see include/omega.h for the columns
constexpr int kTdThreads = 256;
constexpr int kTdMinFrame = 256, kTdMaxFrame = 8192;
constexpr int kTdMaxBins = 8193;
constexpr double kTdMinRate = 8000.0;
constexpr int kTdFluxLen = 512, kTdFluxBins = 128;     // :152, :166
constexpr int kTdNovLen = 1024, kTdNovBins = 513;      // :324-332
constexpr int kTdPad = 15;           // filtfilt's padlen 3 * max(len(a), len(b))
// the carried state: has_spectrum, has_phase, two reserved words, the last flux spectrum, the last two phase rows
constexpr int kTdStateLen = 4 + kTdFluxBins + 2 * kTdNovBins;
// a frame's workspace row: non-finite flag, the flux spectrum's sum, the flux spectrum, the phases, the magnitudes
constexpr int kTdWsStride = 2 + kTdFluxBins + 2 * kTdNovBins;
enum TdRole : int { kTdEnvelope = 0, kTdFlux = 1, kTdNovelty = 2, kTdHf = 3, kTdScalar = 4, kTdRoles = 5 };
// the order-4 lfilter carry scan (host-designed): P = A^L for the chunk length L, row-major 4 x 4
struct TdScan {
  double Pd[6][16];         // P^(2^k)
  double P64[16];
  double Pl[64][16];        // P^(lane + 1)
};
struct TdetectParams {
  Rows32 spec;              // n_bins float32 values per frame
  Rows audio;               // m samples per frame
  int64_t n_frames;
  int n_bins, m;
  int n_roles;
  int roles[kTdRoles];      // the roles launched, in grid order (workgroup b: roles[b / n_frames], frame b % n_frames)
  int hf, nov;              // the shape has an HF column (m > 256, 5000 Hz below Nyquist) / a novelty (m >= 1024)
  double bin_hz;            // rfftfreq's factor 1.0 / (2 (n_bins - 1) * (1 / fs)): freqs[k] = k * bin_hz
  int band_idx[5];          // searchsorted(freqs, [0, 100, 250, 2000, fs / 2])
  const double* sg;         // [11, 11] Savitzky-Golay (11, 3) weights by output position in the window
  const double2 *tw_m, *tw2_m;      // the m-point real transform's tables (hilbert64.hpp)
  const double2 *tw_f, *tw2_f;      // the 512-point one's
  const double2 *tw_n, *tw2_n;      // the 1024-point one's
  const double *han_f, *han_n;      // np.hanning(512), np.hanning(1024)
  double b[5], a[5], zi[4]; // butter(4, 5000 / (fs / 2), 'high') in ba form and its lfilter_zi
  const TdScan* scan;
  double* ws;               // [n_frames, kTdWsStride]
  const double* state_in;   // [kTdStateLen] or nullptr (a stream's first call)
  double* state_out;        // [kTdStateLen] or nullptr
  double* out;              // [n_frames, kTdCols]
};

// BassZoomPanel's per-frame analysis (basszoom.hip; omega4/panels/bass_zoom.py:51-97, :141-232): one workgroup per
// frame for the windowed 8192-point spectrum's 20..200 Hz bins and the scaled bars, then one workgroup that runs the
// float32 bar recurrence and the peak hold over the call's frames in order
constexpr int kBzFft = 8192;         // :143
constexpr int kBzThreads = 256;
constexpr int kBzMaxBars = 64, kBzMaxBins = 256;  // include/omega.h states both caps
constexpr int kBzRowHead = 3;        // flags, bass_max, scale_factor, then n_bars compressed values
constexpr int kBzStateLen = 3 * kBzMaxBars;       // bars, peaks, peak timestamps (each kBzMaxBars float64)
struct BassZoomParams {
  Rows frames;              // nw samples read per frame
  int64_t n_frames;
  int nw;                   // samples read per frame: min(frame_len, kBzFft)
  int first_bin, n_valid, bins_per_bar, n_bars;
  double comp[kBzMaxBars];  // 0.3 / 0.6 / 1.0 / 0.8 by the bar's centre frequency
  const double* win;        // np.hanning(nw)
  const double2* tw;        // [kBzFft] e^{-2 pi i j / kBzFft}
  const double* times;      // [n_frames] each frame's time (the reference's time.time())
  const double* state_in;   // [kBzStateLen] or nullptr (a new panel)
  double* state_out;        // [kBzStateLen] or nullptr
  double* rows;             // [n_frames, kBzRowHead + n_bars]
  double *bars, *peaks, *peak_times;  // [n_frames, n_bars] each
};

// BeatDetector's and FrequencyBandTracker's per-frame sums (rhythm.hip; omega4/panels/beat_detection.py:64-152,
// :338-349 and frequency_band_tracker.py:71-156): one launch for every frame's flags and sum x^2, then one
// workgroup per frame for the sums over its spectrum and its predecessor's
constexpr int kRhCols = 14;          // see include/omega.h for the columns
constexpr int kRhThreads = 256;
constexpr int kRhEdges = 10;         // 20, 50, 60, 120, 250, 500, 2000, 4000, 8000, 20000 Hz
constexpr int kRhBands = 7;
constexpr int kRhMinBins = 2, kRhMaxBins = 8193;
constexpr int kRhMaxFrame = 16384;
constexpr int kRhSums = 3 + kRhBands + 1;  // spec_sum, flux, kick, the bands, spec_fsum
constexpr double kRhGate = 0.001;    // beat_detection.py:339
enum RhFlag : int { kRhNonFinite = 1, kRhGated = 2, kRhNoFlux = 4 };
// the carried state: valid, n_bins, the last live frame's spectrum (float32 values held as float64)
constexpr int kRhStateHead = 2;
constexpr int64_t rh_state_len(int n_bins) { return kRhStateHead + (int64_t)n_bins; }
struct RhythmParams {
  Rows32 spec;              // n_bins float32 values per frame
  Rows audio;               // m samples per frame; a null base: no audio, no gate, sum x^2 is 0
  int64_t n_frames;
  int n_bins, m;
  const double* freqs;      // [n_bins] the caller's frequency table
  int edge[kRhEdges];       // the bin of each edge frequency; a band's upper edge 0 reads as n_bins
  int* ws;                  // [n_frames] each frame's flag bits 0 and 1 (the first launch's; the second's input)
  const double* state_in;   // [rh_state_len(n_bins)] or nullptr (a stream's first call)
  double* state_out;        // [rh_state_len(n_bins)] or nullptr
  double* out;              // [n_frames, kRhCols]
};

// SpectrogramWaterfall's per-frame update and colour map (waterfall.hip; omega4/panels/spectrogram_waterfall.py
// :71-121, :142-205, :295-305): one launch for every frame's flags, argmax, dB maximum and minimum, then one
// workgroup per frame for the sliding percentiles, the normalised row and its colours
constexpr int kWfThreads = 256;
constexpr int kWfMaxBins = 8193;     // include/omega.h states the cap
constexpr int kWfCols = 7;           // flags, dB max, dB min, peak, floor, argmax index, argmax value
constexpr int kWfHist = 20;          // the (max, min) pairs the percentiles see (:95-96)
enum WfFlag : int { kWfNonFinite = 1 };
// the carried state: valid, dtype tag (1: float64), count, kWfHist maxima and kWfHist minima oldest first (float32
// values widened exactly), the current peak and floor
constexpr int kWfStateMax = 3, kWfStateMin = kWfStateMax + kWfHist, kWfStatePeak = kWfStateMin + kWfHist;
constexpr int kWfStateLen = kWfStatePeak + 2;
struct WaterfallParams {
  Rows spec;                // n_bins values per frame
  int64_t n_frames;
  int n_bins, first_bin, n_cells;
  int auto_gain;            // 0: the carried peak and floor stay in force (:93)
  double gain_db;           // gain_adjustment (:111), rounded to the input's type
  int scheme;               // 0 spectrum, 1 hot, 2 cool, 3 viridis, any other grey (:147-203)
  const double* state_in;   // [kWfStateLen] or nullptr (a new panel: peak 0, floor -80)
  double* state_out;        // [kWfStateLen] or nullptr
  double* stats;            // [n_frames, kWfCols]
  void* rows;               // [n_frames, n_cells] in the input's type
  unsigned char* rgb;       // [n_frames, n_cells, 3] or nullptr
};
// the stand-alone colour map: intensities [n_rows, n_cells] -> rgb [n_rows, n_cells, 3]
struct WaterfallColorParams {
  Rows in;
  int64_t n_rows;
  int n_cells, scheme;
  unsigned char* rgb;
};

// ChromagramAnalyzer's key, chord and alternative-key scores and MusicTheory.analyze_mode for every root
// (tonal.hip; omega4/panels/chromagram.py:215-339, :396-418, :670-812 and music_theory.py:175-200): G lanes per
// frame, kTnThreads / G frames per workgroup
constexpr int kTnThreads = 256;
#ifndef OMEGA_TONAL_LANES           // (64, one wave per frame, builds the measured alternative)
#define OMEGA_TONAL_LANES 16
#endif
constexpr int kTnLanes = OMEGA_TONAL_LANES;  // lanes per frame: 16 (sixteen frames per workgroup) or 64
constexpr int kTnCols = 52;          // see include/omega.h for the columns
constexpr int kTnKeys = 24, kTnTypes = 13, kTnCells = 12 * kTnTypes, kTnModes = 7;
constexpr int kTnStateLen = 13;      // has-previous flag, the previous frame's rolled row
enum TnFlag : int { kTnNonFinite = 1, kTnZeroSum = 2, kTnFlat = 4 };
enum TnGenre : int { kTnPop = 0, kTnJazz, kTnClassical, kTnMetal, kTnRock, kTnOther, kTnGenres };
// the per-genre table (design.hpp tonal_table): the 24 weighted normalised profiles (index 2 root + minor), the
// key factors, Mw + mw, the 24 plain rotated profiles
constexpr int kTnTabKey = 0, kTnTabFac = kTnTabKey + kTnKeys * 12, kTnTabW = kTnTabFac + kTnKeys,
              kTnTabAlt = kTnTabW + 12, kTnTabLen = kTnTabAlt + kTnKeys * 12;
// chord_types in dict order (chromagram.py:79-93; tonal.hip has the intervals): the per-genre tested sets as bit masks
constexpr int kTnPower = 10;
constexpr unsigned kTnTypesAll = 0x1FFF;
constexpr unsigned kTnTypesMetal = 1u << 0 | 1u << 1 | 1u << 6 | 1u << 10 | 1u << 11 | 1u << 12;  // :680-681
constexpr unsigned kTnTypesBasic = 0x3F;                                                          // :684-685
struct TonalParams {
  const double* raw;        // [n_frames, 12] chroma_kernel's rows
  int64_t n_frames;
  const int* roll;          // [n_frames] -11..11 or nullptr (0)
  const int* first;         // [n_frames] or nullptr (0): the frame has no predecessor
  int genre;                // TnGenre
  double blend;             // 0.7 / 0.5 / 0.3
  double tolerance;         // chromatic_tolerance
  const double* tab;        // [kTnTabLen] the genre's table
  const double* state_in;   // [kTnStateLen] or nullptr
  double* state_out;        // [kTnStateLen] or nullptr
  double* rows;             // [n_frames, kTnCols]
  double* key_corr;         // [n_frames, 24] or nullptr
  double* alt_corr;         // [n_frames, 24] or nullptr
  double* chord;            // [n_frames, 2, 12, 13] or nullptr
  double* mode;             // [n_frames, 12, 7] or nullptr
};

// ProfessionalMetersPanel.update's own work (meterpanel.hip; omega4/panels/professional_meters.py:348-397, :568-579):
// per frame the attack scan and the crest-factor operands in the frame's dtype, then one wave that carries the peak
// hold, the transient values, the three histories and the level histogram over the call's frames in order
constexpr int kMpThreads = 256;
constexpr int kMpMaxFrame = 16384;   // np_rms_f32's range
constexpr int kMpMaxLeaves = 256;    // numpy's pairwise leaves hold 64..128 elements above 128
constexpr int kMpMaxHist = 4096;     // the cap of each history length
constexpr int kMpMaxBins = 62;       // lanes 62 and 63 run the hold machine and the transient carry
constexpr int kMpRowCols = 8;        // see include/omega.h for the columns
constexpr int kMpWsCols = 5;         // per-frame record: attack count, first attack, max |x|, rms, non-finite flag
// the state blob: kMpHead values, then the level, true-peak and range rings
enum MpState : int { kMpHold = 0, kMpCounter, kMpAttack, kMpPunch, kMpCount, kMpLevelFill, kMpLevelPos, kMpPeakFill,
                     kMpPeakPos, kMpRangeFill, kMpRangePos, kMpHead = 16 };
enum MpFlag : int { kMpFlagAttack = 1, kMpFlagNonFinite = 2 };
#ifndef OMEGA_MP_WAVE_MAX            // frames up to this length take one wave each, four to a workgroup
#define OMEGA_MP_WAVE_MAX 2048
#endif
constexpr int kMpWaveMax = OMEGA_MP_WAVE_MAX;
constexpr int kMpHistChunk = 256;    // frames per workgroup of the prefix-count histogram kernel
#ifdef OMEGA_MP_TRACK_WALK           // builds the measured alternative: the histogram walked by the track kernel's wave
constexpr bool kMpTrackWalk = true;
#else
constexpr bool kMpTrackWalk = false;
#endif
struct MeterPanelParams {
  Rows frames;              // frame_len samples per frame
  int64_t n_frames;
  int frame_len;
  double sample_rate;
  int level_len, peak_len, range_len, n_bins;
  const double* edges;      // [n_bins + 1] np.linspace(hist_lo, hist_hi, n_bins + 1)
  const double* meters;     // [n_frames, 5] momentary, short_term, integrated, range, true_peak
  int64_t hold_samples;     // peak_hold_samples
  int reset_hold;           // reset_peak_hold before the first frame
  double* ws;               // [n_frames, kMpWsCols] the frame kernel's records
  const double* state_in;   // [kMpHead + level_len + peak_len + range_len] or nullptr (a new panel)
  double* state_out;        // the same, or nullptr
  double* rows;             // [n_frames, kMpRowCols]
  int32_t* hist;            // [n_frames, n_bins] or nullptr
};

// Frames of any length (anyfft.hip): mixed-radix Stockham transform, true peak and windowed rfft
constexpr int kAnyMaxStages = 32;
constexpr int kAnyLdsMax = 6826;  // 3 N float2 in 160 KiB of LDS; above: global scratch
constexpr int kAnyF32Radix = 7;   // radices above it (the remaining primes) accumulate in float64
struct AnyFftParams {
  const float* x;           // frame f at x + f * frame_stride
  int64_t frame_stride;
  int64_t n;
  int N;
  int n_stages;
  int radix[kAnyMaxStages];
  const float2* tw;         // [N] e^{-2 pi i m / N}
  const double2* tw64;      // [N] the same table unrounded, for the radices above kAnyF32Radix (nullptr: none)
  const float2* rot;        // [3 (N / 2) + 1] e^{2 pi i m / (4N)} (true peak)
  float nyq_cos[4];         // cos(pi p / 4)
  int phases;               // true peak: bit p set for each phase p in 1..3
  float* tp_out;            // [n] dBTP
  const float* win;         // rfft: window [N] or nullptr
  float* mag;               // rfft: [n, N/2 + 1] or nullptr
  float* cplx;              // rfft: [n, N/2 + 1, 2] or nullptr
  float2* scratch;          // [n, 3N] when N > kAnyLdsMax, else nullptr (LDS)
};

}  // namespace omega
